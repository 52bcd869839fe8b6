"""GPU parity of the ParallelSum FLP kernels on the limb-form coefficient rows K1 stages (jx_kernels.h: ten
26-bit limbs per call, 40 bytes), bit for bit against the C oracle: verdicts, Finish messages, aggregate,
count and checksum (helper) and every prep share (leader).

The ring kernel (flp_psum_part_glds_kernel) keeps measurement rows four calls deep and coefficient rows three
deep and runs its calls in unrolled groups of twelve (three blocks of four) with a generic loop for the rest,
so the call counts here sit below, at and past both depths (1..5), one past two blocks of four (9), at the
longest all-generic count (15), at the first count that enters the unrolled loop (16), and at two turns of it
(28). SumVec bits = 1 with length = calls * chunk - 1 makes the last call ragged. chunk 5 has three slot groups
(a padding wave in its only workgroup), chunk 11 six (a second workgroup with two padding waves and a
half-real last group). chunk_length 1 takes the register-prefetch kernel, which reads the same rows."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from janus_amd.engine import HelperEngine
from janus_amd.vdaf import Prio3
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VK = bytes(range(70, 86))
# (calls, chunk_length)
RING_SHAPES = [(1, 5), (2, 5), (3, 5), (4, 5), (5, 11), (9, 11), (15, 5), (16, 11), (28, 5)]


def _sumvec(calls, chunk):
    length = calls * chunk - 1 if chunk > 1 else calls  # (chunk_length 1 has no ragged call)
    v = Prio3.sum_vec(1, length, chunk)
    assert v.calls == calls
    return v, _oracle(v)


def _key(v: Prio3):
    return v.algo_id, v.bits, v.length, v.chunk_length


def _oracle(v: Prio3) -> O.Prio3Oracle:
    return O.Prio3Oracle(*_key(v))


@functools.lru_cache(maxsize=None)
def _pool(algo, bits, length, chunk, n=65, tamper_every=6):
    """n client reports (the C oracle's client and leader), one random bit of the verifier part of every
    6th leader prep share flipped, and the oracle's helper results. Computed once; callers do not write."""
    orc = O.Prio3Oracle(algo, bits, length, chunk)
    rng = np.random.default_rng(1000 * length + 10 * chunk + algo)
    if algo == O.HISTOGRAM:
        meas = rng.integers(0, length, size=(n, 1), dtype=np.uint64)
    else:
        meas = rng.integers(0, 1 << bits, size=(n, length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    ps, his, lps, _ = orc.client_leader_batch(VK, meas, nonces, rands, nthreads=16)
    ver = lps.shape[1] - orc.sizes.seed  # the verifier elements (the joint-rand part follows them)
    for i in range(0, n, tamper_every):
        # a low byte of one verifier element: the element stays below p, so the FLP decides (verdict 3)
        lps[i, 16 * int(rng.integers(0, ver // 16)) + int(rng.integers(0, 8))] ^= 1 << int(rng.integers(0, 8))
    want = orc.helper_prep_batch(VK, nonces, ps, his, lps, nthreads=16, want_out_shares=True)
    assert (want["verdicts"] == 3).sum() >= n // tamper_every and (want["verdicts"] == 0).sum() > n // 2
    for a in (nonces, ps, his, lps, *[x for x in want.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return nonces, ps, his, lps, want


@functools.lru_cache(maxsize=None)
def _want(key, first, n):
    """The oracle's helper results for reports [first, first + n) of the pool (the whole pool: computed with it)."""
    nonces, ps, his, lps, want = _pool(*key)
    if (first, n) == (0, nonces.shape[0]):
        return want
    sl = slice(first, first + n)
    return O.Prio3Oracle(*key).helper_prep_batch(VK, nonces[sl], ps[sl], his[sl], lps[sl], nthreads=16,
                                                 want_out_shares=True)


def _check_helper(vdaf, n, first=0, split=0):
    """Reports [first, first + n) of the shape's pool through a helper engine: verdicts, Finish messages,
    output shares, then aggregate, count and checksum, all == the oracle's for exactly those reports."""
    nonces, ps, his, lps, _ = _pool(*_key(vdaf))
    want = _want(_key(vdaf), first, n)
    sl = slice(first, first + n)
    with HelperEngine(vdaf, VK) as eng:
        if split:
            eng.debug(3, split)
        res = eng.helper_initialized_batch(nonces[sl], ps[sl], his[sl], lps[sl], want_out_shares=True)
        np.testing.assert_array_equal(res.verdicts, want["verdicts"])
        fin = want["verdicts"] == 0
        np.testing.assert_array_equal(res.prep_msgs[fin], want["prep_msgs"][fin])
        np.testing.assert_array_equal(res.out_shares[fin], want["out_shares"][fin])
        eng.accumulate(n)
        assert eng.aggregate_share(0) == (want["agg"], want["count"], want["checksum"])
    return want


@pytest.mark.parametrize("calls,chunk", RING_SHAPES, ids=[f"calls{c}_chunk{k}" for c, k in RING_SHAPES])
def test_ring_call_counts(calls, chunk):
    """65 reports (a full block and a one-report block), every 6th tampered."""
    _check_helper(_sumvec(calls, chunk)[0], 65)


@pytest.mark.parametrize("first,n", [(1, 1), (0, 1), (0, 64)], ids=["one_valid", "one_tampered", "one_block"])
def test_report_counts(first, n):
    """One report (a valid one: count 1; the tampered report 0: verdict 3, an empty aggregate) and exactly one
    block (65 is every other case), 5 calls of chunk 11."""
    want = _check_helper(_sumvec(5, 11)[0], n, first=first)
    assert want["count"] == int((want["verdicts"] == 0).sum())
    assert want["verdicts"][0] == (3 if first == 0 else 0)


def test_prefetch_kernel_chunk_length_1():
    _check_helper(_sumvec(7, 1)[0], 65)


def test_histogram():
    """Histogram 50 / 7: 8 calls, the last with one real element, four slot groups, the sum-of-x column."""
    _check_helper(Prio3.histogram(50, 7), 65)


@pytest.mark.parametrize("split", [3, 5, 6, 7], ids=["lanes", "fused", "pairs", "words"])
def test_every_helper_k1_writes_the_rows(split):
    """Each helper K1 forced in turn (all of them stage the rows through the same tail), 9 calls of chunk 11."""
    _check_helper(_sumvec(9, 11)[0], 65, split=split)


@pytest.mark.parametrize("calls,chunk", [(3, 5), (9, 11), (16, 11)], ids=["calls3", "calls9", "calls16"])
def test_leader_in_place_padded_rows(calls, chunk):
    """The leader reads its measurement share in place from input-share rows at a padded stride (garbage in
    the padding), 65 rows: every prep share == the oracle's prepare_init; then the helper decides on them."""
    import torch

    vdaf, orc = _sumvec(calls, chunk)
    n, K = 65, 13
    rng = np.random.default_rng(77 + calls)
    meas = rng.integers(0, 1 << vdaf.bits, size=(K, vdaf.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(K, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(K, orc.sizes.client_rand), dtype=np.uint8)
    shards = [orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()) for i in range(K)]
    ps, lis, his = (np.frombuffer(b"".join(s[k] for s in shards), np.uint8).reshape(K, -1) for k in range(3))
    want = [orc.prep_init(VK, 0, nonces[i].tobytes(), ps[i].tobytes(), lis[i].tobytes()) for i in range(K)]
    assert all(w[0] == 0 for w in want)
    idx = np.arange(n) % K
    stride = -(-lis.shape[1] // 128) * 128 + 16
    rows = np.full((K, stride), 0xA5, np.uint8)
    rows[:, :lis.shape[1]] = lis
    dev = torch.device("cuda", 0)
    d_n, d_ps, d_lis = (torch.from_numpy(np.ascontiguousarray(a[idx])).to(dev) for a in (nonces, ps, rows))
    d_lps = torch.empty((n, vdaf.prep_share_len), dtype=torch.uint8, device=dev)
    with HelperEngine(vdaf, VK) as leader:
        leader.leader_init_device(n, d_n.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(), d_lps.data_ptr(),
                                  lis_stride=stride)
        leader.sync()
        got = d_lps.cpu().numpy()
    for i in range(n):
        assert got[i].tobytes() == want[idx[i]][1], f"row {i} (report {idx[i]})"
    lps = got.copy()
    lps[4, 16] ^= 2  # a wire value of report 4: the FLP fails
    hw = orc.helper_prep_batch(VK, nonces[idx], ps[idx], his[idx], lps, nthreads=16)
    assert hw["verdicts"].tolist() == [3 if i == 4 else 0 for i in range(n)]
    with HelperEngine(vdaf, VK) as helper:
        res = helper.helper_initialized_batch(nonces[idx], ps[idx], his[idx], lps)
        np.testing.assert_array_equal(res.verdicts, hw["verdicts"])
        np.testing.assert_array_equal(res.prep_msgs[res.verdicts == 0], hw["prep_msgs"][hw["verdicts"] == 0])
        helper.accumulate(n)
        assert helper.aggregate_share(0) == (hw["agg"], hw["count"], hw["checksum"])
