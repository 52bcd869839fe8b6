"""GPU parity of the ParallelSum FLP kernels at chunk_length 1 and past the points where they fold their lazy
wire sums, bit for bit against the C oracle (pinned at these shapes by tests/test_oracle_long_gadgets.py).

What the shapes (tests/golden/make_golden.py LONG_GADGETS) reach that no other test does:
  * chunk_length 1: the one-slot-per-wave kernels (flp_psum_part_kernel<1, ..>, mp_flp_part_kernel<1, ..>),
    whose call loop runs in blocks of 512 (Field128: a normalise after each) or 1024 (Field64: a fold) and
    reloads its prefetch registers at each block start: 512 / 1024 calls (the block ends on the last call) and
    513 / 1025 (one call in the next block).
  * chunk_length 2 and 3 with more than 512 / 1024 calls: the normalise inside the LDS ring loop and the
    Field64 two-slot kernel's fold, with a ragged last call, a half-real last group and an odd proof count.
  * one call with chunk_length > the measurement length, and three calls: fewer than the ring's depth of 4.
  * a leader whose every measurement and proof element has near-maximal limbs, at call counts where a sum
    that is never normalised (folded) wraps 64 bits.

Shown to bite on an MI355X, one line altered per build (this file plus test_gpu_parity.test_golden):
  * the one-slot block loop stepping `k0 += 511` (call 512 taken twice): every chunk_length 1 Field128 case
    fails (512, 513, 600, 2600 calls, the ping-pong, the coalesced jobs, the 4400-call fixture);
  * the ring loop's normalise removed: leader sumvec_1x5200_2 and the sumvec_1x8800_2 fixture fail;
  * the Field64 block loop's fold removed: leader sumvec_f64mp_2_1x2800_1 and the 5600-call fixture fail
    (1025 calls of random shares do not wrap yet); its guarded loop's fold removed: leader
    sumvec_f64mp_2_1x8400_3 fails;
  * psum_ppw forced to 2, and to 1 for chunk_length 3: everything passes (the results do not depend on the
    choice, and the one-slot kernel is right beyond chunk_length 1, ragged tail included).
Not reached by any instance the engine dispatches: the normalise inside psum_part_finish's guarded tail (the
ring runs every call itself, and the one-slot kernel's tail is at most the one ragged call, and only when that
kernel is chosen for chunk_length > 1, as in the forced build above).
"""
from __future__ import annotations

import functools
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from janus_amd._lib import EngineError
from janus_amd.engine import HelperEngine
from janus_amd.vdaf import Prio3
from oracle import oracle as O
from tests.golden import make_golden as MG

pytestmark = pytest.mark.gpu

P128 = 2**128 - 28 * 2**64 + 1
P64 = 2**64 - 2**32 + 1
# below p with near-maximal limbs (every 26-bit limb of the Field128 one but the top is 2^26 - 1 or close)
X128 = 0xFFFFFFFFFFFFFFE3FFFFFFFFFFFFFFFF
X64 = 0xFFFFFFFEFFFFFFFF

VERY_LONG = ["sumvec_1x4400_1", "sumvec_1x8800_2", "sumvec_f64mp_2_1x5600_1"]  # fixtures only (test_golden)
SHAPES = {k: c for k, c in MG.LONG_GADGETS.items() if k not in VERY_LONG}  # 512 .. 1030 calls, 1 call, 3 calls
# Leader only, every element at X: a Field128 column of 5 limb products grows by ~2^53.1 per call and passes
# 2^64 near 1900 calls (2600 calls: mean 2^64.45); a Field64 column by ~2^53, passing 2^64 near 2048 calls.
OVERFLOW = {
    "sumvec_1x2600_1": dict(algo=O.SUMVEC, bits=1, length=2600, chunk=1),
    "sumvec_1x5200_2": dict(algo=O.SUMVEC, bits=1, length=5200, chunk=2),
    "sumvec_f64mp_2_1x2800_1": dict(algo=O.SUMVEC_F64_MULTIPROOF, bits=1, length=2800, chunk=1, proofs=2),
    # chunk_length 3: the half-real second group runs all 2800 calls in the Field64 kernel's guarded loop,
    # which folds on its own count
    "sumvec_f64mp_2_1x8400_3": dict(algo=O.SUMVEC_F64_MULTIPROOF, bits=1, length=8400, chunk=3, proofs=2),
}


def _vdaf(cfg) -> Prio3:
    return Prio3(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg.get("proofs", 1))


def _oracle(cfg) -> O.Prio3Oracle:
    return O.Prio3Oracle(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg.get("proofs", 1))


def _vk(v: Prio3) -> bytes:
    return bytes(range(50, 50 + v.verify_key_len))


def _measurements(cfg, rng, n):
    if cfg["algo"] == O.HISTOGRAM:
        return rng.integers(0, cfg["length"], size=(n, 1), dtype=np.uint64)
    return rng.integers(0, 1 << cfg["bits"], size=(n, cfg["length"]), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _pool(name, n=70, tamper_every=7):
    """n client reports of SHAPES[name] (C-oracle client and leader), one random bit flipped in every 7th
    leader prep share, and the oracle's helper results. Computed once per shape; callers do not write to it."""
    cfg = SHAPES[name]
    v, orc = _vdaf(cfg), _oracle(cfg)
    vk = _vk(v)
    rng = np.random.default_rng(sum(map(ord, name)) + 17)
    meas = _measurements(cfg, rng, n)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    ps, his, lps, _ = orc.client_leader_batch(vk, meas, nonces, rands, nthreads=16)
    for i in range(0, n, tamper_every):
        lps[i, int(rng.integers(0, lps.shape[1]))] ^= 1 << int(rng.integers(0, 8))
    want = orc.helper_prep_batch(vk, nonces, ps, his, lps, nthreads=16, want_out_shares=True)
    for a in (nonces, ps, his, lps, *[x for x in want.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return v, orc, vk, nonces, ps, his, lps, want


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_batches_vs_oracle(name):
    """70 reports (a full 64-report block and a partial one, so lanes past the fixtures' 12), every 7th
    tampered: verdicts, Finish messages, output shares, aggregate, count and checksum, and the fused
    prepare-and-aggregate path into a second segment."""
    v, orc, vk, nonces, ps, his, lps, want = _pool(name)
    n = nonces.shape[0]
    fin = want["verdicts"] == 0
    assert fin.sum() > n // 2
    with HelperEngine(v, vk) as eng:
        res = eng.helper_initialized_batch(nonces, ps, his, lps, want_out_shares=True)
        np.testing.assert_array_equal(res.verdicts, want["verdicts"])
        np.testing.assert_array_equal(res.prep_msgs[fin], want["prep_msgs"][fin])
        np.testing.assert_array_equal(res.out_shares[fin], want["out_shares"][fin])
        eng.accumulate(n)
        assert eng.aggregate_share(0) == (want["agg"], want["count"], want["checksum"])
        v2, m2 = eng.prep_and_aggregate(nonces, ps, his, lps, segment=5)
        np.testing.assert_array_equal(v2, want["verdicts"])
        np.testing.assert_array_equal(m2[fin], want["prep_msgs"][fin])
        assert eng.aggregate_share(5) == (want["agg"], want["count"], want["checksum"])


def _crafted_elements(rng, count, field_bytes, all_x):
    """count field elements, little-endian: each X, p - 1, 0, 1 or a random element below p (all_x: each X)."""
    kind = np.zeros(count, np.int64) if all_x else rng.integers(0, 5, size=count)
    if field_bytes == 16:
        x, pm1 = (X128 & (2**64 - 1), X128 >> 64), ((P128 - 1) & (2**64 - 1), (P128 - 1) >> 64)
        lo = rng.integers(0, 2**64, size=count, dtype=np.uint64)
        hi = rng.integers(0, P128 >> 64, size=count, dtype=np.uint64)  # hi < p's high word: below p
        for k, (a, b) in enumerate([x, pm1, (0, 0), (1, 0)]):
            lo[kind == k], hi[kind == k] = a, b
        return np.stack([lo, hi], axis=1).astype("<u8").tobytes()
    el = rng.integers(0, 2**64 - 2**32, size=count, dtype=np.uint64)  # below p
    for k, a in enumerate([X64, P64 - 1, 0, 1]):
        el[kind == k] = a
    return el.astype("<u8").tobytes()


@pytest.mark.parametrize("name", list(SHAPES) + list(OVERFLOW))
def test_leader_crafted_shares_every_verifier_element(name):
    """The leader's whole prep share (v, every wire value at t, G(t), the joint-rand part) == the oracle's
    prep_init, on leader input shares built directly (a leader share needs no valid proof): report 0 is X in
    every measurement and proof element, the other three draw each element from {X, p - 1, 0, 1, random}.
    The four are tiled over 66 rows (two blocks). SumVec takes the leader's in-place ring loads, Histogram
    the staged ones."""
    cfg = SHAPES.get(name) or OVERFLOW[name]
    v, orc = _vdaf(cfg), _oracle(cfg)
    vk, s = _vk(v), orc.sizes
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    K, n = 4, 66
    nel = s.meas_len + v.num_proofs * s.proof_len
    assert s.leader_input_share == nel * s.field_bytes + s.seed
    lis = np.stack([np.frombuffer(_crafted_elements(rng, nel, s.field_bytes, i == 0) + rng.bytes(s.seed), np.uint8)
                    for i in range(K)])
    nonces = rng.integers(0, 256, size=(K, 16), dtype=np.uint8)
    ps = rng.integers(0, 256, size=(K, s.public_share), dtype=np.uint8)
    with ThreadPoolExecutor(K) as ex:  # the oracle call releases the GIL
        want = list(ex.map(lambda i: orc.prep_init(vk, 0, nonces[i].tobytes(), ps[i].tobytes(), lis[i].tobytes()),
                           range(K)))
    assert all(w[0] == 0 for w in want)
    idx = np.arange(n) % K
    with HelperEngine(v, vk) as eng:
        init = eng.leader_initialized_batch(nonces[idx], ps[idx], lis[idx])
    assert not init.verdicts.any()
    fb = s.field_bytes
    for i in range(n):
        got, exp = init.prep_shares[i].tobytes(), want[idx[i]][1]
        if got != exp:  # name the first wrong verifier element
            e = next(j for j in range(0, len(exp), fb) if got[j:j + fb] != exp[j:j + fb]) // fb
            raise AssertionError(f"row {i} (report {idx[i]}): prep share element {e} of {len(exp) // fb} differs")


def _decode(agg: bytes, fb: int):
    return [int.from_bytes(agg[i:i + fb], "little") for i in range(0, len(agg), fb)]


@pytest.mark.parametrize("name", ["sumvec_1x513_1", "sumvec_f64mp_2_1x1025_1"])
def test_ping_pong_leader_helper_on_device(name):
    """Both roles' one-slot kernels in one flow: leader prepare_init -> helper prepare (one tampered leader
    prep share) -> leader prepare_next (one corrupted Finish message); the prep shares, verdicts and messages
    equal the oracle's and the two aggregates sum to the measurements of the reports both sides finished."""
    cfg = SHAPES[name]
    v, orc = _vdaf(cfg), _oracle(cfg)
    vk, s = _vk(v), orc.sizes
    n = 24
    rng = np.random.default_rng(sum(map(ord, name)) + 9)
    meas = _measurements(cfg, rng, n)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, s.client_rand), dtype=np.uint8)

    def client(i):
        a, b, c = orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes())
        rc, share, out, _ = orc.prep_init(vk, 0, nonces[i].tobytes(), a, b)
        assert rc == 0
        return a, b, c, share, out

    with ThreadPoolExecutor(8) as ex:
        rows = list(ex.map(client, range(n)))
    ps, lis, his, lshare, lout = (np.stack([np.frombuffer(r[k], np.uint8) for r in rows]) for k in range(5))
    with HelperEngine(v, vk) as leader, HelperEngine(v, vk) as helper:
        init = leader.leader_initialized_batch(nonces, ps, lis)
        assert not init.verdicts.any()
        np.testing.assert_array_equal(init.prep_shares, lshare)
        lps = init.prep_shares.copy()
        lps[2, 0] ^= 1
        hres = helper.helper_initialized_batch(nonces, ps, his, lps, want_out_shares=True)
        want = orc.helper_prep_batch(vk, nonces, ps, his, lps, nthreads=8, want_out_shares=True)
        np.testing.assert_array_equal(hres.verdicts, want["verdicts"])
        assert hres.verdicts[2] != 0 and (hres.verdicts != 0).sum() == 1
        ok = want["verdicts"] == 0
        np.testing.assert_array_equal(hres.prep_msgs[ok], want["prep_msgs"][ok])
        np.testing.assert_array_equal(hres.out_shares[ok], want["out_shares"][ok])
        msgs = hres.prep_msgs.copy()
        msgs[4, 7] ^= 0x10
        fin = leader.leader_continued_batch(msgs, want_out_shares=True)
        assert fin.verdicts.tolist() == [4 if i == 4 else 0 for i in range(n)]
        np.testing.assert_array_equal(fin.out_shares[fin.verdicts == 0], lout[fin.verdicts == 0])
        accept = ((hres.verdicts == 0) & (fin.verdicts == 0)).astype(np.uint8)
        leader.accumulate(n, accept_mask=accept)
        helper.accumulate(n, accept_mask=accept)
        agg_l, cnt_l, cs_l = leader.aggregate_share(0)
        agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    acc = accept.astype(bool)
    assert cnt_l == cnt_h == int(acc.sum()) == n - 2 and cs_l == cs_h
    p, fb = (P64, 8) if v.field_bytes == 8 else (P128, 16)
    total = [(a + b) % p for a, b in zip(_decode(agg_l, fb), _decode(agg_h, fb))]
    assert total == [int(meas[acc, j].astype(object).sum()) for j in range(v.length)]


def test_coalesced_jobs_chunk_length_1():
    """SumVec 1x513/1 as 8 jobs of 20 reports from 8 threads on one coalescing engine (the same kernels
    behind the shared launch): each job gets the oracle's verdicts and messages for its own reports."""
    v, orc, vk, nonces, ps, his, lps, want = _pool("sumvec_1x513_1")
    K, n, jobs = nonces.shape[0], 20, 8
    results, errs = {}, []
    with HelperEngine(v, vk) as eng:
        eng.coalesce(True)

        def job(t):
            try:
                idx = (t * 9 + np.arange(n)) % K
                res = eng.helper_initialized_batch(nonces[idx], ps[idx], his[idx], lps[idx])
                eng.release(res.batch_id)
                results[t] = (idx, res.verdicts.copy(), res.prep_msgs.copy())
            except BaseException as e:  # noqa: BLE001 - re-raised below
                errs.append(e)

        th = [threading.Thread(target=job, args=(t,)) for t in range(jobs)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        if errs:
            raise errs[0]
        assert eng.memory()["coalesced_jobs"] == jobs
    assert len(results) == jobs
    tampered = 0
    for t, (idx, verdicts, msgs) in results.items():
        np.testing.assert_array_equal(verdicts, want["verdicts"][idx], err_msg=f"job {t}")
        fin = want["verdicts"][idx] == 0
        tampered += int((~fin).sum())
        np.testing.assert_array_equal(msgs[fin], want["prep_msgs"][idx][fin], err_msg=f"job {t}")
    assert tampered > 0


def test_field128_calls_limit():
    """A Field128 ParallelSum instance with more than 2^16 gadget calls is refused at creation (wacc_reduce
    takes sums of at most 2^16 products); 2^16 calls are accepted. No reports run."""
    vk = bytes(16)
    for v in (Prio3.histogram(65537, 1), Prio3.sum_vec(1, 131073, 2)):
        assert v.calls == 65537
        with pytest.raises(EngineError, match="65536 gadget calls"):
            HelperEngine(v, vk)
    with HelperEngine(Prio3.histogram(65536, 1), vk) as eng:
        assert eng.output_len == 65536
