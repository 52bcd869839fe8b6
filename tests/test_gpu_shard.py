"""Prio3.shard on the GPU (jx_client_shard_batch / jx_client_shard_device) against the C oracle's jo_shard with the
same nonce and client randomness: the public share, the leader input share and the helper input share byte for
byte, for Count, Sum, SumVec and Histogram; then the loop closed on the device: shard -> leader init -> helper
prepare -> leader finish -> aggregate -> Prio3.unshard."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import shard_shapes as SS
from janus_amd._lib import EngineError
from janus_amd.engine import SHARD_INVALID_MEASUREMENT, SHARD_MAX_P, HelperEngine
from janus_amd.vdaf import Prio3
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VK = bytes(range(16))
SIZES = (1, 64, 65)


def _oracle(v: Prio3):
    return O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)


def _random_meas(v: Prio3, rng, n):
    if v.algo_id == O.COUNT:
        return rng.integers(0, 2, size=(n, 1), dtype=np.uint64)
    if v.algo_id == O.HISTOGRAM:
        return rng.integers(0, v.length, size=(n, 1), dtype=np.uint64)
    width = v.length if v.algo_id == O.SUMVEC else 1
    if v.bits == 64:
        return rng.integers(0, 1 << 64, size=(n, width), dtype=np.uint64)
    return rng.integers(0, 1 << v.bits, size=(n, width), dtype=np.uint64)


def _inputs(v: Prio3, n, seed, meas=None):
    rng = np.random.default_rng(seed)
    if meas is None:
        meas = _random_meas(v, rng, n)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    return np.ascontiguousarray(meas, dtype=np.uint64), nonces, rands


def _expected(v: Prio3, meas, nonces, rands):
    orc = _oracle(v)
    assert orc.sizes.client_rand == v.client_rand_len
    rows = [orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()) for i in range(len(nonces))]
    return [np.frombuffer(b"".join(r[k] for r in rows), np.uint8).reshape(len(rows), -1) for k in range(3)]


def _check(v: Prio3, meas, nonces, rands, sizes=SIZES):
    """Every n of `sizes`: the first n reports sharded in one call equal the oracle's rows."""
    want = _expected(v, meas, nonces, rands)
    with HelperEngine(v, VK) as eng:
        assert eng.client_rand_bytes() == v.client_rand_len
        for n in sizes:
            got = eng.shard_batch(meas[:n], nonces[:n], rands[:n])
            assert not got.status.any(), n
            for name, g, w in zip(("public share", "leader input share", "helper input share"),
                                  (got.public_shares, got.leader_input_shares, got.helper_input_shares), want):
                bad = np.nonzero((g != w[:n].reshape(g.shape)).any(axis=1))[0] if g.size else []
                assert len(bad) == 0, f"{v.name()} n={n}: {name} of reports {list(bad[:8])} differs"


def test_count():
    v = Prio3.count()
    meas = (np.arange(130, dtype=np.uint64) % 3 == 1).astype(np.uint64).reshape(130, 1)  # 0 and 1 mixed
    meas[[0, 63, 64, 129]] = [[1], [0], [1], [1]]
    _, nonces, rands = _inputs(v, 130, 1)
    _check(v, meas, nonces, rands, sizes=(130,))


@pytest.mark.parametrize("bits", [1, 3, 4, 64])
def test_sum(bits):
    """bits 1: P = 2; bits 3: calls = P - 1, no zero tail; bits 4: P = 8 with a zero tail; bits 64: the extremes."""
    v = Prio3.sum(bits)
    meas, nonces, rands = _inputs(v, 65, 10 + bits)
    meas[0, 0] = 0
    meas[1, 0] = (1 << bits) - 1
    _check(v, meas, nonces, rands)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 3), (1, 3, 8), (1, 300, 1), (1, 600, 1)], ids=str)
def test_sum_vec(shape):
    """(2,5,3): a ragged last call with padded slots; (1,3,8): the chunk is longer than the measurement;
    (1,300,1): P = 512, more than two points per lane; (1,600,1): P = 1024, the cap."""
    v = Prio3.sum_vec(*shape)
    meas, nonces, rands = _inputs(v, 65, 100 + sum(shape))
    meas[0] = 0
    meas[1] = (1 << v.bits) - 1
    _check(v, meas, nonces, rands)


def test_sum_vec_8x1000_88():
    v = Prio3.sum_vec(8, 1000, 88)
    _check(v, *_inputs(v, 65, 200), sizes=(65,))


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (256, 16)], ids=str)
def test_histogram(shape):
    v = Prio3.histogram(*shape)
    meas, nonces, rands = _inputs(v, 65, 300 + sum(shape))
    for i in range(65):  # every index of the small shapes; 0, 255 and a middle one of the large
        meas[i, 0] = (0, v.length - 1, v.length // 2)[i % 3] if v.length > 3 else i % v.length
    _check(v, meas, nonces, rands)


def _matrix_inputs(v: Prio3, n):
    """Report 0 all zeros, report 1 all max (Histogram: the first and the last index), the rest seeded random."""
    meas, nonces, rands = _inputs(v, n, 7000 + 31 * v.meas_len + v.chunk_length)
    meas[0] = 0
    meas[1] = v.length - 1 if v.algo_id == O.HISTOGRAM else (1 << v.bits) - 1
    return meas, nonces, rands


@pytest.mark.parametrize("v", SS.INSTANCES, ids=SS.shape_id)
def test_shape_matrix(v):
    """The matrix of shard_shapes.py (its ledger: test_shard_shapes.py): every transform size of both wire paths,
    every wave layout, every residue of the absorb kernel's tail and every exit of xof_stream128, a full wave and
    one report more in one call."""
    _check(v, *_matrix_inputs(v, 65), sizes=(65,))


@pytest.mark.parametrize("v", [SS.W2_P512, SS.W4_P256], ids=SS.shape_id)
def test_multi_wave_layouts_in_a_ragged_launch(v):
    """The two layouts at the LDS limit (two waves at P = 512 with three slots; four waves at P = 256) through
    shard_device with a padded row stride, the call cut into launches of 64, 64 and 2 reports."""
    import torch

    n = 130
    meas, nonces, rands = _matrix_inputs(v, n)
    dev = torch.device("cuda", 0)
    lis_len = v.leader_input_share_len
    stride = (lis_len + 127) // 128 * 128 + 128
    d_m = torch.from_numpy(meas.view(np.int64)).to(dev)
    d_n, d_r = torch.from_numpy(nonces).to(dev), torch.from_numpy(rands).to(dev)
    u8 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device=dev)  # noqa: E731
    d_ps, d_lis, d_his, d_st = u8(n, v.public_share_len), u8(n, stride), u8(n, v.helper_input_share_len), u8(n)
    torch.cuda.synchronize()
    with HelperEngine(v, VK) as eng:
        eng.debug(10, 64)
        eng.shard_device(n, d_m.data_ptr(), d_n.data_ptr(), d_r.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(),
                         d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)
        st, ps, lis, his = (t.cpu().numpy() for t in (d_st, d_ps, d_lis, d_his))
    assert not st.any()
    want_ps, want_lis, want_his = _expected(v, meas, nonces, rands)
    np.testing.assert_array_equal(ps, want_ps)
    np.testing.assert_array_equal(his, want_his)
    np.testing.assert_array_equal(lis[:, :lis_len], want_lis)
    assert not lis[:, lis_len:].any()  # the padding is zeroed


def test_rejected_samples():
    """Count reports whose helper seeds are those of tests/golden/reject_count.json: real rejected samples in the
    helper measurement-share and proof-share streams."""
    doc = json.load(open(os.path.join(GOLDEN, "reject_count.json")))
    assert {r["stream"] for r in doc["rejections"]} >= {"meas", "proofs"}
    reps = doc["reports"]
    v = Prio3.count()
    n = len(reps)
    meas = np.array([r["measurement"] for r in reps], dtype=np.uint64).reshape(n, 1)
    nonces = np.frombuffer(b"".join(bytes.fromhex(r["nonce"]) for r in reps), np.uint8).reshape(n, 16)
    rands = np.random.default_rng(5).integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    for i, r in enumerate(reps):
        rands[i, :32] = np.frombuffer(bytes.fromhex(r["helper_input_share"]), np.uint8)
    _check(v, meas, nonces, rands, sizes=(n,))


def test_call_cut_into_launches():
    """More reports than one launch holds (debug option 10 sets that to 64): the host call's launches, the last a
    ragged one, together equal the oracle."""
    v = Prio3.histogram(3, 2)
    meas, nonces, rands = _inputs(v, 150, 350)
    want = _expected(v, meas, nonces, rands)
    with HelperEngine(v, VK) as eng:
        eng.debug(10, 64)
        got = eng.shard_batch(meas, nonces, rands)
    assert not got.status.any()
    for g, w in zip((got.public_shares, got.leader_input_shares, got.helper_input_shares), want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("v,bad", [(Prio3.sum(5), [1 << 5]), (Prio3.sum_vec(3, 4, 2), [1, 7, 1 << 3, 0]),
                                   (Prio3.histogram(6, 2), [6]), (Prio3.count(), [2])],
                         ids=["sum", "sumvec", "histogram", "count"])
def test_out_of_range_measurement_is_refused(v, bad):
    """An out-of-range measurement in the middle of a wave: its status is JX_SHARD_INVALID_MEASUREMENT and its rows
    are zeros; every other report of the wave equals the oracle."""
    n, k = 70, 37
    meas, nonces, rands = _inputs(v, n, 400 + v.algo_id)
    meas[k] = bad
    good = np.arange(n) != k
    want = _expected(v, meas[good], nonces[good], rands[good])
    with HelperEngine(v, VK) as eng:
        got = eng.shard_batch(meas, nonces, rands)
    assert got.status[k] == SHARD_INVALID_MEASUREMENT and not got.status[good].any()
    for g, w in zip((got.public_shares, got.leader_input_shares, got.helper_input_shares), want):
        assert not g[k].any()
        np.testing.assert_array_equal(g[good], w.reshape(n - 1, -1) if g.shape[1] else g[good])


@pytest.mark.parametrize("v", [Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 1, 8, 2),
                               Prio3.fixedpoint_boundedl2_vec_sum(16, 4)], ids=["multiproof", "fixedpoint"])
def test_unsupported_instances(v):
    with HelperEngine(v, bytes(v.verify_key_len)) as eng:
        with pytest.raises(EngineError, match=r"\(-2\).*algo id 4.*algo id 5"):
            eng.shard_batch(np.zeros((2, v.length), np.uint64), bytes(32))


def test_transform_size_above_the_cap_is_refused():
    v = Prio3.sum_vec(1, SHARD_MAX_P, 1)  # SHARD_MAX_P calls: P = 2 SHARD_MAX_P
    assert v.P == 2 * SHARD_MAX_P
    with HelperEngine(v, VK) as eng:
        with pytest.raises(EngineError, match=r"\(-2\).*JX_SHARD_MAX_P"):
            eng.shard_batch(np.zeros((1, v.length), np.uint64), bytes(16))


@pytest.mark.parametrize("v", [Prio3.sum_vec(2, 5, 3), Prio3.histogram(3, 2)], ids=["sumvec_2_5_3", "histogram_3_2"])
def test_end_to_end_on_the_device(v):
    """shard_device with a padded row stride -> leader_init_device -> helper prepare + aggregate -> leader finish ->
    leader accumulate, every call queued behind a producer kernel on torch's stream and nothing synchronised
    before the final reads: every report finishes, and Prio3.unshard of the two aggregate shares is the column
    sums of the measurements. The sharded rows equal the oracle's as well."""
    import torch

    n = 130
    meas, nonces, rands = _inputs(v, n, 500 + v.algo_id)
    dev = torch.device("cuda", 0)
    lis_len = v.leader_input_share_len
    stride = (lis_len + 127) // 128 * 128 + 128
    leader, helper = HelperEngine(v, VK), HelperEngine(v, bytes(range(16)))
    pinned = lambda a: torch.from_numpy(np.array(a, copy=True)).pin_memory()  # noqa: E731
    h_m, h_n, h_r = pinned(meas.view(np.int64)), pinned(nonces), pinned(rands)
    d_m = torch.empty(h_m.shape, dtype=torch.int64, device=dev)
    d_n, d_r = (torch.empty(t.shape, dtype=torch.uint8, device=dev) for t in (h_n, h_r))
    u8 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device=dev)  # noqa: E731
    d_ps, d_lis, d_his, d_st = u8(n, v.public_share_len), u8(n, stride), u8(n, v.helper_input_share_len), u8(n)
    d_lps, d_msgs = u8(n, v.prep_share_len), u8(n, v.prep_msg_len)
    d_lver, d_hver, d_fver = u8(n), u8(n), u8(n)
    leader.debug(10, 64)  # 64 reports per launch: the call is cut into three, the last of two reports
    torch.cuda.synchronize()
    try:
        torch.cuda._sleep(200_000_000)
        for dst, src in ((d_m, h_m), (d_n, h_n), (d_r, h_r)):
            dst.copy_(src, non_blocking=True)
        leader.shard_device(n, d_m.data_ptr(), d_n.data_ptr(), d_r.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(),
                            d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)
        bid = leader.leader_init_device(n, d_n.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(), d_lps.data_ptr(),
                                        d_lver.data_ptr(), lis_stride=stride)
        helper.prep_and_aggregate_device(d_n.data_ptr(), d_ps.data_ptr(), d_his.data_ptr(), d_lps.data_ptr(), n,
                                         d_out_prep_msgs=d_msgs.data_ptr(), d_out_verdicts=d_hver.data_ptr())
        leader.leader_finish_device(bid, n, d_msgs.data_ptr(), d_hver.data_ptr(), d_fver.data_ptr())
        leader.accumulate_device(bid, n)
        st, lver, hver, fver, ps, lis, his = (t.cpu().numpy() for t in (d_st, d_lver, d_hver, d_fver, d_ps, d_lis, d_his))
        agg_l, cnt_l, cs_l = leader.aggregate_share(0)
        agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    finally:
        leader.close()
        helper.close()
    assert not st.any() and not lver.any() and not hver.any() and not fver.any()  # JX_FINISHED everywhere
    assert cnt_l == cnt_h == n and cs_l == cs_h
    if v.algo_id == O.HISTOGRAM:
        sums = [int(np.sum(meas[:, 0] == b)) for b in range(v.length)]
    else:
        sums = [int(meas[:, j].astype(object).sum()) for j in range(v.length)]
    assert v.unshard([agg_l, agg_h], n) == sums
    want_ps, want_lis, want_his = _expected(v, meas, nonces, rands)
    np.testing.assert_array_equal(ps, want_ps)
    np.testing.assert_array_equal(his, want_his)
    np.testing.assert_array_equal(lis[:, :lis_len], want_lis)
    assert not lis[:, lis_len:].any()  # the padding is zeroed
