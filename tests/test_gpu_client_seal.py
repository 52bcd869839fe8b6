"""GPU: the client's second half (jx_client_seal_batch / jx_client_seal_device, HelperEngine.seal_reports,
janus_amd.client.prepare_reports): both shares of a report sealed on the device from the rows of the C oracle's
jo_shard, byte for byte against tests/hpke_suites_ref.py's seal_base over PlaintextInputShare([], row) and the
InputShareAad; a call cut into launches; then the loop closed on the device through both sealed front doors: shard ->
seal -> the leader's upload open -> leader init -> the helper's sealed prepare-and-aggregate -> finish -> accumulate."""
from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

import hpke_suites_ref as S
from janus_amd import client, hpke
from janus_amd.aggregator import StoredReport, UploadTask, handle_aggregate_init_encrypted, handle_upload
from janus_amd.engine import KEY_NONE, SEAL_OK, SEAL_SKIPPED, HelperEngine
from janus_amd.messages import PingPongMessage, PlaintextInputShare, PrepareInit, ReportShare
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O
from tests.golden.make_golden import fixedpoint_measurements

pytestmark = pytest.mark.gpu

TASK = bytes(range(100, 132))
VK = bytes(range(16))
INFO_L = H.dap_info(recipient=hpke.ROLE_LEADER)
INFO_H = H.dap_info(recipient=hpke.ROLE_HELPER)
T0 = 1_700_000_000

# (instance, the leader's suite, the helper's suite)
INSTANCES = {
    "count": (Prio3.count(), (1, 1), (1, 1)),
    "sum_3": (Prio3.sum(3), (1, 2), (2, 1)),
    "sumvec_2_5_3": (Prio3.sum_vec(2, 5, 3), (1, 3), (1, 1)),
    "histogram_3_2": (Prio3.histogram(3, 2), (3, 1), (1, 3)),
    "multiproof": (Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 1, 8, 2), (2, 3), (3, 2)),
    "fixedpoint_16_4": (Prio3.fixedpoint_boundedl2_vec_sum(16, 4), (1, 1), (2, 2)),
}


def _oracle(v: Prio3):
    return O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)


def _measurements(v: Prio3, rng, n):
    if v.algo_id == O.COUNT:
        return rng.integers(0, 2, size=(n, 1), dtype=np.uint64)
    if v.algo_id == O.HISTOGRAM:
        return rng.integers(0, v.length, size=(n, 1), dtype=np.uint64)
    if v.algo_id == O.FIXEDPOINT_L2:
        return fixedpoint_measurements(v.bits, v.length, rng, n)
    return rng.integers(0, 1 << v.bits, size=(n, v.length if v.algo_id != O.SUM else 1), dtype=np.uint64)


def _oracle_rows(v: Prio3, n, seed):
    orc, rng = _oracle(v), np.random.default_rng(seed)
    meas = _measurements(v, rng, n)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    rows = [orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()) for i in range(n)]
    ps, lis, his = (np.frombuffer(b"".join(r[k] for r in rows), np.uint8).reshape(n, -1) for k in range(3))
    return nonces, ps, lis, his


@pytest.mark.parametrize("name", list(INSTANCES))
def test_rows(name):
    """n = 1 and 65, a padded row stride, and report 37 (mid-wave) refused by the shard."""
    v, (lkdf, laead), (hkdf, haead) = INSTANCES[name]
    n, k = 65, 37
    rnd = random.Random(v.algo_id)
    nonces, ps, lis, his = _oracle_rows(v, n, 900 + v.algo_id)
    assert lis.shape[1] == v.leader_input_share_len and his.shape[1] == v.helper_input_share_len
    stride = (v.leader_input_share_len + 15) // 16 * 16 + 32
    padded = np.full((n, stride), 0x5A, np.uint8)
    padded[:, :lis.shape[1]] = lis
    times = [T0 + 3 * i for i in range(n)]
    sks = np.frombuffer(rnd.randbytes(64 * n), np.uint8).reshape(n, 64)
    pkl, pkh = H.x25519_base(rnd.randbytes(32)), H.x25519_base(rnd.randbytes(32))
    want = []
    for i in range(n):
        aad = hpke.input_share_aad(TASK, nonces[i].tobytes(), times[i], ps[i].tobytes())
        want.append((S.seal_base(lkdf, laead, pkl, INFO_L, aad, PlaintextInputShare((), lis[i].tobytes()).encode(),
                                 sks[i, :32].tobytes()),
                     S.seal_base(hkdf, haead, pkh, INFO_H, aad, PlaintextInputShare((), his[i].tobytes()).encode(),
                                 sks[i, 32:].tobytes())))
    status = np.zeros(n, np.uint8)
    status[k] = 1
    with hpke.HpkeSealer(pkl, INFO_L, kdf_id=lkdf, aead_id=laead) as sl, \
            hpke.HpkeSealer(pkh, INFO_H, kdf_id=hkdf, aead_id=haead) as sh, \
            HelperEngine(v, bytes(range(v.verify_key_len))) as eng:
        assert eng.client_seal_sizes() == (6 + lis.shape[1] + 16, 6 + his.shape[1] + 16)
        one = eng.seal_reports(nonces[:1], times[:1], ps[:1], padded[:1], his[:1], TASK, sl, sh, sks[:1])
        got = eng.seal_reports(nonces, times, ps, padded, his, TASK, sl, sh, sks, shard_status=status)
    assert one.status.tolist() == [SEAL_OK]
    assert ((one.leader_encs[0].tobytes(), one.leader_cts[0].tobytes()),
            (one.helper_encs[0].tobytes(), one.helper_cts[0].tobytes())) == want[0]
    assert got.status.tolist() == [SEAL_SKIPPED if i == k else SEAL_OK for i in range(n)]
    for i in range(n):
        g = ((got.leader_encs[i].tobytes(), got.leader_cts[i].tobytes()),
             (got.helper_encs[i].tobytes(), got.helper_cts[i].tobytes()))
        if i == k:
            assert all(not any(x) for pair in g for x in pair)
        else:
            assert g == want[i], f"{name}: report {i} differs"


def test_multi_launch():
    """150 reports in launches of 64 (the last one of 22) equal the one launch. The seal only reads rows: any bytes do."""
    v = Prio3.sum_vec(2, 5, 3)
    n = 150
    rng = np.random.default_rng(150)
    u8 = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)  # noqa: E731
    ids, ps, lis, his, sks = u8(n, 16), u8(n, v.public_share_len), u8(n, v.leader_input_share_len), \
        u8(n, v.helper_input_share_len), u8(n, 64)
    times = [T0 + i for i in range(n)]
    status = np.zeros(n, np.uint8)
    status[[63, 64, 149]] = 1
    pkl, pkh = H.x25519_base(bytes(range(32))), H.x25519_base(bytes(range(1, 33)))
    with hpke.HpkeSealer(pkl, INFO_L, aead_id=3) as sl, hpke.HpkeSealer(pkh, INFO_H) as sh, HelperEngine(v, VK) as eng:
        a = eng.seal_reports(ids, times, ps, lis, his, TASK, sl, sh, sks, shard_status=status)
        eng.debug(11, 64)
        b = eng.seal_reports(ids, times, ps, lis, his, TASK, sl, sh, sks, shard_status=status)
    assert (a.status == status).all() and a.leader_cts[0].any() and a.helper_cts[149 - 1].any()
    for f in ("leader_encs", "leader_cts", "helper_encs", "helper_cts", "status"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


@pytest.mark.parametrize("v", [Prio3.sum_vec(2, 5, 3), Prio3.histogram(3, 2)], ids=["sumvec_2_5_3", "histogram_3_2"])
def test_end_to_end_on_the_device(v):
    """Every call queued behind a producer kernel on torch's stream, nothing synchronised before the final reads:
    every report opens at both aggregators and finishes, and Prio3.unshard of the two aggregate shares is the column
    sums of the measurements."""
    import torch

    n = 130
    rng = np.random.default_rng(700 + v.algo_id)
    meas = np.ascontiguousarray(_measurements(v, rng, n), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    sks = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    times = np.arange(T0, T0 + n, dtype=np.uint64)
    rnd = random.Random(9)
    skl, skh = rnd.randbytes(32), rnd.randbytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    dev = torch.device("cuda", 0)
    lis_len = v.leader_input_share_len
    stride = (lis_len + 127) // 128 * 128 + 128
    leader, helper = HelperEngine(v, VK), HelperEngine(v, VK)
    lct, hct = leader.client_seal_sizes()
    sl, sh = hpke.HpkeSealer(pkl, INFO_L, aead_id=3), hpke.HpkeSealer(pkh, INFO_H, kdf_id=3)
    ol, oh = hpke.HpkeOpener(skl, pkl, INFO_L, aead_id=3), hpke.HpkeOpener(skh, pkh, INFO_H, kdf_id=3)
    pinned = lambda a: torch.from_numpy(np.array(a, copy=True)).pin_memory()  # noqa: E731
    h_m, h_n, h_r, h_k = pinned(meas.view(np.int64)), pinned(nonces), pinned(rands), pinned(sks)
    d_m = torch.empty(h_m.shape, dtype=torch.int64, device=dev)
    d_n, d_r, d_k = (torch.empty(t.shape, dtype=torch.uint8, device=dev) for t in (h_n, h_r, h_k))
    u8 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device=dev)  # noqa: E731
    d_ps, d_lis, d_his, d_st = u8(n, v.public_share_len), u8(n, stride), u8(n, v.helper_input_share_len), u8(n)
    d_lenc, d_lcts, d_henc, d_hcts, d_seal = u8(n, 32), u8(n, lct), u8(n, 32), u8(n, hct), u8(n)
    d_rows, d_ext, d_open_l, d_open_h = u8(n, stride), u8(n * lct), u8(n), u8(n)
    d_extlen = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_lps, d_msgs = u8(n, v.prep_share_len), u8(n, v.prep_msg_len)
    d_lver, d_hver, d_fver = u8(n), u8(n), u8(n)
    key_index = np.array([[0, KEY_NONE]] * n, np.uint8)
    l_off, h_off = np.arange(n + 1, dtype=np.uint64) * lct, np.arange(n + 1, dtype=np.uint64) * hct
    task = np.frombuffer(TASK, np.uint8).copy()
    u64p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    leader.debug(10, 64)  # the shard and the seal each cut into three launches
    leader.debug(11, 64)
    torch.cuda.synchronize()
    try:
        torch.cuda._sleep(200_000_000)
        for dst, src in ((d_m, h_m), (d_n, h_n), (d_r, h_r), (d_k, h_k)):
            dst.copy_(src, non_blocking=True)
        leader.shard_device(n, d_m.data_ptr(), d_n.data_ptr(), d_r.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(),
                            d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)
        leader.seal_reports_device(n, d_n.data_ptr(), times, d_ps.data_ptr(), d_lis.data_ptr(), d_his.data_ptr(), TASK, sl,
                                   sh, d_k.data_ptr(), d_lenc.data_ptr(), d_lcts.data_ptr(), d_henc.data_ptr(),
                                   d_hcts.data_ptr(), d_seal.data_ptr(), d_shard_status=d_st.data_ptr(), lis_stride=stride)
        with leader._ordered(None):
            st = leader._L.jx_leader_upload_open_device(
                leader.handle, n, d_n.data_ptr(), times.ctypes.data_as(u64p), d_ps.data_ptr(),
                task.ctypes.data_as(vp), (vp * 1)(ol.handle), 1, key_index.ctypes.data_as(vp), d_lenc.data_ptr(), None,
                d_lcts.data_ptr(), l_off.ctypes.data_as(u64p), d_rows.data_ptr(), stride, d_ext.data_ptr(),
                d_extlen.data_ptr(), d_open_l.data_ptr())
            assert st == 0
        bid = leader.leader_init_device(n, d_n.data_ptr(), d_ps.data_ptr(), d_rows.data_ptr(), d_lps.data_ptr(),
                                        d_lver.data_ptr(), lis_stride=stride)
        helper.prep_and_aggregate_encrypted_device(d_n.data_ptr(), times, d_ps.data_ptr(), TASK, [oh], key_index,
                                                   d_henc.data_ptr(), d_hcts.data_ptr(), h_off, d_lps.data_ptr(), n,
                                                   d_out_prep_msgs=d_msgs.data_ptr(), d_out_verdicts=d_hver.data_ptr(),
                                                   d_out_open_status=d_open_h.data_ptr())
        leader.leader_finish_device(bid, n, d_msgs.data_ptr(), d_hver.data_ptr(), d_fver.data_ptr())
        leader.accumulate_device(bid, n)
        st, seal, open_l, open_h, lver, hver, fver, extlen, rows, lis = (
            t.cpu().numpy() for t in (d_st, d_seal, d_open_l, d_open_h, d_lver, d_hver, d_fver, d_extlen, d_rows, d_lis))
        agg_l, cnt_l, cs_l = leader.aggregate_share(0)
        agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    finally:
        for x in (leader, helper, sl, sh, ol, oh):
            x.close()
    assert not st.any() and not seal.any()
    assert not open_l.any() and not open_h.any() and not extlen.any()  # JX_OPEN_OK at both front doors
    assert not lver.any() and not hver.any() and not fver.any()        # JX_FINISHED everywhere
    np.testing.assert_array_equal(rows[:, :lis_len], lis[:, :lis_len])  # what the leader opened is what was sharded
    assert cnt_l == cnt_h == n and cs_l == cs_h
    if v.algo_id == O.HISTOGRAM:
        sums = [int(np.sum(meas[:, 0] == b)) for b in range(v.length)]
    else:
        sums = [int(meas[:, j].astype(object).sum()) for j in range(v.length)]
    assert v.unshard([agg_l, agg_h], n) == sums


def test_python_layer():
    """client.prepare_reports -> aggregator.handle_upload (the leader) -> handle_aggregate_init_encrypted (the helper)."""
    v = Prio3.sum_vec(2, 5, 3)
    n = 40
    rng = np.random.default_rng(40)
    meas = _measurements(v, rng, n)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    ids = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    times = [T0 + i for i in range(n)]
    rnd = random.Random(3)
    skl, skh = rnd.randbytes(32), rnd.randbytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    with hpke.HpkeSealer(pkl, INFO_L) as sl, hpke.HpkeSealer(pkh, INFO_H, aead_id=2) as sh, \
            hpke.HpkeOpener(skl, pkl, INFO_L) as ol, hpke.HpkeOpener(skh, pkh, INFO_H, aead_id=2) as oh, \
            HelperEngine(v, VK) as leader, HelperEngine(v, VK) as helper:
        reports = client.prepare_reports(leader, TASK, sl, sh, meas, times, rands=rands, report_ids=ids.tobytes(),
                                         leader_config_id=5, helper_config_id=6)
        again = client.prepare_reports(leader, TASK, sl, sh, meas, times, rands=rands, report_ids=ids.tobytes(),
                                       leader_config_id=5, helper_config_id=6)
        # fresh ephemeral keys each time: the same rows under other ciphertexts
        assert all(a.public_share == b.public_share and a.leader_encrypted_input_share != b.leader_encrypted_input_share
                   for a, b in zip(reports, again))
        with pytest.raises(ValueError, match="out of range"):
            client.prepare_reports(leader, TASK, sl, sh, np.full((1, v.length), 1 << v.bits, np.uint64), [T0])
        shard = leader.shard_batch(meas, ids, rands)
        up = handle_upload(leader, UploadTask(TASK, {5: ol}), reports, now=T0 + n)
        assert all(isinstance(r, StoredReport) for r in up.results) and not up.status
        np.testing.assert_array_equal(up.rows.cpu().numpy()[:, :v.leader_input_share_len], shard.leader_input_shares)
        init = leader.leader_initialized_batch(ids, shard.public_shares, shard.leader_input_shares)
        inits = [PrepareInit(ReportShare(r.metadata, r.public_share, r.helper_encrypted_input_share),
                             PingPongMessage.initialize(init.prep_shares[i].tobytes())) for i, r in enumerate(reports)]
        got = handle_aggregate_init_encrypted(helper, oh, 6, TASK, inits)
        assert got.finished.all() and not got.step_failures
