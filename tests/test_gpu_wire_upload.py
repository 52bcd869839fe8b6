"""GPU: the upload message on the device (jx_report_encode / jx_upload_decode, HelperEngine.encode_reports /
decode_uploads, client.prepare_report_bodies, aggregator.handle_upload_wire).

What the encode must write is janus_amd.messages' encoding of exactly the reports that take room; what the decode must
give is what messages.Report.decode and the Python integers of aggregator.handle_upload extract from the same bodies
(test_wire_upload_host.expected_decode); end to end the wire path must equal the object path (prepare_reports ->
handle_upload -> leader_aggregate_init_wire) under the same randomness. None of it comes from the engine.

Shapes: 1, 64, 65 and 257 reports for the pack (one lane, a full wave, one past it, 64 workgroups of four waves plus
one); 70 for the decode, with encapsulated keys of 32, 65 and 0 bytes mixed so every packed offset is arbitrary mod 16;
1025 and 2049 for the scan (one and two full passes of the workgroup of 1024, plus one)."""
from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest
import torch

import test_wire_upload_host as U
from janus_amd import _lib, client, hpke
from janus_amd._lib import EngineError
from janus_amd.aggregator import (StoredReport, UploadTask, handle_upload, handle_upload_wire, leader_abandon_wire,
                                  leader_aggregate_init_wire)
from janus_amd.engine import (KEY_NONE, UPLOAD_MALFORMED, UPLOAD_NO_ROW, UPLOAD_ODD_PUBLIC_SHARE, UPLOAD_OK, UPLOAD_TOO_EARLY,
                              HelperEngine)
from janus_amd.messages import HpkeCiphertext, PartialBatchSelector, Report, ReportMetadata
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
VK = bytes(range(16))
TASK = bytes(range(100, 132))
NOW = 1_700_000_000
ENGINES = {"count": Prio3.count(), "sumvec": Prio3.sum_vec(2, 5, 3)}


def dev(a, skew: int = 0):
    """The bytes of `a` on the device, starting `skew` bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a).reshape(-1).view(np.uint8)
    t = torch.zeros(a.size + 32, dtype=torch.uint8, device=DEV)
    at = (-t.data_ptr()) % 16 + skew
    t[at:at + a.size] = torch.from_numpy(a.copy()).to(DEV)
    return t[at:at + a.size] if a.size else t[at:at + 1]


def offsets_of(bodies) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.uint64)


def decoded(req, eng) -> dict:
    """An UploadReq's arrays in the form of test_wire_upload_host.expected_decode."""
    db = lambda name: req.device_bytes(name).cpu().numpy().tobytes()  # noqa: E731
    return dict(status=req.status, row_of=req.row_of, ids_all=req.report_ids, times_all=req.all_times, m=req.m,
                index=req.index, ids=db("report_ids"), times=req.times, ps=db("public_shares"),
                key_index=req.key_index.tobytes(), config_ids=req.helper_config_ids.tobytes(),
                offs=[req.leader_enc_offsets, req.leader_payload_offsets, req.helper_enc_offsets, req.helper_payload_offsets],
                packed=[db("leader_encs"), db("leader_payloads"), db("helper_encs"), db("helper_payloads")])


def decode_and_compare(eng, bodies, now, skew, exp, age, kf, ks, on_device: bool, skew_bytes: int = 0):
    body, off = b"".join(bodies), offsets_of(bodies)
    want = U.expected_decode(bodies, eng.public_share_len, now, skew, exp, age, kf, ks)
    if on_device:
        d_body = dev(body, skew_bytes)
        req = eng.decode_uploads(d_body, off, now, kf, ks, skew, exp, age, length=len(body))
    else:
        req = eng.decode_uploads(body, off, now, kf, ks, skew, exp, age)
    with req:
        assert (req.n, req.m) == (len(bodies), want["m"])
        assert req.status_count == np.bincount(want["status"], minlength=6).tolist()
        U.assert_decode_equal(decoded(req, eng), want)
    return want


# ----------------------------------------------------------------------------- encode


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("name", list(ENGINES))
def test_encode_equals_the_codec(name, n):
    v = ENGINES[name]
    rnd = random.Random(1000 * n + len(name))
    with HelperEngine(v, VK) as eng:
        PS = eng.public_share_len
        lct, hct = eng.client_seal_sizes()
        reports = [U.make_report(rnd, PS, 32, lct, 32, hct, lcfg=5, hcfg=201) for _ in range(n)]
        status = np.zeros(n, np.uint8)
        if n > 37:
            status[37] = 1
        j = b"".join
        L = [r.leader_encrypted_input_share for r in reports]
        Hs = [r.helper_encrypted_input_share for r in reports]
        d = [dev(j(r.metadata.report_id for r in reports), 3), dev(j(r.public_share for r in reports), 5),
             dev(j(c.encapsulated_key for c in L), 1), dev(j(c.payload for c in L), 7), dev(j(c.encapsulated_key for c in Hs), 9),
             dev(j(c.payload for c in Hs), 11), dev(status, 2)]
        times = [r.metadata.time for r in reports]
        bodies, offs = eng.encode_reports(n, d[0].data_ptr(), times, d[1].data_ptr() if PS else None, d[2].data_ptr(),
                                          d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 5, 201, d_seal_status=d[6].data_ptr())
        enc = [b"" if s else r.encode() for r, s in zip(reports, status)]
        np.testing.assert_array_equal(offs, offsets_of(enc))
        assert bodies.cpu().numpy().tobytes() == j(enc)
        if n > 37:
            assert offs[38] == offs[37]
        assert eng.report_bound(n) == sum(len(r.encode()) for r in reports)
        # without a status every report takes room; the host form gives the same bytes
        bodies2, offs2 = eng.encode_reports(n, d[0].data_ptr(), times, d[1].data_ptr() if PS else None, d[2].data_ptr(),
                                            d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 5, 201)
        assert bodies2.cpu().numpy().tobytes() == j(r.encode() for r in reports) and offs2[-1] == eng.report_bound(n)
        arr = lambda xs: np.frombuffer(j(xs), np.uint8).reshape(n, -1)  # noqa: E731
        body3, offs3 = eng.encode_reports_host(arr(r.metadata.report_id for r in reports), times, j(r.public_share for r in reports),
                                               arr(c.encapsulated_key for c in L), arr(c.payload for c in L),
                                               arr(c.encapsulated_key for c in Hs), arr(c.payload for c in Hs), 5, 201, status)
        assert body3 == j(enc) and offs3.tolist() == offs.tolist()


def test_encode_other_key_lengths():
    """Nothing assumes 32-byte encapsulated keys: 65 and 0 bytes, passed as arguments."""
    rnd = random.Random(7)
    n = 5
    with HelperEngine(ENGINES["sumvec"], VK) as eng:
        lct, hct = eng.client_seal_sizes()
        reports = [U.make_report(rnd, 32, 65, lct, 0, hct, lcfg=1, hcfg=2) for _ in range(n)]
        j = b"".join
        d = [dev(j(r.metadata.report_id for r in reports)), dev(j(r.public_share for r in reports)),
             dev(j(r.leader_encrypted_input_share.encapsulated_key for r in reports)),
             dev(j(r.leader_encrypted_input_share.payload for r in reports)), dev(b"\0"),
             dev(j(r.helper_encrypted_input_share.payload for r in reports))]
        bodies, offs = eng.encode_reports(n, d[0].data_ptr(), [r.metadata.time for r in reports], d[1].data_ptr(), d[2].data_ptr(),
                                          d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 1, 2, leader_enc_len=65,
                                          helper_enc_len=0)
        assert bodies.cpu().numpy().tobytes() == j(r.encode() for r in reports)


# ----------------------------------------------------------------------------- decode

CLASSES = ["none", "cut_at_boundary", "cut_before_boundary", "cut_after_boundary", "trailing_byte", "u16_overrun",
           "u32_overrun", "length_near_max", "empty_body", "short_body", "corrupt_length"]


@pytest.fixture(scope="module")
def sumvec_engine():
    with HelperEngine(ENGINES["sumvec"], VK) as eng:
        yield eng


@pytest.fixture(scope="module")
def count_engine():
    with HelperEngine(ENGINES["count"], VK) as eng:
        yield eng


@pytest.mark.parametrize("cls", CLASSES)
def test_decode_equals_the_codec(sumvec_engine, cls):
    eng = sumvec_engine
    rnd = random.Random(20241005)
    PS = eng.public_share_len
    kf, ks = U.key_tables(rnd)
    reports = U.mixed_batch(rnd, 70, PS, NOW)
    bodies = [r.encode() for r in reports]
    bodies[3] = U.make_report(rnd, PS + 1, time=NOW).encode()
    k = CLASSES.index(cls)
    if cls != "none":
        cases = U.malformed(rnd, reports[37])[cls]
        bodies[37] = cases[k % len(cases)][0]
    want = decode_and_compare(eng, bodies, NOW, 10, NOW + 5, 40, kf, ks, on_device=k % 2 == 0, skew_bytes=k % 16)
    assert want["status"][37] == (UPLOAD_OK if cls == "none" else UPLOAD_MALFORMED)
    assert want["status"][3] == UPLOAD_ODD_PUBLIC_SHARE and want["row_of"][3] == UPLOAD_NO_ROW
    assert want["status"][36] == UPLOAD_OK and want["status"][38] == UPLOAD_OK  # the neighbours are unaffected
    assert want["row_of"][38] == want["row_of"][36] + (2 if cls == "none" else 1)
    assert set(want["status"].tolist()) >= {0, 2, 3, 4, 5}


def test_kats_on_the_count_engine(count_engine):
    """KAT 1 (an empty public share) decodes; KAT 2 (4 bytes) is an odd public share for Count, its id and time right."""
    bodies = [bytes.fromhex(k["hex"]) for k in U.KATS]
    kf, ks = bytes([KEY_NONE] * 42 + [2] + [KEY_NONE] * 213), bytes([KEY_NONE] * 256)
    with count_engine.decode_uploads(b"".join(bodies), offsets_of(bodies), 60000, kf, ks) as req:
        assert req.status.tolist() == [UPLOAD_OK, UPLOAD_ODD_PUBLIC_SHARE] and req.m == 1
        for i, k in enumerate(U.KATS):
            assert req.report_ids[i].tobytes().hex() == k["report_id"] and int(req.all_times[i]) == k["time"]
        k = U.KATS[0]
        assert req.key_index.tolist() == [[2, KEY_NONE]] and req.helper_config_ids.tolist() == [13]
        assert req.device_bytes("leader_encs").cpu().numpy().tobytes().hex() == k["leader_encrypted_input_share"]["encapsulated_key"]
        assert req.device_bytes("leader_payloads").cpu().numpy().tobytes().hex() == k["leader_encrypted_input_share"]["payload"]
        assert req.device_bytes("helper_encs").cpu().numpy().tobytes().hex() == k["helper_encrypted_input_share"]["encapsulated_key"]
        assert req.device_bytes("helper_payloads").cpu().numpy().tobytes().hex() == k["helper_encrypted_input_share"]["payload"]
    decode_and_compare(count_engine, bodies, 60000, 0, None, None, kf, ks, on_device=True)


LIMITS = [(NOW, 300, NOW + 100, 86_400), (NOW, 0, NOW, 0), (NOW, 300, NOW - 2 * 86_400, 86_400), (NOW, 0, None, None),
          (U.U64, 5, None, None), (U.U64, 0, None, 100), (U.U64, 0, None, 10), (U.U64, 0, None, 9), (U.U64 - 1, 1, U.U64 - 1, None),
          (0, 0, 0, 0), (5, U.U64, 4, U.U64)]


@pytest.mark.parametrize("k", range(len(LIMITS)))
def test_time_checks_at_every_boundary(count_engine, k):
    """time == the limit passes and limit + 1 fails for each of the three checks, precedence when two fail, and both
    sums where they overflow 64 bits: the device's statuses are those of Python's unbounded integers."""
    now, skew, exp, age = LIMITS[k]
    rnd = random.Random(k)
    cand = {0, 1, 4, 5, now, U.U64, U.U64 - 10, U.U64 - 11}
    for lim in (now + skew, exp, None if age is None else now - age):
        if lim is not None:
            cand |= {lim - 1, lim, lim + 1}
    times = sorted(t for t in cand if 0 <= t <= U.U64)
    bodies = [U.make_report(rnd, 0, 32, 20, 32, 20, time=t).encode() for t in times]
    kf, ks = U.key_tables(rnd)
    want = decode_and_compare(count_engine, bodies, now, skew, exp, age, kf, ks, on_device=False)
    assert want["status"].tolist() == [U.python_check(t, now, skew, exp, age) for t in times]
    st = dict(zip(times, want["status"].tolist()))
    if k == 0:  # the expiration lies before now + skew, or no time could be past it without being too early
        assert (st[exp], st[exp + 1], st[now - age], st[now - age - 1], st[now + skew + 1]) == (0, 3, 0, 4, 2)
    if k == 3:
        assert (st[now + skew], st[now + skew + 1]) == (0, 2)


@pytest.mark.parametrize("n", [1025, 2049])
def test_scan_past_its_fold_points(count_engine, n):
    """More uploads than one pass of the scan's workgroup: bodies of varying lengths, every fifth one rejected."""
    rnd = random.Random(n)
    kf, ks = U.key_tables(rnd)
    bodies = [U.make_report(rnd, 0, (32, 65, 0)[i % 3], 17 + i % 23, 32, 9 + i % 11, time=NOW + (100 if i % 5 == 4 else 0)).encode()
              for i in range(n)]
    want = decode_and_compare(count_engine, bodies, NOW, 10, None, None, kf, ks, on_device=True, skew_bytes=5)
    assert want["m"] == n - n // 5 and want["status"][4] == UPLOAD_TOO_EARLY
    assert want["index"].tolist() == [i for i in range(n) if i % 5 != 4]


# ----------------------------------------------------------------------------- end to end


def test_wire_path_equals_the_object_path():
    """client.prepare_report_bodies -> handle_upload_wire against handle_upload(prepare_reports(...)) under the same
    randomness, with one tampered ciphertext, one unknown config id, one odd public share and one too-early report;
    then leader_init_device on the rows and encode_init_req fed with helper_shares against leader_aggregate_init_wire
    over the object path's StoredReports."""
    v = ENGINES["sumvec"]
    n = 70
    rng = np.random.default_rng(70)
    meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    ids = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    eph = rng.integers(0, 256, size=(n, 64), dtype=np.uint8).tobytes()
    times = [NOW + i for i in range(n)]
    rnd = random.Random(5)
    skl, skh = rnd.randbytes(32), rnd.randbytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    info_l, info_h = H.dap_info(recipient=hpke.ROLE_LEADER), H.dap_info(recipient=hpke.ROLE_HELPER)
    now = NOW + n
    with hpke.HpkeSealer(pkl, info_l) as sl, hpke.HpkeSealer(pkh, info_h) as sh, hpke.HpkeOpener(skl, pkl, info_l) as ol, \
            HelperEngine(v, VK) as leader, HelperEngine(v, VK) as leader2:
        kw = dict(rands=rands, ephemeral=eph, report_ids=ids.tobytes(), leader_config_id=5, helper_config_id=6)
        reports = client.prepare_reports(leader, TASK, sl, sh, meas, times, **kw)
        d_bodies, offs = client.prepare_report_bodies(leader, TASK, sl, sh, meas, times, **kw)
        enc = [r.encode() for r in reports]
        assert d_bodies.cpu().numpy().tobytes() == b"".join(enc)
        np.testing.assert_array_equal(offs, offsets_of(enc))

        def edit(i, **ch):
            r = reports[i]
            L = r.leader_encrypted_input_share
            reports[i] = Report(ch.get("metadata", r.metadata), ch.get("public_share", r.public_share),
                                ch.get("leader", L), r.helper_encrypted_input_share)

        L10, L20 = reports[10].leader_encrypted_input_share, reports[20].leader_encrypted_input_share
        edit(10, leader=HpkeCiphertext(5, L10.encapsulated_key, L10.payload[:-1] + bytes([L10.payload[-1] ^ 1])))
        edit(20, leader=HpkeCiphertext(9, L20.encapsulated_key, L20.payload))
        edit(30, public_share=reports[30].public_share + b"\0")
        edit(40, metadata=ReportMetadata(reports[40].metadata.report_id, now + 31))
        task = UploadTask(TASK, {5: ol}, tolerable_clock_skew=30)
        enc = [r.encode() for r in reports]
        up = handle_upload(leader, task, reports, now)
        with handle_upload_wire(leader, task, dev(b"".join(enc), 3), offsets_of(enc), now) as out:
            want_status = np.zeros(n, np.uint8)
            want_status[30], want_status[40] = UPLOAD_ODD_PUBLIC_SHARE, UPLOAD_TOO_EARLY
            np.testing.assert_array_equal(out.status, want_status)
            assert out.results() == up.results
            assert sum(isinstance(r, StoredReport) for r in up.results) == n - 4
            assert {int(out.req.index[k]): int(s) for k, s in enumerate(out.open_status) if s} == up.status == {10: 1, 20: 7}
            assert out.counters == up.counters and out.lis_stride == up.lis_stride
            assert torch.equal(out.rows, up.rows)
            # the host form of the same bodies
            with handle_upload_wire(leader, task, b"".join(enc), offsets_of(enc), now) as out_h:
                assert out_h.results() == up.results and torch.equal(out_h.rows, up.rows)

            # ---- the next step: the request body from the arrays that never left the device
            m, a = out.req.m, out.req.d
            cfg, d_encs, eoff, d_pays, poff = out.helper_shares
            d_lps = torch.empty(m * leader.prep_share_len, dtype=torch.uint8, device=DEV)
            d_v = torch.zeros(m, dtype=torch.uint8, device=DEV)
            bid = leader.leader_init_device(m, a.d_report_ids, a.d_public_shares, out.rows.data_ptr(), d_lps.data_ptr(),
                                            d_v.data_ptr(), lis_stride=out.lis_stride)
            with leader.encode_init_req(m, a.d_report_ids, out.req.times, a.d_public_shares, cfg, d_encs, d_pays, poff,
                                        d_lps.data_ptr(), d_v.data_ptr(), b"", 1, None, enc_offsets=eoff,
                                        exclude=out.open_status != 0) as req:
                body = req.body
                assert req.n_sent == n - 4
            leader.release(bid)
        stored = [r for r in up.results if isinstance(r, StoredReport)]
        step = leader_aggregate_init_wire(leader2, stored, up.rows, up.lis_stride, b"", PartialBatchSelector.time_interval())
        try:
            assert body == step.body
        finally:
            leader_abandon_wire(leader2, step)


# ----------------------------------------------------------------------------- refusals


def test_refusals_write_nothing(sumvec_engine):
    eng = sumvec_engine
    rnd = random.Random(9)
    kf, ks = U.key_tables(rnd)
    PS = eng.public_share_len
    bodies = [r.encode() for r in U.mixed_batch(rnd, 6, PS, NOW)]
    body, off = b"".join(bodies), offsets_of(bodies)
    bad = off.copy()
    bad[3] = bad[2] - 1
    with pytest.raises(EngineError, match="must not decrease"):
        eng.decode_uploads(body, bad, NOW, kf, ks)
    past = off.copy()
    past[-1] += 1
    for form in (dict(), dict(length=len(body))):
        with pytest.raises(EngineError, match="past the bodies"):
            eng.decode_uploads(dev(body) if form else body, past, NOW, kf, ks, **form)
    # n >= 2^31 - 1 is refused from the count alone: the offsets are never read
    ck = _lib.JxUploadChecks(NOW, 0, 0, 0, 0, 0)
    h = ctypes.c_void_p()
    one = np.zeros(2, np.uint64)
    buf = np.zeros(1, np.uint8)
    st = eng._L.jx_upload_decode(eng._h, buf.ctypes.data_as(ctypes.c_void_p), 0, (1 << 31) - 1,
                                 one.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(ck),
                                 np.frombuffer(kf, np.uint8).ctypes.data_as(ctypes.c_void_p),
                                 np.frombuffer(ks, np.uint8).ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    assert st == -2 and not h.value  # JX_E_UNSUPPORTED
    # release before and after use, and twice
    req = eng.decode_uploads(body, off, NOW, kf, ks)
    req.release()
    req = eng.decode_uploads(body, off, NOW, kf, ks, 100)
    assert req.m == 6 and req.device_bytes("leader_payloads").numel() == int(req.leader_payload_offsets[-1])
    req.release()
    req.release()
    with eng.decode_uploads(b"", np.zeros(1, np.uint64), NOW, kf, ks) as empty:
        assert (empty.n, empty.m) == (0, 0)

    # the encode: a capacity one byte short is refused before a byte is written
    n = 5
    lct, hct = eng.client_seal_sizes()
    reports = [U.make_report(rnd, PS, 32, lct, 32, hct, lcfg=1, hcfg=2) for _ in range(n)]
    j = b"".join
    d = [dev(j(r.metadata.report_id for r in reports)), dev(j(r.public_share for r in reports)),
         dev(j(r.leader_encrypted_input_share.encapsulated_key for r in reports)),
         dev(j(r.leader_encrypted_input_share.payload for r in reports)),
         dev(j(r.helper_encrypted_input_share.encapsulated_key for r in reports)),
         dev(j(r.helper_encrypted_input_share.payload for r in reports))]
    total = eng.report_bound(n)
    out = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    args = (n, d[0].data_ptr(), [r.metadata.time for r in reports], d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
            d[4].data_ptr(), d[5].data_ptr(), 1, 2)
    with pytest.raises(EngineError, match="shorter than the report bodies"):
        eng.encode_reports(*args, d_out=out.data_ptr(), capacity=total - 1)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    with pytest.raises(EngineError, match="2\\^16"):
        eng.encode_reports(*args, d_out=out.data_ptr(), capacity=total, leader_enc_len=1 << 16)
    assert bool((out == 0xA5).all())
    bodies2, offs2 = eng.encode_reports(*args, d_out=out.data_ptr(), capacity=total)
    assert bodies2.cpu().numpy().tobytes() == j(r.encode() for r in reports) and int(offs2[-1]) == total
    assert bool((out[total:] == 0xA5).all())
