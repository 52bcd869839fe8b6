"""GPU: the leader's upload path (jx_leader_upload_open_*, HelperEngine.leader_upload_open, aggregator.handle_upload)
against a restated loop of handle_upload_generic (aggregator/src/aggregator.rs:1513-1694) over the Python HPKE
references, with leader input shares from the C oracle's shard.

Instances: Prio3Histogram 256/16 (LIS 5,632 bytes: 5.6 strides of the wave), Prio3Sum bits=8 (656 bytes), Prio3Count
(Field64, no blind, 48 bytes) and Prio3SumVecField64MultiproofHmacSha256Aes128 2 x (1, 7, 3) (296 bytes: no multiple
of 16). Each instance's reports are sealed once and shared by its tests."""
from __future__ import annotations

import functools
import random
import struct

import numpy as np
import pytest

import hpke_p256_ref as R
import hpke_suites_ref as S
from janus_amd import hpke
from janus_amd.aggregator import ReportRejection, ReportRejectionReason, StoredReport, UploadTask, handle_upload
from janus_amd.engine import HelperEngine
from janus_amd.messages import Extension, HpkeCiphertext, Report, ReportMetadata
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INFO = H.dap_info(recipient=hpke.ROLE_LEADER)
TASK = bytes(range(32))
P128 = 2**128 - 28 * 2**64 + 1
P64 = 2**64 - 2**32 + 1
OK, DECRYPT, PLAINTEXT, INPUT_SHARE, UNKNOWN = 0, 1, 2, 6, 7

INSTANCES = {
    "hist": Prio3.histogram(256, 16),
    "sum": Prio3.sum(8),
    "count": Prio3.count(),
    "mp": Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 1, 7, 3),
}


class Key:
    def __init__(self, rnd, kem=hpke.KEM_X25519_HKDF_SHA256, kdf=1, aead=1):
        self.kem, self.kdf, self.aead = kem, kdf, aead
        if kem == hpke.KEM_P256_HKDF_SHA256:
            self.sk = rnd.randrange(1, R.N).to_bytes(32, "big")
            self.pk = R.public_key(self.sk)
        else:
            self.sk = rnd.randbytes(32)
            self.pk = H.x25519_base(self.sk)

    def opener(self):
        return hpke.HpkeOpener(self.sk, self.pk, INFO, kem_id=self.kem, kdf_id=self.kdf, aead_id=self.aead)

    def seal(self, rnd, aad, pt):
        if self.kem == hpke.KEM_P256_HKDF_SHA256:
            return R.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, rnd.randrange(1, R.N).to_bytes(32, "big"))
        return S.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, rnd.randbytes(32))

    def open(self, enc, aad, ct):
        if self.kem == hpke.KEM_P256_HKDF_SHA256:
            return R.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 65 else None
        return S.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 32 else None


_rk = random.Random(77)
TASK_KEY = Key(_rk)                                   # config id 1 (task)
GLOBAL_SAME = Key(_rk, aead=2)                        # config id 1 (global): the fallback of the same id
GLOBAL_P256 = Key(_rk, kem=hpke.KEM_P256_HKDF_SHA256)  # config id 2 (global only)
STRANGER = Key(_rk)                                   # nobody's key
TASK_KEYS = {1: TASK_KEY}
GLOBAL_KEYS = {1: GLOBAL_SAME, 2: GLOBAL_P256}


def _oracle(v: Prio3):
    return O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)


def _measurement(v: Prio3, rnd):
    if v.algo_id == 3:
        return rnd.randrange(v.length)
    if v.algo_id == 1:
        return rnd.randrange(2**v.bits)
    if v.algo_id == 0:
        return rnd.randrange(2)
    return [rnd.randrange(2**v.bits) for _ in range(v.length)]


def _set_elem(v: Prio3, lis: bytes, idx: int, value: int) -> bytes:
    fb = v.field_bytes
    return lis[:fb * idx] + value.to_bytes(fb, "little") + lis[fb * (idx + 1):]


def _plaintext(exts: bytes, payload: bytes) -> bytes:
    return struct.pack(">H", len(exts)) + exts + struct.pack(">I", len(payload)) + payload


EXT1 = Extension(0x0000, b"hello").encode()
EXT2 = EXT1 + Extension(0xFF00, b"").encode()


def _cases(name: str):
    """(kind, sealing key, config id, plaintext builder) per report of the instance."""
    v = INSTANCES[name]
    p = P64 if v.field_bytes == 8 else P128
    nm, ne = v.meas_len, v.meas_len + v.num_proofs * v.proof_len
    good = lambda lis: _plaintext(b"", lis)  # noqa: E731
    cases = [("good", TASK_KEY, 1, good), ("good_ext1", TASK_KEY, 1, lambda lis: _plaintext(EXT1, lis)),
             ("good_ext2", TASK_KEY, 1, lambda lis: _plaintext(EXT2, lis))]
    # an element equal to p is rejected and p - 1 accepted, at both ends of the measurement and of the proofs part
    for where, idx in (("meas_first", 0), ("meas_last", nm - 1), ("proof_first", nm), ("proof_last", ne - 1)):
        cases.append((f"p_{where}", TASK_KEY, 1, lambda lis, idx=idx: _plaintext(b"", _set_elem(v, lis, idx, p))))
        cases.append((f"pm1_{where}", TASK_KEY, 1, lambda lis, idx=idx: _plaintext(b"", _set_elem(v, lis, idx, p - 1))))
    if name == "hist":
        # the long instance (a Python seal and open of 5.6 KB take 0.7 s together) carries the wave's cases: the range
        # check past the first stride, the second trial and a tampered block of the second stride; the short ones
        # carry the decoder's
        keep = ("good_ext1", "p_proof_last", "pm1_proof_last", "pm1_meas_first")
        return [c for c in cases if c[0] in keep] + [("fallback", GLOBAL_SAME, 1, good), ("tamper_stride2", TASK_KEY, 1, good)]
    cases += [
        ("unknown_config", TASK_KEY, 9, good),
        ("fallback", GLOBAL_SAME, 1, good),           # the task's key fails, the global one of the same id opens
        ("global_p256", GLOBAL_P256, 2, good),        # a config id only the global keys hold, 65-byte encapsulated key
        ("both_fail", STRANGER, 1, good),
        ("truncated", TASK_KEY, 1, lambda lis: _plaintext(b"", lis)[:-1]),
        ("truncated_ext", TASK_KEY, 1, lambda lis: _plaintext(EXT1, lis)[:5]),
        ("empty", TASK_KEY, 1, lambda lis: b""),
        ("trailing", TASK_KEY, 1, lambda lis: _plaintext(b"", lis) + b"\0"),
        ("unknown_ext", TASK_KEY, 1, lambda lis: _plaintext(Extension(0x0001, b"x").encode(), lis)),
        # an extension whose data length runs past the list
        ("ext_overrun", TASK_KEY, 1, lambda lis: struct.pack(">H", 5) + b"\x00\x00\x00\xffx" + struct.pack(">I", len(lis)) + lis),
        ("lis_plus1", TASK_KEY, 1, lambda lis: _plaintext(b"", lis + b"\0")),
        ("lis_minus1", TASK_KEY, 1, lambda lis: _plaintext(b"", lis[:-1])),
        ("wrong_enc_len", TASK_KEY, 2, good),         # a 32-byte key for the P-256 keypair: fails without an open
    ]
    if v.joint_rand_len:  # the blind is opaque: all ones is fine
        cases.append(("blind_ones", TASK_KEY, 1, lambda lis: _plaintext(b"", lis[:-v.seed_size] + b"\xff" * v.seed_size)))
    return cases


@functools.lru_cache(maxsize=None)
def _sealed(name: str):
    """The instance's reports: (kinds, Reports, the oracle's leader input shares, verify key)."""
    v = INSTANCES[name]
    orc = _oracle(v)
    rnd = random.Random(name)
    vk = rnd.randbytes(v.verify_key_len)
    kinds, reports, shares = [], [], []
    for i, (kind, key, cfg, build) in enumerate(_cases(name)):
        rid = rnd.randbytes(16)
        ps, lis, his = orc.shard(_measurement(v, rnd), rid, rnd.randbytes(orc.sizes.client_rand))
        assert len(lis) == v.leader_input_share_len
        t = 1_700_000_000 + i
        enc, ct = key.seal(rnd, hpke.input_share_aad(TASK, rid, t, ps), build(lis))
        if kind == "tamper_stride2":
            ct = bytearray(ct)
            ct[16 * (64 + 5) + 2] ^= 4
            ct = bytes(ct)
        kinds.append(kind)
        shares.append(lis)
        reports.append(Report(ReportMetadata(rid, t), ps, HpkeCiphertext(cfg, enc, ct), HpkeCiphertext(3, b"h" * 32, b"helper")))
    return kinds, reports, shares, vk


def _ref_upload(v: Prio3, rep: Report):
    """handle_upload_generic after its time checks, restated: (status, extension bytes, payload)."""
    ct = rep.leader_encrypted_input_share
    keys = [k for k in (TASK_KEYS.get(ct.config_id), GLOBAL_KEYS.get(ct.config_id)) if k is not None]
    if not keys:
        return UNKNOWN, b"", None
    aad = hpke.input_share_aad(TASK, rep.metadata.report_id, rep.metadata.time, rep.public_share)
    pt = None
    for k in keys:
        pt = k.open(ct.encapsulated_key, aad, ct.payload)
        if pt is not None:
            break
    if pt is None:
        return DECRYPT, b"", None
    # PlaintextInputShare::get_decoded
    if len(pt) < 2 or 2 + int.from_bytes(pt[:2], "big") > len(pt):
        return PLAINTEXT, b"", None
    end = 2 + int.from_bytes(pt[:2], "big")
    i = 2
    while i < end:
        if i + 4 > end or int.from_bytes(pt[i:i + 2], "big") not in (0x0000, 0xFF00):
            return PLAINTEXT, b"", None
        i += 4 + int.from_bytes(pt[i + 2:i + 4], "big")
        if i > end:
            return PLAINTEXT, b"", None
    if end + 4 > len(pt) or end + 4 + int.from_bytes(pt[end:end + 4], "big") != len(pt):
        return PLAINTEXT, b"", None
    payload = pt[end + 4:]
    # A::InputShare::get_decoded_with_param(&(&vdaf, 0), payload)
    fb, p = v.field_bytes, (P64 if v.field_bytes == 8 else P128)
    ne = v.meas_len + v.num_proofs * v.proof_len
    if len(payload) != v.leader_input_share_len or any(
            int.from_bytes(payload[fb * k:fb * (k + 1)], "little") >= p for k in range(ne)):
        return INPUT_SHARE, b"", None
    return OK, pt[2:end], payload


def _open(eng, reports, openers, lis_stride=0):
    keypairs = [openers[id(k)] for k in (TASK_KEY, GLOBAL_SAME, GLOBAL_P256)]
    idx = {id(TASK_KEY): 0, id(GLOBAL_SAME): 1, id(GLOBAL_P256): 2}
    ki = []
    for r in reports:
        cfg = r.leader_encrypted_input_share.config_id
        ks = [k for k in (TASK_KEYS.get(cfg), GLOBAL_KEYS.get(cfg)) if k is not None]
        ki.append([idx[id(ks[0])] if ks else 0xFF, idx[id(ks[1])] if len(ks) > 1 else 0xFF])
    n = len(reports)
    return eng.leader_upload_open(
        np.frombuffer(b"".join(r.metadata.report_id for r in reports), np.uint8).reshape(n, 16),
        [r.metadata.time for r in reports], np.frombuffer(b"".join(r.public_share for r in reports), np.uint8), TASK,
        keypairs, np.array(ki, np.uint8), [r.leader_encrypted_input_share.encapsulated_key for r in reports],
        [r.leader_encrypted_input_share.payload for r in reports], lis_stride=lis_stride)


@pytest.fixture(scope="module")
def openers():
    ops = {id(k): k.opener() for k in (TASK_KEY, GLOBAL_SAME, GLOBAL_P256)}
    yield ops
    for o in ops.values():
        o.close()


@pytest.mark.parametrize("name", ["sum", "count", "mp", "hist"])
def test_upload_open_vs_restated_loop(name, openers):
    """Status, extension bytes and row of every report equal the restated loop's; rejected rows are zero; the rows go
    straight into leader_init_device at stride LIS (rounded up to 16 where LIS is no multiple) and at LIS rounded up
    to 128, and give the prepare shares and verdicts of jx_leader_prep_init_batch on the plaintext shares."""
    import torch

    v = INSTANCES[name]
    kinds, reports, shares, vk = _sealed(name)
    want = [_ref_upload(v, r) for r in reports]
    by_kind = dict(zip(kinds, want))
    # the cases mean what their names say
    assert by_kind["good_ext1"][:2] == (OK, EXT1) and by_kind["fallback"][0] == OK
    for kind, (st, _, _) in by_kind.items():
        if kind.startswith("p_"):
            assert st == INPUT_SHARE, kind
        elif kind.startswith("pm1_"):
            assert st == OK, kind
    if name == "hist":
        assert by_kind["tamper_stride2"][0] == DECRYPT and by_kind["p_proof_last"][0] == INPUT_SHARE
    else:
        assert len([k for k in kinds if k.startswith(("p_", "pm1_"))]) == 8
        assert by_kind["good"][:2] == (OK, b"") and by_kind["good_ext2"][:2] == (OK, EXT2)
        assert by_kind["global_p256"][0] == OK
        assert {by_kind[k][0] for k in ("truncated", "truncated_ext", "empty", "trailing", "unknown_ext", "ext_overrun")} == {PLAINTEXT}
        assert {by_kind[k][0] for k in ("lis_plus1", "lis_minus1")} == {INPUT_SHARE}
        assert by_kind["unknown_config"][0] == UNKNOWN and by_kind["both_fail"][0] == by_kind["wrong_enc_len"][0] == DECRYPT
    n, lis = len(reports), v.leader_input_share_len
    nonces = np.frombuffer(b"".join(r.metadata.report_id for r in reports), np.uint8).reshape(n, 16)
    ps = np.frombuffer(b"".join(r.public_share for r in reports), np.uint8)
    # what the leader would prepare from the plaintext shares (zeros for the rejected ones), host path
    plain = np.zeros((n, lis), np.uint8)
    for i, (st, _, payload) in enumerate(want):
        if st == OK:
            plain[i] = np.frombuffer(payload, np.uint8)
    with HelperEngine(v, vk) as eng:
        ref = eng.leader_initialized_batch(nonces, ps, plain)
        eng.release(ref.batch_id)
        for stride in sorted({(lis + 15) // 16 * 16, (lis + 127) // 128 * 128}):
            got = _open(eng, reports, openers, lis_stride=0 if stride == lis else stride)
            assert got.status.tolist() == [w[0] for w in want], (name, stride, kinds)
            assert got.extensions == [w[1] for w in want]
            rows = got.rows.cpu().numpy()
            assert rows.shape == (n, stride) and got.rows.data_ptr() % 16 == 0
            assert rows[:, :lis].tobytes() == plain.tobytes()
            assert not rows[:, lis:].any()
            d_nonces, d_ps = torch.from_numpy(nonces.copy()).cuda(), torch.from_numpy(ps.copy()).cuda()
            d_out = torch.zeros((n, v.prep_share_len), dtype=torch.uint8, device="cuda")
            d_ver = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            bid = eng.leader_init_device(n, d_nonces.data_ptr(), d_ps.data_ptr() if v.public_share_len else None,
                                         got.rows.data_ptr(), d_out.data_ptr(), d_ver.data_ptr(), lis_stride=got.lis_stride)
            eng.sync()
            ver = d_ver.cpu().numpy()
            assert ver.tolist() == ref.verdicts.tolist()
            ok = ver == 0
            assert ok.sum() >= sum(w[0] == OK for w in want) >= 4 and d_out.cpu().numpy()[ok].tobytes() == ref.prep_shares[ok].tobytes()
            eng.release(bid)


def test_host_buffer_call(openers):
    """jx_leader_upload_open_batch (host buffers, rows of LIS bytes) gives the same as the device call."""
    import ctypes

    v = INSTANCES["mp"]
    kinds, reports, shares, vk = _sealed("mp")
    want = [_ref_upload(v, r) for r in reports]
    n, lis = len(reports), v.leader_input_share_len
    keypairs = [openers[id(k)] for k in (TASK_KEY, GLOBAL_SAME, GLOBAL_P256)]
    ki = np.zeros((n, 2), np.uint8)
    for i, r in enumerate(reports):
        ki[i] = {1: (0, 1), 2: (2, 0xFF)}.get(r.leader_encrypted_input_share.config_id, (0xFF, 0xFF))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u64p = ctypes.POINTER(ctypes.c_uint64)
    ids = np.frombuffer(b"".join(r.metadata.report_id for r in reports), np.uint8).copy()
    ps = np.frombuffer(b"".join(r.public_share for r in reports), np.uint8).copy()
    times = np.array([r.metadata.time for r in reports], np.uint64)
    encs = [r.leader_encrypted_input_share.encapsulated_key for r in reports]
    cts = [r.leader_encrypted_input_share.payload for r in reports]
    pad = 7  # the call reads payloads and encapsulated keys at the caller's offsets, not from 0
    en = np.frombuffer(bytes(pad) + b"".join(encs), np.uint8).copy()
    eoff = (pad + np.concatenate([[0], np.cumsum([len(x) for x in encs])])).astype(np.uint64)
    ct = np.frombuffer(bytes(pad) + b"".join(cts), np.uint8).copy()
    off = (pad + np.concatenate([[0], np.cumsum([len(x) for x in cts])])).astype(np.uint64)
    task = np.frombuffer(TASK, np.uint8).copy()
    out_rows = np.full((n, lis), 0xA5, np.uint8)
    out_ext = np.full(ct.size, 0xA5, np.uint8)
    out_len = np.full(n, 99, np.uint32)
    out_st = np.full(n, 99, np.uint8)
    hs = (ctypes.c_void_p * 3)(*[k.handle for k in keypairs])
    with HelperEngine(v, vk) as eng:
        st = eng._L.jx_leader_upload_open_batch(eng.handle, n, p(ids), times.ctypes.data_as(u64p), p(ps), p(task), hs, 3,
                                                p(ki), p(en), eoff.ctypes.data_as(u64p), p(ct), off.ctypes.data_as(u64p),
                                                p(out_rows), p(out_ext), out_len.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                p(out_st))
        assert st == 0, eng._L.jx_last_error(eng.handle)
    assert out_st.tolist() == [w[0] for w in want]
    for i, (s, ext, payload) in enumerate(want):
        assert out_rows[i].tobytes() == (payload if s == OK else bytes(lis)), kinds[i]
        assert out_len[i] == len(ext) and out_ext[int(off[i]):int(off[i]) + len(ext)].tobytes() == ext


def test_handle_upload_end_to_end(openers):
    """aggregator.handle_upload on the encoded Reports: the records and rejections of the restated loop, with the
    time checks and a public share of the wrong length in front of it."""
    v = INSTANCES["sum"]
    kinds, reports, shares, vk = _sealed("sum")
    now = 1_700_000_000
    task = UploadTask(TASK, {1: openers[id(TASK_KEY)]}, tolerable_clock_skew=len(reports) - 3, task_expiration=None,
                      report_expiry_age=1000)
    bad_ps = Report(reports[0].metadata, reports[0].public_share + b"\0", reports[0].leader_encrypted_input_share,
                    reports[0].helper_encrypted_input_share)
    old = Report(ReportMetadata(b"o" * 16, now - 1001), reports[0].public_share, reports[0].leader_encrypted_input_share,
                 reports[0].helper_encrypted_input_share)
    batch = list(reports) + [bad_ps, old]
    with HelperEngine(v, vk) as eng:
        out = handle_upload(eng, task, [r.encode() for r in batch], now,
                            global_keypairs={1: openers[id(GLOBAL_SAME)], 2: openers[id(GLOBAL_P256)]})
        rows = out.rows.cpu().numpy()
    RR = ReportRejectionReason
    reason = {DECRYPT: RR.DecryptFailure, PLAINTEXT: RR.DecodeFailure, INPUT_SHARE: RR.DecodeFailure,
              UNKNOWN: RR.OutdatedHpkeConfig}
    seen = set()
    for i, r in enumerate(batch):
        got = out.results[i]
        md = r.metadata
        if md.time > now + task.tolerable_clock_skew:  # the last two sealed reports
            want = ReportRejection(TASK, md.report_id, md.time, RR.TooEarly)
        elif r is old:
            want = ReportRejection(TASK, md.report_id, md.time, RR.Expired)
        elif r is bad_ps:
            want = ReportRejection(TASK, md.report_id, md.time, RR.DecodeFailure)
        else:
            st, ext, payload = _ref_upload(v, r)
            if st == OK:
                assert isinstance(got, StoredReport), (i, kinds[i], got)
                assert (got.task_id, got.metadata, got.public_share) == (TASK, md, r.public_share)
                assert b"".join(e.encode() for e in got.extensions) == ext
                assert got.helper_encrypted_input_share == r.helper_encrypted_input_share
                assert rows[got.row, :v.leader_input_share_len].tobytes() == payload
                seen.add("stored")
                continue
            want = ReportRejection(TASK, md.report_id, md.time, reason[st],
                                   r.leader_encrypted_input_share.config_id if st == UNKNOWN else None)
        assert got == want, (i, got, want)
        seen.add(want.reason)
    assert seen == {"stored", RR.TooEarly, RR.Expired, RR.DecodeFailure, RR.DecryptFailure, RR.OutdatedHpkeConfig}
    assert out.counters["upload_decrypt_failure"] >= 1 and out.counters["upload_decode_failure"] >= 8
