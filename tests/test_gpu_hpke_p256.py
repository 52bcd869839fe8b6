"""GPU: the HPKE open under DHKEM(P-256, HKDF-SHA256) (KEM 0x0010) with every KDF and AEAD, in the stand-alone batch
open (hpke_open_p256_kernel) and inside helper prepare launches, direct and coalesced (hpke_rows_p256_kernel beside
the X25519 rows kernels), with both KEMs in one wave.

Expectations come from the RFC 9180 vectors the reference ships (tests/golden/hpke_rfc9180_p256.json) and from
tests/hpke_p256_ref.py, which those vectors pin (tests/test_hpke_p256_ref.py); the prepare results from the C
oracle. HKDF-SHA384 has no vector offline: its suites are checked against the Python reference alone."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import hpke_p256_ref as R
import hpke_suites_ref as S
import test_gpu_encrypted as E
import test_gpu_hpke_suites as T
from janus_amd import hpke
from janus_amd.engine import HelperEngine, _ptr, _u8
from janus_amd.messages import (HpkeCiphertext, PingPongMessage, PlaintextInputShare, PrepareError, PrepareInit,
                                PrepareResp, PrepareStepResult, ReportMetadata, ReportShare)
from oracle import hpke_oracle as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hpke_rfc9180_p256.json")
INFO = H.dap_info()
P256 = hpke.KEM_P256_HKDF_SHA256
X25519 = hpke.KEM_X25519_HKDF_SHA256


def _scalar(rnd) -> bytes:
    return rnd.randrange(1, R.N).to_bytes(32, "big")


def test_rfc9180_vectors_on_gpu():
    vectors = json.load(open(GOLDEN))["vectors"]
    assert len(vectors) == 6
    for v in vectors:
        kdf, aead = v["kdf_id"], v["aead_id"]
        sk, pk, info, enc = (bytes.fromhex(v[k]) for k in ("skRm", "pkRm", "info", "enc"))
        e = v["encryptions"][0]
        ct, aad = bytes.fromhex(e["ct"]), bytes.fromhex(e["aad"])
        with hpke.HpkeOpener(sk, pk, info, kem_id=P256, kdf_id=kdf, aead_id=aead) as op:
            assert op.suite == (P256, kdf, aead) and op.enc_len == 65
            out = op.open_batch([enc], [ct], [aad])
        assert out[0] is not None and out[0].hex() == e["pt"], (kdf, aead)
        # the suite id binds: the same key under another suite opens nothing
        other = (1, 1) if (kdf, aead) != (1, 1) else (3, 3)
        with hpke.HpkeOpener(sk, pk, info, kem_id=P256, kdf_id=other[0], aead_id=other[1]) as op:
            assert op.open_batch([enc], [ct], [aad]) == [None]


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_batch_vs_reference(kdf, aead):
    """One full wave plus six lanes: the payload and associated-data lengths of the X25519 suites' test, and every
    failure the helper maps to HpkeDecryptError, an encapsulated key that is no point among them. Exactly the
    reference's output; half of the rows stay valid."""
    rnd = random.Random(2560 + 10 * kdf + aead)
    sk = _scalar(rnd)
    pk = R.public_key(sk)
    task = rnd.randbytes(32)
    n = 70
    encs, cts, aads, want = [], [], [], []
    for i in range(n):
        kind = i % 10
        alen = 92 if kind % 2 else T.AAD_LENS[(i // 2) % 5]  # the failing kinds are the odd ones
        aad = hpke.input_share_aad(task, rnd.randbytes(16), 1_700_000_000 + i, rnd.randbytes(32))[:alen]
        pt = rnd.randbytes(T.PAYLOAD_LENS[i % len(T.PAYLOAD_LENS)])
        enc, ct = R.seal_base(kdf, aead, pk, INFO, aad, pt, _scalar(rnd))
        if kind == 3:  # flipped ciphertext (or tag) bit
            ct = bytearray(ct)
            ct[rnd.randrange(len(ct))] ^= 1 << rnd.randrange(8)
            ct = bytes(ct)
        elif kind == 5:  # wrong associated data
            aad = aad[:-1] + bytes([aad[-1] ^ 0x80])
        elif kind == 7:  # an encapsulated key off the curve: one bit of x or y flipped
            enc = bytearray(enc)
            enc[1 + rnd.randrange(64)] ^= 1 << rnd.randrange(8)
            enc = bytes(enc)
            assert R.decode(enc) is None
        elif kind == 9:  # shorter than a tag
            ct = ct[:15]
        elif kind == 1:  # an encapsulated key of 64 or 66 bytes
            enc = enc[:64] if i % 20 == 1 else enc + b"\0"
        encs.append(enc)
        cts.append(ct)
        aads.append(aad)
        want.append(R.open_base(kdf, aead, sk, pk, INFO, enc, aad, ct) if len(ct) >= 16 else None)
    with hpke.HpkeOpener(sk, pk, INFO, kem_id=P256, kdf_id=kdf, aead_id=aead) as op:
        got = op.open_batch(encs, cts, aads)
    assert got == want
    assert sum(x is not None for x in got) == n // 2


def test_exceptional_scalars_on_device():
    """Recipient keys sk = 1, n - 1 and 2^128 (pk = G, -G and a scalar with 127 leading zero bits and one set bit):
    the complete formulas take them like any other; eight rows each, all open."""
    rnd = random.Random(1)
    for k in (1, R.N - 1, 2**128):
        sk = k.to_bytes(32, "big")
        pk = R.public_key(sk)
        encs, cts, aads, want = [], [], [], []
        for i in range(8):
            aad, pt = rnd.randbytes(92), rnd.randbytes(40 + i)
            enc, ct = R.seal_base(1, 1, pk, INFO, aad, pt, _scalar(rnd))
            encs.append(enc), cts.append(ct), aads.append(aad), want.append(pt)
        assert [R.open_base(1, 1, sk, pk, INFO, e, a, c) for e, a, c in zip(encs, aads, cts)] == want
        with hpke.HpkeOpener(sk, pk, INFO, kem_id=P256) as op:
            assert op.open_batch(encs, cts, aads) == want, hex(k)


def test_create_key_refusals_and_x25519_through_create_key():
    rnd = random.Random(3)
    sk = _scalar(rnd)
    pk = R.public_key(sk)
    with pytest.raises(ValueError, match="base point"):
        hpke.HpkeOpener(sk, R.public_key(_scalar(rnd)), INFO, kem_id=P256)
    with pytest.raises(ValueError, match=r"\[1, n - 1\]"):
        hpke.HpkeOpener(R.N.to_bytes(32, "big"), pk, INFO, kem_id=P256)
    # the 32-byte entry keeps refusing the id (its keys cannot be P-256 ones)
    with pytest.raises(hpke.UnsupportedSuite):
        hpke.HpkeOpener(bytes(32), bytes(32), INFO, kem_id=P256)
    # an X25519 keypair through jx_hpke_create_key is the context jx_hpke_create_suite makes
    L = hpke._declare(hpke._lib.load())
    xsk = rnd.randbytes(32)
    xpk = H.x25519_base(xsk)
    aad, pt = rnd.randbytes(92), rnd.randbytes(33)
    enc, ct = S.seal_base(2, 3, xpk, INFO, aad, pt, rnd.randbytes(32))
    h = ctypes.c_void_p()
    assert L.jx_hpke_create_key(X25519, 2, 3, xsk, 32, xpk, 32, INFO, len(INFO), 0, ctypes.byref(h)) == 0
    try:
        assert L.jx_hpke_enc_len(h) == 32
        ok, out = ctypes.create_string_buffer(1), ctypes.create_string_buffer(len(pt))
        co, ao = (ctypes.c_uint64 * 2)(0, len(ct)), (ctypes.c_uint64 * 2)(0, len(aad))
        assert L.jx_hpke_open_batch(h, 1, enc, ct, co, aad, ao, out, ok) == 0
        assert ok.raw == b"\x01" and out.raw == pt
    finally:
        L.jx_hpke_destroy(h)


# ---------------------------------------------------------------------------- sealed prepare, KEMs mixed

V = T.V
N_JOB = T.N_JOB
KINDS = ["task_key", "global_key", "tampered", "unknown_cfg", "other_kem_len", "off_curve"]


class Key:
    """A recipient keypair of either KEM with the interface of test_gpu_hpke_suites.Key."""

    def __init__(self, rnd, kem, suite):
        self.kem = kem
        self.kdf, self.aead = suite
        if kem == P256:
            self.sk = _scalar(rnd)
            self.pk = R.public_key(self.sk)
        else:
            self.sk = rnd.randbytes(32)
            self.pk = H.x25519_base(self.sk)

    def opener(self):
        return hpke.HpkeOpener(self.sk, self.pk, INFO, kem_id=self.kem, kdf_id=self.kdf, aead_id=self.aead)

    def seal(self, aad, pt, rnd):
        if self.kem == P256:
            return R.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, _scalar(rnd))
        return S.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, rnd.randbytes(32))

    def open(self, enc, aad, ct):
        """hpke::open: an encapsulated key of another length than the KEM's does not deserialise."""
        if self.kem == P256:
            return R.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 65 else None
        return S.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 32 else None


def _task(k: int, reports, task_key: Key, global_key: Key, stray: dict):
    """One task's 24-report job under config id 10 + k, four rows of each kind, with the reference's responses: the
    Python references open (the task's key, then the global one), the C oracle prepares. stray: a keypair of each
    KEM that no aggregator holds (the other_kem_len rows are sealed to the one whose KEM is NOT the task key's)."""
    vk, task_id, nonces, ps, his, lps = reports
    rnd = random.Random(5000 + k)
    cfg = 10 + k
    inits = []
    for i in range(N_JOB):
        kind = KINDS[i % 6]
        md = ReportMetadata(nonces[i].tobytes(), 1_700_000_000 + i)
        pt = PlaintextInputShare((), his[i].tobytes()).encode()
        aad = E._aad(task_id, md.report_id, md.time, ps[i].tobytes())
        if kind in ("global_key", "off_curve"):
            to = global_key
        elif kind == "other_kem_len":
            to = stray[X25519 if task_key.kem == P256 else P256]
        else:
            to = task_key
        enc, ct = to.seal(aad, pt, rnd)
        if kind == "tampered":
            ct = bytearray(ct)
            ct[rnd.randrange(len(ct))] ^= 1 << rnd.randrange(8)
            ct = bytes(ct)
        elif kind == "off_curve":
            assert len(enc) == 65
            enc = enc[:64] + bytes([enc[64] ^ (1 << (i % 8))])
            assert R.decode(enc) is None
        elif kind == "other_kem_len":
            assert len(enc) == (32 if task_key.kem == P256 else 65)
        inits.append(PrepareInit(ReportShare(md, ps[i].tobytes(), HpkeCiphertext(99 if kind == "unknown_cfg" else cfg, enc, ct)),
                                 PingPongMessage.initialize(lps[i].tobytes())))
    # the reference's loop (aggregator.rs:1781-1832)
    res: list = [None] * N_JOB
    ok_rows = []
    for i, pi in enumerate(inits):
        c = pi.report_share.encrypted_input_share
        if c.config_id != cfg:
            res[i] = PrepareStepResult(2, error=PrepareError.HpkeUnknownConfigId)
            continue
        aad = E._aad(task_id, pi.report_share.metadata.report_id, pi.report_share.metadata.time, pi.report_share.public_share)
        pt = task_key.open(c.encapsulated_key, aad, c.payload)
        if pt is None:
            pt = global_key.open(c.encapsulated_key, aad, c.payload)
        if pt is None:
            res[i] = PrepareStepResult(2, error=PrepareError.HpkeDecryptError)
            continue
        dec = E._decode_plaintext(pt)
        assert dec is not None and dec[0] == [] and dec[1] == his[i].tobytes()
        ok_rows.append(i)
    assert [KINDS[i % 6] for i in ok_rows] == ["task_key", "global_key"] * (N_JOB // 6)
    orc = T._orc()
    want = orc.helper_prep_batch(vk, nonces[ok_rows], ps[ok_rows], his[ok_rows], lps[ok_rows], nthreads=4,
                                 want_out_shares=True)
    assert not want["verdicts"].any()
    for j, i in enumerate(ok_rows):
        res[i] = PrepareStepResult(0, message=PingPongMessage.finish(want["prep_msgs"][j].tobytes()[: V.prep_msg_len]))
    checksum = bytes(32)
    for i in ok_rows:
        checksum = bytes(a ^ b for a, b in zip(checksum, hashlib.sha256(nonces[i].tobytes()).digest()))
    return {"vk": vk, "task_id": task_id, "cfg": cfg, "key": task_key, "global": global_key, "inits": inits,
            "want": [PrepareResp(inits[i].report_share.metadata.report_id, res[i]) for i in range(N_JOB)],
            "agg": orc.aggregate([want["out_shares"][j].tobytes() for j in range(len(ok_rows))]),
            "count": len(ok_rows), "checksum": checksum}


@pytest.fixture(scope="module")
def tasks():
    """Four tasks: P-256 task keys of suites (1,1) and (3,3), the X25519 default suite, X25519 (2,2); a P-256 global
    keypair of suite (1,2). 96 rows with both KEMs in every wave once coalesced."""
    rnd = random.Random(161803)
    reports = [T._reports(k) for k in range(4)]
    glob = Key(rnd, P256, (1, 2))
    stray = {P256: Key(rnd, P256, (1, 1)), X25519: Key(rnd, X25519, (1, 1))}
    keys = [Key(rnd, P256, (1, 1)), Key(rnd, P256, (3, 3)), Key(rnd, X25519, (1, 1)), Key(rnd, X25519, (2, 2))]
    return [_task(k, reports[k], keys[k], glob, stray) for k in range(4)]


def _check(tasks, results):
    for k, (t, (resps, agg, count, checksum)) in enumerate(zip(tasks, results)):
        assert resps == t["want"], f"task {k}"
        assert count == t["count"] == N_JOB // 3 and agg == t["agg"] and checksum == t["checksum"], f"task {k}"


@pytest.mark.parametrize("coalesced", [False, True], ids=["direct", "coalesced"])
def test_sealed_prepare_mixed_kems(tasks, coalesced):
    """Every PrepareResp of the four jobs equals the restated reference loop; coalesced, the four jobs share ONE
    launch, in which the X25519 rows kernel and the P-256 rows kernel each take their rows."""
    results, delta = T._run(tasks, coalesced=coalesced)
    _check(tasks, results)
    if coalesced:
        assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 4}


def _marshal(sel):
    return (np.frombuffer(b"".join(p.report_share.metadata.report_id for p in sel), np.uint8).reshape(-1, 16),
            [p.report_share.metadata.time for p in sel],
            np.frombuffer(b"".join(p.report_share.public_share for p in sel), np.uint8),
            [p.report_share.encrypted_input_share.payload for p in sel],
            np.frombuffer(b"".join(p.message.prep_share for p in sel), np.uint8))


def _old_entry(eng, nonces, times, ps, task_id, keypairs, key_index, encs32, payloads, lps):
    """jx_helper_prep_encrypted_batch itself (n x 32 encapsulated keys), as HelperEngine called it before
    jx_helper_prep_encrypted_batch2 existed."""
    n = len(payloads)
    nn, psa, lpa = _u8(nonces, n, 16, "n"), _u8(ps, n, eng.public_share_len, "ps"), _u8(lps, n, eng.prep_share_len, "lps")
    tm = np.ascontiguousarray(np.asarray(times, dtype=np.uint64))
    ki = np.ascontiguousarray(np.asarray(key_index, dtype=np.uint8).reshape(n, 2))
    en = _u8(encs32, n, 32, "encs")
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in payloads])
    ct = np.frombuffer(b"".join(payloads), np.uint8).copy()
    task = np.frombuffer(task_id, np.uint8).copy()
    hs = (ctypes.c_void_p * len(keypairs))(*[k.handle for k in keypairs])
    verdicts, status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    msgs = np.zeros((n, max(eng.prep_msg_len, 1)), np.uint8)
    bid = ctypes.c_uint64()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    st = eng._L.jx_helper_prep_encrypted_batch(eng._h, n, _ptr(nn), tm.ctypes.data_as(u64p), _ptr(psa), _ptr(task), hs,
                                               len(keypairs), _ptr(ki), _ptr(en), _ptr(ct), off.ctypes.data_as(u64p), 0,
                                               _ptr(lpa), _ptr(msgs), _ptr(verdicts), _ptr(status), ctypes.byref(bid))
    assert st == 0
    eng.release(bid.value)
    return verdicts, msgs[:, : eng.prep_msg_len], status


def test_all_x25519_job_new_entry_equals_old_entry(tasks):
    """Task 3's rows whose encapsulated keys are 32 bytes (task key X25519 (2,2), then an X25519 fallback), through
    jx_helper_prep_encrypted_batch2 with offsets and through the old entry: byte-identical verdicts, prep messages
    and open statuses. Then a P-256 context handed to the old entry: simply a failed trial."""
    t = tasks[3]
    sel = [p for p in t["inits"] if len(p.report_share.encrypted_input_share.encapsulated_key) == 32]
    assert len(sel) == 12
    key_index = np.array([(0xFF, 0xFF) if p.report_share.encrypted_input_share.config_id != t["cfg"] else (0, 1)
                          for p in sel], np.uint8)
    nonces, times, ps, payloads, lps = _marshal(sel)
    encs = [p.report_share.encrypted_input_share.encapsulated_key for p in sel]
    rnd = random.Random(9)
    fallback = Key(rnd, X25519, (1, 1))
    with t["key"].opener() as ot, fallback.opener() as of, t["global"].opener() as og, HelperEngine(V, t["vk"]) as eng:
        new = eng.helper_initialized_encrypted_batch(nonces, times, ps, t["task_id"], [ot, of], key_index, encs, payloads,
                                                     lps, keep=False)
        old = _old_entry(eng, nonces, times, ps, t["task_id"], [ot, of], key_index,
                         np.frombuffer(b"".join(encs), np.uint8).reshape(-1, 32), payloads, lps)
        assert new.verdicts.tobytes() == old[0].tobytes()
        assert new.prep_msgs.tobytes() == old[1].tobytes()
        assert new.open_status.tobytes() == old[2].tobytes()
        assert sorted(set(new.open_status.tolist())) == [0, 1, 7] and (new.open_status == 0).sum() == 4
        # the P-256 global key as the fallback of the old entry: the trial fails, nothing else changes
        old_p = _old_entry(eng, nonces, times, ps, t["task_id"], [ot, og], key_index,
                           np.frombuffer(b"".join(encs), np.uint8).reshape(-1, 32), payloads, lps)
        assert [x.tobytes() for x in old_p] == [x.tobytes() for x in old]
        # and alone: every row with a known config id is a decrypt error
        only_p = _old_entry(eng, nonces, times, ps, t["task_id"], [og, og], key_index,
                            np.frombuffer(b"".join(encs), np.uint8).reshape(-1, 32), payloads, lps)
        assert only_p[2].tolist() == [7 if k == 0xFF else 1 for k in key_index[:, 0]]
