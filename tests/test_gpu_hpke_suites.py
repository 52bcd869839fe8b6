"""GPU: the HPKE open under every X25519 suite Janus accepts (KEM 0x0020; KDF HKDF-SHA256 / -SHA384 / -SHA512;
AEAD AES-128-GCM / AES-256-GCM / ChaCha20Poly1305), in the stand-alone batch open (hpke_open_suite_kernel) and
inside helper prepare launches, direct and coalesced (hpke_rows_suite_kernel), with several suites in one wave.

Expectations come from the RFC 9180 vectors the reference ships (tests/golden/hpke_rfc9180_suites.json) and from
tests/hpke_suites_ref.py, which those vectors pin (tests/test_hpke_suites_ref.py); the prepare results from the C
oracle. HKDF-SHA384 has no vector offline: its suites are checked against the Python reference alone."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import random
import threading

import numpy as np
import pytest

import hpke_suites_ref as S
import test_gpu_encrypted as E
from janus_amd import hpke
from janus_amd.aggregator import handle_aggregate_init_encrypted
from janus_amd.engine import HelperEngine
from janus_amd.messages import (HpkeCiphertext, PingPongMessage, PlaintextInputShare, PrepareError, PrepareInit,
                                PrepareResp, PrepareStepResult, ReportMetadata, ReportShare)
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hpke_rfc9180_suites.json")
INFO = H.dap_info()


def test_rfc9180_vectors_on_gpu():
    vectors = json.load(open(GOLDEN))["vectors"]
    assert len(vectors) == 6
    for v in vectors:
        kdf, aead = v["kdf_id"], v["aead_id"]
        sk, pk, info, enc = (bytes.fromhex(v[k]) for k in ("skRm", "pkRm", "info", "enc"))
        e = v["encryptions"][0]
        ct, aad = bytes.fromhex(e["ct"]), bytes.fromhex(e["aad"])
        with hpke.HpkeOpener(sk, pk, info, kdf_id=kdf, aead_id=aead) as op:
            assert op.suite == (hpke.KEM_X25519_HKDF_SHA256, kdf, aead)
            out = op.open_batch([enc], [ct], [aad])
        assert out[0] is not None and out[0].hex() == e["pt"], (kdf, aead)
        # the suite id binds: the same key under another suite (the default one, unless this is it) opens nothing
        other = (1, 1) if (kdf, aead) != (1, 1) else (3, 3)
        with hpke.HpkeOpener(sk, pk, info, kdf_id=other[0], aead_id=other[1]) as op:
            assert op.open_batch([enc], [ct], [aad]) == [None]


PAYLOAD_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
AAD_LENS = [92, 0, 1, 16, 17]


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_batch_vs_reference(kdf, aead):
    """One full wave plus six lanes: every payload length around the AES and ChaCha20 block sizes, DAP-shaped and
    short associated data, and every failure the helper maps to HpkeDecryptError. Exactly the reference's output;
    half of the rows stay valid."""
    rnd = random.Random(9180 + 10 * kdf + aead)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    task = rnd.randbytes(32)
    n = 70
    encs, cts, aads, want = [], [], [], []
    for i in range(n):
        kind = i % 10
        alen = 92 if kind % 2 else AAD_LENS[(i // 2) % 5]  # the failing kinds are the odd ones
        aad = hpke.input_share_aad(task, rnd.randbytes(16), 1_700_000_000 + i, rnd.randbytes(32))
        assert len(aad) == 92
        aad = aad[:alen]
        pt = rnd.randbytes(PAYLOAD_LENS[i % len(PAYLOAD_LENS)])
        enc, ct = S.seal_base(kdf, aead, pk, INFO, aad, pt, rnd.randbytes(32))
        if kind == 3:  # flipped ciphertext (or tag) bit
            ct = bytearray(ct)
            ct[rnd.randrange(len(ct))] ^= 1 << rnd.randrange(8)
            ct = bytes(ct)
        elif kind == 5:  # wrong associated data
            aad = aad[:-1] + bytes([aad[-1] ^ 0x80])
        elif kind == 7:  # a low-order point: all-zero DH
            enc = bytes(32)
        elif kind == 9:  # shorter than a tag
            ct = ct[:15]
        elif kind == 1:  # an encapsulated key of 31 or 33 bytes
            enc = enc[:31] if i % 20 == 1 else enc + b"\0"
        encs.append(enc)
        cts.append(ct)
        aads.append(aad)
        want.append(S.open_base(kdf, aead, sk, pk, INFO, enc, aad, ct) if len(ct) >= 16 and len(enc) == 32 else None)
    with hpke.HpkeOpener(sk, pk, INFO, kdf_id=kdf, aead_id=aead) as op:
        got = op.open_batch(encs, cts, aads)
    assert got == want
    assert sum(x is not None for x in got) == n // 2


def test_unsupported_ids():
    L = hpke._declare(hpke._lib.load())
    key = (ctypes.c_uint8 * 32)()
    for kem, kdf, aead in ((0x0010, 1, 1), (0x0020, 4, 1), (0x0020, 1, 4)):
        h = ctypes.c_void_p()
        assert L.jx_hpke_create_suite(kem, kdf, aead, key, key, None, 0, 0, ctypes.byref(h)) == hpke.E_UNSUPPORTED
        assert not h.value and b"unsupported HPKE suite" in L.jx_hpke_last_error(None)
        with pytest.raises(hpke.UnsupportedSuite):
            hpke.HpkeOpener(bytes(32), bytes(32), INFO, kem_id=kem, kdf_id=kdf, aead_id=aead)


# ---------------------------------------------------------------------------- sealed prepare, suites mixed

V = Prio3.sum_vec(8, 12, 4)
N_JOB = 24
KINDS = ["task_key", "global_key", "tampered", "unknown_cfg"]


class Key:
    def __init__(self, rnd, suite):
        self.sk = rnd.randbytes(32)
        self.pk = H.x25519_base(self.sk)
        self.kdf, self.aead = suite

    def opener(self):
        return hpke.HpkeOpener(self.sk, self.pk, INFO, kdf_id=self.kdf, aead_id=self.aead)

    def seal(self, aad, pt, ske):
        return S.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, ske)

    def open(self, enc, aad, ct):
        return S.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct)


def _orc():
    return O.Prio3Oracle(V.algo_id, V.bits, V.length, V.chunk_length)


def _reports(k: int):
    """Task k's client reports (the C oracle's), made once: (vk, task id, nonces, ps, his, lps)."""
    rng = np.random.default_rng(900 + k)
    orc = _orc()
    vk = bytes((53 * k + i) % 256 for i in range(16))
    task_id = random.Random(70 + k).randbytes(32)
    meas = rng.integers(0, 1 << V.bits, size=(N_JOB, V.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(N_JOB, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(N_JOB, orc.sizes.client_rand), dtype=np.uint8)
    ps, his, lps, _ = orc.client_leader_batch(vk, meas, nonces, rands, nthreads=4)
    assert ps.shape[1] == 32
    return vk, task_id, nonces, ps, his, lps


def _task(k: int, reports, task_key: Key, global_key: Key):
    """One task's 24-report job under config id 10 + k, six rows of each kind, with the reference's responses:
    tests/hpke_suites_ref.py opens (the task's key, then the global one), the C oracle prepares."""
    vk, task_id, nonces, ps, his, lps = reports
    rnd = random.Random(4000 + k)
    cfg = 10 + k
    inits = []
    for i in range(N_JOB):
        kind = KINDS[i % 4]
        md = ReportMetadata(nonces[i].tobytes(), 1_700_000_000 + i)
        pt = PlaintextInputShare((), his[i].tobytes()).encode()
        aad = E._aad(task_id, md.report_id, md.time, ps[i].tobytes())
        enc, ct = (global_key if kind == "global_key" else task_key).seal(aad, pt, rnd.randbytes(32))
        if kind == "tampered":
            ct = bytearray(ct)
            ct[rnd.randrange(len(ct))] ^= 1 << rnd.randrange(8)
            ct = bytes(ct)
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
    assert [KINDS[i % 4] for i in ok_rows] == ["task_key", "global_key"] * (N_JOB // 4)
    orc = _orc()
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


def _run(tasks, coalesced: bool):
    """Every task's job on an engine of its own: coalesced, the four jobs in ONE launch (debug option 7); else four
    direct calls. Returns per task (responses, aggregate, count, checksum) and the launch / job counters' deltas."""
    openers = [t["key"].opener() for t in tasks]
    glob = tasks[0]["global"].opener()  # one global keypair, registered under every task's config id
    engs = [HelperEngine(V, t["vk"]) for t in tasks]
    warm = HelperEngine(V, tasks[0]["vk"]) if coalesced else None
    out: list = [None] * len(tasks)
    errs = []
    try:
        delta = None
        if coalesced:
            for e in engs + [warm]:
                e.coalesce(True, window_us=1_000_000)
            # a first encrypted job (on an engine of its own, so that the tasks' aggregates hold their jobs alone):
            # from then on the coalescer's helper lanes carry the encrypted-input regions
            handle_aggregate_init_encrypted(warm, openers[0], tasks[0]["cfg"], tasks[0]["task_id"], tasks[0]["inits"][:4],
                                            global_keypairs={tasks[0]["cfg"]: glob})
            engs[0].debug(7, len(tasks))
            m0 = engs[0].memory()

        def job(k):
            try:
                t = tasks[k]
                out[k] = handle_aggregate_init_encrypted(engs[k], openers[k], t["cfg"], t["task_id"], t["inits"],
                                                         global_keypairs={t["cfg"]: glob})
            except BaseException as e:  # noqa: BLE001 - re-raised below
                errs.append(e)

        if coalesced:
            th = [threading.Thread(target=job, args=(k,)) for k in range(len(tasks))]
            for x in th:
                x.start()
            for x in th:
                x.join()
            m1 = engs[0].memory()
            delta = {k: m1[k] - m0[k] for k in ("coalesced_helper_launches", "coalesced_encrypted_jobs")}
            engs[0].debug(7, 0)
        else:
            for k in range(len(tasks)):
                job(k)
        if errs:
            raise errs[0]
        shares = [e.aggregate_share(0) for e in engs]
        return [(out[k].responses,) + tuple(shares[k]) for k in range(len(tasks))], delta
    finally:
        for e in engs + ([warm] if warm else []):
            e.close()
        for o in openers + [glob]:
            o.close()


@pytest.fixture(scope="module")
def reports():
    return [_reports(k) for k in range(4)]


def _check(tasks, results):
    for k, (t, (resps, agg, count, checksum)) in enumerate(zip(tasks, results)):
        assert resps == t["want"], f"task {k}"
        assert count == t["count"] == N_JOB // 2 and agg == t["agg"] and checksum == t["checksum"], f"task {k}"


def test_mixed_suites_in_one_coalesced_launch(reports):
    """Four tasks with keys of suites (1,1), (3,3), (2,2) and (1,3) and a global key of suite (3,2): 96 rows in one
    launch, several suites in each wave, and a fallback trial that changes suite within a lane."""
    rnd = random.Random(31337)
    suites = [(1, 1), (3, 3), (2, 2), (1, 3)]
    glob = Key(rnd, (3, 2))
    tasks = [_task(k, reports[k], Key(rnd, suites[k]), glob) for k in range(4)]
    results, delta = _run(tasks, coalesced=True)
    _check(tasks, results)
    assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 4}
    # the same jobs without coalescing: the direct path's suite kernel
    direct, _ = _run(tasks, coalesced=False)
    _check(tasks, direct)


def test_default_path_is_not_contaminated(reports):
    """All five keys of the default suite: the coalesced launch (hpke_rows_kernel) equals four direct calls. Then one
    task's key at (3,3): every row goes through hpke_rows_suite_kernel, and the three default jobs' outputs are
    what they were."""
    rnd = random.Random(2718)
    glob = Key(rnd, (1, 1))
    keys = [Key(rnd, (1, 1)) for _ in range(4)]
    tasks = [_task(k, reports[k], keys[k], glob) for k in range(4)]
    direct, _ = _run(tasks, coalesced=False)
    _check(tasks, direct)
    all_default, delta = _run(tasks, coalesced=True)
    assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 4}
    _check(tasks, all_default)
    assert all_default == direct
    # task 1 under (3,3); tasks 0, 2 and 3 unchanged (the same PrepareInits)
    mixed_tasks = list(tasks)
    mixed_tasks[1] = _task(1, reports[1], Key(rnd, (3, 3)), glob)
    mixed, delta = _run(mixed_tasks, coalesced=True)
    assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 4}
    _check(mixed_tasks, mixed)
    for k in (0, 2, 3):
        assert mixed[k] == all_default[k]
