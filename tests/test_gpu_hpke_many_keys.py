"""GPU: any number of tasks' HPKE keypairs in one sealed prepare launch. The keys live in the device's key registry
(one row per jx_hpke context from its creation to jx_hpke_destroy, include/jx_hpke.h); the rows of a launch name
registry slots, so a gather never closes for its keys.

Expectations come from the test-side restatement of the reference loop (aggregator/src/aggregator.rs:1781-1832) that
tests/test_gpu_encrypted.py has, reference_responses, sealing with oracle/hpke_oracle.py; where a job holds keys of
other suites or of the P-256 KEM, from the same loop restated over tests/hpke_suites_ref.py and
tests/hpke_p256_ref.py (the Key class of tests/test_gpu_hpke_p256.py). Shapes are tiny: Histogram(40, 5), 6 reports
per job (8 in the one request that carries 8 keypairs).
"""
from __future__ import annotations

import random
import threading

import numpy as np
import pytest

import test_gpu_encrypted as E
import test_gpu_hpke_p256 as P
from janus_amd import hpke
from janus_amd.aggregator import handle_aggregate_init_encrypted
from janus_amd.engine import HelperEngine
from janus_amd.messages import (HpkeCiphertext, PingPongMessage, PlaintextInputShare, PrepareError, PrepareInit,
                                PrepareResp, PrepareStepResult, ReportMetadata, ReportShare)
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

V = Prio3.histogram(40, 5)
INFO = E.INFO
X25519, P256 = P.X25519, P.P256
DEFAULT = (1, 1)  # (HKDF-SHA256, AES-128-GCM)
# one job: valid reports sealed to the task key; one sealed to the global key under config id 2 (the first trial is
# the global key); one sealed to the global key under id 1 (the task trial fails, the global trial opens it); a
# corrupted ciphertext; an unknown config id
KINDS = ["valid", "valid", "global_id2", "global_id1", "corrupt_ct", "unknown_cfg"]
N_JOB = len(KINDS)
WANT_ERRORS = [None, None, None, None, PrepareError.HpkeDecryptError, PrepareError.HpkeUnknownConfigId]


def _orc():
    return O.Prio3Oracle(V.algo_id, V.bits, V.length, V.chunk_length)


def _is_default(k) -> bool:
    return k.kem == X25519 and (k.kdf, k.aead) == DEFAULT


def _reference_any_suite(orc, vk, task_id, keys, inits):
    """E.reference_responses' loop for keypairs of any suite and KEM (Key.open: a key of another length than the
    KEM's does not deserialise); every report here has a well-formed plaintext and leader message."""
    n = len(inits)
    res: list = [None] * n
    rows, payloads = [], []
    for i, pi in enumerate(inits):
        rs = pi.report_share
        ct = rs.encrypted_input_share
        ks = [k for k in keys.get(ct.config_id, []) if k]
        if not ks:
            res[i] = PrepareStepResult(2, error=PrepareError.HpkeUnknownConfigId)
            continue
        aad = E._aad(task_id, rs.metadata.report_id, rs.metadata.time, rs.public_share)
        pt = None
        for k in ks:
            pt = k.open(ct.encapsulated_key, aad, ct.payload) if len(ct.payload) >= 16 else None
            if pt is not None:
                break
        if pt is None:
            res[i] = PrepareStepResult(2, error=PrepareError.HpkeDecryptError)
            continue
        dec = E._decode_plaintext(pt)
        assert dec is not None and dec[0] == [] and len(dec[1]) == V.helper_input_share_len
        rows.append(i)
        payloads.append(dec[1])
    m = len(rows)
    cat = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(m, w)  # noqa: E731
    want = orc.helper_prep_batch(vk, cat([inits[i].report_share.metadata.report_id for i in rows], 16),
                                 cat([inits[i].report_share.public_share for i in rows], V.public_share_len),
                                 cat(payloads, V.helper_input_share_len),
                                 cat([inits[i].message.prep_share for i in rows], V.prep_share_len), nthreads=4)
    for j, i in enumerate(rows):
        if want["verdicts"][j]:
            res[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
        else:
            res[i] = PrepareStepResult(0, message=PingPongMessage.finish(want["prep_msgs"][j].tobytes()[: V.prep_msg_len]))
    return [PrepareResp(inits[i].report_share.metadata.report_id, res[i]) for i in range(n)]


def _task(k: int, key, glob):
    """Task k (its own verify key, task id and keypair `key` under config id 1; the global keypair `glob` under ids
    1 and 2): one 6-report job, one report of each of KINDS, and the reference's PrepareResps."""
    rnd = random.Random(9000 + k)
    rng = np.random.default_rng(9000 + k)
    orc = _orc()
    vk = bytes((29 * k + 7 * i + 1) % 256 for i in range(16))
    task_id = rnd.randbytes(32)
    meas = rng.integers(0, V.length, size=(N_JOB, 1), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(N_JOB, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(N_JOB, orc.sizes.client_rand), dtype=np.uint8)
    ps, his, lps, _ = orc.client_leader_batch(vk, meas, nonces, rands, nthreads=4)
    inits = []
    for i, kind in enumerate(KINDS):
        md = ReportMetadata(nonces[i].tobytes(), 1_700_000_000 + i)
        pt = PlaintextInputShare((), his[i].tobytes()).encode()
        aad = E._aad(task_id, md.report_id, md.time, ps[i].tobytes())
        to = glob if kind.startswith("global") else key
        enc, ct = H.seal_base(to.pk, INFO, aad, pt, rnd.randbytes(32)) if _is_default(to) else to.seal(aad, pt, rnd)
        if kind == "corrupt_ct":
            ct = bytearray(ct)
            ct[rnd.randrange(len(ct))] ^= 1 << rnd.randrange(8)
            ct = bytes(ct)
        cfg = {"global_id2": 2, "unknown_cfg": 9}.get(kind, 1)
        inits.append(PrepareInit(ReportShare(md, ps[i].tobytes(), HpkeCiphertext(cfg, enc, ct)),
                                 PingPongMessage.initialize(lps[i].tobytes())))
    if _is_default(key) and _is_default(glob):
        kt, kg = (key.sk, key.pk), (glob.sk, glob.pk)
        want, _, _ = E.reference_responses(orc, vk, V, task_id, {1: [kt, kg], 2: [None, kg]}, inits)
    else:
        want = _reference_any_suite(orc, vk, task_id, {1: [key, glob], 2: [None, glob]}, inits)
    # the job is what the docstring says: four reports finish, in the reference too
    got = [r.result.error if r.result.kind == 2 else None for r in want]
    assert got == WANT_ERRORS, (k, got)
    return {"vk": vk, "task_id": task_id, "key": key, "inits": inits, "want": want}


@pytest.fixture(scope="module")
def glob():
    return P.Key(random.Random(4), X25519, DEFAULT)


@pytest.fixture(scope="module")
def tasks(glob):
    """40 tasks with default-suite X25519 keypairs, made once and left unchanged."""
    rnd = random.Random(1618)
    return [_task(k, P.Key(rnd, X25519, DEFAULT), glob) for k in range(40)]


def _filler(rnd):
    """A context that only takes a registry slot: no report is sealed to it (an X25519 public key is not checked
    against the private key, and no open uses it)."""
    return hpke.HpkeOpener(rnd.randbytes(32), rnd.randbytes(32), INFO)


def _run_one_launch(jobs, glob_opener):
    """jobs: (task, its opener). Every job on an engine of its own, all of them in ONE coalesced launch (a one-second
    window and debug option 7 hold the gather until every job has joined). Returns the jobs' PrepareResp lists and
    the counters' deltas."""
    n = len(jobs)
    engs = [HelperEngine(V, t["vk"]) for t, _ in jobs]
    warm = HelperEngine(V, jobs[0][0]["vk"])
    out: list = [None] * n
    errs = []
    try:
        for e in engs + [warm]:
            e.coalesce(True, window_us=1_000_000)
        # a first sealed job: from then on the coalescer's helper lanes carry the encrypted-input regions
        t0, o0 = jobs[0]
        first = handle_aggregate_init_encrypted(warm, o0, 1, t0["task_id"], t0["inits"][:2],
                                                global_keypairs={1: glob_opener, 2: glob_opener})
        assert first.responses == t0["want"][:2]
        engs[0].debug(7, n)
        m0 = engs[0].memory()

        def job(k):
            try:
                t, o = jobs[k]
                out[k] = handle_aggregate_init_encrypted(engs[k], o, 1, t["task_id"], t["inits"],
                                                         global_keypairs={1: glob_opener, 2: glob_opener}).responses
            except BaseException as e:  # noqa: BLE001 - re-raised below
                errs.append(e)

        th = [threading.Thread(target=job, args=(k,)) for k in range(n)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        m1 = engs[0].memory()
        engs[0].debug(7, 0)
        if errs:
            raise errs[0]
        return out, {k: m1[k] - m0[k] for k in ("coalesced_helper_launches", "coalesced_encrypted_jobs")}
    finally:
        for e in engs + [warm]:
            e.close()


def _check(jobs, out):
    for k, ((t, _), resps) in enumerate(zip(jobs, out)):
        assert resps == t["want"], f"job {k}"


def test_24_tasks_in_one_launch(tasks, glob):
    """24 tasks' jobs, 25 keypairs, in ONE launch: the 144 rows are contiguous, so the first wave alone holds more
    than 16 distinct keys. (A launch that carried its keys in a 16-row table closed the gather when the 16th task
    joined, and ran two or more launches.)"""
    openers = [t["key"].opener() for t in tasks[:24]]
    g = glob.opener()
    try:
        jobs = list(zip(tasks[:24], openers))
        out, delta = _run_one_launch(jobs, g)
        _check(jobs, out)
        assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 24}
    finally:
        for o in openers + [g]:
            o.close()


def test_mixed_suites_in_one_launch(tasks, glob):
    """The same with 4 of the 24 tasks under P-256 keys (65-byte encapsulated keys) and 4 under (X25519, HKDF-SHA512,
    ChaCha20Poly1305) keys: one launch (the suite kernel and the P-256 kernel), every response the reference's."""
    rnd = random.Random(256512)
    mixed = list(tasks[:24])
    for j, k in enumerate((1, 7, 13, 22)):
        mixed[k] = _task(100 + k, P.Key(rnd, P256, [(1, 1), (3, 3), (2, 2), (1, 2)][j]), glob)
    for k in (2, 8, 17, 23):
        mixed[k] = _task(100 + k, P.Key(rnd, X25519, (3, 3)), glob)
    openers = [t["key"].opener() for t in mixed]
    g = glob.opener()
    try:
        assert sorted(o.enc_len for o in openers) == [32] * 20 + [65] * 4
        jobs = list(zip(mixed, openers))
        out, delta = _run_one_launch(jobs, g)
        _check(jobs, out)
        assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 24}
    finally:
        for o in openers + [g]:
            o.close()


def test_slot_reuse(tasks, glob):
    """40 openers, the even ones closed, 20 more with fresh keys in the freed slots: one job per live opener, in one
    launch. A slot that still held the closed opener's key would answer HpkeDecryptError."""
    rnd = random.Random(40)
    g = glob.opener()
    first = [tasks[j]["key"].opener() if j % 2 else _filler(rnd) for j in range(40)]
    live = {j: first[j] for j in range(1, 40, 2)}
    try:
        for j in range(0, 40, 2):
            first[j].close()
        for j in range(0, 40, 2):
            live[j] = tasks[j]["key"].opener()
        jobs = [(tasks[j], live[j]) for j in range(40)]
        out, delta = _run_one_launch(jobs, g)
        _check(jobs, out)
        assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 40}
    finally:
        for o in list(live.values()) + first + [g]:
            o.close()


def test_slots_above_255(tasks, glob):
    """260 contexts: jobs of the last 20 (slots past one byte) in one launch; then ONE request with 8 of them as
    its keypairs through the direct path, coalescing off."""
    rnd = random.Random(260)
    g = glob.opener()
    fill = [_filler(rnd) for _ in range(239)]  # with the global keypair's, 240 contexts before the tasks'
    openers = [t["key"].opener() for t in tasks[:20]]
    try:
        jobs = list(zip(tasks[:20], openers))
        out, delta = _run_one_launch(jobs, g)
        _check(jobs, out)
        assert delta == {"coalesced_helper_launches": 1, "coalesced_encrypted_jobs": 20}
        # the direct path: report i sealed to tasks[12 + i]'s key. Report 0's is the task's keypair (config id 10), the
        # others' are global keypairs under ids 11..17: 8 keypairs in the request, JX_ENC_MAX_KEYPAIRS
        keys = [tasks[12 + i]["key"] for i in range(8)]
        pair = lambda k: (k.sk, k.pk)  # noqa: E731
        t = tasks[0]
        orc = _orc()
        inits = E._make_inits(random.Random(8), orc, V, t["vk"], t["task_id"], 8, lambda i: "valid",
                              lambda i: pair(keys[i]), lambda i: 10 + i, seed=88)
        ref_keys = {10 + i: [None, pair(keys[i])] for i in range(1, 8)}
        ref_keys[10] = [pair(keys[0]), None]
        want, fin, _ = E.reference_responses(orc, t["vk"], V, t["task_id"], ref_keys, inits)
        assert fin.all()
        with HelperEngine(V, t["vk"]) as eng:
            got = handle_aggregate_init_encrypted(eng, openers[12], 10, t["task_id"], inits,
                                                  global_keypairs={10 + i: openers[12 + i] for i in range(1, 8)})
        assert got.responses == want
    finally:
        for o in openers + fill + [g]:
            o.close()


def test_two_tasks_two_launches_at_nonzero_slots(tasks, glob):
    """The small case the other sealed tests cover, two tasks' jobs one after the other in a launch each, but with
    keypairs whose registry slots are not 0, 1 and 2."""
    rnd = random.Random(5)
    fill = [_filler(rnd) for _ in range(3)]
    g = glob.opener()
    openers = [tasks[k]["key"].opener() for k in (30, 31)]
    engs = [HelperEngine(V, tasks[k]["vk"]) for k in (30, 31)]
    try:
        for e in engs:
            e.coalesce(True)
        m0 = engs[0].memory()
        for k in range(2):
            t = tasks[30 + k]
            got = handle_aggregate_init_encrypted(engs[k], openers[k], 1, t["task_id"], t["inits"],
                                                  global_keypairs={1: g, 2: g})
            assert got.responses == t["want"], f"task {k}"
        m1 = engs[0].memory()
        assert m1["coalesced_helper_launches"] - m0["coalesced_helper_launches"] == 2
        assert m1["coalesced_encrypted_jobs"] - m0["coalesced_encrypted_jobs"] == 2
    finally:
        for e in engs:
            e.close()
        for o in openers + fill + [g]:
            o.close()
