"""GPU: real XOF rejections and exact decode bounds, bit for bit against the C oracle.

The reject_*.json fixtures (tests/golden/make_reject_golden.py) hold reports with a raw Field64 sample
>= p in a known stream at a known index: the fast kernels must notice it, the slow kernels must skip it and
move on, for the helper and the leader, alone, mixed within a wave, a whole wave of them, and through the
coalesced path. tests/test_rejection_fixtures.py checks the fixtures and the references themselves on the
CPU, so a mismatch here is the engine's.

The second half puts every boundary encoding around p into explicit elements (leader input shares, leader
prep shares): an element decodes exactly when it is < p, wherever it sits.

No tolerances anywhere: verdicts, prepare messages, output shares, aggregate shares, counts and checksums are
compared as bytes.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest

from janus_amd.engine import HelperEngine
from janus_amd.vdaf import Prio3
from oracle import oracle as O
from tests.golden import make_reject_golden as MG
from tests.test_gpu_coalesce import _record, _run_threads

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["reject_count", "reject_mp2_1x32_5", "reject_mp2_partial_chunk"]
P128 = 2**128 - 28 * 2**64 + 1
P64 = 2**64 - 2**32 + 1


class Fixture:
    def __init__(self, name):
        self.doc = doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
        v = doc["vdaf"]
        self.vdaf = Prio3(v["algo_id"], v["bits"], v["length"], v["chunk_length"], v["num_proofs"])
        self.orc = O.Prio3Oracle(v["algo_id"], v["bits"], v["length"], v["chunk_length"], v["num_proofs"])
        self.vk = bytes.fromhex(doc["verify_key"])
        reps = doc["reports"]
        self.n = n = len(reps)

        def cat(key, width):
            if not width:
                return np.zeros((n, 0), np.uint8)
            return np.frombuffer(b"".join(bytes.fromhex(r[key]) for r in reps), np.uint8).reshape(n, width).copy()

        s = self.orc.sizes
        self.nonces, self.ps = cat("nonce", 16), cat("public_share", s.public_share)
        self.his, self.lps = cat("helper_input_share", s.helper_input_share), cat("leader_prep_share", s.prep_share)
        # the clients' measurements and randomness, as the generator seeded them (to shard again for the leader)
        cfg, lanes = MG.fixtures()[name]
        _, self.meas, nonces, self.rands = MG.inputs(name, cfg, lanes)
        assert (nonces == self.nonces).all() and self.meas.tolist() == [r["measurement"] for r in reps]
        self.rejecting = [r["report"] for r in doc["rejections"]]
        self.plain = [i for i in range(n) if i not in self.rejecting]


@functools.lru_cache(maxsize=None)
def _fixture(name) -> Fixture:
    return Fixture(name)


def _want(orc, vk, nonces, ps, his, lps):
    return orc.helper_prep_batch(vk, nonces, ps, his, lps, nthreads=8, want_out_shares=True)


def _assert_batch(res, want, what=""):
    """verdicts, prepare messages and output shares of the finished reports == the oracle's."""
    np.testing.assert_array_equal(res.verdicts, want["verdicts"], err_msg=what)
    fin = want["verdicts"] == 0
    np.testing.assert_array_equal(res.prep_msgs[fin], want["prep_msgs"][fin], err_msg=what)
    if res.out_shares is not None:
        np.testing.assert_array_equal(res.out_shares[fin], want["out_shares"][fin], err_msg=what)


# ---------------------------------------------------------------------------- rejections: helper


@pytest.mark.parametrize("name", FIXTURES)
def test_natural_path_finishes_rejecting_reports(name):
    """No debug switch: the fast kernels flag the rejecting reports, the slow kernels redo them, and they end
    with verdict 0 and the oracle's output share, next to honest and tampered reports of the same wave; by
    helper_initialized_batch + accumulate and by the fused prep_and_aggregate."""
    f = _fixture(name)
    want = _want(f.orc, f.vk, f.nonces, f.ps, f.his, f.lps)
    assert want["verdicts"].tolist() == [r["verdict"] for r in f.doc["reports"]]
    record = (bytes.fromhex(f.doc["aggregate_share"]), f.doc["report_count"], bytes.fromhex(f.doc["checksum"]))
    assert (want["agg"], want["count"], want["checksum"]) == record
    with HelperEngine(f.vdaf, f.vk) as eng:
        res = eng.helper_initialized_batch(f.nonces, f.ps, f.his, f.lps, want_out_shares=True)
        _assert_batch(res, want)
        for r in f.doc["rejections"]:
            i = r["report"]
            assert res.verdicts[i] == 0, r
            assert res.out_shares[i].tobytes().hex() == f.doc["reports"][i]["out_share"], r
            assert res.prep_msgs[i].tobytes().hex() == f.doc["reports"][i]["prep_msg"], r
        eng.accumulate(f.n)
        assert eng.aggregate_share(0) == record
    with HelperEngine(f.vdaf, f.vk) as eng:
        verdicts, msgs = eng.prep_and_aggregate(f.nonces, f.ps, f.his, f.lps)
        np.testing.assert_array_equal(verdicts, want["verdicts"])
        fin = want["verdicts"] == 0
        np.testing.assert_array_equal(msgs[fin], want["prep_msgs"][fin])
        assert not verdicts[f.rejecting].any()
        assert eng.aggregate_share(0) == record


@pytest.mark.parametrize("name", FIXTURES)
def test_block_mixes(name):
    """A first 64-report block of rejecting reports only (the slow kernel's every lane works), a second with
    none (the slow kernel's whole wave leaves at once), a third with exactly one, at lane 63. Reports repeat;
    the oracle prepares the same batch."""
    f = _fixture(name)
    rej, plain = f.rejecting, f.plain
    idx = [rej[k % len(rej)] for k in range(64)] + plain[:64] + plain[:63] + [rej[-1]]
    idx = np.array(idx)
    assert len(idx) == 192
    nonces, ps, his, lps = f.nonces[idx], f.ps[idx], f.his[idx], f.lps[idx]
    want = _want(f.orc, f.vk, nonces, ps, his, lps)
    assert not want["verdicts"][:64].any() and want["verdicts"][191] == 0
    assert (want["verdicts"][64:191] != 0).any() and (want["verdicts"][64:191] == 0).any()
    with HelperEngine(f.vdaf, f.vk) as eng:
        res = eng.helper_initialized_batch(nonces, ps, his, lps, want_out_shares=True)
        _assert_batch(res, want)
        eng.accumulate(len(idx))
        assert eng.aggregate_share(0) == (want["agg"], want["count"], want["checksum"])


@pytest.mark.parametrize("name", ["reject_count", "reject_mp2_1x32_5"])
def test_coalesced_jobs_two_tasks(name):
    """100-report jobs from four threads through the coalesced path, two tasks (verify keys) of one VDAF
    sharing launches. The second task holds the same clients' reports prepared under its own key: the
    rejections in the measurement, proof and joint-randomness streams come along (they do not depend on the
    verify key), the query-randomness one does not: it belongs to the first task only."""
    f = _fixture(name)
    P = MG.pyref_of(MG.cfg_of_doc(f.doc))
    vk2 = bytes((x * 7 + 3) % 256 for x in range(len(f.vk)))
    ps2, his2, lps2, _ = f.orc.client_leader_batch(vk2, f.meas, f.nonces, f.rands, nthreads=8)
    np.testing.assert_array_equal(his2, f.his)
    MG.tamper(lps2, f.orc.sizes, set(f.rejecting))
    pools = [(f.vk, f.nonces, f.ps, f.his, f.lps), (vk2, f.nonces, ps2, his2, lps2)]
    wants = [_want(f.orc, *p) for p in pools]
    # what each task's rejecting reports really reject, from the reference XOFs
    listed = {(r["report"], r["stream"], r["raw_index"]) for r in f.doc["rejections"]}
    qlanes = {r["report"] for r in f.doc["rejections"] if r["stream"] == "query_rand"}
    assert qlanes
    seen2 = set()
    for i in f.rejecting:
        rep = dict(f.doc["reports"][i], public_share=ps2[i].tobytes().hex())
        seen2 |= {(i, st, k) for st, k in MG.report_rejections(P, vk2, rep)}
    assert seen2 == {x for x in listed if x[1] != "query_rand"}
    for i in f.rejecting:
        assert wants[0]["verdicts"][i] == 0 and wants[1]["verdicts"][i] == 0

    engs = [HelperEngine(f.vdaf, p[0]) for p in pools]
    try:
        for e in engs:
            e.coalesce(True, window_us=1_000_000)  # the longest the engine takes
        # a gather waits (at most that long) for one job of every thread, so a launch holds both tasks
        engs[0].debug(7, 4)
        m0 = engs[0].memory()
        n, jobs_per_thread, results = 100, 3, {}

        def worker(t):
            k = t % 2
            _, nonces, ps, his, lps = pools[k]
            for j in range(jobs_per_thread):
                idx = (17 * t + 29 * j + np.arange(n)) % f.n
                # (asking for the output shares would take the job off the coalesced path: the records carry them)
                res = engs[k].helper_initialized_batch(nonces[idx], ps[idx], his[idx], lps[idx])
                rec = engs[k].aggregate_records(res.batch_id, n)[0]
                engs[k].release(res.batch_id)
                results[(t, j)] = (k, idx, res, rec)

        _run_threads(worker, 4)
        m1 = engs[0].memory()
        assert len(results) == 4 * jobs_per_thread
        for (t, j), (k, idx, res, rec) in results.items():
            want = wants[k]
            sub = {key: want[key][idx] for key in ("verdicts", "prep_msgs", "out_shares")}
            _assert_batch(res, sub, what=f"job {t}/{j}")
            assert set(f.rejecting) <= set(idx.tolist())  # every job holds every rejecting report
            assert not res.verdicts[np.isin(idx, f.rejecting)].any()
            assert rec == _record(f.orc, want, pools[k][1], idx), f"job {t}/{j}"
        assert m1["coalesced_jobs"] - m0["coalesced_jobs"] == 4 * jobs_per_thread
        # Both tasks shared a launch: three launches of four jobs are expected, and a thread that misses a
        # gather's window only splits one. Launches of one or two jobs alone would take six for the twelve, so
        # with five or fewer some launch held three jobs, of three threads, that is of both tasks.
        assert m1["coalesced_launches"] - m0["coalesced_launches"] <= 5, (m0, m1)
    finally:
        engs[0].debug(7, 0)
        for e in engs:
            e.close()


# ---------------------------------------------------------------------------- rejections: leader


@pytest.mark.parametrize("name", ["reject_count", "reject_mp2_1x32_5"])
def test_leader_role_with_rejected_query_and_joint_randomness(name):
    """The leader samples the same query and joint randomness as the helper. The fixture's reports, sharded
    again for the leader: prepare_init == the oracle's, then the ping-pong on the device; the two aggregates
    add up to the measurements."""
    f = _fixture(name)
    orc, vk, n = f.orc, f.vk, f.n
    lis = []
    for i in range(n):
        ps, li, hi = orc.shard(f.meas[i], f.nonces[i].tobytes(), f.rands[i].tobytes())
        assert ps == f.ps[i].tobytes() and hi == f.his[i].tobytes()
        lis.append(li)
    lis = np.frombuffer(b"".join(lis), np.uint8).reshape(n, -1)
    lanes = [r["report"] for r in f.doc["rejections"] if r["stream"] in ("query_rand", "joint_rand")]
    assert lanes
    refs = [orc.prep_init(vk, 0, f.nonces[i].tobytes(), f.ps[i].tobytes(), lis[i].tobytes()) for i in range(n)]
    with HelperEngine(f.vdaf, vk) as leader, HelperEngine(f.vdaf, vk) as helper:
        init = leader.leader_initialized_batch(f.nonces, f.ps, lis)
        for i, (rc, share, out, _) in enumerate(refs):
            assert rc == 0 and init.verdicts[i] == 0, i
            assert init.prep_shares[i].tobytes() == share, i
        hres = helper.helper_initialized_batch(f.nonces, f.ps, f.his, init.prep_shares, want_out_shares=True)
        want = _want(orc, vk, f.nonces, f.ps, f.his, init.prep_shares)
        _assert_batch(hres, want)
        assert not hres.verdicts.any()
        fin = leader.leader_continued_batch(hres.prep_msgs, want_out_shares=True)
        assert not fin.verdicts.any()
        for i in range(n):
            assert fin.out_shares[i].tobytes() == refs[i][2], i
        leader.accumulate(n)
        helper.accumulate(n)
        agg_l, cnt_l, cs_l = leader.aggregate_share(0)
        agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    assert agg_l == orc.aggregate([r[2] for r in refs]) and agg_h == want["agg"]
    assert cnt_l == cnt_h == n and cs_l == cs_h == want["checksum"]
    fb = orc.sizes.field_bytes
    dec = lambda b: [int.from_bytes(b[k:k + fb], "little") for k in range(0, len(b), fb)]  # noqa: E731
    total = [(a + b) % P64 for a, b in zip(dec(agg_l), dec(agg_h))]
    assert total == [int(f.meas[:, j].astype(object).sum()) % P64 for j in range(f.meas.shape[1])]


# ---------------------------------------------------------------------------- exact decode bounds

HI = 0xFFFFFFFFFFFFFFE4
VALUES128 = [P128 - 1, P128, P128 + 1, (HI << 64) | 2**32, (HI + 1) << 64, ((HI - 1) << 64) | (2**64 - 1), 2**128 - 1]
VALUES64 = [P64 - 1, P64, 0xFFFFFFFF80000000, 0xFFFFFFFEFFFFFFFF, 2**64 - 1]
BOUNDS = {
    "count": Prio3.count(),
    "sum8": Prio3.sum(8),
    "sumvec_small": Prio3.sum_vec(3, 37, 5),
    "sumvec_8x1000_88": Prio3.sum_vec(8, 1000, 88),  # the leader FLP reads the measurement in place
    "histogram_16_4": Prio3.histogram(16, 4),
    "multiproof_p2_8x12_14": Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 8, 12, 14),
}


def _honest(v: Prio3, vk, n, seed):
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)
    rng = np.random.default_rng(seed)
    if v.algo_id == O.COUNT:
        meas = rng.integers(0, 2, size=(n, 1), dtype=np.uint64)
    elif v.algo_id == O.SUM:
        meas = rng.integers(0, 1 << v.bits, size=(n, 1), dtype=np.uint64)
    elif v.algo_id == O.HISTOGRAM:
        meas = rng.integers(0, v.length, size=(n, 1), dtype=np.uint64)
    else:
        meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    ps, his, lps, _ = orc.client_leader_batch(vk, meas, nonces, rands, nthreads=8)
    lis = np.frombuffer(b"".join(orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes())[1] for i in range(n)),
                        np.uint8).reshape(n, -1).copy()
    return orc, nonces, ps, his, lps, lis


def _overwrite(rows, positions, values, fb):
    """Row k gets value k % len(values) at element position k // len(values); returns [(position, value)]."""
    cases = [(pos, val) for pos in positions for val in values]
    assert len(cases) == rows.shape[0]
    for k, (pos, val) in enumerate(cases):
        rows[k, pos * fb:(pos + 1) * fb] = np.frombuffer(val.to_bytes(fb, "little"), np.uint8)
    return cases


@pytest.mark.parametrize("name", list(BOUNDS))
def test_leader_input_share_decodes_exactly_below_p(name):
    """One report per (position, value): the first and last measurement element and the first and last proof
    element of the leader input share, set to each boundary encoding. prepare_init fails exactly for the
    encodings >= p; everywhere else the prep share is the oracle's."""
    v = BOUNDS[name]
    fb = v.field_bytes
    values, p = (VALUES64, P64) if fb == 8 else (VALUES128, P128)
    vk = bytes(range(50, 50 + v.verify_key_len))
    s = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs).sizes
    nproof = s.proof_len * v.num_proofs
    positions = [0, s.meas_len - 1, s.meas_len, s.meas_len + nproof - 1]
    n = len(positions) * len(values)
    orc, nonces, ps, his, lps, lis = _honest(v, vk, n, seed=sum(map(ord, name)) + 11)
    assert lis.shape[1] == (s.meas_len + nproof) * fb + (s.seed if s.joint_rand_len else 0)
    cases = _overwrite(lis, positions, values, fb)
    with HelperEngine(v, vk) as eng:
        init = eng.leader_initialized_batch(nonces, ps, lis)
    outcomes = set()
    for k, (pos, val) in enumerate(cases):
        rc, share, _, _ = orc.prep_init(vk, 0, nonces[k].tobytes(), ps[k].tobytes() if ps.shape[1] else b"",
                                        lis[k].tobytes())
        assert (rc != 0) == (val >= p), (pos, hex(val))  # the reference itself decodes exactly
        assert int(init.verdicts[k]) == (1 if rc else 0), (pos, hex(val))
        if rc == 0:
            assert init.prep_shares[k].tobytes() == share, (pos, hex(val))
        outcomes.add(rc != 0)
    assert outcomes == {False, True}


@pytest.mark.parametrize("name", list(BOUNDS))
def test_leader_prep_share_decodes_exactly_below_p(name):
    """The first verifier element and the last one before the joint-randomness part of the leader's prep
    share, set to each boundary encoding: leader_prep_share_decode_failure (2) exactly for the encodings
    >= p; an encoding below p decodes and gets the oracle's verdict."""
    v = BOUNDS[name]
    fb = v.field_bytes
    values, p = (VALUES64, P64) if fb == 8 else (VALUES128, P128)
    vk = bytes(range(90, 90 + v.verify_key_len))
    s = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs).sizes
    nver = s.verifier_len * v.num_proofs
    positions = [0, nver - 1]
    n = len(positions) * len(values) + 4  # and four untouched reports, which finish
    orc, nonces, ps, his, lps, _ = _honest(v, vk, n, seed=sum(map(ord, name)) + 23)
    assert lps.shape[1] == nver * fb + (s.seed if s.joint_rand_len else 0)
    cases = _overwrite(lps[:n - 4], positions, values, fb)
    want = _want(orc, vk, nonces, ps, his, lps)
    for k, (pos, val) in enumerate(cases):
        assert (want["verdicts"][k] == 2) == (val >= p), (pos, hex(val))
    assert not want["verdicts"][n - 4:].any()
    assert {2} < set(want["verdicts"].tolist())  # decode failures and other outcomes in one batch
    with HelperEngine(v, vk) as eng:
        res = eng.helper_initialized_batch(nonces, ps, his, lps, want_out_shares=True)
        _assert_batch(res, want)
        eng.accumulate(n)
        assert eng.aggregate_share(0) == (want["agg"], want["count"], want["checksum"])
