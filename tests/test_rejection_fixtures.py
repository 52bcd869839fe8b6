"""The reject_*.json fixtures (tests/golden/make_reject_golden.py) on the CPU: reports whose XOF streams
hold a real rejected Field64 sample (an 8-byte encoding >= p, a 2^-32 event per element).

Three things are pinned here without a GPU: that the inputs really have the listed rejections and no
others (from the reference XOFs alone), that the two independent references (the C oracle and pyref) skip
alike on every report, and that the CPU baseline engine reproduces the Count fixture.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import pytest

from cpu_baseline import cpu_engine as CE
from oracle import oracle as O
from tests.golden import make_reject_golden as MG

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "reject_*.json")))
# the rejection classes the fixtures must cover between them (make_reject_golden.py's class names)
CLASSES = {"count_meas", "count_proofs_4", "count_proofs_early", "count_query", "mp_meas_even", "mp_meas_odd",
           "mp_meas_last", "mp_meas_partial", "mp_proofs", "mp_query", "mp_joint"}


def _load(name):
    doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
    cfg = MG.cfg_of_doc(doc)
    orc = O.Prio3Oracle(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg["proofs"])
    return doc, cfg, orc, MG.pyref_of(cfg), bytes.fromhex(doc["verify_key"])


def _cat(doc, key):
    reps = doc["reports"]
    return np.frombuffer(b"".join(bytes.fromhex(r[key]) for r in reps), np.uint8).reshape(len(reps), -1)


def _pyref_helper_prep(P, vk, nonce, ps, his, lps):
    """pyref.Prio3.helper_prep, one prep_init only, also returning the helper's prep share."""
    (out_share, corrected), hshare = P.prep_init(vk, 1, nonce, ps, his)
    try:
        msg = P.prep_shares_to_prep([lps, hshare])
    except ValueError:
        return (2, b"", None), hshare
    except AssertionError:
        return (3, b"", None), hshare
    if P.valid.JOINT_RAND_LEN and msg != corrected:
        return (4, b"", None), hshare
    return (0, msg, P.F.encode_vec(out_share)), hshare


def test_every_class_has_a_fixture():
    assert "reject_count" in FIXTURES
    seen = {r["class"] for name in FIXTURES for r in _load(name)[0]["rejections"]}
    assert seen == CLASSES


@pytest.mark.parametrize("name", FIXTURES)
def test_layout(name):
    """More than one 64-report block, rejecting reports honest and finishing, at the lanes that matter, with
    tampered (refused) reports between them."""
    doc, cfg, orc, P, vk = _load(name)
    reps, rej = doc["reports"], doc["rejections"]
    assert len(reps) > 64 and rej
    lanes = [r["report"] for r in rej]
    assert len(set(lanes)) == len(lanes)  # one hit per report
    for r in rej:
        rep = reps[r["report"]]
        assert rep["tamper"] == "" and rep["verdict"] == 0
        assert r["stream"] in ("meas", "proofs", "joint_rand", "query_rand")
    verdicts = [r["verdict"] for r in reps]
    assert {1, 2, 3} & set(verdicts[:64]) and {1, 2, 3} & set(verdicts[64:])
    assert sum(v == 0 for v in verdicts) - len(lanes) >= 30  # honest reports without a rejection
    s = orc.sizes
    if name == "reject_count":
        assert {0, 63} <= set(lanes) and any(x >= 64 for x in lanes)
        assert sorted((r["stream"], r["raw_index"]) for r in rej if r["stream"] == "proofs")[-1] == ("proofs", 4)
    if name == "reject_mp2_1x32_5":
        assert {0, 63} <= set(lanes) and any(x >= 64 for x in lanes)
        by = {r["class"]: r for r in rej}
        assert by["mp_meas_even"]["raw_index"] % 2 == 0 and by["mp_meas_odd"]["raw_index"] % 2 == 1
        assert s.meas_len % 8 == 0 and by["mp_meas_last"]["raw_index"] == s.meas_len - 1
        assert {by[c]["stream"] for c in ("mp_meas_even", "mp_meas_odd", "mp_meas_last")} == {"meas"}
    if name == "reject_mp2_partial_chunk":
        assert s.meas_len % 8 != 0 and s.meas_len // 8 * 8 <= rej[0]["raw_index"] < s.meas_len
    assert s.meas_len <= 256


@pytest.mark.parametrize("name", FIXTURES)
def test_precondition_rejections_are_exactly_the_listed_ones(name):
    """Every stream of every report, recomputed with the C oracle's XOFs: the raw samples >= p are the
    listed ones, no more and no fewer."""
    doc, cfg, orc, P, vk = _load(name)
    listed = sorted((r["report"], r["stream"], r["raw_index"]) for r in doc["rejections"])
    seen = sorted((i, st, k) for i, rep in enumerate(doc["reports"]) for st, k in MG.report_rejections(P, vk, rep))
    assert seen == listed


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_and_pyref_agree_on_every_report(name):
    """helper_prep (verdict, prepare message, output share) and the leader's prep_init (prep share, output
    share) of the C oracle and of pyref, which share no code: pins the references' own skipping."""
    doc, cfg, orc, P, vk = _load(name)
    rejecting = {r["report"] for r in doc["rejections"]}
    _, measurements, _, rands = MG.inputs(name, *MG.fixtures()[name])  # as the generator seeded the clients
    for i, rep in enumerate(doc["reports"]):
        nonce, ps, his, lps = (bytes.fromhex(rep[k]) for k in ("nonce", "public_share", "helper_input_share",
                                                                "leader_prep_share"))
        got_c = orc.helper_prep(vk, nonce, ps, his, lps)
        got_py, py_share = _pyref_helper_prep(P, vk, nonce, ps, his, lps)
        if got_c[0] != 0:  # the buffers of a refused report are unspecified
            got_c, got_py = got_c[:1], got_py[:1]
        assert got_c == got_py, i
        assert got_c[0] == rep["verdict"], i
        if rep["verdict"] == 0:
            assert got_c[1].hex() == rep["prep_msg"], i
        if i in rejecting:
            assert got_c[2].hex() == rep["out_share"], i
        rc, hshare, hout, _ = orc.prep_init(vk, 1, nonce, ps, his)  # the helper's prep share, by both
        assert rc == 0 and hshare == py_share, i
        # the leader's side of the same report (sharded again from the recorded client randomness)
        assert measurements[i].tolist() == rep["measurement"], i
        meas = rep["measurement"] if cfg["algo"] != O.COUNT else rep["measurement"][0]
        ps2, lis, his2 = orc.shard(rep["measurement"], nonce, rands[i].tobytes())
        assert (ps2, his2) == (ps, his), i
        if i in rejecting:
            assert P.shard(meas, nonce, rands[i].tobytes()) == (ps2, lis, his2), i
        rc, lshare, lout, _ = orc.prep_init(vk, 0, nonce, ps, lis)
        (py_out, _), py_share = P.prep_init(vk, 0, nonce, ps, lis)
        assert rc == 0 and lshare == py_share and lout == P.F.encode_vec(py_out), i
        if rep["tamper"] == "":
            assert lshare == lps, i


@pytest.mark.parametrize("threads", [1, 5])
def test_cpu_engine_reproduces_reject_count(threads):
    doc, cfg, orc, P, vk = _load("reject_count")
    n = len(doc["reports"])
    res = CE.helper_prep_aggregate(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], vk, _cat(doc, "nonce"),
                                   np.zeros((n, 0), np.uint8), _cat(doc, "helper_input_share"),
                                   _cat(doc, "leader_prep_share"), nthreads=threads)
    assert res["verdicts"].tolist() == [r["verdict"] for r in doc["reports"]]
    for r in doc["rejections"]:
        assert res["verdicts"][r["report"]] == 0
    assert res["agg"].hex() == doc["aggregate_share"]
    assert res["count"] == doc["report_count"] and res["checksum"].hex() == doc["checksum"]


def test_regeneration_is_byte_for_byte(tmp_path, monkeypatch):
    """make_reject_golden.py's plain run (recorded hits, no search) rewrites the committed files as they are."""
    monkeypatch.setattr(MG, "HERE", str(tmp_path))
    for name, (cfg, lanes) in MG.fixtures().items():
        MG.make(name, cfg, lanes)
        assert open(tmp_path / f"{name}.json", "rb").read() == open(os.path.join(GOLDEN, name + ".json"), "rb").read()
