"""The C oracle at long and degenerate ParallelSum gadgets (the LONG_GADGETS fixtures of
tests/golden/make_golden.py, which tests/test_gpu_long_gadgets.py and test_gpu_parity.test_golden hold the
HIP kernels to).

pyref cannot check the oracle at 500 and more gadget calls (one SumVec 1x520/1 report takes it over ten
minutes), so there the oracle is pinned by the invariants of tests/test_oracle_crosscheck.py: honest reports
are accepted, leader + helper output shares sum to the measurement, and a flipped bit anywhere in the leader
prep share is refused. At one and three calls pyref is fast, and the oracle must equal it.
"""
from __future__ import annotations

import json
import os
import random

import numpy as np
import pytest

from oracle import oracle as O
from oracle import pyref
from tests.golden import make_golden as MG

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# 4400 and more calls: fixtures only (test_gpu_parity.test_golden), see test_regeneration_is_byte_for_byte
VERY_LONG = ["sumvec_1x4400_1", "sumvec_1x8800_2", "sumvec_f64mp_2_1x5600_1"]
SMALL = ["sumvec_1x3_5", "histogram_3_8", "sumvec_f64mp_2_1x3_5", "sumvec_1x9_3"]  # 1 call (chunk > meas_len), 3 calls
MID = [k for k in MG.LONG_GADGETS if k not in VERY_LONG + SMALL]  # 512 .. 1030 calls


def _oracle(cfg) -> O.Prio3Oracle:
    return O.Prio3Oracle(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg.get("proofs", 1))


def _pyref(cfg) -> pyref.Prio3:
    if cfg["algo"] == O.HISTOGRAM:
        return pyref.Prio3("histogram", length=cfg["length"], chunk=cfg["chunk"])
    kw = dict(bits=cfg["bits"], length=cfg["length"], chunk=cfg["chunk"])
    if cfg["algo"] == O.SUMVEC_F64_MULTIPROOF:
        return pyref.Prio3("sumvec_f64_multiproof", proofs=cfg["proofs"], **kw)
    return pyref.Prio3("sumvec", **kw)


def _measurement(cfg, rng):
    if cfg["algo"] == O.HISTOGRAM:
        return rng.randrange(cfg["length"])
    return [rng.randrange(1 << cfg["bits"]) for _ in range(cfg["length"])]


def _expected_output(cfg, m):
    return [int(b == m) for b in range(cfg["length"])] if cfg["algo"] == O.HISTOGRAM else list(m)


def _flip_each_element(lshare: bytes, s: O.Sizes, rng) -> np.ndarray:
    """One copy of the leader prep share per verifier element and one for the joint-rand part, each with one
    random bit of that element (part) flipped."""
    nver = (len(lshare) - s.seed) // s.field_bytes
    assert nver * s.field_bytes + s.seed == len(lshare) and s.joint_rand_len
    rows = np.tile(np.frombuffer(lshare, np.uint8), (nver + 1, 1))
    for e in range(nver):
        rows[e, e * s.field_bytes + rng.randrange(s.field_bytes)] ^= 1 << rng.randrange(8)
    rows[nver, nver * s.field_bytes + rng.randrange(s.seed)] ^= 1 << rng.randrange(8)
    return rows


def _check_invariants(name, cfg, C, Py=None, reports=2):
    rng = random.Random(sum(map(ord, name)))
    s = C.sizes
    vk = rng.randbytes(s.verify_key)
    for _ in range(reports):
        nonce, rand = rng.randbytes(16), rng.randbytes(s.client_rand)
        m = _measurement(cfg, rng)
        ps, lin, hin = C.shard(m, nonce, rand)
        rc, lshare, lout, _ = C.prep_init(vk, 0, nonce, ps, lin)
        assert rc == 0
        got = C.helper_prep(vk, nonce, ps, hin, lshare)
        assert got[0] == 0  # the honest report is accepted
        agg = C.aggregate([lout, got[2]])
        E = s.field_bytes
        assert [int.from_bytes(agg[i:i + E], "little") for i in range(0, len(agg), E)] == _expected_output(cfg, m)
        bad = _flip_each_element(lshare, s, rng)
        k = bad.shape[0]
        tile = lambda b: np.tile(np.frombuffer(b, np.uint8), (k, 1))  # noqa: E731
        v = C.helper_prep_batch(vk, tile(nonce), tile(ps), tile(hin), bad, nthreads=8)["verdicts"]
        assert set(v.tolist()) <= {2, 3, 4}, v.tolist()
        assert v[-1] == 4  # the joint-rand part alone: the FLP decides, prepare_next fails
        if Py is not None:
            assert (ps, lin, hin) == Py.shard(m, nonce, rand)
            assert lshare == Py.prep_init(vk, 0, nonce, ps, lin)[1]
            assert got == Py.helper_prep(vk, nonce, ps, hin, lshare)
            for i in range(k):
                assert Py.helper_prep(vk, nonce, ps, hin, bad[i].tobytes())[0] == v[i], i


@pytest.mark.parametrize("name", MID)
def test_long_gadget_invariants(name):
    cfg = MG.LONG_GADGETS[name]
    C = _oracle(cfg)
    assert 512 <= C.sizes.calls <= 1030
    _check_invariants(name, cfg, C)


@pytest.mark.parametrize("name", SMALL)
def test_degenerate_gadgets_equal_pyref(name):
    cfg = MG.LONG_GADGETS[name]
    C = _oracle(cfg)
    assert C.sizes.calls == (3 if name == "sumvec_1x9_3" else 1)
    if C.sizes.calls == 1:
        assert C.sizes.chunk > C.sizes.meas_len
    _check_invariants(name, cfg, C, _pyref(cfg), reports=3)


@pytest.mark.parametrize("name", list(MG.LONG_GADGETS))
def test_fixture_verdict_pattern(name):
    """Untampered reports finish (so a kernel whose wire sums wrap refuses them), tampered ones do not."""
    doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
    cfg = MG.LONG_GADGETS[name]
    assert doc["sizes"]["calls"] == _oracle(cfg).sizes.calls and len(doc["reports"]) == cfg["n"]
    want = {"": 0, "verifier_bitflip": 3, "verifier_ge_p": 2, "joint_rand_part": 4}
    assert [r["verdict"] for r in doc["reports"]] == [want[r["tamper"]] for r in doc["reports"]]
    assert doc["report_count"] == cfg["n"] // 2


def test_regeneration_is_byte_for_byte(tmp_path, monkeypatch):
    """make_golden.py's plain run rewrites the committed LONG_GADGETS fixtures as they are: 4.4 s for the
    twelve of up to 1030 calls. The three of 4400 and more calls are left out: they take 21.5 s more (measured:
    7.3 s, 7.7 s and 6.5 s, eight oracle threads), 25.9 s in all."""
    monkeypatch.setattr(MG, "HERE", str(tmp_path))
    for name, cfg in MG.LONG_GADGETS.items():
        if name in VERY_LONG:
            continue
        MG.make(name, cfg)
        assert open(tmp_path / f"{name}.json", "rb").read() == open(os.path.join(GOLDEN, name + ".json"), "rb").read()
