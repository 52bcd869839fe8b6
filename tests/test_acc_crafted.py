"""CPU: the crafted output shares of tests/acc_crafted.py and their Python model, against the C oracle.

tests/test_gpu_accumulate_edges.py compares the engine's aggregations with acc_crafted.model() on reports from
acc_crafted.craft(). Here, without a GPU: every instance and value pattern crafts (the oracle's leader prep_init
accepts each report and returns exactly the crafted row as its output share); the model equals the oracle's
aggregate of the same rows and the oracle's SHA-256 checksum; and a rejected row of either kind gets the intended
oracle outcome. hist6000 is left to its one GPU case (craft() makes the same per-report assertions there)."""
from __future__ import annotations

import numpy as np
import pytest

import acc_crafted as A
from oracle import oracle as O

NAMES = [n for n in A.INSTANCES if n != "hist6000"]
CASES = [(n, pat) for n in NAMES for pat in A.pattern_names(A.instance(n))]


def _oracle_expected(inst, c, idx):
    agg = inst.orc.aggregate([c.out_bytes(i) for i in idx]) if len(idx) else bytes(inst.out_len * inst.fb)
    cs = bytes(32)
    for i in idx:
        cs = bytes(a ^ b for a, b in zip(cs, O.sha256(c.nonces[i].tobytes())))
    return agg, len(idx), cs


@pytest.mark.parametrize("name,pat", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_craft_and_model_match_oracle(name, pat):
    inst = A.instance(name)
    n = 70 if inst.out_len <= 5 else 20
    init, fin = A.spread_rejects(inst, n)
    c = A.craft(inst, A.pattern(inst, pat, n, seed=3), seed=11, reject_init=init, reject_finish=fin)
    assert c.n == n and (c.verdicts[init] == A.REJECT_INIT).all() and (c.verdicts[fin] == A.REJECT_FINISH).all()
    assert int(c.accepted.sum()) == n - len(init) - len(fin) and len(init) >= 1
    assert len(fin) >= 1 or not inst.joint_rand
    assert all(0 <= x < inst.p for row in c.elems for x in row)
    rng = np.random.default_rng(5)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    for sel in (c.accepted, c.accepted & (mask != 0), np.zeros(n, bool), c.accepted & (np.arange(n) % 2 == 0)):
        idx = [int(i) for i in np.nonzero(sel)[0]]
        assert A.model(inst.p, inst.fb, c.elems, c.nonces, sel) == _oracle_expected(inst, c, idx)
        assert A.model(inst.p, inst.fb, c.elems, c.nonces, np.array(idx, np.int64)) == _oracle_expected(inst, c, idx)
    # merging into an existing aggregation == merging everything at once
    half = c.accepted & (np.arange(n) < n // 2)
    first = A.model(inst.p, inst.fb, c.elems, c.nonces, half)
    both = A.model(inst.p, inst.fb, c.elems, c.nonces, c.accepted & ~half, prev=first)
    assert both == A.model(inst.p, inst.fb, c.elems, c.nonces, c.accepted)


@pytest.mark.parametrize("name", NAMES)
def test_patterns_reach_the_edges(name):
    """all_max sums to p - n, an even cancel selection to 0, and with p - 1 already there one more report wraps."""
    inst = A.instance(name)
    p, fb, m = inst.p, inst.fb, inst.out_len
    n = 8
    nonces = np.zeros((n, 16), np.uint8)
    agg, cnt, _ = A.model(p, fb, A.pattern(inst, "all_max", n), nonces, np.ones(n, bool))
    assert agg == (p - n).to_bytes(fb, "little") * m and cnt == n
    agg, _, cs = A.model(p, fb, A.pattern(inst, "cancel", n), nonces, np.ones(n, bool))
    assert agg == bytes(fb * m) and cs == bytes(32)  # the same id eight times cancels too
    prev = ((p - 1).to_bytes(fb, "little") * m, 2**32 - 1, b"\xff" * 32)
    agg, cnt, _ = A.model(p, fb, A.pattern(inst, "cancel", 2), nonces[:2], np.array([1]), prev=prev)
    assert agg == bytes(fb * m) and cnt == 2**32
    names = A.pattern_names(inst)
    assert ("carry64" in names) == (fb == 16)
    assert {x for row in A.pattern(inst, "edge_cycle", 40) for x in row} == set(A._edges(inst))


@pytest.mark.parametrize("name", NAMES)
def test_rejected_rows_get_the_intended_outcome(name):
    """An element of p fails the oracle's leader decode; a flipped prep-message bit differs from the oracle's own
    corrected seed (what leader_finish compares) while the undamaged message equals it."""
    inst = A.instance(name)
    n = 6
    elems = A.pattern(inst, "edge_cycle", n)
    fin = [2] if inst.joint_rand else []
    c = A.craft(inst, elems, seed=1, reject_init=[4], reject_finish=fin)
    clean = A.craft(inst, elems, seed=1)
    assert list(c.verdicts) == [0, 0, A.REJECT_FINISH if fin else 0, 0, A.REJECT_INIT, 0] and not clean.verdicts.any()
    np.testing.assert_array_equal(c.nonces, clean.nonces)
    assert int.from_bytes(c.lis[4, :inst.fb].tobytes(), "little") == inst.p
    np.testing.assert_array_equal(np.delete(c.lis, 4, 0), np.delete(clean.lis, 4, 0))
    if fin:
        diff = c.msgs[2] ^ clean.msgs[2]
        assert bin(int.from_bytes(diff.tobytes(), "little")).count("1") == 1
        np.testing.assert_array_equal(np.delete(c.msgs, [2, 4], 0), np.delete(clean.msgs, [2, 4], 0))
        for r in (0, 2):
            _, _, _, corr = inst.orc.prep_init(inst.vk, 0, c.nonces[r].tobytes(), c.ps[r].tobytes(), c.lis[r].tobytes())
            assert (corr[:inst.vdaf.seed_size] == c.msgs[r].tobytes()) == (r == 0)
    else:
        assert c.msgs is None
    with pytest.raises(AssertionError):
        A.craft(inst, [[inst.p] * inst.out_len], seed=1)  # elements are canonical by contract


def test_take_keeps_rows_together():
    c = A.pool("hist5", "random", 40)
    t = c.take(np.array([7, 3, 3, 39]))
    assert t.elems == [c.elems[7], c.elems[3], c.elems[3], c.elems[39]]
    np.testing.assert_array_equal(t.nonces, c.nonces[[7, 3, 3, 39]])
    np.testing.assert_array_equal(t.msgs, c.msgs[[7, 3, 3, 39]])
    assert c.take(slice(5, 9)).n == 4
