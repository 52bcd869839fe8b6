"""The cheat, wire, sweep and order cases of tests/dishonest.py have their designed verdicts in both
restatements (the C oracle and oracle/pyref.py), on the CPU.

This is what keeps tests/test_gpu_dishonest.py from passing emptily: a cheat that the references
accepted, or a sweep copy they did not reject, would make the GPU comparison say nothing. A case
that is not rejected as designed is a reason to change the input in tests/dishonest.py, never the
assertion here.
"""
import numpy as np
import pytest

import dishonest as D


def _pyref(inst, row):
    return inst.py.helper_prep(inst.vk, row.nonce, row.ps, row.his, row.lps)


def _check(batch, designed):
    """Oracle verdicts are the designed ones; pyref agrees on every bad lane and on two honest ones."""
    inst, got = batch.inst, batch.want["verdicts"]
    for k, row in enumerate(batch.rows):
        assert row.rc == 0, f"{batch.describe(k)}: leader prep_init rc {row.rc}"
        if not row.label:
            assert got[k] == 0, batch.describe(k)
        elif row.expect is None:
            assert got[k] != 0, batch.describe(k)
        else:
            assert got[k] == row.expect, f"{batch.describe(k)}: oracle says {got[k]}, designed {row.expect}"
    assert {got[k] for k in batch.bad} <= designed
    honest = [k for k in range(batch.n) if not batch.rows[k].label][:2]
    for k in batch.bad + honest:
        v, msg, out = _pyref(inst, batch.rows[k])
        assert v == got[k], f"{batch.describe(k)}: pyref says {v}, the C oracle {got[k]}"
        if v == 0:
            assert msg == batch.want["prep_msgs"][k].tobytes() and out == batch.want["out_shares"][k].tobytes()
    n = batch.n
    assert n > 64 and n % 64 and all(batch.rows[k].label for k in (0, 63, 64, n - 1))
    assert batch.want["count"] == sum(1 for r in batch.rows if not r.label)


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_cheats_have_the_designed_verdict(name):
    batch = D.cheat_batch(name)
    _check(batch, {3})
    # a cheat's shares are all in range: only the proof system can tell
    inst = batch.inst
    for k in batch.bad:
        lis = batch.rows[k].lis
        nel = inst.vdaf.meas_len + inst.vdaf.num_proofs * inst.vdaf.proof_len
        assert all(int.from_bytes(lis[i * inst.fb:(i + 1) * inst.fb], "little") < inst.p for i in range(nel))


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_wire_edits_are_rejected(name):
    batch = D.wire_batch(name)
    _check(batch, {1, 2, 3, 4})
    want = 8 if batch.inst.vdaf.joint_rand_len else 4
    assert len(batch.bad) == want and sum(batch.rows[k].leader_side for k in batch.bad) == want - (3 if want == 8 else 2)


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_sweep_and_order_cases(name):
    batch = D.sweep_batch(name)
    _check(batch, {2, 3, 4})
    v = batch.inst.vdaf
    c = D.counts(name)
    assert c["sweep"] == v.verifier_len * v.num_proofs + (v.seed_size if v.joint_rand_len else 0)
    assert c["order"] == (4 if v.joint_rand_len else 1)
    got = batch.want["verdicts"]
    for k in batch.bad:
        label = batch.rows[k].label
        if label.startswith("sweep: proof"):
            assert got[k] == 3, label
        elif label.startswith("sweep: joint"):
            assert got[k] == 4, label


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_shard_encoded_is_shard(name):
    """shard_encoded(encode(m)) == shard(m) == the C oracle's jo_shard, byte for byte."""
    inst = D.instance(name)
    rng = np.random.default_rng(inst.seed + 3)
    m = inst.honest_measurement(rng)
    nonce = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    rand = rng.integers(0, 256, inst.orc.sizes.client_rand, dtype=np.uint8).tobytes()
    want = inst.orc.shard(m, nonce, rand)
    assert inst.py.shard(m, nonce, rand) == want
    assert inst.py.shard_encoded(inst.encode(m), nonce, rand) == want
