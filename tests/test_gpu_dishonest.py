"""The engine against reports from a cheating client (tests/dishonest.py).

Honest reports with a damaged leader prep share pin the kernels' linear arithmetic; they cannot
pin the decision. Here every rejected report is one the verifier exists for: a proof that is
consistent with an invalid measurement (its only defect is v != 0, or one of the two combined
Histogram / FixedPoint checks), a share altered on the wire before the leader prepared, or an
honest report whose leader prep share differs in exactly one verifier element of one proof.
Expected verdicts, prepare messages, output shares and aggregates are the C oracle's;
tests/test_oracle_dishonest.py shows on the CPU that they are the designed ones.

Bar: bit-exact. No cheat may reach an aggregate on the batch path, the fused path or the slow path.
"""
from __future__ import annotations

import numpy as np
import pytest

import dishonest as D
from janus_amd.engine import HelperEngine

pytestmark = pytest.mark.gpu


def _same_verdicts(batch, got, what):
    want = batch.want["verdicts"]
    wrong = [f"{batch.describe(k)}: {what} says {int(got[k])}, the oracle {int(want[k])}"
             for k in range(batch.n) if got[k] != want[k]]
    assert not wrong, "\n".join(wrong[:12]) + (f"\n... {len(wrong)} lanes in all" if len(wrong) > 12 else "")


def _helper_matches(eng, batch, what, want_agg=True):
    want, n = batch.want, batch.n
    res = eng.helper_initialized_batch(batch.nonces, batch.ps, batch.his, batch.lps, want_out_shares=True)
    _same_verdicts(batch, res.verdicts, what)
    fin = want["verdicts"] == 0
    np.testing.assert_array_equal(res.prep_msgs[fin], want["prep_msgs"][fin])
    np.testing.assert_array_equal(res.out_shares[fin], want["out_shares"][fin])
    if want_agg:
        eng.accumulate(n)
        assert eng.aggregate_share(0) == (want["agg"], want["count"], want["checksum"])
    else:
        eng.release(res.batch_id)
    return res


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_cheating_client_is_rejected(name):
    batch = D.cheat_batch(name)
    inst, want = batch.inst, batch.want
    assert all(want["verdicts"][k] == 3 for k in batch.bad) and want["count"] == batch.n - len(batch.bad)
    with HelperEngine(inst.vdaf, inst.vk) as eng:
        _helper_matches(eng, batch, "helper_initialized_batch")
        v2, m2 = eng.prep_and_aggregate(batch.nonces, batch.ps, batch.his, batch.lps, segment=3)
        _same_verdicts(batch, v2, "prep_and_aggregate")
        fin = want["verdicts"] == 0
        np.testing.assert_array_equal(m2[fin], want["prep_msgs"][fin])
        assert eng.aggregate_share(3) == (want["agg"], want["count"], want["checksum"])
        eng.debug(1, 1)
        _helper_matches(eng, batch, "the slow path", want_agg=False)


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_decide_every_element(name):
    """Labels name the proof and the element ("sweep: proof 2 element 5 + 1")."""
    batch = D.sweep_batch(name)
    inst = batch.inst
    with HelperEngine(inst.vdaf, inst.vk) as eng:
        _helper_matches(eng, batch, "helper_initialized_batch")


@pytest.mark.parametrize("name", list(D.INSTANCES))
def test_wire_tampering(name):
    batch = D.wire_batch(name)
    inst = batch.inst
    lps = batch.lps.copy()
    with HelperEngine(inst.vdaf, inst.vk) as eng:
        # the leader prepares from what it received: its prep share goes to the helper
        side = [k for k in batch.bad if batch.rows[k].leader_side]
        init = eng.leader_initialized_batch(batch.nonces[side], batch.ps[side], batch.lis[side])
        for j, k in enumerate(side):
            assert init.verdicts[j] == 0, batch.describe(k)
            assert init.prep_shares[j].tobytes() == batch.rows[k].lps, batch.describe(k)
            lps[k] = init.prep_shares[j]
        eng.release(init.batch_id)
        np.testing.assert_array_equal(lps, batch.lps)
        assert all(batch.want["verdicts"][k] != 0 for k in batch.bad)
        _helper_matches(eng, batch, "helper_initialized_batch")


def _decode(agg: bytes, fb: int):
    return [int.from_bytes(agg[i:i + fb], "little") for i in range(0, len(agg), fb)]


@pytest.mark.parametrize("name", D.BOTH_ROLES)
def test_both_roles_on_the_device(name):
    batch = D.cheat_batch(name)
    inst, n = batch.inst, batch.n
    v, p = inst.vdaf, inst.p
    with HelperEngine(v, inst.vk) as leader, HelperEngine(v, inst.vk) as helper:
        init = leader.leader_initialized_batch(batch.nonces, batch.ps, batch.lis)
        assert not init.verdicts.any()  # a cheat's shares are all in range
        np.testing.assert_array_equal(init.prep_shares, batch.lps)
        hres = helper.helper_initialized_batch(batch.nonces, batch.ps, batch.his, init.prep_shares)
        _same_verdicts(batch, hres.verdicts, "the helper")
        fin = leader.leader_continued_batch(hres.prep_msgs, want_out_shares=True)
        accept = ((hres.verdicts == 0) & (fin.verdicts == 0)).astype(np.uint8)
        leader.accumulate(n, accept_mask=accept)
        helper.accumulate(n, accept_mask=accept)
        agg_l, cnt_l, cs_l = leader.aggregate_share(0)
        agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    honest = [r.truth for r in batch.rows if not r.label]
    assert [bool(a) for a in accept] == [not r.label for r in batch.rows]
    assert cnt_l == cnt_h == len(honest) == n - len(batch.bad)
    assert cs_l == cs_h
    total = [(a + b) % p for a, b in zip(_decode(agg_l, v.field_bytes), _decode(agg_h, v.field_bytes))]
    assert total == [sum(col) % p for col in zip(*honest)]
    if name != "mp3_1x7_3":  # Prio3.unshard covers Count, Sum, SumVec and Histogram
        assert v.unshard([agg_l, agg_h], cnt_l) == total


def test_dap_layer_reports_vdaf_prep_error():
    """The DAP-level mirrors with two cheats among 40 reports: the helper answers VdafPrepError for
    exactly those two, the leader leaves them unfinished, and the totals exclude them."""
    from janus_amd.aggregator import (LeaderReport, handle_aggregate_init, leader_aggregate_init,
                                      leader_process_helper_response)
    from janus_amd.messages import HpkeCiphertext, PrepareError, ReportMetadata
    from janus_amd.vdaf import Prio3
    from oracle import oracle as O
    from oracle import pyref

    v = Prio3.sum_vec(4, 50, 7)
    vk = bytes(range(7, 23))
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length)
    py = pyref.Prio3("sumvec", bits=4, length=50, chunk=7)
    n, cheats = 40, {11: (0, 2), 29: (v.meas_len - 1, D.P128 - 1)}
    rng = np.random.default_rng(4507)
    meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    shards = []
    for i in range(n):
        if i in cheats:
            elems = py.valid.encode([int(x) for x in meas[i]])
            elems[cheats[i][0]] = cheats[i][1]
            shards.append(py.shard_encoded(elems, nonces[i].tobytes(), rands[i].tobytes()))
        else:
            shards.append(orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()))
    for i in cheats:  # the oracle rejects them for the proof alone
        ps, lis, his = shards[i]
        rc, lps, _, _ = orc.prep_init(vk, 0, nonces[i].tobytes(), ps, lis)
        assert rc == 0 and orc.helper_prep(vk, nonces[i].tobytes(), ps, his, lps)[0] == 3
    reports = [LeaderReport(ReportMetadata(nonces[i].tobytes(), 1_700_000_000 + i), shards[i][0], shards[i][1],
                            HpkeCiphertext(1, b"enc", b"ct")) for i in range(n)]
    with HelperEngine(v, vk) as leader, HelperEngine(v, vk) as helper:
        step = leader_aggregate_init(leader, reports)
        assert not step.failed and list(step.stepped) == list(range(n))
        out = handle_aggregate_init(helper, list(step.prepare_inits), [shards[i][2] for i in step.stepped])
        errors = {i for i, r in enumerate(out.responses) if getattr(r.result, "error", None) is not None}
        assert errors == set(cheats)
        by_id = {r.report_id: r.result for r in out.responses}
        for i in cheats:
            assert by_id[nonces[i].tobytes()].error == PrepareError.VdafPrepError
        assert out.step_failures["prepare_message_failure"] == 2
        lead = leader_process_helper_response(leader, step, out.responses)
        ok = np.array([bool(lead.finished[i]) for i in range(n)])
        assert [i for i in range(n) if not ok[i]] == sorted(cheats)
        agg_l, cnt_l, _ = leader.aggregate_share(0)
        agg_h, cnt_h, _ = helper.aggregate_share(0)
    assert cnt_l == cnt_h == n - 2
    total = [(a + b) % D.P128 for a, b in zip(_decode(agg_l, 16), _decode(agg_h, 16))]
    assert total == [int(meas[ok, j].astype(object).sum()) for j in range(v.length)]
