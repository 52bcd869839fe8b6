"""GPU: the leader's end of the wire (jx_init_req_encode / jx_init_resp_decode, aggregator.leader_aggregate_init_wire
and leader_process_helper_response_wire): the AggregationJobInitializeReq body written on the device from the arrays
the leader holds, and the helper's AggregationJobResp body turned into the rows jx_leader_prep_finish_device reads.

What the encode must write is janus_amd.messages' encoding of exactly the sent reports; what the decode must give is
what aggregator.leader_process_helper_response derives from the same responses; the aggregate shares are the C
oracle's over exactly the reports both sides finish. None comes from the engine.

Shapes: 1, 64, 65 and 193 reports (one lane, a full wave, one past it, and three waves plus one at four reports per
workgroup); 130 where two waves and two reports matter."""
from __future__ import annotations

import dataclasses
import random

import numpy as np
import pytest
import torch

import test_wire_host as W
from janus_amd import client, hpke
from janus_amd._lib import EngineError
from janus_amd.aggregator import (LeaderReport, UploadTask, handle_aggregate_init_encrypted, handle_aggregate_init_wire,
                                  handle_upload, leader_aggregate_init, leader_aggregate_init_wire,
                                  leader_process_helper_response, leader_process_helper_response_wire)
from janus_amd.batch_aggregation import AGGREGATING, BatchAggregation, BatchAggregationWriter
from janus_amd.engine import _DeviceBytes  # noqa: PLC2701
from janus_amd.engine import (KEY_NONE, RESP_CONTINUED, RESP_FINISHED, RESP_MESSAGE_MISMATCH, RESP_REJECTED, WIRE_MALFORMED,
                              WIRE_NO_ERROR, WIRE_OK, WIRE_RESP_MISMATCH, HelperEngine)
from janus_amd.messages import (QUERY_FIXED_SIZE, QUERY_TIME_INTERVAL, AggregationJobInitializeReq, AggregationJobResp,
                                CodecError, Extension, HpkeCiphertext, PartialBatchSelector, PingPongMessage, PrepareError,
                                PrepareInit, PrepareResp, PrepareStepResult, Report, ReportMetadata, ReportShare)
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O
from test_gpu_sealed_fused import INSTANCES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ALL = dict(INSTANCES, sumvec=(Prio3.sum_vec(8, 100, 10), 16))
BATCH_ID = bytes(range(100, 132))
TIME0 = 1_700_000_000


def dev(a, skew: int = 0):
    """The bytes of `a` on the device, starting `skew` bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.zeros(a.size + 32, dtype=torch.uint8, device=DEV)
    at = (-t.data_ptr()) % 16 + skew
    t[at:at + a.size] = torch.from_numpy(a.copy()).to(DEV)
    return t[at:at + a.size] if a.size else t[at:at + 1]


class Rows:
    """n reports of an instance's lengths filled with random bytes, as the leader holds them after its init."""

    def __init__(self, rnd, v, n, enc=lambda i: 32, pay=None):
        self.v, self.n = v, n
        PS, LPS = v.public_share_len, v.prep_share_len
        pay = pay or (lambda i: 22 + v.helper_input_share_len)
        self.ids = [rnd.randbytes(16) for _ in range(n)]
        self.times = np.array([TIME0 + rnd.randrange(1000) for _ in range(n)], np.uint64)
        self.cfg = np.array([rnd.randrange(256) for _ in range(n)], np.uint8)
        self.ps = [rnd.randbytes(PS) for _ in range(n)]
        self.lps = [rnd.randbytes(LPS) for _ in range(n)]
        self.encs = [rnd.randbytes(enc(i)) for i in range(n)]
        self.pays = [rnd.randbytes(pay(i)) for i in range(n)]
        self.eoff = np.concatenate([[0], np.cumsum([len(x) for x in self.encs])]).astype(np.uint64)
        self.poff = np.concatenate([[0], np.cumsum([len(x) for x in self.pays])]).astype(np.uint64)

    def init(self, i) -> PrepareInit:
        return PrepareInit(ReportShare(ReportMetadata(self.ids[i], int(self.times[i])), self.ps[i],
                                       HpkeCiphertext(int(self.cfg[i]), self.encs[i], self.pays[i])),
                           PingPongMessage.initialize(self.lps[i]))

    def body(self, sent, param: bytes, fixed: bool) -> bytes:
        sel = PartialBatchSelector.fixed_size(BATCH_ID) if fixed else PartialBatchSelector.time_interval()
        return AggregationJobInitializeReq(param, sel, tuple(self.init(i) for i in sent)).encode()

    def device(self, stride: int = 0, skew: int = 0):
        LPS = self.v.prep_share_len
        lps = b"".join(x + bytes((stride or LPS) - LPS) for x in self.lps)
        j = lambda xs: np.frombuffer(b"".join(xs) or b"\0", np.uint8)  # noqa: E731
        return dict(ids=dev(j(self.ids), skew), ps=dev(j(self.ps), skew), encs=dev(j(self.encs), skew),
                    pays=dev(j(self.pays), skew), lps=dev(j([lps]), skew))

    def encode(self, eng, verdicts, exclude, param=b"agg", fixed=False, stride=0, skew=0, host=False, **kw):
        q = QUERY_FIXED_SIZE if fixed else QUERY_TIME_INTERVAL
        bid = BATCH_ID if fixed else None
        j = b"".join
        if host:
            return eng.encode_init_req_host(j(self.ids), self.times, j(self.ps), self.cfg, j(self.encs), j(self.pays),
                                            self.poff, j(self.lps), verdicts, param, q, bid, enc_offsets=self.eoff,
                                            exclude=exclude)
        d = self.device(stride, skew)
        d_v = dev(np.asarray(verdicts, np.uint8), skew)
        self._keep = (d, d_v)
        return eng.encode_init_req(self.n, d["ids"].data_ptr(), self.times, d["ps"].data_ptr() if self.v.public_share_len else None,
                                   self.cfg, d["encs"].data_ptr(), d["pays"].data_ptr(), self.poff, d["lps"].data_ptr(),
                                   d_v.data_ptr(), param, q, bid, enc_offsets=self.eoff, exclude=exclude,
                                   prep_share_stride=stride, **kw)


def masks(rnd, n):
    verdicts = np.array([rnd.choice((1, 2, 4)) if rnd.random() < 0.25 else 0 for _ in range(n)], np.uint8)
    exclude = np.array([rnd.random() < 0.15 for _ in range(n)], np.uint8)
    return verdicts, exclude, [i for i in range(n) if verdicts[i] == 0 and not exclude[i]]


# ----------------------------------------------------------------------------- 1. encode equals the Python codec


@pytest.mark.parametrize("name", list(ALL))
def test_encode_equals_the_codec(name):
    v, vkl = ALL[name]
    rnd = random.Random(sum(map(ord, name)))
    with HelperEngine(v, bytes(vkl)) as eng:
        for n in (1, 64, 65, 193):
            rows = Rows(rnd, v, n)
            verdicts, exclude, sent = masks(rnd, n)
            fixed = n % 2 == 0
            want = rows.body(sent, b"agg", fixed)
            with rows.encode(eng, verdicts, exclude, fixed=fixed, stride=v.prep_share_len + 5 if n == 65 else 0) as req:
                assert (req.n, req.n_sent, req.body_len) == (n, len(sent), len(want)), (name, n)
                np.testing.assert_array_equal(req.sent_index, np.array(sent, np.uint32))
                assert req.body == want, (name, n)
                if sent:  # the compaction list on the device
                    d_idx = torch.as_tensor(_DeviceBytes(req.d_sent_index, 4 * len(sent)), device=DEV).cpu().numpy()
                    np.testing.assert_array_equal(d_idx.view(np.uint32), req.sent_index)
            with rows.encode(eng, verdicts, exclude, fixed=fixed, host=True) as req:
                assert req.body == want and req.sent_index.tolist() == sent, (name, n, "host form")
        rows = Rows(rnd, v, 65)
        zeros, ones = np.zeros(65, np.uint8), np.ones(65, np.uint8)
        for what, verdicts, exclude, sent in (("all", zeros, None, list(range(65))), ("none by verdict", ones, None, []),
                                              ("none by exclusion", zeros, ones, []),
                                              ("one", (np.arange(65) != 40).astype(np.uint8), zeros, [40])):
            for host in (False, True):
                with rows.encode(eng, verdicts, exclude, param=b"", host=host) as req:
                    assert req.body == rows.body(sent, b"", False), (name, what, host)
                    assert req.n_sent == len(sent) and req.sent_index.tolist() == sent
        empty = Rows(rnd, v, 0)
        with empty.encode(eng, zeros[:0], None, fixed=True) as req:  # a job without reports: an empty vector
            assert req.body == empty.body([], b"agg", True) and (req.n, req.n_sent) == (0, 0)
        assert eng.resident_batches()[0] == 0


# ----------------------------------------------------------------------------- 2. every destination alignment


def test_every_destination_alignment():
    v = Prio3.sum_vec(8, 100, 10)
    rnd = random.Random(2)
    n = 65
    pay_lens = (0, 1, 15, 16, 17, 6 + v.helper_input_share_len + 16)
    rows = Rows(rnd, v, n, enc=lambda i: 32 + i % 16, pay=lambda i: pay_lens[(i // 3) % 6])  # (i % 6 would leave two residues out)
    verdicts, exclude = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    verdicts[[7, 30]] = 1
    sent = [i for i in range(n) if i not in (7, 30)]
    want = rows.body(sent, b"agg", False)
    recs = W.expected_records(want, AggregationJobInitializeReq.decode(want, QUERY_TIME_INTERVAL))
    for k, what in ((2, "public share"), (4, "encapsulated key"), (6, "payload"), (12, "prep share")):
        assert {r[k] % 16 for r in recs} == set(range(16)), what  # the body starts on a 16-byte boundary below
    guard = 64
    with HelperEngine(v, bytes(16)) as eng:
        for skew in (0, 1, 7, 15):  # the inputs that far off a 16-byte boundary; the output too
            buf = torch.full((len(want) + guard + 32,), 0xA5, dtype=torch.uint8, device=DEV)
            at = (-buf.data_ptr()) % 16 + skew
            with rows.encode(eng, verdicts, exclude, skew=skew, d_out=buf.data_ptr() + at, capacity=len(want)) as req:
                got = buf.cpu().numpy()
                assert req.body_len == len(want) and req.sent_index.tolist() == sent
                assert got[at:at + len(want)].tobytes() == want, skew
                assert (got[:at] == 0xA5).all() and (got[at + len(want):] == 0xA5).all(), skew  # the guard bytes
        buf = torch.full((len(want) + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        with pytest.raises(EngineError, match=r"\(-1\)"):
            rows.encode(eng, verdicts, exclude, d_out=buf.data_ptr(), capacity=len(want) - 1)
        assert (buf.cpu().numpy() == 0xA5).all()
        assert eng.init_req_bound(n, rows.poff, 3, QUERY_TIME_INTERVAL, rows.eoff) == len(rows.body(range(n), b"agg", False))


# ----------------------------------------------------------------------------- 3. round trip through the helper's decode


@pytest.mark.parametrize("name", ["sumvec", "count"])
def test_round_trip_through_the_helper_decode(name):
    v, vkl = ALL[name]
    rnd = random.Random(3)
    n = 130
    rows = Rows(rnd, v, n, enc=lambda i: 65 if i % 3 == 0 else 32)
    verdicts, exclude, sent = masks(rnd, n)
    kf, ks = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    with HelperEngine(v, bytes(vkl)) as leader, HelperEngine(v, bytes(vkl)) as helper:
        with rows.encode(leader, verdicts, exclude, fixed=True) as req:
            body = req.body
        with helper.decode_init_req(body, QUERY_FIXED_SIZE, kf, ks) as got:
            assert (got.status, got.n, got.batch_id) == (WIRE_OK, len(sent), BATCH_ID)
            d = {k: got.device_bytes(k).cpu().numpy().tobytes() for k in ("report_ids", "public_shares", "leader_prep_shares",
                                                                          "encs", "payloads", "wire_status")}
            j = lambda xs: b"".join(xs[i] for i in sent)  # noqa: E731
            assert d["report_ids"] == j(rows.ids) and d["public_shares"] == j(rows.ps)
            assert d["leader_prep_shares"] == j(rows.lps) and d["encs"] == j(rows.encs) and d["payloads"] == j(rows.pays)
            assert d["wire_status"] == bytes(len(sent))
            np.testing.assert_array_equal(got.times, rows.times[sent])
            np.testing.assert_array_equal(np.diff(got.enc_offsets), [len(rows.encs[i]) for i in sent])
            np.testing.assert_array_equal(np.diff(got.payload_offsets), [len(rows.pays[i]) for i in sent])
            np.testing.assert_array_equal(got.records["config_id"], rows.cfg[sent])


# ----------------------------------------------------------------------------- 4. response decode equals the object path


def _responses(rnd, rows, sent, pm):
    """A shuffled mix of the four result kinds for the sent reports, and what leader_process_helper_response makes of
    each: (result, error, prep message or None)."""
    kinds = [k % 7 for k in range(len(sent))]
    rnd.shuffle(kinds)
    resps, want = [], []
    for k, i in zip(kinds, sent):
        if k in (0, 1, 2):
            m = rnd.randbytes(pm)
            res, w = PrepareStepResult(0, message=PingPongMessage.finish(m)), (RESP_CONTINUED, WIRE_NO_ERROR, m)
        elif k == 3:
            e = PrepareError(rnd.randrange(10))
            res, w = PrepareStepResult(2, error=e), (RESP_REJECTED, int(e), None)
        elif k == 4:
            res, w = PrepareStepResult(1), (RESP_FINISHED, int(PrepareError.VdafPrepError), None)
        elif k == 5:
            res = PrepareStepResult(0, message=PingPongMessage.finish(rnd.randbytes(pm + 1)))
            w = (RESP_MESSAGE_MISMATCH, int(PrepareError.VdafPrepError), None)
        else:
            res = PrepareStepResult(0, message=PingPongMessage.initialize(rnd.randbytes(pm)))
            w = (RESP_MESSAGE_MISMATCH, int(PrepareError.VdafPrepError), None)
        resps.append(PrepareResp(rows.ids[i], res))
        want.append(w)
    return resps, want


@pytest.mark.parametrize("name", ["sumvec", "count"])
def test_response_decode_equals_the_object_path(name):
    v, vkl = ALL[name]
    rnd = random.Random(4)
    n, pm = 130, v.prep_msg_len
    rows = Rows(rnd, v, n)
    verdicts, exclude, sent = masks(rnd, n)
    resps, want = _responses(rnd, rows, sent, pm)
    # what leader_process_helper_response passes to leader_continued_batch: msgs[row], continued[row]
    msgs, continued = np.zeros((n, max(pm, 1)), np.uint8), np.zeros(n, bool)
    for (res, err, m), i in zip(want, sent):
        if res == RESP_CONTINUED:
            continued[i] = True
            if pm:
                msgs[i, :pm] = np.frombuffer(m, np.uint8)
    stride = pm + 3 if pm else 0
    body = AggregationJobResp(tuple(resps)).encode()
    k = len(sent) // 2
    swapped = list(resps)
    swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    extra = PrepareResp(rnd.randbytes(16), PrepareStepResult(1))
    bad = [(AggregationJobResp(tuple(swapped)).encode(), k), (AggregationJobResp(tuple(resps[:k] + resps[k + 1:])).encode(), k),
           (AggregationJobResp(tuple(resps[:-1])).encode(), len(sent) - 1),
           (AggregationJobResp(tuple(resps[:k] + [extra] + resps[k:])).encode(), k),
           (AggregationJobResp(tuple(resps + [extra])).encode(), len(sent))]
    with HelperEngine(v, bytes(vkl)) as eng, rows.encode(eng, verdicts, exclude) as req:
        d_m = torch.full((n, max(stride, 1)), 0xA5, dtype=torch.uint8, device=DEV)
        d_p = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
        for b, at in bad:
            dec = eng.decode_init_resp(req, b, d_m.data_ptr() if pm else None, d_p.data_ptr(), prep_msg_stride=stride)
            assert (dec.status, dec.mismatch_index) == (WIRE_RESP_MISMATCH, at)
        for cut in (len(body) - 1, 4 + 16, 3):
            dec = eng.decode_init_resp(req, body[:cut], d_m.data_ptr() if pm else None, d_p.data_ptr(), prep_msg_stride=stride)
            assert dec.status == WIRE_MALFORMED and dec.error_offset <= cut
            with pytest.raises(CodecError):
                AggregationJobResp.decode(body[:cut])
        eng.sync()
        assert (d_m.cpu().numpy() == 0xA5).all() and (d_p.cpu().numpy() == 0xA5).all()  # a refused response writes nothing
        dec = eng.decode_init_resp(req, body, d_m.data_ptr() if pm else None, d_p.data_ptr(), prep_msg_stride=stride)
        assert (dec.status, dec.n) == (WIRE_OK, len(sent))
        assert dec.results.tolist() == [w[0] for w in want] and dec.errors.tolist() == [w[1] for w in want]
        got_m, got_p = d_m.cpu().numpy(), d_p.cpu().numpy()
        np.testing.assert_array_equal(got_p == 0, continued)
        assert (got_p[[i for i in range(n) if i not in sent]] != 0).all()  # rows never sent
        if pm:
            np.testing.assert_array_equal(got_m[:, :pm], msgs[:, :pm])
            assert (got_m[:, pm:] == 0xA5).all()  # the stride's padding is not written
        assert {w[0] for w in want} == {RESP_CONTINUED, RESP_REJECTED, RESP_FINISHED, RESP_MESSAGE_MISMATCH}


# ----------------------------------------------------------------------------- 5. both ends through wire bytes

TASK = bytes(range(100, 132))
INFO_L = H.dap_info(recipient=hpke.ROLE_LEADER)
INFO_H = H.dap_info(recipient=hpke.ROLE_HELPER)
E2E = {"count": Prio3.count(), "sum": Prio3.sum(3), "sumvec": Prio3.sum_vec(2, 5, 3), "histogram": Prio3.histogram(3, 2)}


def _tamper_prep_share(p: PrepareInit) -> PrepareInit:
    s = p.message.prep_share
    return PrepareInit(p.report_share, PingPongMessage.initialize(bytes([s[0] ^ 1]) + s[1:]))


@pytest.mark.parametrize("name", list(E2E))
def test_both_ends_through_wire_bytes(name):
    """client.prepare_reports -> handle_upload -> leader_aggregate_init_wire -> (the request body) ->
    handle_aggregate_init_wire -> (the response body) -> leader_process_helper_response_wire, against the object path
    (leader_aggregate_init + handle_aggregate_init_encrypted + leader_process_helper_response) on the same reports
    with fresh engines. The object path has no extension check, so there the report with duplicate extensions carries
    a leader input share one byte short: it fails with the same InvalidMessage under the label
    input_share_decode_failure where the wire path counts duplicate_extension."""
    v = E2E[name]
    vk = bytes(range(16))
    n = 193
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)
    rng = np.random.default_rng(193)
    if v.algo_id == O.COUNT:
        meas = rng.integers(0, 2, size=(n, 1), dtype=np.uint64)
    elif v.algo_id == O.HISTOGRAM:
        meas = rng.integers(0, v.length, size=(n, 1), dtype=np.uint64)
    else:
        meas = rng.integers(0, 1 << v.bits, size=(n, v.length if v.algo_id != O.SUM else 1), dtype=np.uint64)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    ids = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    times = [TIME0 + i for i in range(n)]
    rnd = random.Random(5)
    skl, skh = rnd.randbytes(32), rnd.randbytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    bad_leader, bad_ct, bad_lps, replayed_i, dup_ext = {10, 64, 150}, {20, 63, 128}, {30, 65}, {40, 192}, {50}
    segs = [7 if i % 16 == 3 else 8 for i in range(n)]  # batch 7 was collected
    special = bad_leader | bad_ct | bad_lps | replayed_i | dup_ext
    assert not any(segs[i] == 7 for i in special)
    LIS = v.leader_input_share_len

    def writer():
        w = BatchAggregationWriter(field_bytes=v.field_bytes)
        w.datastore.rows[(7, 0)] = BatchAggregation(7, 0, state=AGGREGATING, field_bytes=v.field_bytes).collected()
        return w

    with hpke.HpkeSealer(pkl, INFO_L) as sl, hpke.HpkeSealer(pkh, INFO_H) as sh, hpke.HpkeOpener(skl, pkl, INFO_L) as ol, \
            hpke.HpkeOpener(skh, pkh, INFO_H) as oh, HelperEngine(v, vk) as leader, HelperEngine(v, vk) as helper, \
            HelperEngine(v, vk) as leader2, HelperEngine(v, vk) as helper2:
        reports = client.prepare_reports(leader, TASK, sl, sh, meas, times, rands=rands, report_ids=ids.tobytes(),
                                         leader_config_id=5, helper_config_id=6)
        shard = leader.shard_batch(meas, ids, rands)
        for i in bad_ct:
            ct = reports[i].helper_encrypted_input_share
            reports[i] = Report(reports[i].metadata, reports[i].public_share, reports[i].leader_encrypted_input_share,
                                HpkeCiphertext(ct.config_id, ct.encapsulated_key, ct.payload[:-1] + bytes([ct.payload[-1] ^ 1])))
        up = handle_upload(leader, UploadTask(TASK, {5: ol}), reports, now=TIME0 + n)
        stored = list(up.results)
        assert not up.status and [s.row for s in stored] == list(range(n))
        for i in bad_leader:  # an element of the leader's measurement share that is no field element
            up.rows[i, :v.field_bytes] = 0xFF
        for i in dup_ext:
            stored[i] = dataclasses.replace(stored[i], extensions=(Extension(0), Extension(0)))
        rid = lambda i: ids[i].tobytes()  # noqa: E731
        replayed = {rid(i) for i in replayed_i}
        sel = PartialBatchSelector.time_interval()

        # ---- the wire path
        w = writer()
        step = leader_aggregate_init_wire(leader, stored, up.rows, up.lis_stride, b"", sel, segs, writer=w)
        not_sent = bad_leader | dup_ext | {i for i in range(n) if segs[i] == 7}
        assert step.stepped == [i for i in range(n) if i not in not_sent] and step.req.n_sent == len(step.stepped)
        req = AggregationJobInitializeReq.decode(step.body, QUERY_TIME_INTERVAL)
        assert [p.report_share.metadata.report_id for p in req.prepare_inits] == [rid(i) for i in step.stepped]
        inits = [_tamper_prep_share(p) if i in bad_lps else p for p, i in zip(req.prepare_inits, step.stepped)]
        body = AggregationJobInitializeReq(b"", sel, tuple(inits)).encode()
        assert len(body) == len(step.body) and body != step.body
        resp_body, hfin, hfail = handle_aggregate_init_wire(helper, body, TASK, oh, 6, QUERY_TIME_INTERVAL, replayed=replayed,
                                                            segment=8)
        out = leader_process_helper_response_wire(leader, step, resp_body, segs, writer=w)
        assert leader.resident_batches()[0] == 0

        # ---- the object path
        rows_host = up.rows.cpu().numpy()
        lreports = [LeaderReport(s.metadata, s.public_share, rows_host[s.row, :LIS - (i in dup_ext)].tobytes(),
                                 s.helper_encrypted_input_share) for i, s in enumerate(stored)]
        w2 = writer()
        step2 = leader_aggregate_init(leader2, lreports, segs, writer=w2)
        assert step2.stepped == step.stepped
        inits2 = [_tamper_prep_share(p) if i in bad_lps else p for p, i in zip(step2.prepare_inits, step2.stepped)]
        assert AggregationJobInitializeReq(b"", sel, tuple(inits2)).encode() == body
        hout = handle_aggregate_init_encrypted(helper2, oh, 6, TASK, inits2, replayed=replayed)
        out2 = leader_process_helper_response(leader2, step2, hout.responses, segs, writer=w2)

        assert resp_body == AggregationJobResp(tuple(hout.responses)).encode()
        np.testing.assert_array_equal(hfin, hout.finished)
        assert hfail == hout.step_failures
        assert out.responses == out2.responses
        np.testing.assert_array_equal(out.finished, out2.finished)
        relabel = lambda c: {("input_share_decode_failure" if k == "duplicate_extension" else k): x for k, x in c.items()}  # noqa: E731
        assert relabel(out.step_failures) == dict(out2.step_failures), (out.step_failures, out2.step_failures)
        assert step.failed == step2.failed
        fin = [i for i in range(n) if i not in not_sent | bad_ct | bad_lps | replayed_i]
        assert np.nonzero(out.finished)[0].tolist() == fin and len(fin) > n // 2
        by_id = {r.report_id: r.result for r in AggregationJobResp.decode(resp_body).prepare_resps}
        assert all(by_id[rid(i)].error == PrepareError.HpkeDecryptError for i in bad_ct)
        assert all(by_id[rid(i)].error == PrepareError.VdafPrepError for i in bad_lps)
        assert all(by_id[rid(i)].error == PrepareError.ReportReplayed for i in replayed_i)
        assert all(step.failed[i] == PrepareError.VdafPrepError for i in bad_leader)
        assert all(step.failed[i] == PrepareError.InvalidMessage for i in dup_ext)
        assert all(step.failed[i] == PrepareError.BatchCollected for i in range(n) if segs[i] == 7)

        # ---- both aggregate shares against the C oracle over exactly the finished reports
        ps = shard.public_shares
        outs = [[orc.prep_init(vk, a, rid(i), ps[i].tobytes(), share[i].tobytes())[2] for i in fin]
                for a, share in ((0, shard.leader_input_shares), (1, shard.helper_input_shares))]
        row_l, row_l2 = w.batch_aggregation(8), w2.batch_aggregation(8)
        agg_h, cnt_h, cs_h = helper.aggregate_share(8)
        assert (row_l.aggregate_share, row_l.report_count) == (orc.aggregate(outs[0]), len(fin))
        assert (row_l2.aggregate_share, row_l2.report_count, row_l2.checksum) == (row_l.aggregate_share, len(fin), row_l.checksum)
        assert (agg_h, cnt_h) == (orc.aggregate(outs[1]), len(fin)) and cs_h == row_l.checksum
        assert helper2.aggregate_share(0) == (agg_h, cnt_h, cs_h)
        if v.algo_id == O.HISTOGRAM:
            sums = [int(np.sum(meas[fin, 0] == b)) for b in range(v.length)]
        else:
            sums = [int(meas[fin, j].astype(object).sum()) for j in range(meas.shape[1])]
        total = v.unshard([row_l.aggregate_share, agg_h], len(fin))
        assert (total if isinstance(total, list) else [total]) == sums


# ----------------------------------------------------------------------------- 6. lifetime


def test_lifetime():
    """The handle released before and after the finish; a second decode on one handle after a refused response; the
    arena's checked-out bytes back at their level after the release."""
    v = Prio3.sum_vec(2, 5, 3)
    vk = bytes(range(16))
    n = 65
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)
    rng = np.random.default_rng(6)
    meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, orc.sizes.client_rand), dtype=np.uint8)
    sh = [orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()) for i in range(n)]
    ps, lis, his = (np.frombuffer(b"".join(s[k] for s in sh), np.uint8).reshape(n, -1) for k in range(3))
    pm, LPS = v.prep_msg_len, v.prep_share_len
    rnd = random.Random(6)
    rows = Rows(rnd, v, n)
    rows.ids, rows.ps = [x.tobytes() for x in nonces], [x.tobytes() for x in ps]
    with HelperEngine(v, vk) as eng:
        for release_first in (True, False):
            d_ids, d_ps, d_lis = dev(nonces), dev(ps), dev(lis)
            d_lps = torch.zeros(n * LPS, dtype=torch.uint8, device=DEV)
            d_v = torch.zeros(n, dtype=torch.uint8, device=DEV)
            bid = eng.leader_init_device(n, d_ids.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(), d_lps.data_ptr(), d_v.data_ptr())
            lps = d_lps.cpu().numpy().reshape(n, LPS)
            level = eng.memory()["arena_in_use"]  # the resident leader batch (and, the second time, the aggregation)
            exclude = np.zeros(n, np.uint8)
            exclude[[5, 64]] = 1
            sent = [i for i in range(n) if not exclude[i]]
            d = rows.device()
            req = eng.encode_init_req(n, d_ids.data_ptr(), rows.times, d_ps.data_ptr(), rows.cfg, d["encs"].data_ptr(),
                                      d["pays"].data_ptr(), rows.poff, d_lps.data_ptr(), d_v.data_ptr(), b"", enc_offsets=rows.eoff,
                                      exclude=exclude)
            rows.lps = [x.tobytes() for x in lps]
            assert req.body == rows.body(sent, b"", False) and not d_v.cpu().numpy().any()
            assert eng.memory()["arena_in_use"] > level
            helper = [orc.helper_prep(vk, rows.ids[i], rows.ps[i], his[i].tobytes(), rows.lps[i]) for i in sent]
            assert all(h[0] == 0 for h in helper)
            resps = [PrepareResp(rows.ids[i], PrepareStepResult(0, message=PingPongMessage.finish(h[1])))
                     for i, h in zip(sent, helper)]
            body = AggregationJobResp(tuple(resps)).encode()
            d_m = torch.zeros((n, pm), dtype=torch.uint8, device=DEV)
            d_p = torch.zeros(n, dtype=torch.uint8, device=DEV)
            d_f = torch.zeros(n, dtype=torch.uint8, device=DEV)
            assert eng.decode_init_resp(req, body[:-1], d_m.data_ptr(), d_p.data_ptr()).status == WIRE_MALFORMED
            assert eng.decode_init_resp(req, AggregationJobResp(tuple(resps[1:])).encode(), d_m.data_ptr(),
                                        d_p.data_ptr()).status == WIRE_RESP_MISMATCH
            assert eng.decode_init_resp(req, body, d_m.data_ptr(), d_p.data_ptr()).status == WIRE_OK
            if release_first:
                req.release()
            eng.leader_finish_device(bid, n, d_m.data_ptr(), d_p.data_ptr(), d_f.data_ptr())
            fv = d_f.cpu().numpy()
            assert (fv[sent] == 0).all() and (fv[[5, 64]] == 5).all()  # never sent: JX_HELPER_STEP_FAILURE
            req.release()
            req.release()  # idempotent
            assert eng.memory()["arena_in_use"] == level  # the handle's memory and every call's scratch are back
            eng.accumulate(n, None, None, batch_id=bid)
            assert eng.aggregate_share(0)[1] == len(sent) * (1 if release_first else 2)
            assert eng.resident_batches()[0] == 0
