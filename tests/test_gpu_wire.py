"""GPU: wire in, wire out (jx_init_req_decode / jx_init_resp_encode, janus_amd.aggregator.handle_aggregate_init_wire):
an AggregationJobInitializeReq body decoded on the device into the arrays the sealed fused call reads, and the
AggregationJobResp body encoded on the device from that call's outputs.

What the decode must give is what janus_amd.messages extracts from the same bytes; which requests it must refuse, and
at which byte, is what the stand-alone host program over the same rule says (tests/test_wire_host.py); the responses
are the reference's per-report loop as tests/test_gpu_encrypted.py restates it (reference_responses), and the
aggregate is the C oracle's over exactly the reports that loop finishes. None comes from the engine.

Shapes: 1, 64, 65 and 193 reports (one lane, a full wave, one past it, and three launches of 64 plus one report);
130 for the duplicate check (two waves and two reports) and the other instances."""
from __future__ import annotations

import random
import struct

import numpy as np
import pytest

import test_gpu_encrypted as E
import test_wire_host as W
from janus_amd import hpke
from janus_amd.aggregator import EmptyAggregation, handle_aggregate_init_wire
from janus_amd.engine import (KEY_NONE, ROUTE_OUT, WIRE_DUPLICATE_ID, WIRE_MALFORMED, WIRE_NO_ERROR, WIRE_OK,
                              WIRE_WRONG_QUERY_TYPE, HelperEngine)
from janus_amd.messages import (QUERY_FIXED_SIZE, QUERY_TIME_INTERVAL, AggregationJobInitializeReq, AggregationJobResp,
                                CodecError, HpkeCiphertext, PartialBatchSelector, PingPongMessage, PrepareError,
                                PrepareInit, PrepareResp, PrepareStepResult, ReportMetadata, ReportShare)
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O
from test_gpu_sealed_fused import INSTANCES, KINDS, _orc

pytestmark = pytest.mark.gpu

INFO = H.dap_info()
MIX = KINDS + ["odd_ps", "finish_msg", "short_enc"]  # 24 kinds
CHUNK = 64
TIME0 = 1_700_000_000


def tables(first: dict, second: dict | None = None):
    kf, ks = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    for c, k in first.items():
        kf[c] = k
    for c, k in (second or {}).items():
        ks[c] = k
    return kf, ks


def request(inits, fixed=False, param=b"agg") -> bytes:
    sel = PartialBatchSelector.fixed_size(bytes(range(100, 132))) if fixed else PartialBatchSelector.time_interval()
    return AggregationJobInitializeReq(param, sel, tuple(inits)).encode()


def random_init(rnd, v, i, enc=32, pay=None, kind=0, ps=None, sh=None, cfg=7, rid=None) -> PrepareInit:
    """A PrepareInit of the instance's lengths filled with random bytes: for tests that only decode."""
    pay = 22 + v.helper_input_share_len if pay is None else pay
    ps = v.public_share_len if ps is None else ps
    sh = v.prep_share_len if sh is None else sh
    msg = PingPongMessage(kind, rnd.randbytes(v.prep_msg_len) if kind else b"", rnd.randbytes(sh) if kind < 2 else b"")
    return PrepareInit(ReportShare(ReportMetadata(rnd.randbytes(16) if rid is None else rid, TIME0 + i), rnd.randbytes(ps),
                                   HpkeCiphertext(cfg, rnd.randbytes(enc), rnd.randbytes(pay))), msg)


def extract(inits, v, kf, ks, deadline=None) -> dict:
    """What janus_amd.messages says the decode's arrays hold."""
    n, PS, LPS = len(inits), v.public_share_len, v.prep_share_len
    out = dict(report_ids=b"".join(p.report_share.metadata.report_id for p in inits),
               times=np.array([p.report_share.metadata.time for p in inits], np.uint64))
    ws, ps, lps, ki, route = [], [], [], [], []
    for p in inits:
        rs, m = p.report_share, p.message
        s = (1 if len(rs.public_share) != PS else 2 if m.kind != PingPongMessage.INITIALIZE else
             3 if len(m.prep_share) != LPS else 0)
        ws.append(s)
        ps.append(rs.public_share if s != 1 else bytes(PS))
        lps.append(m.prep_share if m.kind == 0 and len(m.prep_share) == LPS else bytes(LPS))
        c = rs.encrypted_input_share.config_id
        ki.append((KEY_NONE, KEY_NONE) if s == 1 else (int(kf[c]), int(ks[c])))
        route.append(ROUTE_OUT if s or (deadline is not None and rs.metadata.time > deadline) else 0)
    encs = [p.report_share.encrypted_input_share.encapsulated_key for p in inits]
    pays = [p.report_share.encrypted_input_share.payload for p in inits]
    out.update(wire_status=np.array(ws, np.uint8), public_shares=b"".join(ps), leader_prep_shares=b"".join(lps),
               key_index=np.array(ki, np.uint8).reshape(n, 2), route=np.array(route, np.uint32), encs=b"".join(encs),
               payloads=b"".join(pays),
               enc_offsets=np.concatenate([[0], np.cumsum([len(x) for x in encs])]).astype(np.uint64),
               payload_offsets=np.concatenate([[0], np.cumsum([len(x) for x in pays])]).astype(np.uint64))
    return out


def check_decode(eng, inits, body, kf, ks, deadline=None, query=QUERY_TIME_INTERVAL, what=""):
    v = eng.vdaf
    want = extract(inits, v, kf, ks, deadline)
    n = len(inits)
    with eng.decode_init_req(body, query, kf, ks, deadline) as req:
        assert (req.status, req.n) == (WIRE_OK, n), (what, req.status, req.error_offset)
        dev = {k: req.device_bytes(k).cpu().numpy() for k in ("report_ids", "times", "public_shares", "leader_prep_shares",
                                                              "encs", "enc_offsets", "payloads", "payload_offsets",
                                                              "key_index", "wire_status", "route")}
        assert dev["report_ids"].tobytes() == want["report_ids"], what
        np.testing.assert_array_equal(dev["times"].view(np.uint64), want["times"], err_msg=what)
        assert dev["public_shares"].tobytes() == want["public_shares"], what
        assert dev["leader_prep_shares"].tobytes() == want["leader_prep_shares"], what
        assert dev["encs"].tobytes() == want["encs"] and dev["payloads"].tobytes() == want["payloads"], what
        np.testing.assert_array_equal(dev["enc_offsets"].view(np.uint64), want["enc_offsets"], err_msg=what)
        np.testing.assert_array_equal(dev["payload_offsets"].view(np.uint64), want["payload_offsets"], err_msg=what)
        np.testing.assert_array_equal(dev["key_index"].reshape(n, 2), want["key_index"], err_msg=what)
        np.testing.assert_array_equal(dev["wire_status"], want["wire_status"], err_msg=what)
        np.testing.assert_array_equal(dev["route"].view(np.uint32), want["route"], err_msg=what)
        # the pinned host copy
        np.testing.assert_array_equal(req.times, want["times"])
        np.testing.assert_array_equal(req.enc_offsets, want["enc_offsets"])
        np.testing.assert_array_equal(req.payload_offsets, want["payload_offsets"])
        np.testing.assert_array_equal(req.key_index, want["key_index"])
        np.testing.assert_array_equal(req.wire_status, want["wire_status"])
        assert req.report_ids.tobytes() == want["report_ids"]
        rec = W.expected_records(body, AggregationJobInitializeReq.decode(body, query))
        names = ("off", "len", "public_share_off", "public_share_len", "enc_off", "enc_len", "payload_off", "payload_len",
                 "message_off", "message_len", "prep_msg_off", "prep_msg_len", "prep_share_off", "prep_share_len",
                 "config_id", "ping_pong_type")
        assert [tuple(int(r[k]) for k in names) for r in req.records] == rec, what
        assert req.odd_public_shares == int((want["wire_status"] == 1).sum())
        return req.fallback_iterations, req.batch_id, req.agg_param_span


class Mixed:
    """193 sealed SumVec reports of the 24 kinds with the reference's results; reports 190-192 are valid and, under
    `deadline`, too early."""

    def __init__(self, v, vk, n, seed, late=3):
        rnd = random.Random(seed)
        self.v, self.vk, self.n = v, vk, n
        self.orc = _orc(v)
        self.task_id = rnd.randbytes(32)
        self.kt, self.g7 = E._keypair(rnd), E._keypair(rnd)
        self.kinds = [MIX[i % len(MIX)] for i in range(n)]
        for i in range(n - late, n):
            self.kinds[i] = "valid"
        kind_of = lambda i: self.kinds[i]  # noqa: E731
        self.inits = E._make_inits(rnd, self.orc, v, vk, self.task_id, n, kind_of,
                                   lambda i: self.g7 if kind_of(i) == "global_fallback" else self.kt,
                                   lambda i: 9 if kind_of(i) == "unknown_cfg" else 7, seed=seed, time0=TIME0)
        self.deadline = TIME0 + n - late - 1
        self.keys = {7: [self.kt, self.g7]}
        self.ids = [p.report_share.metadata.report_id for p in self.inits]

    def reference(self, deadline=None, replayed=()):
        want, fin, outs = E.reference_responses(self.orc, self.vk, self.v, self.task_id, self.keys, self.inits,
                                                deadline=deadline)
        fin = fin.copy()
        for i in range(self.n):
            if fin[i] and self.ids[i] in replayed:  # aggregator.rs:2127-2132
                want[i] = PrepareResp(self.ids[i], PrepareStepResult(2, error=PrepareError.ReportReplayed))
                fin[i] = False
        idx = [i for i in range(self.n) if fin[i]]
        agg = self.orc.aggregate([outs[i] for i in idx]) if idx else bytes(self.orc.sizes.output_len * self.orc.sizes.field_bytes)
        cs = bytes(32)
        for i in idx:
            cs = bytes(a ^ b for a, b in zip(cs, O.sha256(self.ids[i])))
        return want, fin, (agg, len(idx), cs)

    def openers(self):
        return hpke.HpkeOpener(*self.kt, INFO), hpke.HpkeOpener(*self.g7, INFO)


@pytest.fixture(scope="module")
def mixed():
    m = Mixed(Prio3.sum_vec(8, 100, 10), bytes(range(11, 27)), 193, seed=1193)
    assert {"odd_ps", "finish_msg", "short_enc", "too_early"} - set(m.kinds) == {"too_early"}
    assert len({len(p.encode()) for p in m.inits}) >= 5  # irregular boundaries
    return m


# ----------------------------------------------------------------------------- 1. decode


@pytest.mark.parametrize("n", [1, 64, 65, 193])
def test_decode_uniform_and_mixed(mixed, n):
    """Every device array, both offset arrays and key_index equal what messages.py extracts: a uniform request (no
    fallback iteration), and the first n of the 24-kind mix (the fallback loop runs as soon as two lengths differ)."""
    v = mixed.v
    rnd = random.Random(n)
    kf, ks = tables({7: 0, 11: 2}, {7: 1})
    with HelperEngine(v, mixed.vk) as eng:
        uni = [random_init(rnd, v, i, cfg=(7, 11, 9)[i % 3]) for i in range(n)]
        iters, bid, span = check_decode(eng, uni, request(uni, fixed=True, param=b"0123456"), kf, ks, query=QUERY_FIXED_SIZE,
                                        deadline=TIME0 + n // 2, what=f"uniform {n}")
        assert iters == 0 and bid == bytes(range(100, 132)) and span == (4, 7)
        sub = mixed.inits[:n]
        iters, bid, span = check_decode(eng, sub, request(sub), kf, ks, what=f"mixed {n}")
        print(f"n={n}: mixed body, {iters} fallback iterations")
        assert (iters > 0) == (len({len(p.encode()) for p in sub}) > 1) and bid is None and span == (4, 3)


def test_decode_alternating_kems():
    """A P-256 and an X25519 report alternating (65- and 32-byte encapsulated keys): the fallback loop takes them a
    wave's worth at a time; payloads that grow by a byte each are its worst case, one message per iteration; and a
    request without reports."""
    v = Prio3.sum_vec(8, 100, 10)
    rnd = random.Random(65)
    kf, ks = tables({7: 1, 8: 0}, {7: 0, 8: 1})
    n = 130
    inits = [random_init(rnd, v, i, enc=65 if i % 2 else 32, cfg=7 if i % 2 else 8) for i in range(n)]
    with HelperEngine(v, bytes(16)) as eng:
        iters, _, _ = check_decode(eng, inits, request(inits), kf, ks, what="alternating")
        assert iters == 3  # message 0 by the fast pass, then 64 + 64 + 1
        grow = [random_init(rnd, v, i, pay=70 + i) for i in range(n)]
        iters, _, _ = check_decode(eng, grow, request(grow), kf, ks, what="growing")
        assert iters == n - 1
        with eng.decode_init_req(request([]), QUERY_TIME_INTERVAL, kf, ks) as req:
            assert (req.status, req.n, req.fallback_iterations) == (WIRE_OK, 0, 0)
            body, fin = eng.encode_init_resp(req, None, None, None)
            assert body == bytes(4) and fin.shape == (0,)


# ----------------------------------------------------------------------------- 2. request errors


def test_request_errors_match_the_host_program(tmp_path):
    """One body of each malformed kind at n = 65, the corruption in message 0, 63, 64 and the last: the status and the
    byte offset the device reports are the stand-alone host program's, and the engine's aggregations do not move."""
    v = Prio3.sum_vec(8, 100, 10)
    rnd = random.Random(2)
    n = 65
    inits = [random_init(rnd, v, i) for i in range(n)]
    body = request(inits)
    req0 = AggregationJobInitializeReq.decode(body, QUERY_TIME_INTERVAL)
    recs = W.expected_records(body, req0)
    voff = 4 + 3 + 1
    vl = struct.unpack(">I", body[voff:voff + 4])[0]
    bad: list[tuple[int, bytes, str]] = [(1, body + b"\0", "trailing"), (2, body, "wrong_query"),
                                         (1, body[:voff] + struct.pack(">I", vl + 1) + body[voff + 4:], "veclen+1"),
                                         (1, body[:voff] + struct.pack(">I", vl - 1) + body[voff + 4:], "veclen-1"),
                                         (1, body[:-1], "short")]
    for k in (0, 63, 64):
        r = recs[k]
        off, ln, ps_off, enc_off, pay_off, msg_off, msg_len = r[0], r[1], r[2], r[4], r[6], r[8], r[9]
        for d in (-1, 1):
            bad.append((1, body[:msg_off - 4] + struct.pack(">I", msg_len + d) + body[msg_off:], f"msglen{d:+d}@{k}"))
            inner = struct.unpack(">I", body[msg_off + 1:msg_off + 5])[0]
            bad.append((1, body[:msg_off + 1] + struct.pack(">I", inner + d) + body[msg_off + 5:], f"inner{d:+d}@{k}"))
        bad.append((1, body[:msg_off] + b"\x03" + body[msg_off + 1:], f"type3@{k}"))
        for at, w in ((ps_off - 4, 4), (enc_off - 2, 2), (pay_off - 4, 4), (msg_off - 4, 4), (msg_off + 1, 4)):
            bad.append((1, body[:at] + b"\xff" * w + body[at + w:], f"ff@{at}/{k}"))
        for cut in (off + 16, ps_off, enc_off + 5, pay_off + 1, msg_off, msg_off + 3):  # message k cut short, the
            short = body[:cut]                                                          # vector length made to fit
            bad.append((1, short[:voff] + struct.pack(">I", len(short) - voff - 4) + short[voff + 4:], f"cut{cut}@{k}"))
    host = W.run_bodies([(q, b) for q, b, _ in bad], tmp_path, sanitize=False)
    kf, ks = tables({7: 0})
    with HelperEngine(v, bytes(16)) as eng:
        before = eng.aggregate_share(0)
        seen = set()
        for (q, b, name), h in zip(bad, host):
            assert h["walk"][0] != 0, name
            with pytest.raises(CodecError):
                AggregationJobInitializeReq.decode(b, q)
            with eng.decode_init_req(b, q, kf, ks) as req:
                assert (req.status, req.error_offset) == (h["walk"][0], h["walk"][1]), (name, h)
                assert req.status in (WIRE_MALFORMED, WIRE_WRONG_QUERY_TYPE) and req.d is None
                seen.add(req.status)
        assert seen == {WIRE_MALFORMED, WIRE_WRONG_QUERY_TYPE}
        with hpke.HpkeOpener(*E._keypair(rnd), INFO) as op:
            with pytest.raises(CodecError, match="malformed at byte"):
                handle_aggregate_init_wire(eng, bad[-1][1], bytes(32), op, 7, QUERY_TIME_INTERVAL)
            with pytest.raises(EmptyAggregation):
                handle_aggregate_init_wire(eng, request([]), bytes(32), op, 7, QUERY_TIME_INTERVAL)
        assert eng.aggregate_share(0) == before and eng.resident_batches()[0] == 0


# ----------------------------------------------------------------------------- 3. duplicates


def _dup_cases(rnd):
    n = 130
    base = [rnd.randbytes(16) for _ in range(n)]

    def with_(edits):
        ids = list(base)
        for i, j in edits:
            ids[i] = ids[j] if isinstance(j, int) else j
        return ids

    z = bytes(16)
    return {
        "none": base,
        "pair_in_a_wave": with_([(40, 12)]),
        "pair_70_apart": with_([(99, 29)]),
        "three_equal": with_([(17, 5), (120, 5)]),
        "prefix_or_suffix_only": with_([(50, base[3][:8] + base[50][8:]), (51, base[51][:8] + base[3][8:])]),
        "one_zero_id": with_([(77, z)]),
        "two_zero_ids": with_([(77, z), (128, z)]),
        "all_equal": [base[0]] * n,
        "two_pairs": with_([(129, 0), (64, 63)]),
    }


def test_duplicate_report_ids():
    """The reported index is the lowest i with an equal id at a lower index, or none (then the request decodes)."""
    v = Prio3.count()
    rnd = random.Random(3)
    kf, ks = tables({7: 0})
    with HelperEngine(v, bytes(16)) as eng:
        for name, ids in _dup_cases(rnd).items():
            first = {}
            want = next((i for i, x in enumerate(ids) if first.setdefault(x, i) != i), None)
            inits = [random_init(rnd, v, i, rid=rid) for i, rid in enumerate(ids)]
            for rep in range(3 if name == "three_equal" else 1):  # the answer does not depend on which lane came first
                with eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, kf, ks) as req:
                    if want is None:
                        assert (req.status, req.n) == (WIRE_OK, 130), name
                    else:
                        assert (req.status, req.duplicate_index, req.n) == (WIRE_DUPLICATE_ID, want, 130), name
        with hpke.HpkeOpener(*E._keypair(rnd), INFO) as op:
            inits = [random_init(rnd, v, i, rid=rid) for i, rid in enumerate(_dup_cases(rnd)["pair_70_apart"])]
            with pytest.raises(ValueError, match="duplicate report IDs.*report 99"):
                handle_aggregate_init_wire(eng, request(inits), bytes(32), op, 7, QUERY_TIME_INTERVAL)
        assert eng.aggregate_share(0)[1] == 0


# ----------------------------------------------------------------------------- 4. wire in, wire out


def _wire_in_wire_out(m: Mixed, P: int):
    replayed = {m.ids[i] for i in [i for i in range(m.n) if m.kinds[i] == "valid"][1:3]}
    want, fin, agg = m.reference(deadline=m.deadline, replayed=replayed)
    early = [i for i in range(m.n) if m.inits[i].report_share.metadata.time > m.deadline]
    assert len(early) == 3 and all(want[i].result.error == PrepareError.ReportTooEarly for i in early)
    assert sum(w.result.kind == 2 and w.result.error == PrepareError.ReportReplayed for w in want) == 2
    ot, o7 = m.openers()
    eng = HelperEngine(m.v, m.vk)
    try:
        eng.debug(5, CHUNK)
        eng.debug(4, P)
        body, got_fin, failures = handle_aggregate_init_wire(eng, request(m.inits), m.task_id, ot, 7, QUERY_TIME_INTERVAL,
                                                             global_keypairs={7: o7}, report_deadline=m.deadline,
                                                             replayed=replayed, segment=5)
        resp = AggregationJobResp.decode(body)
        for i, (g, w) in enumerate(zip(resp.prepare_resps, want)):
            assert g == w, (i, m.kinds[i], g, w)
        assert body == AggregationJobResp(tuple(want)).encode()
        np.testing.assert_array_equal(got_fin, fin)
        assert eng.aggregate_share(5) == agg and fin.sum() == agg[1] > 0
        print(f"{m.n} reports: {int(fin.sum())} finished; failures {dict(failures)}")
        assert failures["public_share_decode_failure"] == m.kinds.count("odd_ps")
        assert failures["leader_ping_pong_message_mismatch"] == m.kinds.count("finish_msg")
        assert failures["decrypt_failure"] >= m.kinds.count("short_enc") + m.kinds.count("corrupt_ct")
        assert eng.resident_batches()[0] == 0
    finally:
        eng.close()
        ot.close()
        o7.close()


def test_wire_in_wire_out(mixed):
    """193 reports at 64 per launch over two pipelines, the 24 kinds, three reports too early and two replayed: the
    response body equals u32 len || the reference's PrepareResps byte for byte, the finished mask is the reference's,
    and the aggregation holds exactly the reports the reference finishes and does not mark replayed."""
    _wire_in_wire_out(mixed, 2)


@pytest.mark.parametrize("name", ["count", "multiproof"])
def test_wire_in_wire_out_instances(name):
    """The same for Count (no public share, S = 0) and the multiproof instance (S = 32) at n = 130."""
    v, vkl = INSTANCES[name]
    _wire_in_wire_out(Mixed(v, bytes(range(5, 5 + vkl)), 130, seed=sum(map(ord, name))), 2)


# ----------------------------------------------------------------------------- 5. encode alone


@pytest.mark.parametrize("name", ["sumvec", "count"])
def test_encode_alone(name):
    """Hand-set verdicts, open statuses, host-resolved errors and a replayed mask over a request whose reports have
    every wire_status, covering every row of the precedence table and the pairs that decide its order."""
    import torch

    v = Prio3.sum_vec(8, 100, 10) if name == "sumvec" else Prio3.count()
    S = v.prep_msg_len
    rnd = random.Random(5)
    n = 65
    kind = {10: 2, 11: 2, 12: 2, 13: 2, 14: 2}                 # not Initialize: wire_status 2
    odd_sh = {20, 21, 22}                                       # prep share of another length: 3
    odd_ps = {30, 31}                                           # public share of another length: 1
    inits = [random_init(rnd, v, i, kind=kind.get(i, 0), sh=v.prep_share_len + 1 if i in odd_sh else None,
                         ps=v.public_share_len + 2 if i in odd_ps else None) for i in range(n)]
    deadline = TIME0 + 59                                       # reports 60..64 are too early
    verdict = np.zeros(n, np.uint8)
    opened = np.zeros(n, np.uint8)
    override = np.full(n, WIRE_NO_ERROR, np.uint8)
    replayed = np.zeros(n, bool)
    for i, st in enumerate([1, 2, 3, 4, 5, 6, 7]):
        opened[i] = st                                          # rows 2: every open status
        verdict[i] = 6
    verdict[[8, 9, 40]] = [1, 3, 4]                             # row 5
    replayed[[41, 42, 8, 10, 20, 60, 1]] = True                 # row 6, and under rows 5, 4, 4, 3, 2
    opened[[11, 21, 61]] = [1, 7, 2]                            # open status over wire_status and too early
    verdict[[12, 22, 62]] = 2                                   # rows 4 / 3 whatever the verdict says
    override[[30, 31]] = [int(PrepareError.InvalidMessage), int(PrepareError.HpkeDecryptError)]  # row 1
    opened[[30, 31]] = 7                                        # as the device leaves a report it cannot carry
    override[43] = int(PrepareError.BatchCollected)             # row 1 over a finished report
    msgs = np.frombuffer(rnd.randbytes(n * max(S, 1)), np.uint8).reshape(n, max(S, 1))
    want = []
    for i, p in enumerate(inits):
        ws = 1 if i in odd_ps else 2 if i in kind else 3 if i in odd_sh else 0
        if override[i] != WIRE_NO_ERROR:
            err = PrepareError(int(override[i]))
        elif opened[i]:
            err = {1: PrepareError.HpkeDecryptError, 7: PrepareError.HpkeUnknownConfigId}.get(int(opened[i]),
                                                                                              PrepareError.InvalidMessage)
        elif p.report_share.metadata.time > deadline:
            err = PrepareError.ReportTooEarly
        elif ws in (2, 3) or verdict[i]:
            err = PrepareError.VdafPrepError
        elif replayed[i]:
            err = PrepareError.ReportReplayed
        else:
            err = None
        res = (PrepareStepResult(2, error=err) if err is not None else
               PrepareStepResult(0, message=PingPongMessage.finish(msgs[i, :S].tobytes())))
        want.append(PrepareResp(p.report_share.metadata.report_id, res))
    errs = {w.result.error for w in want if w.result.kind == 2}
    assert errs == {PrepareError.InvalidMessage, PrepareError.HpkeDecryptError, PrepareError.HpkeUnknownConfigId,
                    PrepareError.ReportTooEarly, PrepareError.VdafPrepError, PrepareError.ReportReplayed,
                    PrepareError.BatchCollected}
    kf, ks = tables({7: 0})
    dev = torch.device("cuda", 0)
    with HelperEngine(v, bytes(16)) as eng, eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, kf, ks, deadline) as req:
        assert req.status == WIRE_OK and req.odd_public_shares == 2
        d_v, d_o, d_m = (torch.from_numpy(a.copy()).to(dev) for a in (verdict, opened, msgs))
        body, fin = eng.encode_init_resp(req, d_v.data_ptr(), d_o.data_ptr(), d_m.data_ptr() if S else None, override,
                                         replayed, prep_msg_stride=max(S, 1) if S else 0)
        assert body == AggregationJobResp(tuple(want)).encode()
        np.testing.assert_array_equal(fin, [w.result.kind == 0 for w in want])
        # the device form: the same bytes in a device buffer, and a buffer one byte short is refused
        d_out = torch.zeros(len(body), dtype=torch.uint8, device=dev)
        d_fin = torch.zeros(n, dtype=torch.uint8, device=dev)
        ln = eng.encode_init_resp(req, d_v.data_ptr(), d_o.data_ptr(), d_m.data_ptr() if S else None, override, replayed,
                                  prep_msg_stride=max(S, 1) if S else 0, d_out=d_out.data_ptr(), capacity=len(body),
                                  d_out_finished=d_fin.data_ptr())
        assert ln == len(body) and d_out.cpu().numpy().tobytes() == body
        np.testing.assert_array_equal(d_fin.cpu().numpy().astype(bool), fin)
        from janus_amd._lib import EngineError
        with pytest.raises(EngineError, match=r"\(-1\)"):
            eng.encode_init_resp(req, d_v.data_ptr(), d_o.data_ptr(), d_m.data_ptr() if S else None, override, replayed,
                                 prep_msg_stride=max(S, 1) if S else 0, d_out=d_out.data_ptr(), capacity=len(body) - 1)
