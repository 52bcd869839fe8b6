"""GPU: a decoded request's reports routed to their batch buckets on the device (jx_init_req_route, InitReq.route,
janus_amd.aggregator.handle_aggregate_init_wire_buckets).

What the route must give is the Python model of tests/test_wire_route_host.py (the sorted set of t - t % P, per bucket
the minimum, the maximum and the counts), which that file also holds the kernels' CPU replay to; the end-to-end
responses are tests/test_gpu_wire.py's reference with BatchCollected put where the writer of the reference puts it
(aggregation_job_writer.rs:608-708), and the aggregates are the C oracle's per bucket. None comes from the engine.

Shapes: 1, 64, 65 and 193 reports (one lane, a full wave, one past it, three waves and a report) with the bucket
edges on wave edges (P = 64), inside waves (P = 50) and nowhere (P = 3600); 130 reports each in a bucket of its own,
descending, for the sort; 2,100 reports over 1,024 and 1,025 buckets for the cap. The decode-only bodies are
Prio3Count's, the smallest there are."""
from __future__ import annotations

import random

import numpy as np
import pytest

import test_gpu_encrypted as E
import test_gpu_wire as G
from janus_amd._lib import EngineError
from janus_amd.aggregator import TooManyBuckets, handle_aggregate_init_wire_buckets
from janus_amd.engine import ROUTE_MAX_BUCKETS, ROUTE_OK, ROUTE_OUT, WIRE_MALFORMED, HelperEngine
from janus_amd.messages import (QUERY_FIXED_SIZE, QUERY_TIME_INTERVAL, AggregationJobResp, PingPongMessage, PrepareError,
                                PrepareInit, PrepareResp, PrepareStepResult, ReportMetadata, ReportShare)
from janus_amd.vdaf import Prio3
from oracle import oracle as O
from test_gpu_wire import TIME0, mixed, random_init, request, tables  # noqa: F401  (mixed: the module's fixture)
from test_wire_route_host import EDGE_PRECISIONS, EDGE_TIMES, route_model

pytestmark = pytest.mark.gpu

KF, KS = tables({7: 0})
assert TIME0 % 64 == 0 and TIME0 % 50 == 0 and TIME0 % 3600 + 192 < 3600


@pytest.fixture(scope="module")
def eng():
    with HelperEngine(Prio3.count(), bytes(16)) as e:
        yield e


def at_time(p: PrepareInit, t: int) -> PrepareInit:
    rs = p.report_share
    return PrepareInit(ReportShare(ReportMetadata(rs.metadata.report_id, t), rs.public_share, rs.encrypted_input_share),
                       p.message)


def count_inits(seed: int, times, special=None) -> list[PrepareInit]:
    """Prio3Count PrepareInits of random bytes with the given times; special: index -> random_init keyword arguments."""
    rnd = random.Random(seed)
    v, special = Prio3.count(), special or {}
    return [at_time(random_init(rnd, v, i, **special.get(i, {})), t) for i, t in enumerate(times)]


def dev_u32(req, name):
    return req.device_bytes(name).cpu().numpy().view(np.uint32).astype(np.int64).tolist()


def check_route(req, times, P, collected=(), what=""):
    """Route req and hold everything the call gives to the model, from the route the handle had before."""
    before = dev_u32(req, "route")
    w_status, w_rows, w_route, w_index, w_col = route_model(list(times), before, P, list(collected))
    status, table = req.route(P, collected)
    assert status == w_status, what
    assert dev_u32(req, "route") == w_route, what
    if status != ROUTE_OK:
        assert len(table) == 0
        return before, table
    got = [tuple(int(b[k]) for k in ("start", "min_time", "max_time", "reports", "routed", "collected")) for b in table]
    assert got == w_rows, what
    assert dev_u32(req, "bucket_index") == w_index, what
    assert req.device_bytes("bucket_collected").cpu().numpy().tolist() == w_col, what
    return before, table


# ----------------------------------------------------------------------------- 1. sizes and bucket shapes


@pytest.mark.parametrize("n", [1, 64, 65, 193])
def test_route_sizes_and_bucket_edges(eng, n):
    times = [TIME0 + i for i in range(n)]
    inits = count_inits(n, times)
    for P, buckets in ((64, (n + 63) // 64), (50, (n + 49) // 50), (3600, 1)):
        with eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, KF, KS) as req:
            before, table = check_route(req, times, P, what=f"n={n} P={P}")
            assert not any(before) and len(table) == buckets and int(table["routed"].sum()) == n


def test_route_every_report_its_own_bucket_descending(eng):
    n = 130
    times = [TIME0 + n - 1 - i for i in range(n)]
    with eng.decode_init_req(request(count_inits(130, times)), QUERY_TIME_INTERVAL, KF, KS) as req:
        _, table = check_route(req, times, 1, what="descending")
        assert len(table) == n and dev_u32(req, "route") == list(range(n - 1, -1, -1))


def test_route_empty_request(eng):
    with eng.decode_init_req(request([]), QUERY_TIME_INTERVAL, KF, KS) as req:
        status, table = req.route(3600)
        assert status == ROUTE_OK and len(table) == 0


# ----------------------------------------------------------------------------- 2. the cap


def _encode_zeros(eng, req, n):
    import torch

    d_v = torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda", eng.device))
    d_o = torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda", eng.device))
    return eng.encode_init_resp(req, d_v.data_ptr(), d_o.data_ptr(), None)


def test_route_at_and_past_the_cap(eng):
    """2,100 reports over exactly 1,024 buckets route; over 1,025 the call says so and leaves route, the handle and
    the response encode as they were: the handle can still be routed, with a precision that gives fewer buckets."""
    n = 2100
    for distinct in (ROUTE_MAX_BUCKETS, ROUTE_MAX_BUCKETS + 1):
        times = [TIME0 + (i % distinct) * 10 + i // distinct for i in range(n)]
        assert len({t - t % 10 for t in times}) == distinct
        inits = count_inits(distinct, times, {5: dict(kind=2)})
        with eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, KF, KS) as req:
            unrouted = _encode_zeros(eng, req, n)
            raw = req.device_bytes("route").cpu().numpy().tobytes()
            before, table = check_route(req, times, 10, [TIME0 + 10], what=f"{distinct} buckets")
            assert before[5] == ROUTE_OUT and sum(before) == ROUTE_OUT
            if distinct == ROUTE_MAX_BUCKETS:
                assert len(table) == distinct
                continue
            assert req.device_bytes("route").cpu().numpy().tobytes() == raw
            with pytest.raises(EngineError, match=r"\(-5\)"):  # not routed: there are no per-report arrays
                req.device_bytes("bucket_index")
            again = _encode_zeros(eng, req, n)
            assert again[0] == unrouted[0] and np.array_equal(again[1], unrouted[1])
            check_route(req, times, 1 << 20, what="routed after a refusal")


# ----------------------------------------------------------------------------- 3. the u64 edges


@pytest.mark.parametrize("P", EDGE_PRECISIONS)
def test_route_u64_edges(eng, P):
    """The time field's eight bytes at 0, P - 1, P, P + 1, 2^63, 2^64 - 2 and 2^64 - 1, through real bodies."""
    times = EDGE_TIMES(P) * 2
    with eng.decode_init_req(request(count_inits(P & 0xFFFF, times)), QUERY_TIME_INTERVAL, KF, KS) as req:
        assert req.times.tolist() == times
        check_route(req, times, P, [0, (1 << 63) - (1 << 63) % P], what=f"P={P}")


# ----------------------------------------------------------------------------- 4. earlier exclusions


def test_route_keeps_earlier_exclusions(eng):
    """A report the decode (not Initialize, a prep share of another length, past the deadline) or exclude() routed out
    counts in its bucket's reports and widens its interval, is not routed, and stays out; exclude() after the route
    still routes out."""
    n = 130
    v = Prio3.count()
    times = [TIME0 + i for i in range(n)]
    special = {0: dict(kind=2), 49: dict(sh=v.prep_share_len + 1), 50: dict(kind=2), 99: dict(kind=1)}
    inits = count_inits(4, times, special)
    deadline = TIME0 + 127  # 128 and 129, the last bucket's maximum, are too early
    mask = np.zeros(n, bool)
    mask[[100, 101, 64]] = True
    out_before = sorted([0, 49, 50, 99, 128, 129, 100, 101, 64])
    with eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, KF, KS, deadline) as req:
        req.exclude(mask)
        before, table = check_route(req, times, 50, what="exclusions")
        assert [i for i in range(n) if before[i]] == out_before
        assert table["reports"].tolist() == [50, 50, 30] and table["routed"].tolist() == [48, 47, 26]
        assert table["min_time"].tolist() == [TIME0, TIME0 + 50, TIME0 + 100]  # 0, 50 and 100 are excluded reports
        assert table["max_time"].tolist() == [TIME0 + 49, TIME0 + 99, TIME0 + 129]
        after = np.zeros(n, bool)
        after[[7, 0]] = True
        req.exclude(after)
        route = dev_u32(req, "route")
        assert [i for i in range(n) if route[i] == ROUTE_OUT] == sorted(out_before + [7])
        assert all(route[i] == i // 50 for i in range(n) if route[i] != ROUTE_OUT)


# ----------------------------------------------------------------------------- 5. collected


def test_route_collected(eng):
    n = 193
    times = [TIME0 + i for i in range(n)]
    starts = [TIME0, TIME0 + 50, TIME0 + 100, TIME0 + 150]
    inits = count_inits(5, times)
    body = request(inits)
    cases = {"none": [], "all": starts, "subset": starts[1:3], "no_bucket": [TIME0 + 1, TIME0 + 200, 0, (1 << 64) - 1],
             "unsorted_repeats": [starts[3], starts[0], starts[3], 5, starts[0]]}
    for name, collected in cases.items():
        with eng.decode_init_req(body, QUERY_TIME_INTERVAL, KF, KS) as req:
            _, table = check_route(req, times, 50, collected, what=name)
            assert table["collected"].tolist() == [int(s in collected) for s in starts], name
            # the encode over a routed handle: BatchCollected for the otherwise finished reports of a collected bucket
            out, fin = _encode_zeros(eng, req, n)
            want = [PrepareResp(p.report_share.metadata.report_id,
                                PrepareStepResult(2, error=PrepareError.BatchCollected)
                                if starts[i // 50] in collected else
                                PrepareStepResult(0, message=PingPongMessage.finish(b"")))
                    for i, p in enumerate(inits)]
            assert out == AggregationJobResp(tuple(want)).encode(), name
            assert fin.tolist() == [starts[i // 50] not in collected for i in range(n)], name


# ----------------------------------------------------------------------------- 6. refusals


def test_route_refusals(eng):
    times = [TIME0 + i for i in range(3)]
    inits = count_inits(6, times)
    with eng.decode_init_req(request(inits), QUERY_TIME_INTERVAL, KF, KS) as req:
        with pytest.raises(EngineError, match=r"\(-1\).*precision"):
            req.route(0)
        assert req.route(50)[0] == ROUTE_OK
        with pytest.raises(EngineError, match=r"\(-5\).*routed already"):
            req.route(50)
    with eng.decode_init_req(request(inits, fixed=True), QUERY_FIXED_SIZE, KF, KS) as req:
        with pytest.raises(EngineError, match=r"\(-1\).*FixedSize"):
            req.route(50)
    with eng.decode_init_req(request(inits)[:-1], QUERY_TIME_INTERVAL, KF, KS) as req:
        assert req.status == WIRE_MALFORMED
        with pytest.raises(EngineError, match=r"\(-5\).*refused"):
            req.route(50)


# ----------------------------------------------------------------------------- 7. end to end


def test_wire_buckets_end_to_end(mixed):  # noqa: F811
    """193 sealed SumVec reports of the 24 kinds at 64 per launch, P = 50, the second bucket collected, two finished
    reports replayed (one of them in the collected bucket), three too early: the response body is the reference's with
    BatchCollected in place of exactly the reports that finished in the collected bucket, and every open bucket's
    aggregation holds exactly the oracle's aggregate of the reports finished there; the collected one holds none."""
    m = mixed
    P = 50
    bucket = [i // P for i in range(m.n)]
    valid = [i for i in range(m.n) if m.kinds[i] == "valid"]
    rep_idx = [next(i for i in valid if bucket[i] == 1), next(i for i in valid if bucket[i] == 2)]
    replayed = {m.ids[i] for i in rep_idx}
    want, fin, outs = E.reference_responses(m.orc, m.vk, m.v, m.task_id, m.keys, m.inits, deadline=m.deadline)
    fin = fin.copy()
    assert all(fin[i] for i in rep_idx)
    for i in rep_idx:  # aggregator.rs:2127-2132: marked before the writer runs
        want[i] = PrepareResp(m.ids[i], PrepareStepResult(2, error=PrepareError.ReportReplayed))
        fin[i] = False
    lost = [i for i in range(m.n) if fin[i] and bucket[i] == 1]
    failed_there = [i for i in range(m.n) if bucket[i] == 1 and not fin[i]]
    assert len(lost) > 5 and len({want[i].result.error for i in failed_there}) >= 3
    for i in lost:  # aggregation_job_writer.rs:608-708
        want[i] = PrepareResp(m.ids[i], PrepareStepResult(2, error=PrepareError.BatchCollected))
        fin[i] = False
    assert sum(w.result.kind == 2 and w.result.error == PrepareError.ReportTooEarly for w in want) == 3
    seg = {TIME0 + P * k: 5 + 3 * k for k in range(4)}
    ot, o7 = m.openers()
    eng = HelperEngine(m.v, m.vk)
    try:
        eng.debug(5, G.CHUNK)
        eng.debug(4, 2)
        body, got_fin, failures, table = handle_aggregate_init_wire_buckets(
            eng, request(m.inits), m.task_id, ot, 7, P, seg.__getitem__, collected=[TIME0 + P, 17],
            global_keypairs={7: o7}, report_deadline=m.deadline, replayed=replayed)
        resp = AggregationJobResp.decode(body)
        for i, (g, w) in enumerate(zip(resp.prepare_resps, want)):
            assert g == w, (i, m.kinds[i], g, w)
        assert body == AggregationJobResp(tuple(want)).encode()
        np.testing.assert_array_equal(got_fin, fin)
        assert table["start"].tolist() == sorted(seg) and table["collected"].tolist() == [0, 1, 0, 0]
        assert table["reports"].tolist() == [50, 50, 50, 43] and table["routed"].tolist()[1] == 0
        assert table["max_time"].tolist()[3] == TIME0 + 192  # a report that is too early still widens the interval
        size = m.orc.sizes.output_len * m.orc.sizes.field_bytes
        for k in range(4):
            idx = [i for i in range(m.n) if fin[i] and bucket[i] == k]
            agg = m.orc.aggregate([outs[i] for i in idx]) if idx else bytes(size)
            cs = bytes(32)
            for i in idx:
                cs = bytes(a ^ b for a, b in zip(cs, O.sha256(m.ids[i])))
            assert eng.aggregate_share(seg[TIME0 + P * k]) == (agg, len(idx), cs), k
            assert (len(idx) == 0) == (k == 1)
        assert failures["leader_ping_pong_message_mismatch"] == m.kinds.count("finish_msg")
        assert eng.resident_batches()[0] == 0
        # a request of more buckets than the route holds queues nothing
        before = eng.aggregate_share(5)
        wide = [at_time(random_init(random.Random(i), m.v, i), TIME0 + i) for i in range(ROUTE_MAX_BUCKETS + 1)]
        with pytest.raises(TooManyBuckets):
            handle_aggregate_init_wire_buckets(eng, request(wide), m.task_id, ot, 7, 1, seg.__getitem__)
        assert eng.aggregate_share(5) == before and eng.resident_batches()[0] == 0
    finally:
        eng.close()
        ot.close()
        o7.close()
