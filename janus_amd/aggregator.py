"""Helper aggregate-init over a batch of PrepareInits — the hot loop of Janus, batched.

Mirror of VdafOps::handle_aggregate_init_generic, /root/reference/aggregator/src/
aggregator.rs:1712-2161, minus the datastore transaction itself (:2051-2156).
handle_aggregate_init_encrypted starts from the encrypted report shares (the HPKE open runs inside the
prepare launch on the GPU); handle_aggregate_init from opened ones. Per report, the reference:
  * decodes the helper input share and public share -> PrepareError::InvalidMessage on
    failure (:1896-1926),
  * runs helper_initialized + evaluate (:1945-1967); any PingPongError becomes
    PrepareError::VdafPrepError via handle_ping_pong_error (error.rs:365-427),
  * answers PrepareStepResult::Continue{Finish{prep_msg}} or Reject(error) (:1969-1993),
  * later fails replayed reports with ReportReplayed (:2101-2136) and accumulates the
    rest into batch aggregations (aggregation_job_writer.rs:608-708).
Here the per-report prio call is one engine batch call that leaves a resident batch (one
per aggregation job in flight), and accumulation is one masked, segmented device reduction:
with a BatchAggregationWriter, into per-batch-identifier deltas merged inside a retryable
datastore transaction (aggregation_job_writer.rs:476-553, 608-708); without one, into the
engine's running aggregations.
"""
from __future__ import annotations

import enum
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from .batch_aggregation import AGGREGATING, SCRUBBED, AlreadyCollected, BatchAggregation, Interval, Scrubbed
from .engine import (COLLECT_BATCH_MISMATCH, COLLECT_INVALID_BATCH_SIZE, COLLECT_OK, FINISHED, VERDICT_LABELS,
                     HelperEngine)
from .messages import (EXTENSION_TASKPROV, QUERY_TIME_INTERVAL, AggregateShare, AggregateShareAad,  # noqa: F401
                       AggregateShareReq, BatchSelector, CodecError, Collection, HpkeCiphertext, PartialBatchSelector,
                       PingPongMessage, PlaintextInputShare, PrepareError, PrepareInit, PrepareResp, PrepareStepResult,
                       ReportMetadata, ReportShare)


@dataclass
class AggregateInitOutcome:
    responses: list[PrepareResp]
    finished: np.ndarray                 # bool per PrepareInit: accumulated
    step_failures: Counter = field(default_factory=Counter)  # janus_step_failures{type=...}


def _dense(seg_of_row: list[int]) -> tuple[np.ndarray, list[int]]:
    """Dense per-row indices into the list of distinct batch identifiers (first-seen order)."""
    ids: dict[int, int] = {}
    idx = np.array([ids.setdefault(int(s), len(ids)) for s in seg_of_row], np.uint32)
    return idx, list(ids)


def handle_aggregate_init(engine: HelperEngine, prepare_inits: list[PrepareInit], input_shares: list[bytes],
                          segments: list[int] | None = None, replayed: set[bytes] | None = None,
                          writer=None, extra_report_times: list[tuple[int, int]] = (),
                          inject_tx_failures: int = 0) -> AggregateInitOutcome:
    """Prepare and aggregate one AggregationJobInitializeReq worth of reports.

    input_shares[i] is the HPKE-decrypted PlaintextInputShare payload of report i (the
    encoded Prio3 helper input share). segments[i] names the batch aggregation the report
    belongs to (batch identifier; default 0). replayed holds report ids the datastore
    already saw (check_other_report_aggregation_exists).

    writer (a batch_aggregation.BatchAggregationWriter): the job's batch aggregations are
    written in one retryable transaction (a one-round Prio3 helper job is written already
    finished: neither job counter moves); every report's timestamp widens its batch's
    interval, failed ones included (extra_report_times: report aggregations of the request
    that never reached this call, e.g. HPKE failures). Reports landing in an already
    collected batch fail with BatchCollected. The engine batch is released afterwards.
    Without a writer the finished reports go into the engine's running aggregations."""
    n = len(prepare_inits)
    if len(input_shares) != n:
        raise ValueError("one input share per PrepareInit")
    ids = [p.report_share.metadata.report_id for p in prepare_inits]
    if len(set(ids)) != n:  # aggregator.rs:1750-1758
        raise ValueError("aggregate request contains duplicate report IDs (invalidMessage)")
    v = engine.vdaf
    failures: Counter = Counter()
    results: list[PrepareStepResult | None] = [None] * n
    batch_idx: list[int] = []
    for i, (pi, ins) in enumerate(zip(prepare_inits, input_shares)):
        if len(ins) != v.helper_input_share_len:
            failures["input_share_decode_failure"] += 1
            results[i] = PrepareStepResult(2, error=PrepareError.InvalidMessage)
            continue
        if len(pi.report_share.public_share) != v.public_share_len:
            failures["public_share_decode_failure"] += 1
            results[i] = PrepareStepResult(2, error=PrepareError.InvalidMessage)
            continue
        msg = pi.message
        if msg.kind != PingPongMessage.INITIALIZE:  # PingPongError::PeerMessageMismatch
            failures["leader_ping_pong_message_mismatch"] += 1
            results[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
            continue
        if len(msg.prep_share) != v.prep_share_len:  # PingPongError::CodecPrepShare
            failures["leader_prep_share_decode_failure"] += 1
            results[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
            continue
        batch_idx.append(i)
    finished = np.zeros(n, bool)
    m = len(batch_idx)
    res = None
    accept = np.zeros(m, np.uint8)
    if m:
        nonces = np.frombuffer(b"".join(ids[i] for i in batch_idx), np.uint8).reshape(m, 16)
        ps = np.frombuffer(b"".join(prepare_inits[i].report_share.public_share for i in batch_idx), np.uint8)
        his = np.frombuffer(b"".join(input_shares[i] for i in batch_idx), np.uint8)
        lps = np.frombuffer(b"".join(prepare_inits[i].message.prep_share for i in batch_idx), np.uint8)
        res = engine.helper_initialized_batch(nonces, ps, his, lps)
        for j, i in enumerate(batch_idx):
            verdict = int(res.verdicts[j])
            if verdict != FINISHED:
                failures[VERDICT_LABELS[verdict]] += 1
                results[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
                continue
            if replayed and ids[i] in replayed:  # aggregator.rs:2127-2132
                results[i] = PrepareStepResult(2, error=PrepareError.ReportReplayed)
                continue
            results[i] = PrepareStepResult(0, message=PingPongMessage.finish(res.prep_msgs[j].tobytes()))
            accept[j] = 1
            finished[i] = True
    times = [(int(segments[i]) if segments else 0, p.report_share.metadata.time)
             for i, p in enumerate(prepare_inits)] + list(extra_report_times)
    _write_job(engine, res.batch_id if m else 0, batch_idx, accept, segments, writer, times, inject_tx_failures,
               finished, results)
    responses = [PrepareResp(ids[i], results[i]) for i in range(n)]
    return AggregateInitOutcome(responses, finished, failures)


def _write_job(engine: HelperEngine, batch_id: int, batch_idx: list[int], accept: np.ndarray, segments, writer,
               times, inject_tx_failures: int, finished: np.ndarray, results: list) -> None:
    """Accumulate a helper job's accepted rows (engine row j = report batch_idx[j]): with a writer, as
    per-batch-identifier deltas in one retryable transaction (aggregation_job_writer.rs:476-553, 608-708; the
    batch is released after), else into the engine's running aggregations (which consume the batch). Reports of
    an already collected batch fail with BatchCollected."""
    m = len(batch_idx)
    row_seg = [int(segments[i]) if segments else 0 for i in batch_idx]
    if writer is None:
        if m:
            seg = np.array(row_seg, np.uint32)
            with engine.resident(batch_id):  # accumulate consumes the batch; on an error it is released
                engine.accumulate(m, accept, seg, batch_id=batch_id)
        return
    if m:
        idx, seg_ids = _dense(row_seg)
        try:
            collected = writer.write_job(engine, batch_id, m, accept, idx, seg_ids, times,
                                         initial_write=True, terminal=True, inject_failures=inject_tx_failures)
        finally:
            engine.release(batch_id)
    else:
        collected = writer.write_job(engine, 0, 0, None, None, [], times, initial_write=True, terminal=True,
                                     inject_failures=inject_tx_failures)
    for j, i in enumerate(batch_idx):  # fail_report_aggregations_for_collected_batches
        if finished[i] and row_seg[j] in collected:
            finished[i] = False
            results[i] = PrepareStepResult(2, error=PrepareError.BatchCollected)


# ----------------------------------------------------------------------------- leader side
# Mirror of AggregationJobDriver::step_aggregation_job_aggregate_init and
# process_response_from_helper (aggregator/src/aggregator/aggregation_job_driver.rs:259-436,
# 540-701) minus the HTTP exchange and the datastore: the leader's per-report
# leader_initialized / leader_continued calls become two engine batch calls.


@dataclass
class LeaderReport:
    metadata: ReportMetadata
    public_share: bytes
    leader_input_share: bytes                  # decoded at upload time in Janus; encoded here
    helper_encrypted_input_share: HpkeCiphertext


@dataclass
class LeaderStep:
    prepare_inits: list[PrepareInit]           # the AggregationJobInitializeReq body
    stepped: list[int]                         # report index of each PrepareInit
    failed: dict[int, PrepareError]            # reports that failed before the helper
    n: int                                     # reports in the engine's leader batch
    step_failures: Counter = field(default_factory=Counter)
    init: object = None                        # the engine's LeaderInit (its batch id) when n > 0


def leader_aggregate_init(engine: HelperEngine, reports: list[LeaderReport], segments: list[int] | None = None,
                          writer=None) -> LeaderStep:
    """Prepare every report of a new aggregation job on the leader (agg_id 0) and build the
    PrepareInits to send to the helper (aggregation_job_driver.rs:301-386). writer: the job is
    written in progress (aggregation_jobs_created + 1 per batch identifier) with every report's
    timestamp."""
    v = engine.vdaf
    n = len(reports)
    failures: Counter = Counter()
    failed: dict[int, PrepareError] = {}
    ok = [i for i, r in enumerate(reports) if len(r.leader_input_share) == engine.leader_input_share_len
          and len(r.public_share) == v.public_share_len]
    for i in set(range(n)) - set(ok):
        failed[i] = PrepareError.InvalidMessage
        failures["input_share_decode_failure"] += 1
    inits: list[PrepareInit] = []
    stepped: list[int] = []
    if ok:
        nonces = np.frombuffer(b"".join(reports[i].metadata.report_id for i in ok), np.uint8).reshape(len(ok), 16)
        ps = np.frombuffer(b"".join(reports[i].public_share for i in ok), np.uint8)
        lis = np.frombuffer(b"".join(reports[i].leader_input_share for i in ok), np.uint8)
        res = engine.leader_initialized_batch(nonces, ps, lis)
        for j, i in enumerate(ok):
            if res.verdicts[j] != FINISHED:  # handle_ping_pong_error(Role::Leader, ...)
                failed[i] = PrepareError.VdafPrepError
                failures[VERDICT_LABELS[int(res.verdicts[j])]] += 1
                continue
            r = reports[i]
            inits.append(PrepareInit(ReportShare(r.metadata, r.public_share, r.helper_encrypted_input_share),
                                     PingPongMessage.initialize(res.prep_shares[j].tobytes())))
            stepped.append(i)
    times = [(int(segments[i]) if segments else 0, r.metadata.time) for i, r in enumerate(reports)]
    if writer is not None:  # InitialWrite of the in-progress job: no finished report yet
        try:
            collected = writer.write_job(engine, 0, 0, None, None, [], times, initial_write=True, terminal=False)
        except BaseException:
            if ok:
                engine.release(res.batch_id, missing_ok=True)
            raise
        # fail_report_aggregations_for_collected_batches on the initial write (aggregation_job_writer.rs:
        # 557-605): a report of an already collected batch fails with BatchCollected and is not sent to
        # the helper (its engine row is never continued, so it is never accumulated)
        if collected:
            keep = [k for k, i in enumerate(stepped) if (int(segments[i]) if segments else 0) not in collected]
            for k, i in enumerate(stepped):
                if (int(segments[i]) if segments else 0) in collected:
                    failed[i] = PrepareError.BatchCollected
            inits = [inits[k] for k in keep]
            stepped = [stepped[k] for k in keep]
    step = LeaderStep(inits, stepped, failed, len(ok), failures, res if ok else None)
    step._batch_index = {i: j for j, i in enumerate(ok)}  # report index -> engine batch row
    step._times = times
    return step


def leader_abandon(engine: HelperEngine, step: LeaderStep) -> None:
    """Drop an aggregation job's leader state (the job was abandoned, or its helper exchange failed
    for good): its resident engine batch is released. A later leader_process_helper_response for
    the step fails with JX_E_STATE."""
    if step.init is not None:
        engine.release(step.init.batch_id, missing_ok=True)


def leader_process_helper_response(engine: HelperEngine, step: LeaderStep, prepare_resps: list[PrepareResp],
                                   segments: list[int] | None = None, writer=None) -> AggregateInitOutcome:
    """Finish the leader's reports from the helper's AggregationJobResp and accumulate the
    finished ones (process_response_from_helper, aggregation_job_driver.rs:540-701). writer: the
    job is updated into a terminal state (aggregation_jobs_terminated + 1 per batch identifier),
    its finished reports merged as deltas in one retryable transaction, and the engine batch is
    released. Without a writer they go into the engine's running aggregations."""
    if len(prepare_resps) != len(step.stepped) or any(
            resp.report_id != step.prepare_inits[k].report_share.metadata.report_id
            for k, resp in enumerate(prepare_resps)):
        # the job step fails (process_response_from_helper's error): its device state is released, and
        # the job is stepped again from leader_aggregate_init
        leader_abandon(engine, step)
        raise ValueError("missing, duplicate, out-of-order, or unexpected prepare steps in response")
    failures = Counter(step.step_failures)
    nrep = max([*step.stepped, *step.failed, -1]) + 1
    finished = np.zeros(nrep, bool)
    results: dict[int, PrepareError | None] = dict(step.failed)
    pm = engine.prep_msg_len
    msgs = np.zeros((step.n, max(pm, 1)), np.uint8)
    continued = np.zeros(step.n, bool)
    for k, resp in enumerate(prepare_resps):
        i = step.stepped[k]
        row = step._batch_index[i]
        res = resp.result
        if res.kind == 2:                        # Reject(err): the helper's error
            results[i] = res.error
            failures["helper_step_failure"] += 1
        elif res.kind == 1:                      # Finished, but a 1-round leader is still Continued
            results[i] = PrepareError.VdafPrepError
            failures["finish_mismatch"] += 1
        elif res.message.kind != PingPongMessage.FINISH or len(res.message.prep_msg) != pm:
            results[i] = PrepareError.VdafPrepError  # PingPongError::PeerMessageMismatch / CodecPrepMessage
            failures["leader_ping_pong_message_mismatch"] += 1
        else:
            if pm:
                msgs[row, :pm] = np.frombuffer(res.message.prep_msg, np.uint8)
            continued[row] = True
    if step.n == 0:  # no report reached the engine: nothing to continue or accumulate
        if writer is not None:
            writer.write_job(engine, 0, 0, None, None, [], step._times, initial_write=False, terminal=True)
        responses = [PrepareResp(step.prepare_inits[k].report_share.metadata.report_id,
                                 PrepareStepResult(2, error=results[i])) for k, i in enumerate(step.stepped)]
        return AggregateInitOutcome(responses, finished, failures)
    try:
        fin = engine.leader_continued_batch(msgs[:, :pm] if pm else None, init=step.init)
    except BaseException:
        leader_abandon(engine, step)
        raise
    accept = np.zeros(step.n, np.uint8)
    seg = np.zeros(step.n, np.uint32)
    for i, row in step._batch_index.items():
        if not continued[row]:
            continue
        if fin.verdicts[row] != FINISHED:
            results[i] = PrepareError.VdafPrepError
            failures[VERDICT_LABELS[int(fin.verdicts[row])]] += 1
            continue
        results[i] = None
        accept[row] = 1
        seg[row] = segments[i] if segments else 0
        finished[i] = True
    if writer is None:
        with engine.resident(step.init.batch_id):
            engine.accumulate(step.n, accept, seg, batch_id=step.init.batch_id)
    else:
        row_seg = [0] * step.n
        for i, row in step._batch_index.items():
            row_seg[row] = int(segments[i]) if segments else 0
        idx, seg_ids = _dense(row_seg)
        try:
            collected = writer.write_job(engine, step.init.batch_id, step.n, accept, idx, seg_ids, step._times,
                                         initial_write=False, terminal=True)
        finally:
            engine.release(step.init.batch_id)
        for i, row in step._batch_index.items():
            if finished[i] and row_seg[row] in collected:
                finished[i] = False
                results[i] = PrepareError.BatchCollected
    responses = [PrepareResp(step.prepare_inits[k].report_share.metadata.report_id,
                             PrepareStepResult(1) if results[i] is None else
                             PrepareStepResult(2, error=results[i]))
                 for k, i in enumerate(step.stepped)]
    return AggregateInitOutcome(responses, finished, failures)


# ----------------------------------------------------------------------------- leader side, through wire bytes


@dataclass
class LeaderWireStep:
    body: bytes                                # the AggregationJobInitializeReq body
    req: object                                # the engine's LeaderReq (released by the response, or by leader_abandon_wire)
    stepped: list[int]                         # index into `stored` of each PrepareInit of the body, in order
    failed: dict[int, PrepareError]            # reports that failed before the helper
    n: int                                     # rows of the engine's leader batch
    step_failures: Counter = field(default_factory=Counter)
    batch_id: int = 0                          # the resident leader batch when n > 0
    report_ids: list = field(default_factory=list)
    _row_of: list = field(default_factory=list)  # engine row of each report
    _times: list = field(default_factory=list)


def leader_aggregate_init_wire(engine: HelperEngine, stored: list, rows, lis_stride: int, agg_param: bytes, selector,
                               segments: list[int] | None = None, writer=None) -> LeaderWireStep:
    """leader_aggregate_init from the StoredReports and device rows of a handle_upload outcome to the request body,
    with the prep shares staying in HBM: the duplicate-extension check on the host (aggregation_job_driver.rs:
    325-341: InvalidMessage, counted as duplicate_extension), leader_init_device on the rows in place, the initial
    write and the collected-batch exclusion as leader_aggregate_init does them, then engine.encode_init_req over
    the reports whose init succeeded and that are not excluded. The engine batch holds every row of `rows`; a row no
    StoredReport names (a report the upload rejected) is never sent, so it is never continued or accumulated.
    selector: the job's messages.PartialBatchSelector."""
    import torch

    from .messages import QUERY_FIXED_SIZE

    v = engine.vdaf
    nrep = len(stored)
    m = 0 if rows is None else int(rows.shape[0])
    PS, LPS = v.public_share_len, engine.prep_share_len
    failures: Counter = Counter()
    failed: dict[int, PrepareError] = {}
    seg_of = lambda i: int(segments[i]) if segments else 0  # noqa: E731
    ids = np.zeros((max(m, 1), 16), np.uint8)
    ps = np.zeros((max(m, 1), max(PS, 1)), np.uint8)
    times = np.zeros(max(m, 1), np.uint64)
    cfg = np.zeros(max(m, 1), np.uint8)
    encs, pays = [b""] * m, [b""] * m
    exclude = np.ones(max(m, 1), np.uint8)
    rep_of_row: dict[int, int] = {}
    dup = np.zeros(nrep, bool)
    for i, s in enumerate(stored):
        types = [e.extension_type for e in s.extensions]
        if len(set(types)) != len(types):
            dup[i] = True
            failed[i] = PrepareError.InvalidMessage
            failures["duplicate_extension"] += 1
        r, ct = s.row, s.helper_encrypted_input_share
        if r in rep_of_row or not 0 <= r < m:
            raise ValueError("each StoredReport names its own row of the upload's rows")
        rep_of_row[r] = i
        ids[r] = np.frombuffer(s.metadata.report_id, np.uint8)
        if PS:
            ps[r] = np.frombuffer(s.public_share, np.uint8)
        times[r], cfg[r] = s.metadata.time, ct.config_id
        encs[r], pays[r] = ct.encapsulated_key, ct.payload
        exclude[r] = dup[i]
    eoff, poff = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
    if m:
        eoff[1:] = np.cumsum([len(x) for x in encs])
        poff[1:] = np.cumsum([len(x) for x in pays])
    row_of = [s.row for s in stored]
    job_times = [(seg_of(i), s.metadata.time) for i, s in enumerate(stored)]
    dev = torch.device("cuda", engine.device)
    batch_id = 0
    verdicts = np.zeros(m, np.uint8)
    with torch.cuda.device(dev):
        d_ids, d_ps = torch.from_numpy(ids.reshape(-1)).to(dev), torch.from_numpy(ps.reshape(-1)).to(dev)
        d_en = torch.from_numpy(np.frombuffer(b"".join(encs) or b"\0", np.uint8).copy()).to(dev)
        d_pay = torch.from_numpy(np.frombuffer(b"".join(pays) or b"\0", np.uint8).copy()).to(dev)
        d_lps = torch.empty(max(m, 1) * max(LPS, 1), dtype=torch.uint8, device=dev)
        d_v = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
        if m:
            batch_id = engine.leader_init_device(m, d_ids.data_ptr(), d_ps.data_ptr() if PS else None, rows.data_ptr(),
                                                 d_lps.data_ptr(), d_v.data_ptr(), lis_stride=lis_stride)
            verdicts = d_v.cpu().numpy()[:m]
        try:
            for i in range(nrep):
                vd = int(verdicts[row_of[i]])
                if not dup[i] and vd != FINISHED:  # handle_ping_pong_error(Role::Leader, ...)
                    failed[i] = PrepareError.VdafPrepError
                    failures[VERDICT_LABELS[vd]] += 1
            if writer is not None:  # InitialWrite of the in-progress job, as leader_aggregate_init
                collected = writer.write_job(engine, 0, 0, None, None, [], job_times, initial_write=True, terminal=False)
                for i in range(nrep):
                    if i not in failed and seg_of(i) in collected:
                        failed[i] = PrepareError.BatchCollected
                        exclude[row_of[i]] = 1
            req = engine.encode_init_req(m, d_ids.data_ptr(), times, d_ps.data_ptr() if PS else None, cfg, d_en.data_ptr(),
                                         d_pay.data_ptr(), poff, d_lps.data_ptr(), d_v.data_ptr(), agg_param,
                                         selector.query_type,
                                         selector.batch_id if selector.query_type == QUERY_FIXED_SIZE else None,
                                         enc_offsets=eoff, exclude=exclude)
            body = req.body
        except BaseException:
            if batch_id:
                engine.release(batch_id, missing_ok=True)
            raise
    stepped = [rep_of_row[int(r)] for r in req.sent_index]
    return LeaderWireStep(body, req, stepped, failed, m, failures, batch_id, [s.metadata.report_id for s in stored],
                          row_of, job_times)


def leader_abandon_wire(engine: HelperEngine, step: LeaderWireStep) -> None:
    """Drop a wire step's leader state: its resident engine batch and its request handle."""
    if step.batch_id:
        engine.release(step.batch_id, missing_ok=True)
    step.req.release()


def leader_process_helper_response_wire(engine: HelperEngine, step: LeaderWireStep, resp_body: bytes,
                                        segments: list[int] | None = None, writer=None) -> AggregateInitOutcome:
    """leader_process_helper_response from the AggregationJobResp body: engine.decode_init_resp puts the prep
    messages and peer verdicts into device rows, leader_finish_device continues them, and the finished reports are
    accumulated (or written by `writer`) as the object path does. A malformed response raises CodecError, one whose
    PrepareResps are not the sent reports in order the reference's ValueError; in both cases the batch is abandoned."""
    import torch

    from .engine import RESP_CONTINUED, RESP_FINISHED, RESP_REJECTED, WIRE_MALFORMED, WIRE_RESP_MISMATCH

    n, pm = step.n, engine.prep_msg_len
    dev = torch.device("cuda", engine.device)
    failures = Counter(step.step_failures)
    nrep = max([*step.stepped, *step.failed, -1]) + 1
    finished = np.zeros(nrep, bool)
    results: dict[int, PrepareError | None] = dict(step.failed)
    with torch.cuda.device(dev):
        d_m = torch.empty((max(n, 1), max(pm, 1)), dtype=torch.uint8, device=dev)
        d_p = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        d_fv = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        try:
            dec = engine.decode_init_resp(step.req, resp_body, d_m.data_ptr() if pm else None, d_p.data_ptr(),
                                          prep_msg_stride=max(pm, 1) if pm else 0)
        except BaseException:
            leader_abandon_wire(engine, step)
            raise
        if dec.status == WIRE_MALFORMED:
            leader_abandon_wire(engine, step)
            raise CodecError(f"AggregationJobResp: malformed at byte {dec.error_offset}")
        if dec.status == WIRE_RESP_MISMATCH:
            # the job step fails (process_response_from_helper's error): its device state is released
            leader_abandon_wire(engine, step)
            raise ValueError("missing, duplicate, out-of-order, or unexpected prepare steps in response")
        for k, i in enumerate(step.stepped):
            res = int(dec.results[k])
            if res == RESP_REJECTED:
                results[i] = PrepareError(int(dec.errors[k]))
                failures["helper_step_failure"] += 1
            elif res == RESP_FINISHED:
                results[i] = PrepareError.VdafPrepError
                failures["finish_mismatch"] += 1
            elif res != RESP_CONTINUED:
                results[i] = PrepareError.VdafPrepError
                failures["leader_ping_pong_message_mismatch"] += 1

        def responses():
            return [PrepareResp(step.report_ids[i], PrepareStepResult(1) if results[i] is None else
                                PrepareStepResult(2, error=results[i])) for i in step.stepped]

        if n == 0:
            step.req.release()
            if writer is not None:
                writer.write_job(engine, 0, 0, None, None, [], step._times, initial_write=False, terminal=True)
            return AggregateInitOutcome(responses(), finished, failures)
        try:
            engine.leader_finish_device(step.batch_id, n, d_m.data_ptr() if pm else None, d_p.data_ptr(), d_fv.data_ptr())
            fv = d_fv.cpu().numpy()[:n]
        except BaseException:
            leader_abandon_wire(engine, step)
            raise
    step.req.release()
    accept = np.zeros(n, np.uint8)
    seg = np.zeros(n, np.uint32)
    row_seg = [0] * n
    for i, row in enumerate(step._row_of):
        row_seg[row] = int(segments[i]) if segments else 0
    for k, i in enumerate(step.stepped):
        if int(dec.results[k]) != RESP_CONTINUED:
            continue
        row = step._row_of[i]
        if fv[row] != FINISHED:
            results[i] = PrepareError.VdafPrepError
            failures[VERDICT_LABELS[int(fv[row])]] += 1
            continue
        results[i] = None
        accept[row] = 1
        seg[row] = row_seg[row]
        finished[i] = True
    if writer is None:
        with engine.resident(step.batch_id):
            engine.accumulate(n, accept, seg, batch_id=step.batch_id)
    else:
        idx, seg_ids = _dense(row_seg)
        try:
            collected = writer.write_job(engine, step.batch_id, n, accept, idx, seg_ids, step._times,
                                         initial_write=False, terminal=True)
        finally:
            engine.release(step.batch_id)
        for i, row in enumerate(step._row_of):
            if finished[i] and row_seg[row] in collected:
                finished[i] = False
                results[i] = PrepareError.BatchCollected
    return AggregateInitOutcome(responses(), finished, failures)


# ----------------------------------------------------------------------------- HPKE + prepare


def handle_aggregate_init_encrypted(engine: HelperEngine, opener, hpke_config_id: int, task_id: bytes,
                                    prepare_inits: list[PrepareInit], segments: list[int] | None = None,
                                    replayed: set[bytes] | None = None, writer=None, global_keypairs=None,
                                    require_taskprov: bool = False, report_deadline: int | None = None,
                                    inject_tx_failures: int = 0) -> AggregateInitOutcome:
    """The helper's aggregate-init loop from the encrypted report shares (aggregator.rs:1763-2013), with the
    HPKE open inside the prepare launch (jx_helper_prep_encrypted_batch2; coalesced with other jobs when the
    engine coalesces): per report, the task's keypair (opener, config id hpke_config_id) and then the
    aggregator's global keypair for the report's config id (global_keypairs: {config_id: HpkeOpener}) are
    tried (:1781-1832), the PlaintextInputShare is decoded and its extensions checked (:1834-1893), the payload
    decoded as the helper input share (:1895-1910), the public share decoded (:1912-1925), reports from after
    report_deadline rejected (:1929-1940), then helper_initialized + evaluate (:1945-1967). Failures map as in
    the reference: HpkeUnknownConfigId, HpkeDecryptError, InvalidMessage (plaintext / extension / input share /
    public share), ReportTooEarly, VdafPrepError. A report whose public share has the wrong length cannot ride
    the fixed-stride device rows: it is opened alone (janus_amd.hpke) and fails with InvalidMessage unless an
    earlier check fails it first."""
    from .engine import KEY_NONE, OPEN_STATUS

    v = engine.vdaf
    n = len(prepare_inits)
    ids = [p.report_share.metadata.report_id for p in prepare_inits]
    if len(set(ids)) != n:  # aggregator.rs:1750-1758
        raise ValueError("aggregate request contains duplicate report IDs (invalidMessage)")
    globals_ = dict(global_keypairs or {})
    keypairs = [opener]
    slot: dict[int, int] = {}

    def key_slot(k) -> int:
        if id(k) not in slot:
            slot[id(k)] = len(keypairs) if k is not opener else 0
            if k is not opener:
                keypairs.append(k)
        return slot[id(k)]

    slot[id(opener)] = 0
    failures: Counter = Counter()
    results: list[PrepareStepResult | None] = [None] * n
    rows: list[int] = []           # reports on the device, in row order
    odd: list[int] = []            # public share of the wrong length: opened alone
    key_index = []
    for i, pi in enumerate(prepare_inits):
        ct = pi.report_share.encrypted_input_share
        task_k = opener if ct.config_id == hpke_config_id else None
        glob_k = globals_.get(ct.config_id)
        first, second = (task_k, glob_k) if task_k is not None else (glob_k, None)
        if len(pi.report_share.public_share) != v.public_share_len:
            odd.append(i)
            continue
        if first is None:
            k0, k1 = KEY_NONE, KEY_NONE
        else:  # a keypair whose KEM has another encapsulated-key length is a failed trial (the engine's rule)
            k0, k1 = key_slot(first), (key_slot(second) if second is not None else KEY_NONE)
        if len(keypairs) > 8:
            raise ValueError("more than JX_ENC_MAX_KEYPAIRS distinct keypairs in one request")
        rows.append(i)
        key_index.append((k0, k1))
    finished = np.zeros(n, bool)
    m = len(rows)
    accept = np.zeros(m, np.uint8)
    res = None
    if m:
        md = [prepare_inits[i].report_share.metadata for i in rows]
        nonces = np.frombuffer(b"".join(x.report_id for x in md), np.uint8).reshape(m, 16)
        times = np.array([x.time for x in md], np.uint64)
        ps = np.frombuffer(b"".join(prepare_inits[i].report_share.public_share for i in rows), np.uint8)
        encs = [prepare_inits[i].report_share.encrypted_input_share.encapsulated_key for i in rows]
        payloads = [prepare_inits[i].report_share.encrypted_input_share.payload for i in rows]
        # a leader message that is not Initialize, or a prep share of the wrong length, fails inside
        # helper_initialized, after the open: the row rides with a zero prep share and is fixed up below
        msg_fail: dict[int, str] = {}
        lps_rows = []
        for j, i in enumerate(rows):
            msg = prepare_inits[i].message
            if msg.kind != PingPongMessage.INITIALIZE:  # PingPongError::PeerMessageMismatch
                msg_fail[j] = "leader_ping_pong_message_mismatch"
            elif len(msg.prep_share) != v.prep_share_len:  # PingPongError::CodecPrepShare
                msg_fail[j] = "leader_prep_share_decode_failure"
            lps_rows.append(msg.prep_share if j not in msg_fail else bytes(v.prep_share_len))
        lps = np.frombuffer(b"".join(lps_rows), np.uint8)
        res = engine.helper_initialized_encrypted_batch(nonces, times, ps, task_id, keypairs,
                                                        np.array(key_index, np.uint8), encs, payloads, lps,
                                                        require_taskprov=require_taskprov)
        for j, i in enumerate(rows):
            st = int(res.open_status[j])
            if st:
                label, err = OPEN_STATUS[st]
                failures[label] += 1
                results[i] = PrepareStepResult(2, error=PrepareError(err))
            elif report_deadline is not None and md[j].time > report_deadline:
                results[i] = PrepareStepResult(2, error=PrepareError.ReportTooEarly)
            elif j in msg_fail:
                failures[msg_fail[j]] += 1
                results[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
            elif int(res.verdicts[j]) != FINISHED:
                failures[VERDICT_LABELS[int(res.verdicts[j])]] += 1
                results[i] = PrepareStepResult(2, error=PrepareError.VdafPrepError)
            elif replayed and ids[i] in replayed:  # aggregator.rs:2127-2132
                results[i] = PrepareStepResult(2, error=PrepareError.ReportReplayed)
            else:
                results[i] = PrepareStepResult(0, message=PingPongMessage.finish(res.prep_msgs[j].tobytes()))
                accept[j] = 1
                finished[i] = True
    for i in odd:
        results[i] = PrepareStepResult(2, error=_open_alone(prepare_inits[i], opener, hpke_config_id, globals_,
                                                            task_id, v, require_taskprov, failures))
    times_all = [(int(segments[i]) if segments else 0, p.report_share.metadata.time) for i, p in enumerate(prepare_inits)]
    _write_job(engine, res.batch_id if m else 0, rows, accept, segments, writer, times_all, inject_tx_failures,
               finished, results)
    responses = [PrepareResp(ids[i], results[i]) for i in range(n)]
    return AggregateInitOutcome(responses, finished, failures)


def _open_alone(pi: PrepareInit, opener, hpke_config_id: int, globals_: dict, task_id: bytes, v, require_taskprov: bool,
                failures: Counter) -> PrepareError:
    """A report whose public share has the wrong length (it cannot ride the fixed-stride device rows): the
    reference's checks in order on the host (batched HPKE open on the GPU for this one share); it always fails,
    with public_share_decode_failure at the latest."""
    from .hpke import input_share_aad

    rs = pi.report_share
    ct = rs.encrypted_input_share
    keys = [k for k in ((opener if ct.config_id == hpke_config_id else None), globals_.get(ct.config_id)) if k]
    if not keys:
        failures["unknown_hpke_config_id"] += 1
        return PrepareError.HpkeUnknownConfigId
    aad = input_share_aad(task_id, rs.metadata.report_id, rs.metadata.time, rs.public_share)
    pt = None
    for k in keys:
        pt = k.open_batch([ct.encapsulated_key], [ct.payload], [aad])[0]
        if pt is not None:
            break
    if pt is None:
        failures["decrypt_failure"] += 1
        return PrepareError.HpkeDecryptError
    try:
        pis = PlaintextInputShare.decode(pt)
    except CodecError:
        failures["plaintext_input_share_decode_failure"] += 1
        return PrepareError.InvalidMessage
    types = [e.extension_type for e in pis.extensions]
    if len(set(types)) != len(types):
        failures["duplicate_extension"] += 1
    elif require_taskprov and not any(e.extension_type == EXTENSION_TASKPROV and not e.extension_data
                                      for e in pis.extensions):
        failures["missing_or_malformed_taskprov_extension"] += 1
    elif not require_taskprov and EXTENSION_TASKPROV in types:
        failures["unexpected_taskprov_extension"] += 1
    elif len(pis.payload) != v.helper_input_share_len:
        failures["input_share_decode_failure"] += 1
    else:
        failures["public_share_decode_failure"] += 1
    return PrepareError.InvalidMessage


# ----------------------------------------------------------------------------- wire in, wire out


class EmptyAggregation(ValueError):
    """Error::EmptyAggregation (aggregator.rs:2017-2028): the request holds no PrepareInit."""


def handle_aggregate_init_wire(engine: HelperEngine, body: bytes, task_id: bytes, opener, hpke_config_id: int,
                               query_type: int, global_keypairs=None, require_taskprov: bool = False,
                               report_deadline: int | None = None, replayed=None, segment: int = 0):
    """The helper's aggregate-init exchange from the request body to the response body (aggregator.rs:1740-2013), with
    no per-report host work but for reports the fixed-stride rows cannot carry: the body is decoded on the GPU
    (engine.decode_init_req), the sealed fused call opens, prepares and aggregates from the decoded arrays with the
    decode's route as its segment index (so a report with a wrong leader message, from after report_deadline or
    replayed never reaches the aggregation `segment`), and the AggregationJobResp body is encoded on the GPU.
    replayed: report ids the datastore already saw (a set of bytes), or a mask of n; they are known before the call
    and answered with ReportReplayed unless an earlier check fails them. A malformed request raises CodecError, a
    repeated report id ValueError (invalidMessage), a request without reports EmptyAggregation; none of them queues
    anything. Returns (response body, finished mask, janus_step_failures counter)."""
    import torch

    from .engine import (KEY_NONE, OPEN_STATUS, WIRE_DUPLICATE_ID, WIRE_NO_ERROR, WIRE_OK, WIRE_REPORT_NOT_INITIALIZE,
                         WIRE_REPORT_ODD_PREP_SHARE, WIRE_REPORT_ODD_PUBLIC_SHARE, WIRE_WRONG_QUERY_TYPE)

    v = engine.vdaf
    globals_ = dict(global_keypairs or {})
    keypairs = [opener]
    slot = {id(opener): 0}

    def key_slot(k) -> int:
        if id(k) not in slot:
            slot[id(k)] = len(keypairs)
            keypairs.append(k)
        return slot[id(k)]

    key_first, key_second = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    for cfg in range(256):
        task_k = opener if cfg == hpke_config_id else None
        glob_k = globals_.get(cfg)
        first, second = (task_k, glob_k) if task_k is not None else (glob_k, None)
        if first is not None:
            key_first[cfg] = key_slot(first)
            if second is not None:
                key_second[cfg] = key_slot(second)
    if len(keypairs) > 8:
        raise ValueError("more than JX_ENC_MAX_KEYPAIRS distinct keypairs for one task")
    failures: Counter = Counter()
    with engine.decode_init_req(body, query_type, key_first, key_second, report_deadline) as req:
        if req.status == WIRE_DUPLICATE_ID:  # aggregator.rs:1750-1758
            raise ValueError(f"aggregate request contains duplicate report IDs (invalidMessage): report {req.duplicate_index}")
        if req.status != WIRE_OK:
            what = "unexpected query type" if req.status == WIRE_WRONG_QUERY_TYPE else "malformed"
            raise CodecError(f"AggregationJobInitializeReq: {what} at byte {req.error_offset}")
        n = req.n
        if n == 0:
            raise EmptyAggregation("aggregation job request holds no report")
        ws = req.wire_status
        host_err = None
        odd = np.nonzero(ws == WIRE_REPORT_ODD_PUBLIC_SHARE)[0]
        if odd.size:  # the reports the rows cannot carry: the reference's checks on the host, from the body's bytes
            host_err = np.full(n, WIRE_NO_ERROR, np.uint8)
            for i in odd:
                rec = req.records[i]
                pi = PrepareInit.decode(body[int(rec["off"]):int(rec["off"]) + int(rec["len"])])
                host_err[i] = int(_open_alone(pi, opener, hpke_config_id, globals_, task_id, v, require_taskprov, failures))
        rep = None
        if replayed is not None and not isinstance(replayed, (set, frozenset)):
            rep = np.asarray(replayed).astype(bool).reshape(n)
        elif replayed:
            rep = np.fromiter((r.tobytes() in replayed for r in req.report_ids), bool, n)
        if rep is not None and rep.any():
            req.exclude(rep)
        dev = torch.device("cuda", engine.device)
        with torch.cuda.device(dev):
            d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_m = torch.zeros((n, max(engine.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
            a = req.d
            engine.prep_and_aggregate_encrypted_device(
                a.d_report_ids, req.times, a.d_public_shares, task_id, keypairs, req.key_index, a.d_encs, a.d_payloads,
                req.payload_offsets, a.d_leader_prep_shares, n, enc_offsets=req.enc_offsets,
                require_taskprov=require_taskprov, d_out_prep_msgs=d_m.data_ptr() if engine.prep_msg_len else None,
                d_out_verdicts=d_v.data_ptr(), d_out_open_status=d_st.data_ptr(), d_segments=a.d_route,
                segment_ids=[segment])
            out, finished = engine.encode_init_resp(req, d_v.data_ptr(), d_st.data_ptr(),
                                                    d_m.data_ptr() if engine.prep_msg_len else None, host_err, rep,
                                                    prep_msg_stride=max(engine.prep_msg_len, 1) if engine.prep_msg_len else 0)
            st, vd = d_st.cpu().numpy(), d_v.cpu().numpy()
        # the counters, by the same precedence, whole arrays at a time
        live = ws != WIRE_REPORT_ODD_PUBLIC_SHARE
        for code, cnt in enumerate(np.bincount(st[live & (st != 0)], minlength=8)):
            if cnt:
                failures[OPEN_STATUS[code][0]] += int(cnt)
        rest = live & (st == 0)
        if report_deadline is not None:
            rest &= req.times <= np.uint64(report_deadline)
        for code, label in ((WIRE_REPORT_NOT_INITIALIZE, "leader_ping_pong_message_mismatch"),
                            (WIRE_REPORT_ODD_PREP_SHARE, "leader_prep_share_decode_failure")):
            cnt = int((rest & (ws == code)).sum())
            if cnt:
                failures[label] += cnt
        for code, cnt in enumerate(np.bincount(vd[rest & (ws == 0) & (vd != FINISHED)], minlength=1)):
            if cnt:
                failures[VERDICT_LABELS[code]] += int(cnt)
    return out, finished, failures


class TooManyBuckets(ValueError):
    """The request's reports fall into more batch buckets than the device route holds (engine.ROUTE_MAX_BUCKETS):
    nothing was queued, and the request is served by the object path (handle_aggregate_init with segments=)."""


def _wire_key_tables(opener, hpke_config_id: int, globals_: dict):
    """(keypairs, key_first, key_second) as decode_init_req and the sealed calls take them: per config id the task's
    keypair first and the global one second, each distinct keypair in one slot."""
    from .engine import KEY_NONE

    keypairs = [opener]
    slot = {id(opener): 0}

    def key_slot(k) -> int:
        if id(k) not in slot:
            slot[id(k)] = len(keypairs)
            keypairs.append(k)
        return slot[id(k)]

    key_first, key_second = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    for cfg in range(256):
        task_k = opener if cfg == hpke_config_id else None
        glob_k = globals_.get(cfg)
        first, second = (task_k, glob_k) if task_k is not None else (glob_k, None)
        if first is not None:
            key_first[cfg] = key_slot(first)
            if second is not None:
                key_second[cfg] = key_slot(second)
    if len(keypairs) > 8:
        raise ValueError("more than JX_ENC_MAX_KEYPAIRS distinct keypairs for one task")
    return keypairs, key_first, key_second


def _wire_accept(req) -> int:
    """The request-level refusals of a decoded request (aggregator.rs:1740-1758, :2017-2028); its report count."""
    from .engine import WIRE_DUPLICATE_ID, WIRE_OK, WIRE_WRONG_QUERY_TYPE

    if req.status == WIRE_DUPLICATE_ID:
        raise ValueError(f"aggregate request contains duplicate report IDs (invalidMessage): report {req.duplicate_index}")
    if req.status != WIRE_OK:
        what = "unexpected query type" if req.status == WIRE_WRONG_QUERY_TYPE else "malformed"
        raise CodecError(f"AggregationJobInitializeReq: {what} at byte {req.error_offset}")
    if req.n == 0:
        raise EmptyAggregation("aggregation job request holds no report")
    return req.n


def _wire_host_errors(req, body: bytes, opener, hpke_config_id: int, globals_: dict, task_id: bytes, v,
                      require_taskprov: bool, failures: Counter):
    """host_errors for the reports the rows cannot carry (a public share of another length): the reference's checks on
    the host, from the body's bytes. None when there is no such report."""
    from .engine import WIRE_NO_ERROR, WIRE_REPORT_ODD_PUBLIC_SHARE

    odd = np.nonzero(req.wire_status == WIRE_REPORT_ODD_PUBLIC_SHARE)[0]
    if not odd.size:
        return None
    host_err = np.full(req.n, WIRE_NO_ERROR, np.uint8)
    for i in odd:
        rec = req.records[i]
        pi = PrepareInit.decode(body[int(rec["off"]):int(rec["off"]) + int(rec["len"])])
        host_err[i] = int(_open_alone(pi, opener, hpke_config_id, globals_, task_id, v, require_taskprov, failures))
    return host_err


def _wire_replayed_mask(req, replayed):
    """replayed (a set of report ids, or a mask of n) as a mask of n; None when there is none."""
    if replayed is not None and not isinstance(replayed, (set, frozenset)):
        return np.asarray(replayed).astype(bool).reshape(req.n)
    if replayed:
        return np.fromiter((r.tobytes() in replayed for r in req.report_ids), bool, req.n)
    return None


def _wire_count_failures(failures: Counter, req, st, vd, report_deadline) -> None:
    """janus_step_failures from the open statuses and verdicts, by the handler's precedence, whole arrays at a time."""
    from .engine import OPEN_STATUS, WIRE_REPORT_NOT_INITIALIZE, WIRE_REPORT_ODD_PREP_SHARE, WIRE_REPORT_ODD_PUBLIC_SHARE

    ws = req.wire_status
    live = ws != WIRE_REPORT_ODD_PUBLIC_SHARE
    for code, cnt in enumerate(np.bincount(st[live & (st != 0)], minlength=8)):
        if cnt:
            failures[OPEN_STATUS[code][0]] += int(cnt)
    rest = live & (st == 0)
    if report_deadline is not None:
        rest &= req.times <= np.uint64(report_deadline)
    for code, label in ((WIRE_REPORT_NOT_INITIALIZE, "leader_ping_pong_message_mismatch"),
                        (WIRE_REPORT_ODD_PREP_SHARE, "leader_prep_share_decode_failure")):
        cnt = int((rest & (ws == code)).sum())
        if cnt:
            failures[label] += cnt
    for code, cnt in enumerate(np.bincount(vd[rest & (ws == 0) & (vd != FINISHED)], minlength=1)):
        if cnt:
            failures[VERDICT_LABELS[code]] += int(cnt)


def handle_aggregate_init_wire_buckets(engine: HelperEngine, body: bytes, task_id: bytes, opener, hpke_config_id: int,
                                       time_precision: int, segment_of, collected=(), global_keypairs=None,
                                       require_taskprov: bool = False, report_deadline: int | None = None, replayed=None):
    """handle_aggregate_init_wire for a time-interval task whose request spans batches: between the decode and the
    sealed fused call the reports are routed to their batch buckets on the GPU (InitReq.route: the report time rounded
    down to time_precision, as aggregation_job_writer.rs:557-605 indexes them), so that one call accumulates every
    bucket's aggregation. segment_of maps a bucket start to the deployment's u32 aggregation id; collected: the starts
    of the batches that no longer accept aggregations, whose otherwise finished reports are answered with
    BatchCollected and reach no aggregation (:608-708). The other arguments and the errors raised are
    handle_aggregate_init_wire's; a request of more than ROUTE_MAX_BUCKETS buckets raises TooManyBuckets before
    anything is queued. Returns (response body, finished mask, janus_step_failures counter, bucket table): the table
    is a ROUTE_BUCKET array whose min_time / max_time / reports cover every report of the request, as the writer
    widens each batch's client-timestamp interval."""
    import torch

    from .engine import ROUTE_MAX_BUCKETS, ROUTE_OK
    from .messages import QUERY_TIME_INTERVAL

    globals_ = dict(global_keypairs or {})
    keypairs, key_first, key_second = _wire_key_tables(opener, hpke_config_id, globals_)
    failures: Counter = Counter()
    with engine.decode_init_req(body, QUERY_TIME_INTERVAL, key_first, key_second, report_deadline) as req:
        n = _wire_accept(req)
        host_err = _wire_host_errors(req, body, opener, hpke_config_id, globals_, task_id, engine.vdaf, require_taskprov,
                                     failures)
        rep = _wire_replayed_mask(req, replayed)
        if rep is not None and rep.any():
            req.exclude(rep)
        status, buckets = req.route(time_precision, collected)
        if status != ROUTE_OK:
            raise TooManyBuckets(f"aggregation job request spans more than {ROUTE_MAX_BUCKETS} batch buckets")
        S = engine.prep_msg_len
        dev = torch.device("cuda", engine.device)
        with torch.cuda.device(dev):
            d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_m = torch.zeros((n, max(S, 1)), dtype=torch.uint8, device=dev)
            a = req.d
            engine.prep_and_aggregate_encrypted_device(
                a.d_report_ids, req.times, a.d_public_shares, task_id, keypairs, req.key_index, a.d_encs, a.d_payloads,
                req.payload_offsets, a.d_leader_prep_shares, n, enc_offsets=req.enc_offsets,
                require_taskprov=require_taskprov, d_out_prep_msgs=d_m.data_ptr() if S else None,
                d_out_verdicts=d_v.data_ptr(), d_out_open_status=d_st.data_ptr(), d_segments=a.d_route,
                segment_ids=[int(segment_of(int(b["start"]))) for b in buckets])
            out, finished = engine.encode_init_resp(req, d_v.data_ptr(), d_st.data_ptr(), d_m.data_ptr() if S else None,
                                                    host_err, rep, prep_msg_stride=max(S, 1) if S else 0)
            st, vd = d_st.cpu().numpy(), d_v.cpu().numpy()
        _wire_count_failures(failures, req, st, vd, report_deadline)
    return out, finished, failures, buckets


# ----------------------------------------------------------------------------- upload (leader)


class ReportRejectionReason(enum.Enum):  # aggregator/src/aggregator/error.rs:220-228
    IntervalCollected = "interval_collected"
    DecryptFailure = "decrypt_failure"
    DecodeFailure = "decode_failure"
    TaskExpired = "task_expired"
    Expired = "expired"
    TooEarly = "too_early"
    OutdatedHpkeConfig = "outdated_hpke_config"


@dataclass(frozen=True)
class ReportRejection:
    """ReportRejection::new(task_id, report_id, time, reason) (:1538); config_id: OutdatedHpkeConfig's."""

    task_id: bytes
    report_id: bytes
    time: int
    reason: ReportRejectionReason
    config_id: int | None = None


@dataclass(frozen=True)
class StoredReport:
    """LeaderStoredReport::new (:1680-1687) with the leader input share left on the device: `row` is its row of
    UploadOutcome.rows, which leader_init_device reads in place."""

    task_id: bytes
    metadata: ReportMetadata
    public_share: bytes
    extensions: tuple
    row: int
    helper_encrypted_input_share: HpkeCiphertext


@dataclass
class UploadTask:
    """What handle_upload_generic reads of an AggregatorTask: hpke_keys are the task's keypairs by config id,
    janus_amd.hpke.HpkeOpener contexts created with application_info(recipient=ROLE_LEADER)."""

    task_id: bytes
    hpke_keys: dict
    tolerable_clock_skew: int = 0
    task_expiration: int | None = None
    report_expiry_age: int | None = None


@dataclass
class UploadOutcome:
    results: list                        # per report: StoredReport or ReportRejection
    rows: object = None                  # torch uint8[m, lis_stride] on the device (None: no report reached it)
    lis_stride: int = 0
    status: dict = field(default_factory=dict)      # report index -> open status (OPEN_STATUS key) where not OK
    counters: Counter = field(default_factory=Counter)  # upload_decrypt_failure / upload_decode_failure


def handle_upload(engine: HelperEngine, task: UploadTask, reports: list, now: int, global_keypairs=None,
                  lis_stride: int = 0) -> UploadOutcome:
    """VdafOps::handle_upload_generic (aggregator/src/aggregator.rs:1513-1694) for a batch of Reports (encoded
    bytes or messages.Report), in the reference's order per report: the three time checks on the host (TooEarly:
    time after now + tolerable_clock_skew, :1544-1553; TaskExpired, :1557-1561; Expired: now after time +
    report_expiry_age, :1564-1573), the public share's length (DecodeFailure, :1580-1593), then for all that are
    left one engine.leader_upload_open: HPKE open with the task's keypair and then the global one of the same
    config id (OutdatedHpkeConfig when neither exists, DecryptFailure, :1602-1651), PlaintextInputShare and leader
    input share decode (DecodeFailure, :1653-1678). Each report maps to a StoredReport (what goes to the report
    writer; its input share stays on the device) or to a ReportRejection."""
    from .engine import KEY_NONE, OPEN_OK
    from .messages import Report

    v = engine.vdaf
    reports = [Report.decode(r) if isinstance(r, (bytes, bytearray)) else r for r in reports]
    out = UploadOutcome([None] * len(reports))

    def reject(i: int, reason: ReportRejectionReason, config_id: int | None = None):
        md = reports[i].metadata
        out.results[i] = ReportRejection(task.task_id, md.report_id, md.time, reason, config_id)

    globals_ = dict(global_keypairs or {})
    keypairs: list = []
    slot: dict[int, int] = {}

    def key_slot(k) -> int:
        if id(k) not in slot:
            slot[id(k)] = len(keypairs)
            keypairs.append(k)
        return slot[id(k)]

    deadline = now + task.tolerable_clock_skew
    rows: list[int] = []
    key_index = []
    for i, r in enumerate(reports):
        t = r.metadata.time
        if t > deadline:
            reject(i, ReportRejectionReason.TooEarly)
        elif task.task_expiration is not None and t > task.task_expiration:
            reject(i, ReportRejectionReason.TaskExpired)
        elif task.report_expiry_age is not None and now > t + task.report_expiry_age:
            reject(i, ReportRejectionReason.Expired)
        elif len(r.public_share) != v.public_share_len:
            out.counters["upload_decode_failure"] += 1
            reject(i, ReportRejectionReason.DecodeFailure)
        else:
            cfg = r.leader_encrypted_input_share.config_id
            task_k, glob_k = task.hpke_keys.get(cfg), globals_.get(cfg)
            first, second = (task_k, glob_k) if task_k is not None else (glob_k, None)
            if first is None:
                key_index.append((KEY_NONE, KEY_NONE))
            else:
                key_index.append((key_slot(first), key_slot(second) if second is not None else KEY_NONE))
            if len(keypairs) > 8:
                raise ValueError("more than JX_ENC_MAX_KEYPAIRS distinct keypairs in one upload batch")
            rows.append(i)
    if not rows:
        return out
    md = [reports[i].metadata for i in rows]
    res = engine.leader_upload_open(
        np.frombuffer(b"".join(x.report_id for x in md), np.uint8).reshape(len(rows), 16),
        np.array([x.time for x in md], np.uint64),
        np.frombuffer(b"".join(reports[i].public_share for i in rows), np.uint8), task.task_id, keypairs,
        np.array(key_index, np.uint8), [reports[i].leader_encrypted_input_share.encapsulated_key for i in rows],
        [reports[i].leader_encrypted_input_share.payload for i in rows], lis_stride=lis_stride)
    out.rows, out.lis_stride = res.rows, res.lis_stride
    for j, i in enumerate(rows):
        st = int(res.status[j])
        r = reports[i]
        if st == OPEN_OK:
            exts = PlaintextInputShare.decode(len(res.extensions[j]).to_bytes(2, "big") + res.extensions[j] +
                                              bytes(4)).extensions
            out.results[i] = StoredReport(task.task_id, r.metadata, r.public_share, exts, j,
                                          r.helper_encrypted_input_share)
            continue
        out.status[i] = st
        if st == 7:  # JX_OPEN_UNKNOWN_CONFIG
            reject(i, ReportRejectionReason.OutdatedHpkeConfig, r.leader_encrypted_input_share.config_id)
        elif st == 1:  # JX_OPEN_HPKE_DECRYPT_ERROR
            out.counters["upload_decrypt_failure"] += 1
            reject(i, ReportRejectionReason.DecryptFailure)
        else:  # the plaintext's framing (2) or the input share (6)
            out.counters["upload_decode_failure"] += 1
            reject(i, ReportRejectionReason.DecodeFailure)
    return out


@dataclass
class UploadWireOutcome:
    """handle_upload_wire's result, as arrays: nothing here is a Python object per report until results() is called.
    status: uint8[n], engine.UPLOAD_* per upload; row_of: uint32[n], the upload's row of `rows` (UPLOAD_NO_ROW: none);
    open_status: uint8[m], OPEN_OK or an OPEN_STATUS key per row; rows: torch uint8[m, lis_stride] on the device, the
    leader input shares leader_init_device reads in place (zeros where the open failed; None when m is 0); counters as
    UploadOutcome's; helper_shares: (config_ids uint8[m], d_encs, enc_offsets uint64[m + 1], d_payloads,
    payload_offsets uint64[m + 1]), the helper's ciphertexts of the m rows with device pointers and host offsets, as
    engine.encode_init_req takes them. `req` is the engine's UploadReq: it owns the device memory of helper_shares and
    the ids, times and public shares of the rows (req.d, req.times), so release() (or the end of a `with`) comes after
    their last use."""

    task_id: bytes
    req: object
    status: np.ndarray
    row_of: np.ndarray
    open_status: np.ndarray
    rows: object = None
    lis_stride: int = 0
    counters: Counter = field(default_factory=Counter)
    helper_shares: tuple = ()
    _ext: object = None      # torch uint8 on the device: row k's extension bytes at the leader payload's offset
    _ext_len: object = None  # torch int32[m]
    _unknown_config: dict = field(default_factory=dict)  # upload index -> leader config id, where no keypair has it

    def results(self) -> list:
        """The object path's list (UploadOutcome.results): per upload a StoredReport or a ReportRejection; None for an
        upload that does not parse, which the reference answers with invalidMessage before any handler runs. Copies
        the helper ciphertexts, public shares and extensions to the host."""
        from .engine import (OPEN_OK, UPLOAD_EXPIRED, UPLOAD_MALFORMED, UPLOAD_ODD_PUBLIC_SHARE, UPLOAD_OK,
                             UPLOAD_TASK_EXPIRED, UPLOAD_TOO_EARLY)
        req = self.req
        n, m = req.n, req.m
        reason = {UPLOAD_TOO_EARLY: ReportRejectionReason.TooEarly, UPLOAD_TASK_EXPIRED: ReportRejectionReason.TaskExpired,
                  UPLOAD_EXPIRED: ReportRejectionReason.Expired, UPLOAD_ODD_PUBLIC_SHARE: ReportRejectionReason.DecodeFailure}
        host = lambda name: req.device_bytes(name).cpu().numpy().tobytes()  # noqa: E731
        ps, encs, pays = host("public_shares"), host("helper_encs"), host("helper_payloads")
        PS = len(ps) // m if m else 0
        ext = self._ext.cpu().numpy() if m else None
        ext_len = self._ext_len.cpu().numpy() if m else None
        eo, po, lpo = req.helper_enc_offsets, req.helper_payload_offsets, req.leader_payload_offsets
        out: list = [None] * n
        for i in range(n):
            st, rid, t = int(self.status[i]), req.report_ids[i].tobytes(), int(req.all_times[i])
            if st == UPLOAD_MALFORMED:
                continue
            if st != UPLOAD_OK:
                out[i] = ReportRejection(self.task_id, rid, t, reason[st])
                continue
            k = int(self.row_of[i])
            op = int(self.open_status[k])
            if op == OPEN_OK:
                e = ext[int(lpo[k]):int(lpo[k]) + int(ext_len[k])].tobytes()
                exts = PlaintextInputShare.decode(len(e).to_bytes(2, "big") + e + bytes(4)).extensions
                ct = HpkeCiphertext(int(req.helper_config_ids[k]), encs[int(eo[k]):int(eo[k + 1])], pays[int(po[k]):int(po[k + 1])])
                out[i] = StoredReport(self.task_id, ReportMetadata(rid, t), ps[PS * k:PS * k + PS], exts, k, ct)
            elif op == 7:  # JX_OPEN_UNKNOWN_CONFIG
                out[i] = ReportRejection(self.task_id, rid, t, ReportRejectionReason.OutdatedHpkeConfig, self._unknown_config.get(i))
            elif op == 1:  # JX_OPEN_HPKE_DECRYPT_ERROR
                out[i] = ReportRejection(self.task_id, rid, t, ReportRejectionReason.DecryptFailure)
            else:
                out[i] = ReportRejection(self.task_id, rid, t, ReportRejectionReason.DecodeFailure)
        return out

    def release(self):
        self.rows = self._ext = self._ext_len = None
        self.helper_shares = ()
        self.req.release()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()


def handle_upload_wire(engine: HelperEngine, task: UploadTask, bodies, body_offsets, now: int, global_keypairs=None,
                       lis_stride: int = 0) -> UploadWireOutcome:
    """handle_upload from the upload bodies as wire bytes: n encoded Reports back to back (`bodies`: bytes, or a torch
    uint8 tensor on the engine's device, as client.prepare_report_bodies returns it) with body_offsets[n + 1]. One
    engine.decode_uploads parses every body, makes the three time checks and the public-share check and lays the
    accepted reports out on the device; one jx_leader_upload_open_device over the handle's arrays opens and validates
    their leader shares. The key slots are handle_upload's: per config id the task's keypair first, then the global one
    of the same id; the two tables cover every config id the task and the global keys hold, so more than
    JX_ENC_MAX_KEYPAIRS distinct keypairs among them is a ValueError here, where handle_upload counts only those a batch
    uses. Nothing per report runs in Python; UploadWireOutcome.results() gives the object path's list for callers that
    want it. The helper's ciphertexts never leave the device: outcome.helper_shares feeds
    engine.encode_init_req."""
    import ctypes

    import torch

    from ._lib import check
    from .engine import KEY_NONE, UPLOAD_ODD_PUBLIC_SHARE, _ptr

    globals_ = dict(global_keypairs or {})
    keypairs: list = []
    slot: dict[int, int] = {}

    def key_slot(k) -> int:
        if id(k) not in slot:
            slot[id(k)] = len(keypairs)
            keypairs.append(k)
        return slot[id(k)]

    key_first, key_second = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    for cfg in sorted(set(task.hpke_keys) | set(globals_)):
        task_k, glob_k = task.hpke_keys.get(cfg), globals_.get(cfg)
        first, second = (task_k, glob_k) if task_k is not None else (glob_k, None)
        if first is not None:
            key_first[cfg] = key_slot(first)
            if second is not None:
                key_second[cfg] = key_slot(second)
    if len(keypairs) > 8:
        raise ValueError("more than JX_ENC_MAX_KEYPAIRS distinct keypairs for one upload batch")
    on_device = hasattr(bodies, "data_ptr")
    req = engine.decode_uploads(bodies, body_offsets, now, key_first, key_second, task.tolerable_clock_skew,
                                task.task_expiration, task.report_expiry_age, length=int(bodies.numel()) if on_device else None)
    out = UploadWireOutcome(task.task_id, req, req.status, req.row_of, np.zeros(0, np.uint8))
    out.counters["upload_decode_failure"] += req.status_count[UPLOAD_ODD_PUBLIC_SHARE]
    if not out.counters["upload_decode_failure"]:
        del out.counters["upload_decode_failure"]
    m = req.m
    if m == 0:
        return out
    v = engine.vdaf
    stride = lis_stride or v.leader_input_share_len
    dev = torch.device("cuda", engine.device)
    task_b = np.frombuffer(task.task_id, np.uint8).copy()
    hs = (ctypes.c_void_p * max(1, len(keypairs)))(*[k.handle for k in keypairs])
    u64p = ctypes.POINTER(ctypes.c_uint64)
    a = req.d
    with torch.cuda.device(dev):
        d_rows = torch.zeros(m * stride + 16, dtype=torch.uint8, device=dev)
        skew = (-d_rows.data_ptr()) % 16
        rows = d_rows[skew:skew + m * stride].view(m, stride)
        d_ext = torch.zeros(max(req.leader_payload_bytes, 1), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(m, dtype=torch.int32, device=dev)
        d_st = torch.zeros(m, dtype=torch.uint8, device=dev)
        with engine._ordered(None):
            st = engine._L.jx_leader_upload_open_device(
                engine._h, m, a.d_report_ids, req.times.ctypes.data_as(u64p), a.d_public_shares, _ptr(task_b), hs,
                len(keypairs), _ptr(np.ascontiguousarray(req.key_index)), a.d_leader_encs,
                req.leader_enc_offsets.ctypes.data_as(u64p), a.d_leader_payloads,
                req.leader_payload_offsets.ctypes.data_as(u64p), rows.data_ptr(), lis_stride, d_ext.data_ptr(),
                d_len.data_ptr(), d_st.data_ptr())
            check(st, engine._h, "jx_leader_upload_open_device")
        out.open_status = d_st.cpu().numpy()
    out.rows, out.lis_stride, out._ext, out._ext_len = rows, stride, d_ext, d_len
    counts = np.bincount(out.open_status, minlength=8)
    if counts[1]:
        out.counters["upload_decrypt_failure"] += int(counts[1])
    if counts[2] + counts[6]:
        out.counters["upload_decode_failure"] += int(counts[2] + counts[6])
    out.helper_shares = (req.helper_config_ids, a.d_helper_encs, req.helper_enc_offsets, a.d_helper_payloads,
                         req.helper_payload_offsets)
    if counts[7]:  # OutdatedHpkeConfig names the config id: one byte per such upload, right after its public share
        k = np.nonzero(out.open_status == 7)[0]
        i = req.index[k].astype(np.int64)
        at = np.asarray(body_offsets, np.uint64)[i].astype(np.int64) + 28 + v.public_share_len
        if on_device:
            ids = bodies[torch.from_numpy(at).to(bodies.device)].cpu().numpy()
        else:
            ids = np.frombuffer(bytes(bodies), np.uint8)[at]
        out._unknown_config = dict(zip(i.tolist(), ids.tolist()))
    return out


# ----------------------------------------------------------------------------- collection (time-interval tasks)
#
# The helper's handle_aggregate_share_generic (aggregator/src/aggregator.rs:2766-2965) and the leader's collection step
# (aggregator/src/aggregator/collection_job_driver.rs), with the merge, the checks and the seal of a collection in one
# engine call (HelperEngine.collect_seal). Only NoDifferentialPrivacy is covered: no noise is added to a share. A
# BatchAggregation row's integer batch identifier is its time bucket's number, bucket start // time_precision.


class BatchInvalid(ValueError):
    """The batch interval does not meet the task's time precision (Error::BatchInvalid)."""


class AggregateShareRequestRejected(ValueError):
    """The batch is past its report expiry: eligible for garbage collection (Error::AggregateShareRequestRejected)."""


class InvalidBatchSize(ValueError):
    """task.validate_batch_size refused the batch's report count (Error::InvalidBatchSize)."""

    def __init__(self, task_id: bytes, report_count: int):
        super().__init__(f"invalid batch size: {report_count} reports")
        self.task_id, self.report_count = task_id, report_count


class BatchMismatch(ValueError):
    """The two aggregators' report counts or checksums differ (Error::BatchMismatch, aggregator.rs:2927-2939)."""

    def __init__(self, task_id: bytes, own_report_count: int, own_checksum: bytes, peer_report_count: int,
                 peer_checksum: bytes):
        super().__init__(f"batch mismatch: own {own_report_count} reports / {own_checksum.hex()}, peer "
                         f"{peer_report_count} / {peer_checksum.hex()}")
        self.task_id = task_id
        self.own_report_count, self.own_checksum = own_report_count, own_checksum
        self.peer_report_count, self.peer_checksum = peer_report_count, peer_checksum


class CollectionFailed(RuntimeError):
    """A batch-aggregation row that does not decode (an element >= p), or a seal that did not come about."""


@dataclass(frozen=True)
class CollectTask:
    """What collection reads of an AggregatorTask (aggregator_core/src/task.rs): max_batch_size 0 = none."""

    task_id: bytes
    time_precision: int
    min_batch_size: int
    max_batch_size: int = 0
    report_expiry_age: int | None = None
    collector_config_id: int = 0

    def validate_batch_interval(self, iv) -> bool:
        """TimeInterval::validate_collection_identifier (aggregator_core/src/query_type.rs:270-282)."""
        p = self.time_precision
        return iv.duration >= p and iv.start % p == 0 and iv.duration % p == 0

    def batch_identifiers(self, iv) -> list[int]:
        """batch_identifiers_for_collection_identifier: the interval's time buckets, by number."""
        return [iv.start // self.time_precision + k for k in range(iv.duration // self.time_precision)]


@dataclass(frozen=True)
class AggregateShareJob:
    """models.rs AggregateShareJob: the UNENCRYPTED share, so that a repeated request is sealed to the collector key
    valid then (aggregator.rs:2941-2944)."""

    aggregate_share: bytes
    report_count: int
    checksum: bytes


def _collection_rows(tx, task: CollectTask, writer, iv):
    """The rows of every batch identifier of the interval over every shard ord, and the (identifier, ord) pairs that
    have none (empty_batch_aggregations, aggregator.rs:2968-3008)."""
    rows, missing = [], []
    for s in task.batch_identifiers(iv):
        for ord_ in range(writer.shard_count):
            row = tx.get((s, ord_))
            if row is None:
                missing.append((s, ord_))
            elif row.state == SCRUBBED:
                raise Scrubbed("batch aggregation was scrubbed")  # compute_aggregate_share, aggregate_share.rs:69-71
            else:
                rows.append(row)
    return rows, missing


def _row_records(engine: HelperEngine, rows) -> bytes:
    """The rows as shard records (share || count u64 LE || checksum); a row without a share is a zero share."""
    pt = engine.output_len * engine.field_bytes
    return b"".join((r.aggregate_share if r.aggregate_share is not None else bytes(pt)) +
                    r.report_count.to_bytes(8, "little") + r.checksum for r in rows)


def _raise_collect_status(task: CollectTask, status: int, count: int, checksum: bytes, peer=None):
    if status == COLLECT_OK:
        return
    if status == COLLECT_INVALID_BATCH_SIZE:
        raise InvalidBatchSize(task.task_id, count)
    if status == COLLECT_BATCH_MISMATCH:
        raise BatchMismatch(task.task_id, count, checksum, peer[0], peer[1])
    raise CollectionFailed(f"collection failed with status {status}")


def _aligned(iv, precision: int):
    """Interval::align_to_time_precision (core/src/time.rs:319-335): the start down, the duration up, and one more
    step when the start's move left the end outside."""
    start = iv.start - iv.start % precision
    duration = -(-iv.duration // precision) * precision
    if iv.end > start + duration:
        duration += precision
    return Interval(start, duration)


def handle_aggregate_share(engine: HelperEngine, writer, task: CollectTask, req_body: bytes, collector_sender,
                           ephemeral_sk: bytes, now: int, cache: dict, inject_tx_failures: int = 0) -> bytes:
    """The helper's aggregate-share handler for a time-interval task. collector_sender: an HpkeSealer holding the
    collector's public key with the (AggregateShare, Helper -> Collector) application info; ephemeral_sk: 32 bytes of
    the caller's CSPRNG; cache: the AggregateShareJobs served so far, by (batch interval, aggregation parameter).
    Returns the AggregateShare body."""
    req = AggregateShareReq.decode(req_body, QUERY_TIME_INTERVAL)
    iv = req.batch_selector.batch_interval
    if not task.validate_batch_interval(iv):
        raise BatchInvalid(f"batch interval {iv} does not fit time precision {task.time_precision}")
    if task.report_expiry_age is not None and now > iv.end + task.report_expiry_age:
        raise AggregateShareRequestRejected("aggregate share request too late")
    aad = AggregateShareAad(task.task_id, req.aggregation_parameter, req.batch_selector).encode()
    key = ((iv.start, iv.duration), req.aggregation_parameter)
    peer = (req.report_count, req.checksum)
    job = cache.get(key)
    if job is not None:
        # served before: the stored share is sealed afresh; the comparison runs against this request
        rec = job.aggregate_share + job.report_count.to_bytes(8, "little") + job.checksum
        out = engine.collect_seal(rec, [[0]], [aad], ephemeral_sk, collector_sender, 0, 0, expect=[peer])
        _raise_collect_status(task, int(out.status[0]), job.report_count, job.checksum, peer)
    else:
        def closure(tx):
            rows, missing = _collection_rows(tx, task, writer, iv)
            out = engine.collect_seal(_row_records(engine, rows), [list(range(len(rows)))], [aad], ephemeral_sk,
                                      collector_sender, task.min_batch_size, task.max_batch_size, expect=[peer],
                                      want_shares=True)
            count, checksum = int(out.counts[0]), out.checksums[0].tobytes()
            _raise_collect_status(task, int(out.status[0]), count, checksum, peer)
            for r in rows:
                tx[(r.batch_identifier, r.ord)] = r.scrubbed()
            for s, ord_ in missing:
                tx[(s, ord_)] = BatchAggregation(s, ord_, field_bytes=writer.field_bytes).scrubbed()
            return out, AggregateShareJob(out.shares[0].tobytes(), count, checksum)

        out, job = writer.datastore.run_tx(closure, inject_tx_failures)
        cache[key] = job
    ct = HpkeCiphertext(task.collector_config_id, out.encs[0].tobytes(), out.cts[0].tobytes())
    return AggregateShare(ct).encode()


@dataclass
class LeaderCollection:
    """The leader's half of a collection: what goes to the helper, and what waits for its answer."""

    request_body: bytes            # the AggregateShareReq
    leader_share: HpkeCiphertext   # sealed under (AggregateShare, Leader -> Collector)
    report_count: int
    checksum: bytes
    interval: Interval             # the merged client-timestamp interval, aligned outward to the time precision
    aggregate_share: bytes         # unencrypted (the leader's AggregateShareJob counterpart)


def leader_collect(engine: HelperEngine, writer, task: CollectTask, batch_interval, agg_param: bytes, collector_sender,
                   ephemeral_sk: bytes, inject_tx_failures: int = 0) -> LeaderCollection:
    """The leader's collection step, first half: merge its rows of the batch interval (the same engine call, with
    nothing to compare against), mark them collected, seal its share under the (AggregateShare, Leader -> Collector)
    info of collector_sender, and write the AggregateShareReq for the helper."""
    if not task.validate_batch_interval(batch_interval):
        raise BatchInvalid(f"batch interval {batch_interval} does not fit time precision {task.time_precision}")
    sel = BatchSelector.time_interval(batch_interval)
    aad = AggregateShareAad(task.task_id, agg_param, sel).encode()

    def closure(tx):
        rows, missing = _collection_rows(tx, task, writer, batch_interval)
        if any(r.state != AGGREGATING for r in rows):
            raise AlreadyCollected("batch aggregation was already collected")
        out = engine.collect_seal(_row_records(engine, rows), [list(range(len(rows)))], [aad], ephemeral_sk,
                                  collector_sender, task.min_batch_size, task.max_batch_size, want_shares=True)
        count, checksum = int(out.counts[0]), out.checksums[0].tobytes()
        _raise_collect_status(task, int(out.status[0]), count, checksum)
        span = Interval.EMPTY
        for r in rows:
            span = span.merge(r.client_timestamp_interval)
            tx[(r.batch_identifier, r.ord)] = r.collected()
        for s, ord_ in missing:
            tx[(s, ord_)] = BatchAggregation(s, ord_, field_bytes=writer.field_bytes).collected()
        return out, count, checksum, _aligned(span, task.time_precision)

    out, count, checksum, span = writer.datastore.run_tx(closure, inject_tx_failures)
    body = AggregateShareReq(sel, agg_param, count, checksum).encode()
    ct = HpkeCiphertext(task.collector_config_id, out.encs[0].tobytes(), out.cts[0].tobytes())
    return LeaderCollection(body, ct, count, checksum, span, out.shares[0].tobytes())


def leader_finish_collection(step: LeaderCollection, helper_body: bytes) -> bytes:
    """Second half: the helper's AggregateShare body in, the Collection body for the collector out."""
    helper = AggregateShare.decode(helper_body).encrypted_aggregate_share
    return Collection(PartialBatchSelector.time_interval(), step.report_count, step.interval, step.leader_share,
                      helper).encode()
