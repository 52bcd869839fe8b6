// jx_engine_fused.cpp — fused prepare + aggregate: the four jx_helper_prep_aggregate* calls describe themselves as a
// FusedCall, and run_fused runs its launches on the engine stream or over the pipelines (jx_fused_plan.h).
#include <cstring>
#include <functional>
#include <map>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_fused_plan.h"

using namespace jx;
using namespace jxi;

// Staging for up to P pipelines: the first one may wait for the arena, the others take what is free
// now (so two calls never wait on each other holding half their pipelines). *got = pipelines staged.
static int32_t pipes_acquire(jx_engine* e, uint32_t P, uint64_t chunk, uint32_t flags, uint64_t ct_bytes, Stage* st,
                             uint32_t* got) {
  *got = 0;
  while (e->pipes.size() < P) {
    jx_engine* q = new_child(e);
    if (!q) return fail(e, JX_E_HIP, "pipelines: stream creation failed");
    e->pipes.push_back(q);
  }
  if (!e->ev_pipe) HIPCHK(e, hipEventCreateWithFlags(&e->ev_pipe, hipEventDisableTiming));
  for (uint32_t k = 0; k < P; k++) {
    jx_engine* q = e->pipes[k];
    q->force_slow = e->force_slow;
    q->k1_forced = e->k1_forced;
    q->lanes_wg_cap = e->lanes_wg_cap;
    q->timing = e->timing;
    q->acc_chunks = e->acc_chunks;
    int32_t rc = stage_acquire(q, chunk, flags, st[k], k == 0, ct_bytes);
    if (rc) {
      if (k == 0) return rc;
      thread_error().clear();  // run with the pipelines that fit (retried on the next call)
      break;
    }
    *got = k + 1;
  }
  return JX_OK;
}

// ---------------------------------------------------------------------------- fused prepare + aggregate
// jx_helper_prep_aggregate (host buffers), jx_helper_prep_aggregate_device and their sealed forms
// (jx_helper_prep_aggregate_encrypted[_device]) describe their call with a FusedCall; run_fused runs every launch of
// it, on the engine stream or over the pipelines, as fused_plan says.

// One launch's inputs on the device. status: a sealed call's open status of the launch's reports, which run_fused
// names before it asks for the inputs (the rows kernels write it) and masks the verdicts with after K3; null for
// plaintext input shares.
struct FusedIn {
  const uint8_t *nonces, *ps, *his, *lps;
  uint8_t* status;
};

struct FusedCall {
  bool host;  // the host-buffer form: its launches stage their inputs, `download` brings the results back
  // The inputs of launch [off, off + m) on lane q. The host form queues its four copies into q's staging (pageable:
  // the host thread stages them, so with pipelines they go out while another pipeline's kernels run); the device
  // form names the caller's arrays at off. A sealed call (sealed; its input shares arrive under HPKE) also stages the
  // launch's rows (and, in the host form, its ciphertext span), queues the rows kernels on q's stream and names
  // q->d_his as the launch's helper input shares.
  bool sealed;
  uint64_t ct_bytes;  // sealed: each lane's two ciphertext regions (sealed_setup)
  std::function<int32_t(jx_engine* q, uint64_t off, uint64_t m, FusedIn& in)> inputs;
  // Device arrays for the whole call's verdicts and prep messages (row off is launch [off, ...)'s first). Null:
  // each launch's go to its lane's staging (SG_RES), or, for the pipelined host form, to per-call scratch.
  uint8_t *verdicts, *msgs;
  uint8_t* status;  // sealed: the same for the open status
  const uint32_t* dense;  // the reports' dense segment index (nullable)
  // Host form: copy rows [off, off + m) of the results, which start at dv / dm (sealed: and ds), to the caller's
  // buffers and wait for them. After every launch on the engine stream; once for the whole call after the
  // pipelines' join.
  std::function<int32_t(const uint8_t* dv, const uint8_t* dm, const uint8_t* ds, uint64_t off, uint64_t m)> download;
};

// The staging of one lane of a fused call. The pipelined host form keeps its results in per-call scratch.
// A sealed call's lanes also hold the helper input shares the rows kernels write (SG_HIN), the rows, the plaintext
// scratch and the open status (SG_ENC) and, in the device form, the launch's compact arrays (SG_ENCC).
static uint32_t fused_stage_flags(bool host, bool pipelined, bool sealed) {
  const uint32_t enc = sealed ? SG_ENC | SG_HIN | (host ? 0u : SG_ENCC) : 0u;
  if (!host) return SG_MEAS | SG_PREP | SG_RES | SG_ACC | enc;
  return SG_IN | SG_HIN | SG_MEAS | SG_PREP | SG_ACC | (pipelined ? 0u : SG_RES) | enc;
}

static int32_t run_fused(jx_engine* e, uint64_t n, const FusedPlan& plan, const std::vector<Segment>& targets,
                         const FusedCall& call) {
  const Cfg& c = e->cfg;
  const uint64_t chunk = plan.chunk;
  Stage pst[MAX_PIPES];
  uint32_t P = 0;
  int32_t rc = JX_OK;
  if (plan.pipes > 1) {
    rc = pipes_acquire(e, plan.pipes, chunk, fused_stage_flags(call.host, true, call.sealed), call.ct_bytes, pst, &P);
    if (rc) return rc;
  }
  const bool piped = P > 1;  // the lanes: e->pipes[0..P), else the engine itself
  e->last_pipes = piped ? P : 1;
  Stage st;
  Scratch hout;  // per call, from the arena (handed back after download's copies are queued)
  PtrTable tbl;
  uint8_t *dv = call.verdicts, *dm = call.msgs, *ds = call.status;
  if (piped) {
    if (call.host) {
      const uint64_t mb = c.jr_len ? n * c.seed : 0;
      rc = scratch_get(e, n + mb + (call.sealed ? n : 0), hout);
      if (rc) return rc;
      dv = hout.p();
      dm = hout.p() + n;
      if (call.sealed) ds = hout.p() + n + mb;
    }
    // every pipeline orders after the caller's producers (jx_engine_wait_stream / _event act on the
    // engine stream) and the engine stream after every pipeline (the join), so the call keeps the
    // single-stream ordering contract
    HIPCHK(e, hipEventRecord(e->ev_pipe, e->stream));
    for (uint32_t k = 0; k < P; k++) HIPCHK(e, hipStreamWaitEvent(e->pipes[k]->stream, e->ev_pipe, 0));
  } else {
    if (P == 1) pst[0].release();  // one pipeline's staging only: run on the engine stream
    rc = stage_acquire(e, chunk, fused_stage_flags(call.host, false, call.sealed), st, true, call.ct_bytes);
    if (rc) return rc;
    // several aggregations (one pipeline, says the plan): the pointer table is uploaded once for every launch
    // of the call (no per-launch host sync)
    if (call.dense && targets.size() > 1) {
      rc = upload_targets(e, targets, tbl);
      if (rc) return rc;
    }
  }
  auto run = [&]() -> int32_t {
    uint64_t off = 0;
    for (uint64_t i = 0; i < plan.launches; i++, off += chunk) {
      jx_engine* q = piped ? e->pipes[i % P] : e;
      const uint64_t m = (n - off) < chunk ? (n - off) : chunk;
      FusedIn in{};
      uint8_t* const sout = !call.sealed ? nullptr : ds ? ds + off : q->d_status;
      in.status = sout;
      int32_t r = call.inputs(q, off, m, in);
      if (r) return r;
      uint8_t* vout = dv ? dv + off : q->d_verdicts;
      uint8_t* mout = dm ? dm + off * c.seed : q->d_msgs;
      r = prep_core(q, m, in.nonces, in.ps, in.his, in.lps, vout, mout, staging_outs(q));
      if (r) return r;
      // a report that did not open never reaches an aggregation: its verdict becomes JX_OPEN_FAILURE before K4
      if (sout) HIPCHK(e, launch_open_mask(sout, vout, m, q->stream));
      if (piped && i > 0) HIPCHK(e, hipStreamWaitEvent(q->stream, e->ev_pipe, 0));  // the previous launch's K4
      r = accumulate_into(q, AccSrc{m, staging_outs(q), vout, in.nonces}, nullptr,
                          call.dense ? call.dense + off : nullptr, targets, tbl.d() ? &tbl : nullptr);
      if (r) return r;
      if (piped) HIPCHK(e, hipEventRecord(e->ev_pipe, q->stream));
      else if (call.host && (r = call.download(vout, mout, sout, off, m))) return r;
    }
    return JX_OK;
  };
  rc = run();
  // the join, also after a failed launch: whatever was queued on a pipeline stays ordered before the
  // engine stream's later work (and jx_engine_sync)
  for (uint32_t k = 0; piped && k < P; k++) {
    HIPCHK(e, hipEventRecord(e->pipes[k]->ev_join, e->pipes[k]->stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->pipes[k]->ev_join, 0));
  }
  if (rc || !call.host) return rc;
  if (piped) return call.download(dv, dm, ds, 0, n);  // the pipelines' kernel timings: jx_engine_timing_read drains them
  return drain_timing(e);
}

extern "C" {

int32_t jx_helper_prep_aggregate(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                 const uint8_t* helper_input_shares, const uint8_t* leader_prep_shares,
                                 uint32_t segment, uint8_t* out_prep_msgs, uint8_t* out_verdicts) {
  if (!e || !nonces || !helper_input_shares || !leader_prep_shares) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !public_shares) return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  Segment* seg = nullptr;
  int32_t rc = get_segment(e, segment, &seg);
  if (rc) return rc;
  const std::vector<Segment> targets{*seg};
  const FusedPlan plan =
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, !one_kernel_chain(c), false, true);
  FusedCall call{};
  call.host = true;
  call.inputs = [&](jx_engine* q, uint64_t off, uint64_t m, FusedIn& in) -> int32_t {
    HIPCHK(e, hipMemcpyAsync(q->d_nonces, nonces + off * 16, m * 16, hipMemcpyHostToDevice, q->stream));
    if (c.ps_bytes)
      HIPCHK(e, hipMemcpyAsync(q->d_ps, public_shares + off * c.ps_bytes, m * c.ps_bytes, hipMemcpyHostToDevice,
                               q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_his, helper_input_shares + off * c.his_bytes, m * c.his_bytes,
                             hipMemcpyHostToDevice, q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_lps, leader_prep_shares + off * c.lps_bytes, m * c.lps_bytes,
                             hipMemcpyHostToDevice, q->stream));
    in = FusedIn{q->d_nonces, q->d_ps, q->d_his, q->d_lps, nullptr};
    return JX_OK;
  };
  call.download = [&](const uint8_t* dv, const uint8_t* dm, const uint8_t*, uint64_t off, uint64_t m) -> int32_t {
    if (out_verdicts) HIPCHK(e, hipMemcpyAsync(out_verdicts + off, dv, m, hipMemcpyDeviceToHost, e->stream));
    if (out_prep_msgs && c.jr_len)
      HIPCHK(e, hipMemcpyAsync(out_prep_msgs + off * c.seed, dm, m * c.seed, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return JX_OK;
  };
  return run_fused(e, n, plan, targets, call);
}

int32_t jx_helper_prep_aggregate_device(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_ps,
                                        const void* d_his, const void* d_lps, const void* d_segment,
                                        const uint32_t* segment_ids, uint32_t nsegments, void* d_out_prep_msgs,
                                        void* d_out_verdicts) {
  if (!e || !d_nonces || !d_his || !d_lps || !segment_ids || nsegments == 0) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !d_ps) return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<Segment> targets;
  int32_t rc = segment_targets(e, segment_ids, nsegments, targets);
  if (rc) return rc;
  const uint8_t *N = (const uint8_t*)d_nonces, *PS = (const uint8_t*)d_ps, *H = (const uint8_t*)d_his,
                *L = (const uint8_t*)d_lps;
  const bool many = d_segment && targets.size() > 1;
  const FusedPlan plan =
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, !one_kernel_chain(c), many, false);
  FusedCall call{};
  call.inputs = [&](jx_engine*, uint64_t off, uint64_t, FusedIn& in) -> int32_t {
    in = FusedIn{N + off * 16, PS ? PS + off * c.ps_bytes : nullptr, H + off * c.his_bytes, L + off * c.lps_bytes,
                 nullptr};
    return JX_OK;
  };
  call.verdicts = (uint8_t*)d_out_verdicts;
  call.msgs = c.jr_len ? (uint8_t*)d_out_prep_msgs : nullptr;
  call.dense = (const uint32_t*)d_segment;
  return run_fused(e, n, plan, targets, call);
}

// ---- the fused calls from sealed helper input shares

namespace {
// What the two sealed fused calls share beyond their EncJob: the request's keypairs as the row rule reads them,
// which rows kernels they need, the device's key registry, and per launch of the plan the number of 65-byte
// encapsulated keys (a launch without one runs no P-256 rows kernel).
struct SealedCall {
  EncJob job;
  EncRowKeys keys{};
  bool suites = false, p256 = false;
  const HpkeKeyRow* reg = nullptr;
  uint32_t reg_cap = 0;
  std::vector<uint64_t> n65;
};

// Fill `sc` from its checked job and return the lanes' ct_bytes (FusedCall): the largest ciphertext region any launch of
// the plan needs. Host form: the launch's ciphertext span, then its 65-byte keys (fill_enc_rows's layout). Device
// form: the ciphertexts stay in the caller's array, so the region holds the plaintext scratch of the span (d_pt) and,
// in d_ct, one 65-byte slot per report of a launch that can hold an ENC_ROW_ENC65 row.
uint64_t sealed_setup(jx_engine* e, uint64_t n, const FusedPlan& plan, bool host, SealedCall& sc) {
  const EncJob& j = sc.job;
  sc.keys = enc_row_keys(j);
  for (uint32_t k = 0; k < j.nkeys; k++) {
    sc.suites = sc.suites || !hpke_default_suite(j.keypairs[k]);
    sc.p256 = sc.p256 || sc.keys.klen[k] == 65;
  }
  hpke_registry(e->device, &sc.reg, &sc.reg_cap);
  if (!sc.reg) sc.reg_cap = 0;
  sc.n65.assign(plan.launches, 0);
  uint64_t most = 1, off = 0;
  for (uint64_t i = 0; i < plan.launches; i++, off += plan.chunk) {
    const uint64_t m = (n - off) < plan.chunk ? (n - off) : plan.chunk;
    for (uint64_t r = off; j.enc_offsets && r < off + m; r++) sc.n65[i] += j.enc_offsets[r + 1] - j.enc_offsets[r] == 65;
    const uint64_t span = j.payload_offsets[off + m] - j.payload_offsets[off];
    const uint64_t slots = sc.p256 && sc.n65[i] ? 65 * (host ? sc.n65[i] : m) : 0;
    const uint64_t need = host ? span + slots : (span > slots ? span : slots);
    if (need > most) most = need;
  }
  return most;
}
}  // namespace

int32_t jx_helper_prep_aggregate_encrypted(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                           const uint8_t* public_shares, const uint8_t task_id[32],
                                           jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                           const uint8_t* encs, const uint64_t* enc_offsets, const uint8_t* payloads,
                                           const uint64_t* payload_offsets, uint32_t flags,
                                           const uint8_t* leader_prep_shares, uint32_t segment, uint8_t* out_prep_msgs,
                                           uint8_t* out_verdicts, uint8_t* out_open_status) {
  if (!e || (n && (!nonces || !times || !task_id || !key_index || !encs || !payload_offsets || !leader_prep_shares)))
    return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !public_shares) return JX_E_INVALID;
  SealedCall sc;
  if (const int32_t rc = enc_job_check(e, n, times, task_id, keypairs, nkeypairs, key_index, encs, enc_offsets, payloads,
                                       payload_offsets, flags, sc.job))
    return rc;
  if (n == 0) return JX_OK;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  Segment* seg = nullptr;
  int32_t rc = get_segment(e, segment, &seg);
  if (rc) return rc;
  const std::vector<Segment> targets{*seg};
  const FusedPlan plan =
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, !one_kernel_chain(c), false, true);
  const uint64_t ct_bytes = sealed_setup(e, n, plan, true, sc);
  // A lane's rows and 65-byte keys in pageable host memory, filled per launch on the staging thread (which copies
  // the launch's other inputs anyway) and rewritten for the lane's next launch once their upload has completed.
  struct LaneBuf {
    std::vector<EncRow> rows;
    std::vector<uint8_t> enc65;
    hipEvent_t ev = nullptr;
  };
  std::map<jx_engine*, LaneBuf> lanes;
  FusedCall call{};
  call.host = true;
  call.sealed = true;
  call.ct_bytes = ct_bytes;
  call.inputs = [&](jx_engine* q, uint64_t off, uint64_t m, FusedIn& in) -> int32_t {
    LaneBuf& lb = lanes[q];
    if (!lb.ev) HIPCHK(e, hipEventCreateWithFlags(&lb.ev, hipEventDisableTiming));
    else HIPCHK(e, hipEventSynchronize(lb.ev));
    EncJob sub = sc.job;  // the launch's reports as a job of their own
    sub.times += off;
    sub.key_index += 2 * off;
    sub.payload_offsets += off;
    if (sub.enc_offsets) sub.enc_offsets += off;
    else sub.encs += 32 * off;
    lb.rows.resize(m);
    lb.enc65.resize(65 * sc.n65[off / plan.chunk] + 1);
    const uint64_t pb = sub.payload_bytes(m), n65 = fill_enc_rows(sub, m, lb.rows.data(), 0, lb.enc65.data());
    HIPCHK(e, hipMemcpyAsync(q->d_nonces, nonces + off * 16, m * 16, hipMemcpyHostToDevice, q->stream));
    if (c.ps_bytes)
      HIPCHK(e, hipMemcpyAsync(q->d_ps, public_shares + off * c.ps_bytes, m * c.ps_bytes, hipMemcpyHostToDevice,
                               q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_lps, leader_prep_shares + off * c.lps_bytes, m * c.lps_bytes,
                             hipMemcpyHostToDevice, q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_encrows, lb.rows.data(), m * sizeof(EncRow), hipMemcpyHostToDevice, q->stream));
    if (pb)
      HIPCHK(e, hipMemcpyAsync(q->d_ct, payloads + sub.payload_offsets[0], pb, hipMemcpyHostToDevice, q->stream));
    if (n65) HIPCHK(e, hipMemcpyAsync(q->d_ct + pb, lb.enc65.data(), 65 * n65, hipMemcpyHostToDevice, q->stream));
    HIPCHK(e, hipEventRecord(lb.ev, q->stream));
    const HpkeRowsArgs ha{m, q->d_encrows, q->d_ct, q->d_pt, sc.reg, sc.reg_cap, q->d_nonces, q->d_ps, c.ps_bytes,
                          q->d_his, c.his_bytes, in.status};
    HIPCHK(e, launch_hpke_rows(ha, sc.suites, n65 != 0, q->stream));
    in = FusedIn{q->d_nonces, q->d_ps, q->d_his, q->d_lps, in.status};
    return JX_OK;
  };
  call.download = [&](const uint8_t* dv, const uint8_t* dm, const uint8_t* ds, uint64_t off, uint64_t m) -> int32_t {
    if (out_verdicts) HIPCHK(e, hipMemcpyAsync(out_verdicts + off, dv, m, hipMemcpyDeviceToHost, e->stream));
    if (out_prep_msgs && c.jr_len)
      HIPCHK(e, hipMemcpyAsync(out_prep_msgs + off * c.seed, dm, m * c.seed, hipMemcpyDeviceToHost, e->stream));
    if (out_open_status) HIPCHK(e, hipMemcpyAsync(out_open_status + off, ds, m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return JX_OK;
  };
  rc = run_fused(e, n, plan, targets, call);
  // the lanes' buffers are read by queued copies until the streams have passed them (also after a failed launch)
  for (auto& kv : lanes) {
    if (!kv.second.ev) continue;
    (void)hipEventSynchronize(kv.second.ev);
    (void)hipEventDestroy(kv.second.ev);
  }
  return rc;
}

int32_t jx_helper_prep_aggregate_encrypted_device(jx_engine* e, uint64_t n, const void* d_nonces, const uint64_t* times,
                                                  const void* d_public_shares, const uint8_t task_id[32],
                                                  jx_hpke* const* keypairs, uint32_t nkeypairs,
                                                  const uint8_t* key_index, const void* d_encs,
                                                  const uint64_t* enc_offsets, const void* d_payloads,
                                                  const uint64_t* payload_offsets, uint32_t flags, const void* d_lps,
                                                  const void* d_segment, const uint32_t* segment_ids, uint32_t nsegments,
                                                  void* d_out_prep_msgs, void* d_out_verdicts, void* d_out_open_status) {
  if (!e || !segment_ids || nsegments == 0 ||
      (n && (!d_nonces || !times || !task_id || !key_index || !d_encs || !payload_offsets || !d_lps)))
    return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !d_public_shares) return JX_E_INVALID;
  SealedCall sc;
  if (const int32_t rc = enc_job_check(e, n, times, task_id, keypairs, nkeypairs, key_index, (const uint8_t*)d_encs,
                                       enc_offsets, (const uint8_t*)d_payloads, payload_offsets, flags, sc.job))
    return rc;
  if (n == 0) return JX_OK;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<Segment> targets;
  int32_t rc = segment_targets(e, segment_ids, nsegments, targets);
  if (rc) return rc;
  const uint8_t *N = (const uint8_t*)d_nonces, *PS = (const uint8_t*)d_public_shares, *L = (const uint8_t*)d_lps,
                *ENCS = (const uint8_t*)d_encs, *PAY = (const uint8_t*)d_payloads;
  const bool many = d_segment && targets.size() > 1;
  const FusedPlan plan =
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, !one_kernel_chain(c), many, false);
  const uint64_t ct_bytes = sealed_setup(e, n, plan, false, sc);
  // The compact arrays leave the caller's memory here, into pinned memory that the launches' uploads read after
  // the call has returned: times | payload offsets | encapsulated-key offsets (when given) | key-index pairs.
  const size_t o_tm = 0, o_po = o_tm + n * 8, o_eo = o_po + (n + 1) * 8, o_ki = o_eo + (enc_offsets ? (n + 1) * 8 : 0),
               hbytes = o_ki + 2 * n;
  uint8_t* hb = nullptr;
  HIPCHK(e, e->h_enc.reserve(hbytes, (void**)&hb));
  memcpy(hb + o_tm, times, n * 8);
  memcpy(hb + o_po, payload_offsets, (n + 1) * 8);
  if (enc_offsets) memcpy(hb + o_eo, enc_offsets, (n + 1) * 8);
  memcpy(hb + o_ki, key_index, 2 * n);
  const uint64_t* const po = (const uint64_t*)(hb + o_po);
  FusedCall call{};
  call.sealed = true;
  call.ct_bytes = ct_bytes;
  call.inputs = [&](jx_engine* q, uint64_t off, uint64_t m, FusedIn& in) -> int32_t {
    HIPCHK(e, hipMemcpyAsync(q->d_ec_times, hb + o_tm + off * 8, m * 8, hipMemcpyHostToDevice, q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_ec_poff, hb + o_po + off * 8, (m + 1) * 8, hipMemcpyHostToDevice, q->stream));
    if (enc_offsets)
      HIPCHK(e, hipMemcpyAsync(q->d_ec_eoff, hb + o_eo + off * 8, (m + 1) * 8, hipMemcpyHostToDevice, q->stream));
    HIPCHK(e, hipMemcpyAsync(q->d_ec_kidx, hb + o_ki + off * 2, m * 2, hipMemcpyHostToDevice, q->stream));
    EncRowsArgs ra{};
    ra.n = m;
    ra.first = off;
    ra.times = q->d_ec_times;
    ra.key_index = q->d_ec_kidx;
    ra.enc_offsets = enc_offsets ? q->d_ec_eoff : nullptr;
    ra.payload_offsets = q->d_ec_poff;
    ra.encs = ENCS;
    ra.rows = q->d_encrows;
    // the 65-byte keys lie in the caller's d_encs, the rows kernels read them from their ciphertext base, which is
    // the caller's d_payloads: the row kernel copies them into the lane's d_ct and says where that is from d_payloads
    ra.enc65 = q->d_ct;
    ra.enc65_base = (uint64_t)reinterpret_cast<uintptr_t>(q->d_ct) - (uint64_t)reinterpret_cast<uintptr_t>(PAY);
    memcpy(ra.task_id, task_id, 32);
    ra.keys = sc.keys;
    HIPCHK(e, launch_enc_rows(ra, q->stream));
    // the ciphertexts in place at their own offsets; the plaintext scratch holds the launch's span alone
    const HpkeRowsArgs ha{m, q->d_encrows, PAY, q->d_pt - po[off], sc.reg, sc.reg_cap, N + off * 16,
                          PS ? PS + off * c.ps_bytes : nullptr, c.ps_bytes, q->d_his, c.his_bytes, in.status};
    HIPCHK(e, launch_hpke_rows(ha, sc.suites, sc.p256 && sc.n65[off / plan.chunk] != 0, q->stream));
    in = FusedIn{N + off * 16, PS ? PS + off * c.ps_bytes : nullptr, q->d_his, L + off * c.lps_bytes, in.status};
    return JX_OK;
  };
  call.verdicts = (uint8_t*)d_out_verdicts;
  call.msgs = c.jr_len ? (uint8_t*)d_out_prep_msgs : nullptr;
  call.status = (uint8_t*)d_out_open_status;
  call.dense = (const uint32_t*)d_segment;
  rc = run_fused(e, n, plan, targets, call);
  (void)e->h_enc.mark(e->stream);  // behind the join: every lane's uploads have read the pinned copy
  return rc;
}

}  // extern "C"
