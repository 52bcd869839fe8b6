// jx_engine_acc.cpp — accumulation: a prepared batch (or a fused launch's staging) into the running batch
// aggregations, the deferred small accumulations, and the calls that read, export and combine aggregations.
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "jx_engine_internal.h"

using namespace jx;
using namespace jxi;

// Accumulate the finished (and, with d_mask, accepted) reports of src into one aggregation. With
// d_dense (dense per-report indices), only reports whose index is 0 are taken.
static int32_t accumulate_one(jx_engine* e, const AccSrc& src, const uint8_t* d_mask, const uint32_t* d_dense,
                              const Segment& t) {
  const Cfg& c = e->cfg;
  AccArgs a{};
  a.n = src.n;
  a.outs = src.outs;
  a.out_len = c.out_len;
  a.verdicts = src.verdicts;
  a.mask = d_mask;
  a.seg = d_dense;
  a.seg_id = 0;
  a.partials = e->d_partials;
  a.nchunks = acc_nchunks(e);
  uint64_t nblk = (src.n + 63) / 64;
  a.blocks_per_chunk = (uint32_t)((nblk + a.nchunks - 1) / a.nchunks);
  if (a.blocks_per_chunk == 0) a.blocks_per_chunk = 1;
  a.nonces = src.nonces;
  a.checksum = t.checksum;
  a.count = t.count;
  hipEvent_t ev = nullptr;
  HIPCHK(e, stage_begin(e, &ev));
  if (src.n <= ACC_SMALL)
    HIPCHK(e, launch_accumulate_small(c, a, t.agg, e->stream));
  else
    HIPCHK(e, launch_accumulate(c, a, t.agg, e->stream));
  HIPCHK(e, stage_end(e, ST_ACC, ev));
  return JX_OK;
}

// Run the deferred accumulations (jx_accumulate): per aggregation, up to ACC_MULTI_MAX batches per
// accumulate_multi launch; their slabs go back to the arena stream-ordered after the launches. One launch per
// aggregation instead of one per job takes the per-job kernel launch off the engine mutex (a coalesced 100-report
// job's callers return together, and each one's accumulate launch serialised them).
constexpr uint64_t kAccQReports = 16384;  // a flush once this many reports wait (their batches hold HBM)
constexpr size_t kRecycleBytes = 512ull << 20;  // batch slabs an engine keeps from its flushes
int32_t jxi::flush_acc(jx_engine* e) {
  if (e->accq.empty()) return JX_OK;
  std::vector<std::pair<Batch, uint32_t>> q;
  q.swap(e->accq);
  e->accq_reports = 0;
  e->acc_flushes++;
  std::map<uint32_t, std::vector<size_t>> by;
  for (size_t k = 0; k < q.size(); k++) by[q[k].second].push_back(k);
  auto run = [&]() -> int32_t {
    HIPCHK(e, hipSetDevice(e->device));
    for (auto& kv : by) {
      Segment* s = nullptr;
      int32_t rc = get_segment(e, kv.first, &s);
      if (rc) return rc;
      const std::vector<size_t>& ix = kv.second;
      for (size_t o = 0; o < ix.size(); o += ACC_MULTI_MAX) {
        AccMultiArgs a{};
        a.agg = s->agg;
        a.count = s->count;
        a.checksum = s->checksum;
        for (size_t j = o; j < ix.size() && a.nb < ACC_MULTI_MAX; j++) {
          const Batch& b = q[ix[j]].first;
          a.d[a.nb++] = AccDesc{b.outs, b.verdicts, b.nonces, b.n};
        }
        hipEvent_t ev = nullptr;
        HIPCHK(e, stage_begin(e, &ev));
        HIPCHK(e, launch_accumulate_multi(e->cfg, a, e->stream));
        HIPCHK(e, stage_end(e, ST_ACC, ev));
      }
    }
    return JX_OK;
  };
  int32_t rc = run();
  // the slabs: kept for the engine's next batches behind one event (up to kRecycleBytes), the rest back to the
  // arena, after the launches that read them
  if (rc == JX_OK && !e->ev_flush && hipEventCreateWithFlags(&e->ev_flush, hipEventDisableTiming) != hipSuccess)
    e->ev_flush = nullptr;
  const bool keep = rc == JX_OK && e->ev_flush && hipEventRecord(e->ev_flush, e->stream) == hipSuccess;
  for (auto& p : q) {
    Slab& sl = p.first.slab;
    if (keep && e->recycle_bytes + sl.bytes <= kRecycleBytes) {
      e->recycle_bytes += sl.bytes;
      e->recycle.emplace(sl.bytes, sl);
    } else {
      arena_put(e->arena, sl, e->stream);
    }
  }
  return rc;
}

// Upload the pointer table of `targets` into `tbl`. The pinned host copy is double-buffered and reused only once
// the upload that last read it has completed, so the host never waits for the call's own kernels.
int32_t jxi::upload_targets(jx_engine* e, const std::vector<Segment>& targets, PtrTable& tbl) {
  const uint64_t S = targets.size();
  int32_t rc = scratch_get(e, 3 * S * sizeof(void*), tbl.mem);
  if (rc) return rc;
  PinnedBuf& hb = e->h_ptrs[e->ptrs_k];
  e->ptrs_k ^= 1;
  void** h = nullptr;
  HIPCHK(e, hb.reserve(3 * S * sizeof(void*), (void**)&h));
  for (uint64_t t = 0; t < S; t++) {
    h[t] = targets[t].agg;
    h[S + t] = targets[t].count;
    h[2 * S + t] = targets[t].checksum;
  }
  HIPCHK(e, hipMemcpyAsync(tbl.d(), h, 3 * S * sizeof(void*), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hb.mark(e->stream));
  return JX_OK;
}

// Reports per segmented-accumulate work item: enough items that out_len x items >= 16384 waves.
static uint32_t seg_items_len(const jx_engine* e, uint64_t n) {
  const uint64_t nch = acc_nchunks(e);
  uint64_t L = (n + nch - 1) / nch;
  L = (L + 63) / 64 * 64;
  return (uint32_t)(L < 64 ? 64 : L);
}

// Accumulate the finished, accepted reports of src into the aggregations named by a dense per-report
// index d_dense[r] in [0, S) (S = targets.size(); indices >= S are skipped); one pass per SEG_MAX segments.
// tbl: the targets' pointer table when the caller has uploaded it (one upload for every launch of a call);
// null: uploaded here.
static int32_t accumulate_many(jx_engine* e, const AccSrc& src, const uint8_t* d_mask, const uint32_t* d_dense,
                               const std::vector<Segment>& targets, const PtrTable* tbl) {
  const Cfg& c = e->cfg;
  const uint64_t n = src.n, S = targets.size();
  if (S == 0 || n == 0) return JX_OK;
  PtrTable own;
  if (!tbl) {
    int32_t rc = upload_targets(e, targets, own);
    if (rc) return rc;
    tbl = &own;
  }
  void** const d_ptrs = tbl->d();
  // per-pass segments: SEG_MAX, or fewer when the per-item partials would exceed ~512 MiB
  const uint32_t L = seg_items_len(e, n);
  const uint64_t items_n = (n + L - 1) / L;
  const uint64_t per_item = (uint64_t)c.out_len * 24;
  uint64_t ns_max = (512ull << 20) / per_item;
  ns_max = ns_max > items_n + 64 ? ns_max - items_n : 64;
  if (ns_max > SEG_MAX) ns_max = SEG_MAX;
  const uint64_t wmax = items_n + (S < ns_max ? S : ns_max);
  // the counting-sort state, permutation, work items and partials: one per-call scratch slab (reused from the
  // arena stream-ordered; no allocation or synchronization once warm)
  // d_segx: cnt, off, cursor [SEG_MAX each], ioff [SEG_MAX + 1], nitems [2]
  uint32_t *d_segx = nullptr, *d_perm = nullptr;
  uint4* d_items = nullptr;
  uint64_t* d_spart = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_segx, (4 * SEG_MAX + 3) * sizeof(uint32_t));
    cv.take(d_perm, n * sizeof(uint32_t));
    cv.take(d_items, wmax * sizeof(uint4));
    cv.take(d_spart, wmax * per_item);
    return cv.bytes();
  };
  Scratch work;
  int32_t rc = scratch_get(e, lay(nullptr), work);
  if (rc) return rc;
  lay(work.p());
  uint64_t grid = (n + 255) / 256;
  if (grid > SELECT_WGS) grid = SELECT_WGS;
  for (uint64_t s0 = 0; s0 < S; s0 += ns_max) {
    const uint32_t ns = (uint32_t)(S - s0 < ns_max ? S - s0 : ns_max);
    SegArgs a{};
    a.n = n;
    a.outs = src.outs;
    a.out_len = c.out_len;
    a.fb = c.fb;
    a.verdicts = src.verdicts;
    a.mask = d_mask;
    a.seg = d_dense;
    a.s0 = (uint32_t)s0;
    a.ns = ns;
    a.nonces = src.nonces;
    a.cnt = d_segx;
    a.off = d_segx + SEG_MAX;
    a.cursor = d_segx + 2 * SEG_MAX;
    a.ioff = d_segx + 3 * SEG_MAX;
    a.nitems = d_segx + 4 * SEG_MAX + 1;
    a.perm = d_perm;
    a.L = L;
    a.items = d_items;
    a.wmax = (uint32_t)(items_n + ns);
    a.partials = d_spart;
    a.aggs = reinterpret_cast<uint4* const*>(d_ptrs + s0);
    a.counts = reinterpret_cast<unsigned long long* const*>(d_ptrs + S + s0);
    a.checksums = reinterpret_cast<uint32_t* const*>(d_ptrs + 2 * S + s0);
    HIPCHK(e, hipMemsetAsync(a.cnt, 0, ns * sizeof(uint32_t), e->stream));
    hipEvent_t ev = nullptr;
    HIPCHK(e, stage_begin(e, &ev));
    HIPCHK(e, launch_accumulate_segmented(c, a, (uint32_t)grid, e->stream));
    HIPCHK(e, stage_end(e, ST_ACC, ev));
  }
  return JX_OK;
}

// Densify host segment ids: ids in first-seen order, dense index per report.
static void densify(const uint32_t* seg, uint64_t n, std::vector<uint32_t>& dense, std::vector<uint32_t>& ids) {
  std::unordered_map<uint32_t, uint32_t> m;
  dense.resize(n);
  ids.clear();
  for (uint64_t i = 0; i < n; i++) {
    auto it = m.find(seg[i]);
    if (it == m.end()) {
      it = m.emplace(seg[i], (uint32_t)ids.size()).first;
      ids.push_back(seg[i]);
    }
    dense[i] = it->second;
  }
}

// The running aggregations named by a caller's segment-id table. A repeated id would make two
// segmented-reduce rows update one aggregation without atomics: refused.
int32_t jxi::segment_targets(jx_engine* e, const uint32_t* ids, uint64_t nids, std::vector<Segment>& out) {
  std::unordered_set<uint32_t> seen;
  out.clear();
  for (uint64_t t = 0; t < nids; t++) {
    if (!seen.insert(ids[t]).second)
      return fail(e, JX_E_INVALID, "segment_ids holds a repeated batch-aggregation id");
    Segment* s = nullptr;
    int32_t rc = get_segment(e, ids[t], &s);
    if (rc) return rc;
    out.push_back(*s);
  }
  return JX_OK;
}

// One target takes the coalesced select/accumulate path; several go through their pointer table (accumulate_many).
int32_t jxi::accumulate_into(jx_engine* e, const AccSrc& src, const uint8_t* d_mask, const uint32_t* d_dense,
                             const std::vector<Segment>& targets, const PtrTable* tbl) {
  if (src.n == 0 || targets.empty()) return JX_OK;
  if (targets.size() == 1 || !d_dense) return accumulate_one(e, src, d_mask, d_dense, targets[0]);
  return accumulate_many(e, src, d_mask, d_dense, targets, tbl);
}

// Per-call delta aggregations (zeroed): ns contiguous segment states in per-call scratch `d`.
static int32_t delta_targets(jx_engine* e, uint32_t ns, std::vector<Segment>& out, Scratch& d) {
  const size_t agg_b = (size_t)ns * e->cfg.out_len * 16, bytes = agg_b + (size_t)ns * 8 + (size_t)ns * 32;
  int32_t rc = scratch_get(e, bytes, d);
  if (rc) return rc;
  uint8_t* base = d.p();
  HIPCHK(e, hipMemsetAsync(base, 0, bytes, e->stream));
  out.resize(ns);
  for (uint32_t s = 0; s < ns; s++) {
    out[s].agg = (uint4*)base + (size_t)s * e->cfg.out_len;
    out[s].count = (unsigned long long*)(base + agg_b) + s;
    out[s].checksum = (uint32_t*)(base + agg_b + (size_t)ns * 8) + 8 * s;
  }
  return JX_OK;
}

static uint32_t record_bytes(const Cfg& c) { return c.out_len * c.fb + 40u; }
static AccSrc batch_src(const Batch& b) { return AccSrc{b.n, b.outs, b.verdicts, b.nonces}; }

extern "C" {

// A batch ready to accumulate: helper batches at once, leader batches after prepare_next.
static int32_t ready_batch(jx_engine* e, uint64_t batch_id, uint64_t n, const char* what, Batch** B) {
  int32_t rc = find_batch(e, batch_id, n, what, B);
  if (rc) return rc;
  if ((*B)->leader && !(*B)->finished)
    return fail(e, JX_E_STATE, std::string(what) + ": leader batch not finished (jx_leader_prep_finish_*)");
  return JX_OK;
}

// Upload small host arrays through the engine's pinned buffer (no host wait for the call's own work: the
// buffer is rewritten only after the upload that last read it has completed).
static int32_t upload_small(jx_engine* e, const std::vector<std::pair<const void*, size_t>>& src,
                            const std::vector<void*>& dst) {
  size_t total = 0;
  for (auto& s : src) total += align256(s.second);
  uint8_t* h = nullptr;
  HIPCHK(e, e->h_acc.reserve(total, (void**)&h));
  size_t off = 0;
  for (size_t i = 0; i < src.size(); i++) {
    memcpy(h + off, src[i].first, src[i].second);
    HIPCHK(e, hipMemcpyAsync(dst[i], h + off, src[i].second, hipMemcpyHostToDevice, e->stream));
    off += align256(src[i].second);
  }
  HIPCHK(e, e->h_acc.mark(e->stream));
  return JX_OK;
}

int32_t jx_accumulate(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* accept_mask,
                      const uint32_t* segment) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  Batch* B = nullptr;
  int32_t rc = ready_batch(e, batch_id, n, "accumulate", &B);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  // one aggregation, every finished report, a job-sized batch: deferred (flush_acc)
  bool one_seg = true;
  for (uint64_t i = 1; segment && i < n && one_seg; i++) one_seg = segment[i] == segment[0];
  if (e->acc_defer && n > 0 && n <= ACC_SMALL && !accept_mask && one_seg) {
    const uint32_t sid = segment ? segment[0] : 0;
    Segment* s = nullptr;
    rc = get_segment(e, sid, &s);  // creates it now (its memset is queued before any later flush)
    if (rc) return rc;
    auto it = e->batches.find(batch_id);
    e->accq.emplace_back(it->second, sid);
    e->accq_reports += n;
    e->acc_deferred++;
    if (e->last_batch == it->first) e->last_batch = 0;
    e->batches.erase(it);  // a batch is accumulated at most once
    if (e->accq.size() >= ACC_MULTI_MAX || e->accq_reports >= kAccQReports) return flush_acc(e);
    return JX_OK;
  }
  auto run = [&]() -> int32_t {
    if (n == 0) return JX_OK;
    Stage st;
    // mask / index scratch and the accumulate partials (a small unmasked batch needs neither)
    int32_t r = accept_mask || segment || n > ACC_SMALL ? stage_acquire(e, n, SG_ACC, st) : JX_OK;
    if (r) return r;
    std::vector<uint32_t> ids{0};
    std::vector<std::pair<const void*, size_t>> src;
    std::vector<void*> dst;
    const uint8_t* dm = nullptr;
    const uint32_t* ds = nullptr;
    if (accept_mask) {
      src.push_back({accept_mask, n});
      dst.push_back(e->d_mask);
      dm = e->d_mask;
    }
    if (segment) {
      densify(segment, n, e->h_dense, ids);
      if (ids.size() > 1) {
        src.push_back({e->h_dense.data(), n * 4});
        dst.push_back(e->d_seg);
        ds = e->d_seg;
      }
    }
    if (!src.empty()) {
      r = upload_small(e, src, dst);
      if (r) return r;
    }
    std::vector<Segment> targets;
    r = segment_targets(e, ids.data(), ids.size(), targets);
    if (r) return r;
    r = accumulate_into(e, batch_src(*B), dm, ds, targets);
    if (r) return r;
    return drain_timing(e);
  };
  rc = run();
  if (rc) return rc;
  batch_free(e, e->batches.find(batch_id));  // a batch is accumulated at most once
  return JX_OK;
}

int32_t jx_accumulate_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_accept_mask,
                             const void* d_segment, const uint32_t* segment_ids, uint32_t nsegments) {
  if (!e || !segment_ids || nsegments == 0) return JX_E_INVALID;
  LOCK(e);
  Batch* B = nullptr;
  int32_t rc = ready_batch(e, batch_id, n, "accumulate", &B);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  if (n) {
    Stage st;
    rc = stage_acquire(e, n, SG_ACC, st);  // the accumulate partials
    if (rc) return rc;
    std::vector<Segment> targets;
    rc = segment_targets(e, segment_ids, nsegments, targets);
    if (rc) return rc;
    rc = accumulate_into(e, batch_src(*B), (const uint8_t*)d_accept_mask, (const uint32_t*)d_segment, targets);
    if (rc) return rc;
  }
  batch_free(e, e->batches.find(batch_id));
  return JX_OK;
}

// Deltas: accumulate a batch into zeroed per-call aggregations and export them as records. Pure with
// respect to engine state (the batch stays resident; the running aggregations are not touched).
static int32_t batch_records(jx_engine* e, Batch* B, const uint8_t* d_mask, const uint32_t* d_index, uint32_t ns,
                             uint8_t* d_out) {
  std::vector<Segment> targets;
  Scratch deltas;
  int32_t rc = delta_targets(e, ns, targets, deltas);
  if (rc) return rc;
  rc = accumulate_into(e, batch_src(*B), d_mask, d_index, targets);
  if (rc) return rc;
  HIPCHK(e, launch_record_export(e->cfg, targets[0].agg, targets[0].count, targets[0].checksum, d_out, e->stream, ns));
  return JX_OK;
}

int32_t jx_batch_aggregate_records(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* accept_mask,
                                   const uint32_t* segment_index, uint32_t nsegments, uint8_t* out_records) {
  if (!e || !out_records || nsegments == 0) return JX_E_INVALID;
  LOCK(e);
  Batch* B = nullptr;
  int32_t rc = ready_batch(e, batch_id, n, "aggregate records", &B);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t rb = record_bytes(e->cfg);
  Stage st;
  rc = stage_acquire(e, n ? n : 1, SG_ACC, st);  // mask / index scratch and the accumulate partials
  if (rc) return rc;
  const uint8_t* dm = nullptr;
  const uint32_t* di = nullptr;
  if (n && accept_mask) {
    HIPCHK(e, hipMemcpyAsync(e->d_mask, accept_mask, n, hipMemcpyHostToDevice, e->stream));
    dm = e->d_mask;
  }
  if (n && segment_index) {
    HIPCHK(e, hipMemcpyAsync(e->d_seg, segment_index, n * 4, hipMemcpyHostToDevice, e->stream));
    di = e->d_seg;
  }
  Scratch rec;
  rc = scratch_get(e, rb * nsegments, rec);
  if (rc) return rc;
  rc = batch_records(e, B, dm, di, nsegments, rec.p());
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(out_records, rec.p(), rb * nsegments, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return drain_timing(e);
}

int32_t jx_batch_aggregate_records_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_accept_mask,
                                          const void* d_segment_index, uint32_t nsegments, void* d_out_records) {
  if (!e || !d_out_records || nsegments == 0) return JX_E_INVALID;
  LOCK(e);
  Batch* B = nullptr;
  int32_t rc = ready_batch(e, batch_id, n, "aggregate records", &B);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  Stage st;
  rc = stage_acquire(e, n ? n : 1, SG_ACC, st);  // the accumulate partials
  if (rc) return rc;
  return batch_records(e, B, (const uint8_t*)d_accept_mask, (const uint32_t*)d_segment_index, nsegments,
                       (uint8_t*)d_out_records);
}

int32_t jx_aggregate_read(jx_engine* e, uint32_t segment, uint8_t* out_agg, uint64_t* count) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  const Cfg& c = e->cfg;
  const uint32_t fb = c.fb;
  Segment* s = nullptr;
  int32_t rc = get_segment(e, segment, &s);
  if (rc) return rc;
  Scratch tmp;
  rc = scratch_get(e, (size_t)c.out_len * fb, tmp, true);
  if (rc) return rc;
  HIPCHK(e, launch_agg_encode(c, s->agg, tmp.p(), e->stream));
  if (out_agg) HIPCHK(e, hipMemcpyAsync(out_agg, tmp.p(), (size_t)c.out_len * fb, hipMemcpyDeviceToHost, e->stream));
  unsigned long long cnt = 0;
  HIPCHK(e, hipMemcpyAsync(&cnt, s->count, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (count) *count = cnt;
  return drain_timing(e);
}

int32_t jx_aggregate_checksum(jx_engine* e, uint32_t segment, uint8_t out_checksum[32]) {
  if (!e || !out_checksum) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  Segment* s = nullptr;
  int32_t rc = get_segment(e, segment, &s);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(out_checksum, s->checksum, 32, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

int32_t jx_aggregate_reset(jx_engine* e) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  for (auto& kv : e->segs) {
    HIPCHK(e, hipMemsetAsync(kv.second.agg, 0, (size_t)e->cfg.out_len * 16, e->stream));
    HIPCHK(e, hipMemsetAsync(kv.second.checksum, 0, 32, e->stream));
    HIPCHK(e, hipMemsetAsync(kv.second.count, 0, 8, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

int32_t jx_aggregate_export_device(jx_engine* e, uint32_t segment, void* d_dst) {
  if (!e || !d_dst) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  Segment* s = nullptr;
  int32_t rc = get_segment(e, segment, &s);
  if (rc) return rc;
  HIPCHK(e, launch_agg_encode(e->cfg, s->agg, (uint8_t*)d_dst, e->stream));
  return JX_OK;
}

static int32_t ensure_err(jx_engine* e) {
  if (!e->d_err) {
    HIPCHK(e, hipMalloc((void**)&e->d_err, sizeof(uint32_t)));
    HIPCHK(e, hipMemsetAsync(e->d_err, 0, sizeof(uint32_t), e->stream));
  }
  return JX_OK;
}

int32_t jx_aggregate_combine_device(jx_engine* e, const void* d_parts, uint32_t nparts, void* d_out) {
  if (!e || !d_parts || !d_out || nparts == 0) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  int32_t rc = ensure_err(e);
  if (rc) return rc;
  HIPCHK(e, launch_combine(e->cfg, (const uint8_t*)d_parts, nparts, (uint8_t*)d_out, e->d_err, e->stream));
  return JX_OK;
}

int32_t jx_shard_record_export_device(jx_engine* e, uint32_t segment, void* d_dst) {
  if (!e || !d_dst) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  Segment* s = nullptr;
  int32_t rc = get_segment(e, segment, &s);
  if (rc) return rc;
  HIPCHK(e, launch_record_export(e->cfg, s->agg, s->count, s->checksum, (uint8_t*)d_dst, e->stream));
  return JX_OK;
}

int32_t jx_shard_record_combine_device(jx_engine* e, const void* d_records, uint32_t nrecords, void* d_out) {
  if (!e || !d_records || !d_out || nrecords == 0) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  int32_t rc = ensure_err(e);
  if (rc) return rc;
  HIPCHK(e, launch_record_combine(e->cfg, (const uint8_t*)d_records, nrecords, (uint8_t*)d_out, e->d_err, e->stream));
  return JX_OK;
}

int32_t jx_shard_record_bytes(const jx_engine* e, uint32_t* bytes) {
  if (!e || !bytes) return JX_E_INVALID;
  *bytes = record_bytes(e->cfg);
  return JX_OK;
}

}  // extern "C"
