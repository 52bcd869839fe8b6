// jx_engine.cpp — the engine behind the C ABI in include/jx_prio3.h.
//
// Owns device staging, constant tables, resident prepared batches and per-segment batch
// aggregations; sequences the K1 (XOF) -> K1' (slow path) -> K3 (FLP) launches (prep_core) on one HIP
// stream per engine; creates, destroys and configures engines. The calls themselves are in the family
// files: jx_engine_prep.cpp (prepare into a resident batch), jx_engine_acc.cpp (K4, the aggregations),
// jx_engine_fused.cpp (prepare + aggregate), jx_engine_upload.cpp, jx_engine_shard.cpp; the instance's
// parameters and constant tables in jx_engine_cfg.cpp. Every entry point takes the engine mutex for the
// duration of the call only, so concurrent aggregation jobs can share an engine (each holds a batch
// handle). There is no CPU compute path: if the device or the kernels are unavailable every entry
// point fails with an error status.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_fused_plan.h"

using namespace jx;
using namespace jxi;

// The message of the last failing call, per calling thread: an engine serves several host threads,
// and each reads the error of its own call (jx_last_error), never another thread's.
static thread_local std::string t_err;

namespace jxi {
std::string& thread_error() { return t_err; }
int32_t fail(jx_engine* e, int32_t code, const std::string& msg) {
  (void)e;
  t_err = msg;
  return code;
}
}  // namespace jxi

// ---------------------------------------------------------------------------- staging (per call, from the arena)

// staging element bytes: the multiproof Field64 kernels use 8-byte elements (outputs stay uint4)
static uint32_t stage_eb(const Cfg& c) { return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 8u : 16u; }
static uint64_t coef_elems(const Cfg& c) { return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? (uint64_t)c.np * c.nco : c.ncoef; }
static uint64_t part_bytes(const Cfg& c) {
  return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 24ull * c.np * c.ngroups : 64ull * c.ngt;
}

namespace jxi {
uint32_t vk_row_bytes(const Cfg& c) { return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 64u : 16u; }
void vk_row(const Cfg& c, uint8_t* dst) {
  if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF) {  // the HMAC-SHA256 pads of the 32-byte key: ist[8] || ost[8]
    memcpy(dst, c.vk_ist, 32);
    memcpy(dst + 32, c.vk_ost, 32);
  } else {
    memcpy(dst, c.vk, 16);
  }
}
}  // namespace jxi

// Staging bytes of one report for a fused helper launch (the launch-size budget, jx_engine_create_ex).
static uint64_t per_report_bytes(const Cfg& c, bool with_meas = true) {
  uint64_t b = (uint64_t)stage_eb(c) * ((with_meas ? c.meas_len : 0) + (uint64_t)c.np * c.proof_len + coef_elems(c));
  b += 16ull * (c.out_is_meas ? 0 : c.out_len);
  b += 16 + c.ps_bytes + c.his_bytes + c.lps_bytes + 4 + 1 + c.seed + 1 + 4 + 1;
  b += part_bytes(c);  // FLP partial sums
  return b;
}

// Report chunks of accumulate_kernel: one wave per (output element, chunk), so short outputs
// (Count, Sum: 1 element) need many chunks to fill the device; >= 16384 waves in total.
uint32_t jxi::acc_nchunks(const jx_engine* e) {
  if (e->acc_chunks) return e->acc_chunks;
  const uint32_t want = (16384u + e->cfg.out_len - 1) / e->cfg.out_len;
  return want < 16u ? 16u : (want > 4096u ? 4096u : want);
}

// Lay the regions named by `fl` for `cap` reports out from `base` (nullptr: only size them). ct_bytes: each of
// SG_ENC's two ciphertext regions.
static size_t stage_layout(jx_engine* e, uint64_t cap, uint32_t fl, uint64_t ct_bytes, uint8_t* base) {
  const Cfg& c = e->cfg;
  const uint64_t eb = stage_eb(c);
  Carver cv(base);
  auto take = [&](auto*& p, size_t bytes) { cv.take(p, bytes); };
  if (fl & SG_IN) {
    take(e->d_nonces, cap * 16);
    take(e->d_ps, cap * c.ps_bytes);
  }
  if (fl & SG_HIN) {
    take(e->d_his, cap * c.his_bytes);
    take(e->d_lps, cap * c.lps_bytes);
  }
  if (fl & SG_MEAS) take(e->d_meas, cap * c.meas_len * eb);
  if (fl & SG_PREP) {
    take(e->d_proof, cap * c.np * c.proof_len * eb);
    if (!outs_alias_meas(c)) take(e->d_outs, cap * c.out_len * 16);
    take(e->d_coef, cap * coef_elems(c) * eb);
    take(e->d_flags, cap * 4);
    take(e->d_part, cap * part_bytes(c));
  }
  if (fl & SG_RES) {
    take(e->d_verdicts, cap);
    take(e->d_msgs, cap * c.seed);
  }
  if (fl & SG_ACC) {
    take(e->d_mask, cap);
    take(e->d_seg, cap * 4);
    take(e->d_partials, (size_t)acc_nchunks(e) * c.out_len * 3 * sizeof(uint64_t) + cap);
  }
  if (fl & SG_LEAD) {
    take(e->d_lis, cap * e->lis_stride);
    take(e->d_lps_out, cap * c.lps_bytes);
  }
  if (fl & SG_LMSG) take(e->d_in_msgs, cap * c.seed);
  if (fl & SG_VK) take(e->d_vkeys, cap * vk_row_bytes(c));
  if (fl & SG_JOBS) take(e->d_jobs, (size_t)MAX_JOBS_PER_LAUNCH * sizeof(JobSlice));
  if (fl & SG_ENC) {
    take(e->d_encrows, cap * sizeof(EncRow));
    take(e->d_ct, ct_bytes);
    take(e->d_pt, ct_bytes);
    take(e->d_status, cap);
  }
  if (fl & SG_ENCC) {
    take(e->d_ec_times, cap * 8);
    take(e->d_ec_eoff, (cap + 1) * 8);
    take(e->d_ec_poff, (cap + 1) * 8);
    take(e->d_ec_kidx, cap * 2);
  }
  return cv.bytes();
}

static void stage_clear(jx_engine* e) {
  e->d_nonces = e->d_ps = e->d_his = e->d_lps = nullptr;
  e->d_meas = e->d_proof = e->d_outs = e->d_coef = nullptr;
  e->d_flags = nullptr;
  e->d_part = nullptr;
  e->d_verdicts = e->d_msgs = nullptr;
  e->d_partials = nullptr;
  e->d_mask = nullptr;
  e->d_seg = nullptr;
  e->d_lis = e->d_lps_out = e->d_in_msgs = nullptr;
  e->d_vkeys = nullptr;
  e->d_jobs = nullptr;
  e->d_encrows = nullptr;
  e->d_ct = e->d_pt = e->d_status = nullptr;
  e->d_ec_times = e->d_ec_eoff = e->d_ec_poff = nullptr;
  e->d_ec_kidx = nullptr;
  e->cap = 0;
  e->stage_flags = 0;
}

namespace jxi {
// JX_E_NOMEM naming what holds the device memory (resident batches are the caller's to release).
static int32_t nomem(jx_engine* e, const char* what, size_t bytes) {
  uint64_t held = 0;
  for (auto& kv : e->batches) held += kv.second.slab.bytes;
  Arena* A = e->arena;
  return fail(e, JX_E_NOMEM,
              std::string(what) + ": out of device memory allocating " + std::to_string(bytes) + " B; " +
                  std::to_string(e->batches.size()) + " resident batches of this engine hold " + std::to_string(held) +
                  " B; the device arena holds " + std::to_string(A->allocated) + " of its " + std::to_string(A->budget) +
                  " B budget (release finished or abandoned jobs with jx_batch_release)");
}

int32_t stage_acquire(jx_engine* e, uint64_t n, uint32_t fl, Stage& st, bool may_wait, uint64_t ct_bytes) {
  st.release();
  const uint64_t cap = (n + 63) / 64 * 64;
  const size_t bytes = stage_layout(e, cap, fl, ct_bytes, nullptr);
  hipError_t rc = arena_get(e->arena, bytes, e->stream, true, may_wait, st.slab);
  if (rc == hipErrorOutOfMemory) return nomem(e, "staging", bytes);
  HIPCHK(e, rc);
  st.e = e;
  stage_layout(e, cap, fl, ct_bytes, (uint8_t*)st.slab.p);
  e->cap = cap;
  e->stage_flags = fl;
  return JX_OK;
}

void Stage::release() {
  if (!e) return;
  arena_put(e->arena, slab, e->stream);
  stage_clear(e);
  e = nullptr;
}
}  // namespace jxi

// the fused paths' output shares (engine staging)
uint4* jxi::staging_outs(jx_engine* e) { return outs_alias_meas(e->cfg) ? e->d_meas : e->d_outs; }

// Per-call scratch (Scratch, jx_engine_internal.h).
int32_t jxi::scratch_get(jx_engine* e, size_t bytes, Scratch& out, bool may_wait) {
  out.e = e;
  const hipError_t st = arena_get(e->arena, bytes, e->stream, true, may_wait, out.s);
  if (st == hipErrorOutOfMemory) return nomem(e, "scratch", bytes);
  HIPCHK(e, st);
  return JX_OK;
}

// Running aggregations: segment states (aggregate share | checksum | count) carved from arena slabs of
// kSegsPerSlab states, so a new batch-aggregation id costs no device allocation on the call path (one slab per
// kSegsPerSlab ids, held until the engine is destroyed).
constexpr uint32_t kSegsPerSlab = 64;
static size_t seg_state_bytes(const Cfg& c) { return align256((size_t)c.out_len * 16 + 32 + 8); }

int32_t jxi::get_segment(jx_engine* e, uint32_t id, Segment** out) {
  auto it = e->segs.find(id);
  if (it == e->segs.end()) {
    const size_t sb = seg_state_bytes(e->cfg);
    if (e->seg_slabs.empty() || e->seg_next == kSegsPerSlab) {
      Slab sl;
      const hipError_t st = arena_get(e->arena, sb * kSegsPerSlab, e->stream, false, false, sl);
      if (st == hipErrorOutOfMemory) return nomem(e, "batch aggregations", sb * kSegsPerSlab);
      HIPCHK(e, st);
      e->seg_slabs.push_back(sl);
      e->seg_next = 0;
    }
    uint8_t* m = (uint8_t*)e->seg_slabs.back().p + sb * e->seg_next++;
    Segment s;
    s.agg = (uint4*)m;
    s.checksum = (uint32_t*)(m + (size_t)e->cfg.out_len * 16);
    s.count = (unsigned long long*)(m + (size_t)e->cfg.out_len * 16 + 32);
    HIPCHK(e, hipMemsetAsync(m, 0, sb, e->stream));
    it = e->segs.emplace(id, s).first;
  }
  *out = &it->second;
  return JX_OK;
}

// ---------------------------------------------------------------------------- resident batches

// A new resident batch of n reports (handle in *id), one arena allocation. Slabs handed back by released
// batches (of any engine on the device) are reused stream-ordered.
int32_t jxi::batch_new(jx_engine* e, uint64_t n, bool leader, uint64_t* id, Batch** out) {
  const Cfg& c = e->cfg;
  const uint64_t cap = (n + 63) / 64 * 64;
  Batch b;
  b.n = n;
  b.leader = leader;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(b.outs, (size_t)cap * c.out_len * 16);
    cv.take(b.verdicts, cap);
    cv.take(b.msgs, (size_t)cap * c.seed);
    cv.take(b.nonces, cap * 16);
    return cv.bytes();
  };
  const size_t bytes = n ? lay(nullptr) : 0;  // an empty batch: the arena's smallest slab, nothing carved
  // a slab a deferred-accumulate flush has read (the same job size comes back every time): no arena round trip;
  // its users wait on that flush (e->stream is in order after it already)
  auto rit = e->recycle.lower_bound(bytes);
  if (rit != e->recycle.end() && rit->first <= bytes + bytes / 4) {
    b.slab = rit->second;
    b.wait_ev = e->ev_flush;
    e->recycle_bytes -= rit->first;
    e->recycle.erase(rit);
  } else {
    hipError_t st = arena_get(e->arena, bytes, e->stream, false, false, b.slab);
    if (st == hipErrorOutOfMemory) return nomem(e, "new batch", bytes);
    HIPCHK(e, st);
  }
  if (n) lay(b.slab.p);
  *id = ++e->batch_gen;
  e->last_batch = *id;
  *out = &e->batches.emplace(*id, b).first->second;
  return JX_OK;
}

void jxi::batch_free(jx_engine* e, std::map<uint64_t, Batch>::iterator it) {
  arena_put(e->arena, it->second.slab, e->stream);  // reused after the work queued on the engine stream
  if (e->last_batch == it->first) e->last_batch = 0;
  e->batches.erase(it);
}

int32_t jxi::find_batch(jx_engine* e, uint64_t id, uint64_t n, const char* what, Batch** out) {
  auto it = e->batches.find(id);
  if (id == 0 || it == e->batches.end() || __atomic_load_n(&it->second.pending, __ATOMIC_ACQUIRE))
    return fail(e, JX_E_STATE, std::string(what) + ": batch id names no resident prepared batch (released or never made)");
  if (it->second.n != n)
    return fail(e, JX_E_INVALID, std::string(what) + ": report count differs from the batch's");
  *out = &it->second;
  return JX_OK;
}

// ---------------------------------------------------------------------------- timing

hipError_t jxi::stage_begin(jx_engine* e, hipEvent_t* ev) {
  if (!e->timing) return hipSuccess;
  hipError_t st = hipEventCreate(ev);
  if (st != hipSuccess) return st;
  return hipEventRecord(*ev, e->stream);
}
hipError_t jxi::stage_end(jx_engine* e, int stage, hipEvent_t ev0) {
  e->launches[stage]++;
  if (!e->timing) return hipSuccess;
  hipEvent_t ev1;
  hipError_t st = hipEventCreate(&ev1);
  if (st != hipSuccess) return st;
  st = hipEventRecord(ev1, e->stream);
  e->pending.push_back({stage, {ev0, ev1}});
  return st;
}
int32_t jxi::drain_timing(jx_engine* e) {
  if (e->pending.empty()) return JX_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (auto& p : e->pending) {
    float t = 0;
    HIPCHK(e, hipEventElapsedTime(&t, p.second.first, p.second.second));
    e->ms[p.first] += t;
    (void)hipEventDestroy(p.second.first);
    (void)hipEventDestroy(p.second.second);
  }
  e->pending.clear();
  return JX_OK;
}

// ---------------------------------------------------------------------------- core sequencing

// Prepare n <= cap reports whose inputs are at the given device pointers; the output shares go to
// outs (a batch's buffer, or the staging of the fused paths), verdicts and prep messages / leader
// seeds to verdicts / msgs.
int32_t jxi::prep_core(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* ps, const uint8_t* his,
                       const uint8_t* lps, uint8_t* verdicts, uint8_t* msgs, uint4* outs, const uint8_t* lis,
                       uint8_t* lps_out, uint64_t lis_rs, const uint8_t* vkeys, hipEvent_t before_flp,
                       const std::function<int32_t()>* after_k1) {
  const Cfg& c = e->cfg;
  const bool leader = lis != nullptr;
  Bufs b{};
  b.n = n;
  b.nonces = nonces;
  b.ps = ps;
  b.his = his;
  b.lps = lps;
  b.lis = lis;
  b.lis_rs = lis_rs ? lis_rs : c.lis_bytes;
  b.vkeys = vkeys;
  b.lps_out = lps_out;
  b.leader = leader ? 1u : 0u;
  b.meas = outs_alias_meas(c) ? outs : e->d_meas;
  if (leader && leader_inplace(c)) {
    b.meas_src = lis;
    b.meas_rs = b.lis_rs;
  }
  b.proof = e->d_proof;
  b.outs = outs;
  b.coef = e->d_coef;
  b.flags = e->d_flags;
  b.part = e->d_part;
  b.verdicts = verdicts;
  b.msgs = msgs;
  b.consts = e->d_consts;
  b.force_slow = e->force_slow;
  // which helper K1 runs, and whether the launch splits in two: jx_k1_plan.h
  const bool wide = c.bits > 32 && (c.algo == ALGO_SUM || c.algo == ALGO_SUMVEC);
  const bool big = k1_big(n, e->round_reports);
  const bool no_split = one_kernel_chain(c);
  K1Plan plan = k1_plan(n, e->round_reports, e->k1_forced, leader, wide, no_split, e->lanes_wg_cap, false);
  if (plan.split && arena_big_busy(e->arena, e))  // asked only of a launch that would split
    plan = k1_plan(n, e->round_reports, e->k1_forced, leader, wide, no_split, e->lanes_wg_cap, true);
  hipEvent_t ev = nullptr;
  if (c.algo == ALGO_COUNT) {
    HIPCHK(e, stage_begin(e, &ev));
    HIPCHK(e, launch_count(c, b, e->stream));
    HIPCHK(e, stage_end(e, ST_XOF, ev));
  } else if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF) {
    HIPCHK(e, stage_begin(e, &ev));
    HIPCHK(e, launch_mp_xof(c, b, e->stream));
    HIPCHK(e, stage_end(e, ST_XOF, ev));
    if (!leader) {
      HIPCHK(e, stage_begin(e, &ev));
      HIPCHK(e, launch_mp_slow(c, b, e->stream));
      HIPCHK(e, stage_end(e, ST_SLOW, ev));
    }
    HIPCHK(e, stage_begin(e, &ev));
    HIPCHK(e, launch_mp_flp(c, b, e->stream));
    HIPCHK(e, stage_end(e, ST_FLP, ev));
  } else {
    HIPCHK(e, stage_begin(e, &ev));
    if (plan.split) {
      if (!e->side) HIPCHK(e, hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
      if (!e->ev_fork) HIPCHK(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
      if (!e->ev_side) HIPCHK(e, hipEventCreateWithFlags(&e->ev_side, hipEventDisableTiming));
      Bufs head = b;
      const Bufs tail = bufs_tail(c, b, plan.split);
      head.n = plan.split;
      HIPCHK(e, hipEventRecord(e->ev_fork, e->stream));
      HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_fork, 0));
      HIPCHK(e, launch_xof(c, head, plan.head, e->stream));
      HIPCHK(e, launch_xof(c, tail, plan.tail, e->side));
      HIPCHK(e, hipEventRecord(e->ev_side, e->side));
      HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_side, 0));
    } else {
      HIPCHK(e, launch_xof(c, b, plan.head, e->stream));
    }
    if (big) HIPCHK(e, arena_big_record(e->arena, e, e->stream));
    HIPCHK(e, stage_end(e, ST_XOF, ev));
    if (after_k1) {
      const int32_t rc = (*after_k1)();
      if (rc) return rc;
    }
    if (!leader) {  // the leader's shares are explicit: no rejection-sampled streams to redo
      HIPCHK(e, stage_begin(e, &ev));
      HIPCHK(e, launch_xof_slow(c, b, e->stream));
      HIPCHK(e, stage_end(e, ST_SLOW, ev));
    }
    // the caller's upload of the rest of the leader prep shares (K1 reads only their joint-rand parts)
    if (before_flp) HIPCHK(e, hipStreamWaitEvent(e->stream, before_flp, 0));
    HIPCHK(e, stage_begin(e, &ev));
    HIPCHK(e, launch_flp(c, b, e->stream));
    HIPCHK(e, stage_end(e, ST_FLP, ev));
  }
  return JX_OK;
}

// ---------------------------------------------------------------------------- child engines
// A pipeline of a fused call (jx_engine_fused.cpp) or a lane of the coalescer: its own stream, the parent's tables.
jx_engine* jxi::new_child(jx_engine* parent) {
  jx_engine* q = new jx_engine();
  q->cfg = parent->cfg;
  q->device = parent->device;
  q->is_pipe = true;
  q->arena = parent->arena;
  q->d_consts = parent->d_consts;
  q->default_chunk = parent->default_chunk;
  q->auto_chunk = parent->auto_chunk;
  q->round_reports = parent->round_reports;
  q->lis_stride = parent->lis_stride;
  if (hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&q->ev_join, hipEventDisableTiming) != hipSuccess) {
    jx_engine_destroy(q);
    return nullptr;
  }
  return q;
}

// Move the pipelines' kernel timings into the engine's.
static int32_t collect_pipe_timing(jx_engine* e) {
  for (jx_engine* q : e->pipes) {
    int32_t rc = drain_timing(q);
    if (rc) return rc;
    for (int i = 0; i < NST; i++) {
      e->ms[i] += q->ms[i];
      e->launches[i] += q->launches[i];
      q->ms[i] = 0;
      q->launches[i] = 0;
    }
  }
  return JX_OK;
}

// ---------------------------------------------------------------------------- C ABI: lifetime and plumbing

extern "C" {

int32_t jx_engine_create(const jx_prio3_params* params, const uint8_t verify_key[16], int32_t device,
                         jx_engine** out) {
  return jx_engine_create_ex(params, verify_key, 16, device, out);
}

int32_t jx_engine_create_ex(const jx_prio3_params* params, const uint8_t* verify_key, uint32_t verify_key_len,
                            int32_t device, jx_engine** out) {
  if (!params || !verify_key || !out) return JX_E_INVALID;
  *out = nullptr;
  t_err.clear();  // a refused parameter set leaves its reason here (jx_last_error takes a null engine)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return JX_E_NODEVICE;
  if (device < 0 || device >= ndev) return JX_E_INVALID;
  jx_engine* e = new jx_engine();
  std::string why;
  int32_t rc = make_cfg(params, verify_key, verify_key_len, e->cfg, why);
  if (rc) {
    t_err = why;
    delete e;
    return rc;
  }
  e->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
    delete e;
    return JX_E_HIP;
  }
  e->arena = arena_for(device);
  arena_engine_add(e->arena);
  // staged leader input shares (host-buffer leader path, coalesced leader launches): rows padded to 128 B for
  // the instances whose FLP kernels read the measurement share in place, so those reads take whole lines
  e->lis_stride = leader_inplace(e->cfg) ? (e->cfg.lis_bytes + 127u) / 128u * 128u : e->cfg.lis_bytes;
  std::vector<uint4> consts = make_consts(e->cfg);
  // On the engine stream, synchronized on it alone: creating an engine orders nothing with the caller's
  // streams (that is jx_engine_wait_stream's job).
  if (hipMalloc((void**)&e->d_consts, consts.size() * sizeof(uint4)) != hipSuccess ||
      hipMemcpyAsync(e->d_consts, consts.data(), consts.size() * sizeof(uint4), hipMemcpyHostToDevice, e->stream) !=
          hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_wait, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) {
    jx_engine_destroy(e);
    return JX_E_HIP;
  }
  // Reports per launch of the fused paths: ~48 GiB of staging, enough for several K1 occupancy rounds of
  // the small VDAFs. A VDAF whose reports need megabytes of staging (FixedPointBoundedL2VecSum at
  // length 10000: 2.8 MB) would fill only a few percent of the SIMDs at 48 GiB, and K1 is bound by
  // the per-report sponge latency (15k sequential permutations), so throughput scales with the
  // reports in flight: grow the budget toward one full K1 round, up to 1/3 of the device memory
  // (two roles, e.g. leader and helper, still fit on one MI355X). Staging is checked out of the device
  // arena per call, so this sizes launches, not what an idle engine holds. Debug option 5 overrides it.
  const uint64_t per = per_report_bytes(e->cfg);
  e->round_reports = k1_round_reports(e->cfg, device);
  uint64_t budget = 48ull << 30;
  size_t mem_free = 0, mem_total = 0;
  if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && e->round_reports && e->round_reports * per > budget) {
    const uint64_t cap = mem_total / 3;
    budget = e->round_reports * per < cap ? e->round_reports * per : cap;
    if (budget < (48ull << 30)) budget = 48ull << 30;
  }
  uint64_t chunk = budget / per;
  if (chunk > (1ull << 22)) chunk = 1ull << 22;
  chunk = chunk / 256 * 256;
  if (chunk < 256) chunk = 256;
  if (e->round_reports && chunk >= e->round_reports) chunk = chunk / e->round_reports * e->round_reports;
  e->default_chunk = e->auto_chunk = chunk;
  *out = e;
  return JX_OK;
}

void jx_engine_destroy(jx_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->coal) coalescer_release(e);
  for (jx_engine* p : e->pipes) jx_engine_destroy(p);
  e->pipes.clear();
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (auto& p : e->pending) {
    (void)hipEventDestroy(p.second.first);
    (void)hipEventDestroy(p.second.second);
  }
  e->segs.clear();
  if (e->arena) {
    for (auto& p : e->accq) arena_put(e->arena, p.first.slab, e->stream);  // deferred accumulations: unread
    e->accq.clear();
    for (auto& kv : e->recycle) arena_put(e->arena, kv.second, e->stream);
    e->recycle.clear();
    for (Slab& sl : e->seg_slabs) arena_put(e->arena, sl, e->stream);
    for (auto& kv : e->batches) arena_put(e->arena, kv.second.slab, e->stream);
  }
  e->seg_slabs.clear();
  e->batches.clear();
  if (e->d_consts && !e->is_pipe) (void)hipFree(e->d_consts);
  if (e->ev_pipe) (void)hipEventDestroy(e->ev_pipe);
  if (e->d_err) (void)hipFree(e->d_err);
  if (e->d_shard_tab) (void)hipFree(e->d_shard_tab);
  for (PinnedBuf* b : {&e->h_ptrs[0], &e->h_ptrs[1], &e->h_acc, &e->h_enc}) b->destroy();
  if (e->ev_flush) (void)hipEventDestroy(e->ev_flush);
  if (e->ev_wait) (void)hipEventDestroy(e->ev_wait);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->arena) arena_big_forget(e->arena, e);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_side) (void)hipEventDestroy(e->ev_side);
  if (e->side) (void)hipStreamDestroy(e->side);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  if (e->arena && !e->is_pipe) arena_engine_remove(e->arena);
  delete e;
}

int32_t jx_engine_sizes(const jx_engine* e, uint32_t* ps, uint32_t* his, uint32_t* lps, uint32_t* pm,
                        uint32_t* out_len, uint32_t* fb) {
  if (!e) return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (ps) *ps = c.ps_bytes;
  if (his) *his = c.his_bytes;
  if (lps) *lps = c.lps_bytes;
  if (pm) *pm = c.jr_len ? c.seed : 0;
  if (out_len) *out_len = c.out_len;
  if (fb) *fb = c.fb;
  return JX_OK;
}

// Reserve: warm the device arena with staging for `reports` reports (checked out once, then idle in the
// arena for the next call of any engine on the device).
int32_t jx_engine_set_capacity(jx_engine* e, uint64_t reports) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  Stage st;
  return stage_acquire(e, reports, SG_IN | SG_HIN | SG_MEAS | SG_PREP | SG_RES | SG_ACC, st);
}

int32_t jx_engine_batch_id(const jx_engine* e, uint64_t* batch_id) {
  if (!e || !batch_id) return JX_E_INVALID;
  LOCK(const_cast<jx_engine*>(e));
  auto it = e->batches.find(e->last_batch);
  *batch_id = it != e->batches.end() && !__atomic_load_n(&it->second.pending, __ATOMIC_ACQUIRE) ? e->last_batch.load() : 0;
  return JX_OK;
}

int32_t jx_engine_batches(const jx_engine* e, uint64_t* resident, uint64_t* device_bytes) {
  if (!e) return JX_E_INVALID;
  LOCK(const_cast<jx_engine*>(e));
  uint64_t bytes = 0;
  for (auto& kv : e->batches) bytes += kv.second.slab.bytes;
  if (resident) *resident = e->batches.size();
  if (device_bytes) *device_bytes = bytes;
  return JX_OK;
}

int32_t jx_engine_memory(const jx_engine* e, jx_memory_stats* out) {
  if (!e || !out) return JX_E_INVALID;
  memset(out, 0, sizeof *out);
  {
    LOCK(const_cast<jx_engine*>(e));
    for (auto& kv : e->batches) out->batch_bytes += kv.second.slab.bytes;
    out->resident_batches = e->batches.size();
    out->last_pipelines = e->last_pipes;
  }
  Arena* A = e->arena;
  {
    std::lock_guard<std::mutex> lk(A->mu);
    out->arena_budget = A->budget;
    out->arena_allocated = A->allocated;
    out->arena_in_use = A->in_use;
    out->arena_peak = A->peak;
    out->arena_allocs = A->allocs;
    out->arena_reuses = A->reuses;
    out->arena_waits = A->waits;
    out->arena_engines = A->engines;
  }
  uint64_t cs[16] = {0};
  coalescer_stats(e, cs);
  out->coalesce_pinned_bytes = cs[9];
  out->coalesced_helper_launches = cs[10];
  out->coalesced_helper_jobs = cs[11];
  out->coalesced_leader_launches = cs[12];
  out->coalesced_leader_jobs = cs[13];
  out->coalesced_encrypted_jobs = cs[14];
  out->coalesced_launches = cs[0];
  out->coalesced_jobs = cs[1];
  out->coalesced_reports = cs[2];
  out->coalesce_window_us = cs[3];
  out->coalesce_gather_us = cs[5];
  out->coalesce_copy_us = cs[6];
  out->coalesce_enqueue_us = cs[7];
  out->coalesce_device_us = cs[8];
  {
    std::lock_guard<std::mutex> lk(A->mu);
    out->arena_cross_stream_waits = A->cross_waits;
    out->arena_frees = A->frees;
  }
  return JX_OK;
}

int32_t jx_batch_release(jx_engine* e, uint64_t batch_id) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  auto it = e->batches.find(batch_id);
  if (batch_id == 0 || it == e->batches.end() || __atomic_load_n(&it->second.pending, __ATOMIC_ACQUIRE))
    return fail(e, JX_E_STATE, "release: batch id names no resident prepared batch");
  HIPCHK(e, hipSetDevice(e->device));
  batch_free(e, it);
  return JX_OK;
}

int32_t jx_engine_sync(jx_engine* e) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (e->d_err) {
    uint32_t bad = 0;
    HIPCHK(e, hipMemcpy(&bad, e->d_err, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) {
      HIPCHK(e, hipMemset(e->d_err, 0, sizeof bad));
      return fail(e, JX_E_INVALID, "combine: a merged share holds a non-canonical field element (>= p)");
    }
  }
  return JX_OK;
}

int32_t jx_engine_wait_event(jx_engine* e, void* event) {
  if (!e || !event) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamWaitEvent(e->stream, (hipEvent_t)event, 0));
  return JX_OK;
}

int32_t jx_engine_record_event(jx_engine* e, void* event) {
  if (!e || !event) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  HIPCHK(e, hipEventRecord((hipEvent_t)event, e->stream));
  return JX_OK;
}

int32_t jx_engine_wait_stream(jx_engine* e, void* stream) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  // hipStreamWaitEvent captures the event's current record, so one reused event serves every call
  HIPCHK(e, hipEventRecord(e->ev_wait, (hipStream_t)stream));
  HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_wait, 0));
  return JX_OK;
}

int32_t jx_engine_join_stream(jx_engine* e, void* stream) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  FLUSH_ACC(e);  // the deferred accumulations land first
  HIPCHK(e, hipEventRecord(e->ev_join, e->stream));
  HIPCHK(e, hipStreamWaitEvent((hipStream_t)stream, e->ev_join, 0));
  return JX_OK;
}

int32_t jx_engine_stream(jx_engine* e, void** stream) {
  if (!e || !stream) return JX_E_INVALID;
  LOCK(e);
  FLUSH_ACC(e);  // work the caller queues on the stream sees the deferred accumulations
  *stream = (void*)e->stream;
  return JX_OK;
}

int32_t jx_engine_timing(jx_engine* e, int32_t enable) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  int32_t rc = drain_timing(e);
  if (rc) return rc;
  rc = collect_pipe_timing(e);
  if (rc) return rc;
  for (jx_engine* q : e->pipes) q->timing = enable != 0;
  e->timing = enable != 0;
  for (int i = 0; i < NST; i++) {
    e->ms[i] = 0;
    e->launches[i] = 0;
  }
  return JX_OK;
}

int32_t jx_engine_timing_read(jx_engine* e, float ms[4], uint64_t launches[4]) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  int32_t rc = drain_timing(e);
  if (rc) return rc;
  rc = collect_pipe_timing(e);
  if (rc) return rc;
  for (int i = 0; i < NST; i++) {
    if (ms) ms[i] = (float)e->ms[i];
    if (launches) launches[i] = e->launches[i];
  }
  return JX_OK;
}

int32_t jx_engine_coalesce(jx_engine* e, int32_t enable, uint32_t window_us) {
  if (!e || e->is_pipe) return JX_E_INVALID;
  if (window_us > 1000000) return JX_E_INVALID;
  // under the engine mutex: concurrent enables create (and reference) the device coalescer once
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  if (enable && !e->coal) {
    e->coal = coalescer_for(e);
    if (!e->coal) return fail(e, JX_E_HIP, "coalesce: could not start the device coalescer");
  }
  e->coalesce = enable != 0;
  if (e->coal) coalescer_set_window(e, window_us);
  return JX_OK;
}

int32_t jx_engine_debug(jx_engine* e, int32_t option, int64_t value) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  if (option == 1) {
    e->force_slow = value != 0;
    return JX_OK;
  }
  if (option == 3) {  // helper K1 kernel
    if (!k1_forceable(value)) return JX_E_INVALID;
    // 0: automatic (fused; lane-split below one fused wave per SIMD, lane pairs below one lane-split
    // wave per SIMD, a word per lane for the smallest launches), 3: lane-split, 5: fused, 6: lane pairs,
    // 7: a word per lane (6, 7: bits <= 32)
    e->k1_forced = (K1Kernel)value;
    return JX_OK;
  }
  if (option == 4) {  // pipelines of the fused device path: 0 automatic, 1 single stream, 2..MAX_PIPES (4)
    if (value < 0 || value > (int64_t)MAX_PIPES) return JX_E_INVALID;
    e->npipes = (uint32_t)value;
    return JX_OK;
  }
  if (option == 2) {  // accumulate chunking (tests); staging is sized per call
    // first user: tests/test_gpu_accumulate_edges.py (block splits of accumulate_kernel, work-item lengths of seg_*)
    if (value < 1 || value > 4096) return JX_E_INVALID;
    e->acc_chunks = (uint32_t)value;
    return JX_OK;
  }
  if (option == 6) {  // lane-split K1 workgroups per CU: 0 no cap, 1..8
    if (value < 0 || value > 8) return JX_E_INVALID;
    e->lanes_wg_cap = (uint32_t)value;
    for (jx_engine* q : e->pipes) q->lanes_wg_cap = e->lanes_wg_cap;
    return JX_OK;
  }
  if (option == 8) {  // jx_accumulate of job-sized batches: 1 deferred and flushed together (default), 0 at once
    if (value != 0 && value != 1) return JX_E_INVALID;
    if (!value) FLUSH_ACC(e);
    e->acc_defer = value != 0;
    return JX_OK;
  }
  if (option == 9) {  // tests: run the deferred accumulations now
    FLUSH_ACC(e);
    return JX_OK;
  }
  if (option == 10) {  // reports per launch of jx_client_shard_*: 0 automatic (by the scratch budget)
    if (value < 0) return JX_E_INVALID;
    e->shard_chunk = (uint64_t)value;
    return JX_OK;
  }
  if (option == 11) {  // reports per launch of jx_client_seal_*: 0 automatic
    if (value < 0) return JX_E_INVALID;
    e->seal_chunk = (uint64_t)value;
    return JX_OK;
  }
  if (option == 12) {  // waves per report of the upload gather and the report pack: 0 automatic, 1..64
    if (value < 0 || value > 64) return JX_E_INVALID;
    e->upload_parts = (uint32_t)value;
    return JX_OK;
  }
  if (option == 7) {  // tests: the device coalescer's gathers wait (up to their window) for this many jobs
    if (value < 0 || value > (int64_t)MAX_JOBS_PER_LAUNCH) return JX_E_INVALID;
    if (!e->coal) return fail(e, JX_E_STATE, "debug option 7: coalescing is off");
    coalescer_set_min_jobs(e, (uint32_t)value);
    return JX_OK;
  }
  if (option == 5) {  // reports per launch of the fused paths: 0 automatic, else >= 64 (rounded down to 64)
    if (value != 0 && value < 64) return JX_E_INVALID;
    e->default_chunk = value ? (uint64_t)value / 64 * 64 : e->auto_chunk;
    for (jx_engine* q : e->pipes) q->default_chunk = e->default_chunk;
    return JX_OK;
  }
  return JX_E_INVALID;
}

const char* jx_status_str(int32_t s) {
  switch (s) {
    case JX_OK:
      return "ok";
    case JX_E_INVALID:
      return "invalid argument";
    case JX_E_UNSUPPORTED:
      return "unsupported Prio3 parameters";
    case JX_E_HIP:
      return "HIP runtime error";
    case JX_E_NOMEM:
      return "device out of memory";
    case JX_E_STATE:
      return "call out of order";
    case JX_E_NODEVICE:
      return "no HIP device";
    default:
      return "unknown status";
  }
}

const char* jx_last_error(const jx_engine* e) {
  (void)e;
  return t_err.c_str();
}

}  // extern "C"

