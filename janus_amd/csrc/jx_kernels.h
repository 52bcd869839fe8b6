// jx_kernels.h — kernel argument structs and launchers shared by the kernel units (jx_kernels.hip, jx_flp.hip,
// jx_accumulate.hip, jx_mp64.hip) and the engine's host sources (jx_engine*.cpp), and the device helpers that
// address the interleaved staging. See DESIGN.md for the HBM layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jx_flags.h"
#include "jx_k1_plan.h"
#include "jx_keyreg.h"

namespace jx {

enum Algo : uint32_t {
  ALGO_COUNT = 0,
  ALGO_SUM = 1,
  ALGO_SUMVEC = 2,
  ALGO_HISTOGRAM = 3,
  // Prio3SumVecField64MultiproofHmacSha256Aes128 (core/src/vdaf.rs:173-199): Field64, num_proofs
  // >= 2, XofHmacSha256Aes128 with 32-byte seeds (kernels: jx_mp64.hip)
  ALGO_SUMVEC_F64_MULTIPROOF = 4,
  // Prio3FixedPointBoundedL2VecSum{bitsize 16 | 32, length} (core/src/vdaf.rs:86-91, aggregator.rs:916-932):
  // Field128, TurboSHAKE, two gadgets: ParallelSum(Mul, chunk) range check over every input bit and
  // ParallelSum(PolyEval(2^(2n-2) - 2^n y + y^2), chunk1) over the decoded entries (the squared norm)
  ALGO_FIXEDPOINT_L2 = 5,
};
constexpr uint32_t MP_MAX_PROOFS = 8;  // num_proofs supported by the multiproof kernels

// Interleaved staging: element e of report r lives at [(r/64)][e][r%64] (16 bytes each),
// so a wave (64 reports, one per lane) touching element e moves one coalesced 1 KiB.
constexpr int IL = 64;

struct Cfg {
  uint32_t algo, bits, length, chunk;
  uint32_t meas_len, out_len, jr_len, proof_len, ver_len, calls, P, logP, gpoly_len;
  uint32_t ps_bytes, his_bytes, lps_bytes;
  uint32_t lis_bytes;    // leader input share: meas || proofs || [k_blind]
  uint32_t ncoef;        // coefficient slots per report
  uint32_t out_is_meas;  // truncate == identity (Histogram): output share aliases the meas staging
  uint32_t ppw, ngroups; // ParallelSum FLP: chunk slots per group, groups per 64-report block
  uint32_t ngt;          // partial-sum groups per block over all gadgets (ngroups [+ ngroups1])
  uint32_t vk[4];
  // constant table offsets (uint4 units) in Bufs::consts
  uint32_t c_omega, c_S, c_misc;
  uint32_t fb;      // field element bytes (8: Field64, 16: Field128)
  uint32_t seed;    // XOF SEED_SIZE (16 TurboSHAKE128, 32 HmacSha256Aes128) = prep message bytes
  uint32_t np;      // num_proofs
  uint32_t dst_id;  // algorithm id in the XOF domain-separation tags
  uint32_t nco;     // multiproof: coefficient slots per proof
  // multiproof: HMAC-SHA256 inner/outer states after the key block, for the 32-byte verify key
  // (query randomness) and the all-zero key (joint-rand seed derivations)
  uint32_t vk_ist[8], vk_ost[8], zero_ist[8], zero_ost[8];
  uint32_t trunc_len;  // measurement elements that truncate into the output share (SumVec/Sum/FixedPoint)
  uint32_t qr_len;     // query randomness elements (= gadgets)
  // FixedPointBoundedL2VecSum: the norm bits and gadget 1 (ParallelSum(PolyEval), arity chunk1)
  uint32_t norm_bits;
  uint32_t chunk1, calls1, P1, logP1, gpoly1_len, ppw1, ngroups1;
  uint32_t proof1_off;  // first element of gadget 1's sub-proof [seeds (chunk1) || gadget poly]
  uint32_t coef1;       // first coefficient slot of gadget 1 (G1_* below)
  uint32_t c_omega1, c_S1;  // constant-table offsets of gadget 1's roots and S1_m
  // ParallelSum(Mul) gadget 0 (SumVec, Histogram, FixedPoint): per-report power tables K1 writes so that
  // the FLP group finish needs no exponentiation: c_rpow + j = L r^(j+1) canonical (j < chunk), c_tpow + g
  // = t^(g * per) R, per = ceil(gpoly_len / ngroups) (the group's first gadget-polynomial coefficient)
  uint32_t c_rpow, c_tpow;
};

// coefficient slots (Montgomery form unless noted) for the ParallelSum / Sum FLP. Prio3Sum: as named;
// ParallelSum (SumVec, Histogram, FixedPoint gadget 0) stores them scaled by L for the group finish:
// COEF_L = L canonical, COEF_C0 = c_0 L R, COEF_HALFSUM = L (1/2) sum c_k canonical (xof_tail)
enum : uint32_t {
  COEF_L = 0,        // L = (t^P - 1)/P
  COEF_C0 = 1,       // c_0 = 1/(t - 1)
  COEF_HALFSUM = 2,  // (1/2) * sum_{k>=1} c_k   [canonical]
  COEF_T = 3,        // t
  COEF_R = 4,        // joint_rand[0]
  COEF_R2 = 5,       // joint_rand[1] (Histogram)
  COEF_K = 6,        // first per-call slot
};
// The per-call region from COEF_K on. Prio3Sum: one 16-byte slot c_k per call. ParallelSum gadget 0: call
// k's pair (c_k, d_k) as its ten 26-bit limbs (pack_cd26, jx_field.h), COEF_CALL_U4 uint4 (2.5 KiB) per
// call and 64-report block, at uint4 offset COEF_K * IL + (k - 1) * COEF_CALL_U4 of the block's staging:
//   row A       [lane] uint4  c_k limbs 0-3
//   row B       [lane] uint4  d_k limbs 0-3      (+ COEF_ROWB_U4)
//   half-row C  [lane] uint2  (c_k, d_k) limb 4  (+ COEF_ROWC_U4)
// i.e. exactly the bytes one slot of the K3 ring's coefficient stream holds. coef_call_slots rounds the
// region up to whole 16-byte slots per report.
constexpr uint32_t COEF_CALL_U4 = 2 * IL + IL / 2;
constexpr uint32_t COEF_ROWB_U4 = IL, COEF_ROWC_U4 = 2 * IL;
constexpr uint32_t COEF_CALL_BYTES = COEF_CALL_U4 * 16;
inline uint32_t coef_call_slots(uint32_t calls) { return (5 * calls + 1) / 2; }
// FixedPoint gadget-1 coefficient slots, relative to Cfg::coef1 (Montgomery form)
enum : uint32_t {
  G1_L = 0,   // (t1^P1 - 1)/P1
  G1_C0 = 1,  // c'_0 = 1/(t1 - 1)
  G1_T = 2,   // t1
  G1_K = 3,   // c'_k, k = 1..calls1
};
// misc constants (uint4 slots at Cfg::c_misc): 0 (1/P)R, 1 1/2, 2 R, 3 (1/2)R; FixedPoint: 4 2^n,
// 5 2^(2n-2) R^-1, 6 2^(n-2) (gadget-1 padding, a share of the encoded 0.0), 7 (1/P1)R; 8 zero (the
// source of the FLP ring's loads for measurement elements past the share and for padded slots)
constexpr uint32_t NMISC = 9;
constexpr uint32_t MISC_ZERO = 8;

struct Bufs {
  uint64_t n;  // reports in this launch
  const uint8_t* nonces;
  const uint8_t* ps;
  const uint8_t* his;
  const uint8_t* lps;
  const uint8_t* lis;   // leader role: explicit leader input shares (n rows of lis_rs bytes)
  uint64_t lis_rs;      // leader role: row stride of lis (>= lis_bytes, a multiple of 16)
  // per-report verify keys (nullable: every report uses Cfg::vk / vk_ist, vk_ost): a coalesced launch
  // prepares the jobs of several tasks (engines) of one Prio3 instance. Row r: the 16-byte key
  // (TurboSHAKE instances) or the HMAC-SHA256 pads ist[8] || ost[8] of the 32-byte key (multiproof).
  const uint8_t* vkeys;
  uint8_t* lps_out;     // leader role: outbound prep shares (n x lps_bytes)
  uint32_t leader;      // 1: run prepare_init for agg_id 0 (leader_initialized)
  uint4* meas;
  // leader, read in place: the FLP kernels read measurement element e of report r at
  // meas_src + r * meas_rs + 16 e (the explicit leader input share) instead of the interleaved
  // staging, which K1 then does not write (meas_rs == 0: the staging)
  const uint8_t* meas_src;
  uint64_t meas_rs;
  uint4* proof;
  uint4* outs;
  uint4* coef;
  uint32_t* flags;
  uint4* part;  // ParallelSum FLP partial sums [blk][group][4][lane] (multiproof: uint2 [blk][proof][group][3][lane])
  uint8_t* verdicts;
  uint8_t* msgs;
  const uint4* consts;
  uint32_t force_slow;  // debug: route every report through the slow XOF kernel
};

struct AccArgs {
  uint64_t n;
  const uint4* outs;
  uint32_t out_len;
  const uint8_t* verdicts;
  const uint8_t* mask;     // nullable
  const uint32_t* seg;     // nullable
  uint32_t seg_id;
  uint64_t* partials;      // [nchunks][out_len][3]
  uint32_t blocks_per_chunk;
  uint32_t nchunks;
  const uint8_t* nonces;
  uint32_t* checksum;      // [8] (XOR)
  unsigned long long* count;
};

// Segmented accumulation (batch aggregations of several batch identifiers in one pass,
// aggregation_job_writer.rs:608-708): reports are counting-sorted by dense segment index on the
// device, then summed per (segment, run of <= L sorted positions) work item, then per segment.
constexpr uint32_t SEG_MAX = 4096;
constexpr uint32_t SELECT_WGS = 1024;  // grid-stride workgroups of the select / segment-count kernels  // dense segment indices handled per pass (LDS histogram size)
struct SegArgs {
  uint64_t n;
  const uint4* outs;
  uint32_t out_len;
  uint32_t fb;
  const uint8_t* verdicts;
  const uint8_t* mask;     // nullable
  const uint32_t* seg;     // dense segment index per report
  uint32_t s0, ns;         // this pass: dense indices [s0, s0 + ns)
  const uint8_t* nonces;
  uint32_t* cnt;           // [ns] selected reports per segment (zeroed by the host)
  uint32_t* off;           // [ns] first sorted position of each segment
  uint32_t* cursor;        // [ns] scatter cursors
  uint32_t* ioff;          // [ns + 1] first work item of each segment
  uint32_t* perm;          // [n] selected report indices grouped by segment
  uint32_t L;              // sorted positions per work item
  uint4* items;            // [wmax] (segment, p0, p1, 0)
  uint32_t* nitems;        // [2]: work items, selected reports
  uint32_t wmax;
  uint64_t* partials;      // [wmax][out_len][3]
  uint4* const* aggs;                  // [ns] the segments' aggregate shares
  unsigned long long* const* counts;   // [ns]
  uint32_t* const* checksums;          // [ns] [8]
};
hipError_t launch_accumulate_segmented(const Cfg& c, const SegArgs& a, uint32_t grid, hipStream_t s);

// multiproof coefficient slots (canonical Field64), per proof
enum : uint32_t { MCOEF_L = 0, MCOEF_C0 = 1, MCOEF_HALFSUM = 2, MCOEF_T = 3, MCOEF_R = 4, MCOEF_K = 5 };

// launchers (jx_kernels.hip: K0, K1; jx_flp.hip: K3, leader finish; jx_accumulate.hip: the rest)
hipError_t launch_count(const Cfg& c, const Bufs& b, hipStream_t s);
// the helper K1 that k1_plan chose (jx_k1_plan.h); a leader launch (b.leader) runs the leader kernels
hipError_t launch_xof(const Cfg& c, const Bufs& b, K1Launch k1, hipStream_t s);
hipError_t launch_xof_slow(const Cfg& c, const Bufs& b, hipStream_t s);
hipError_t launch_leader_finish(const Cfg& c, const Bufs& b, const uint8_t* prep_msgs, const uint8_t* peer,
                                hipStream_t s);
hipError_t launch_flp(const Cfg& c, const Bufs& b, hipStream_t s);
hipError_t launch_accumulate(const Cfg& c, const AccArgs& a, uint4* agg, hipStream_t s);
// Accumulations of at most ACC_SMALL reports: one kernel, no partials or selection scratch (a.partials unused).
constexpr uint64_t ACC_SMALL = 1024;
hipError_t launch_accumulate_small(const Cfg& c, const AccArgs& a, uint4* agg, hipStream_t s);
// Several small batches into ONE aggregation in one kernel (jx_accumulate calls the engine deferred and
// flushes together): every finished report of every batch is added. The table travels as the kernel argument.
constexpr uint32_t ACC_MULTI_MAX = 64;
struct AccDesc {
  const uint4* outs;
  const uint8_t* verdicts;
  const uint8_t* nonces;
  uint64_t n;
};
struct AccMultiArgs {
  AccDesc d[ACC_MULTI_MAX];
  uint32_t nb;
  uint4* agg;
  unsigned long long* count;
  uint32_t* checksum;
};
hipError_t launch_accumulate_multi(const Cfg& c, const AccMultiArgs& a, hipStream_t s);
// The host sees a launch complete without a runtime call: one lane stores `seq` into a host-coherent pinned flag
// once the stream reaches this point (a system-scope release store, so the stream's earlier downloads are
// visible first). The coalescer's completer polls the flags instead of querying events.
hipError_t launch_host_signal(uint32_t* flag, uint32_t seq, hipStream_t s);
// Strided row copies between HBM and mapped pinned host memory by a kernel on the caller's stream (a coalesced
// launch's uploads and downloads): no copy-engine command, so a lane's transfers never queue behind another
// lane's download that is waiting for that lane's kernels (measured: ~1-2 ms stalls). Region
// k copies `rows` rows of `width` bytes; 16-byte vectors when every address, stride and the width allow.
struct CopyRegion {
  uint8_t* dst;
  const uint8_t* src;
  uint64_t dst_stride, src_stride, rows;
  uint64_t width;
};
constexpr uint32_t COPY_MAX_REGIONS = 12;
struct CopyArgs {
  CopyRegion r[COPY_MAX_REGIONS];
  uint32_t nr;
};
hipError_t launch_copy_regions(const CopyArgs& a, hipStream_t s);
hipError_t launch_combine(const Cfg& c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err,
                          hipStream_t s);
// ns records of contiguous segment state (agg [ns][out_len], count [ns], checksum [ns][8])
hipError_t launch_record_export(const Cfg& c, const uint4* agg, const unsigned long long* count,
                                const uint32_t* checksum, uint8_t* dst, hipStream_t s, uint32_t ns = 1);
hipError_t launch_record_combine(const Cfg& c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err,
                                 hipStream_t s);
hipError_t launch_transpose_out(const Cfg& c, const uint4* outs, uint64_t n, uint8_t* dst, hipStream_t s);
hipError_t launch_agg_encode(const Cfg& c, const uint4* agg, uint8_t* dst, hipStream_t s);
// one job of a coalesced launch: reports [first, first + n) go to the job's batch buffers
struct JobSlice {
  uint64_t first, n;
  uint4* outs;
  uint8_t* verdicts;
  uint8_t* msgs;
  uint8_t* nonces;
};
constexpr uint32_t MAX_JOBS_PER_LAUNCH = 4096;
hipError_t launch_scatter_jobs(const Cfg& c, const JobSlice* d_jobs, uint32_t njobs, uint64_t max_job_reports,
                               const uint4* outs, const uint8_t* verdicts, const uint8_t* msgs, const uint8_t* nonces,
                               hipStream_t s);
// ---- HPKE open inside a helper prepare launch (jx_hpke.hip; jx_helper_prep_encrypted_batch)
// HpkeKeyRow (a row of the device key registry) and EncRow: jx_keyreg.h
struct HpkeRowsArgs {
  uint64_t n;
  const EncRow* rows;
  const uint8_t* cts;   // ciphertext bytes of the launch
  uint8_t* pts;         // plaintext scratch (same offsets as cts)
  const HpkeKeyRow* keys;  // the device's key registry (jx_keyreg.h), indexed by EncRow::key0 / key1
  uint32_t nkeys;          // its capacity
  const uint8_t* nonces;
  const uint8_t* ps;
  uint32_t ps_bytes;
  uint8_t* his;  // out: the helper input-share rows K1 reads
  uint32_t his_bytes;
  uint8_t* status;  // out: JX_OPEN_* per report
};

// the helper K1 (jx_kernels.hip)
uint64_t k1_round_reports(const Cfg& c, int device);
// The helper reports [S, b.n) of a launch as Bufs of their own (S a multiple of 64: every staging array is
// interleaved by 64-report blocks), for a K1 launch over part of the reports.
Bufs bufs_tail(const Cfg& c, const Bufs& b, uint64_t S);
// multiproof Field64 SumVec (jx_mp64.hip)
uint64_t mp_k1_round_reports(int device);
hipError_t launch_mp_xof(const Cfg& c, const Bufs& b, hipStream_t s);
hipError_t launch_mp_slow(const Cfg& c, const Bufs& b, hipStream_t s);
hipError_t launch_mp_flp(const Cfg& c, const Bufs& b, hipStream_t s);

inline uint32_t nblk_of(uint64_t n) { return (uint32_t)((n + 63) / 64); }  // 64-report blocks of a launch

}  // namespace jx

// ---- the staging layout as the kernels address it (device code: jx_kernels.hip, jx_flp.hip, jx_accumulate.hip)
#if defined(__HIPCC__) || defined(__HIP__)
#include "jx_field.h"

namespace jx {

// interleaved staging address
__device__ __forceinline__ uint64_t il_idx(uint64_t blk, uint32_t len, uint32_t e, uint32_t lane) {
  return (blk * len + e) * IL + lane;
}
// (the staging is global memory: the address-space casts keep these global_load/store even inside the
// non-inlined XOF tail, where a generic pointer would make them flat accesses that wait with vmcnt(0) and
// lgkmcnt(0) each)
// global (not flat) pointers for the staging in the non-inlined XOF tail: flat accesses count in both
// vmcnt and lgkmcnt and force full waits; the host pass of hipcc keeps plain pointers
#ifdef __HIP_DEVICE_COMPILE__
typedef __attribute__((address_space(1))) uint4 g_uint4;
typedef __attribute__((address_space(1))) uint2 g_uint2;
#else
typedef uint4 g_uint4;
typedef uint2 g_uint2;
#endif
__device__ __forceinline__ f128 ld_il(const uint4* base, uint64_t blk, uint32_t len, uint32_t e, uint32_t lane) {
  return u4_to_f(((const g_uint4*)base)[il_idx(blk, len, e, lane)]);
}
__device__ __forceinline__ void st_il(uint4* base, uint64_t blk, uint32_t len, uint32_t e, uint32_t lane, f128 v) {
  ((g_uint4*)base)[il_idx(blk, len, e, lane)] = f_to_u4(v);
}
// ParallelSum call k's staged coefficient limbs (the layout at COEF_K above) of one report: cblk = the
// block's coefficient staging (b.coef + il_idx(blk, ncoef, 0, 0)).
struct CoefCall {
  uint4 a, b;  // rows A, B
  uint2 e;     // half-row C
};
__device__ __forceinline__ CoefCall ld_coef_call(const uint4* cblk, uint32_t lane, uint32_t k) {
  const g_uint4* p = (const g_uint4*)cblk + (uint64_t)COEF_K * IL + (uint64_t)(k - 1) * COEF_CALL_U4;
  CoefCall v;
  v.a = p[lane];
  v.b = p[COEF_ROWB_U4 + lane];
  v.e = ((const g_uint2*)(p + COEF_ROWC_U4))[lane];
  return v;
}
__device__ __forceinline__ void coef_call_limbs(const CoefCall& v, limbs26& c, limbs26& d) {
  const uint32_t w[CD26_WORDS] = {v.a.x, v.a.y, v.a.z, v.a.w, v.b.x, v.b.y, v.b.z, v.b.w, v.e.x, v.e.y};
  unpack_cd26(w, c, d);
}
__device__ __forceinline__ void st_coef_call(uint4* cblk, uint32_t lane, uint32_t k, f128 c, f128 d) {
  uint32_t w[CD26_WORDS];
  pack_cd26(c, d, w);
  g_uint4* p = (g_uint4*)cblk + (uint64_t)COEF_K * IL + (uint64_t)(k - 1) * COEF_CALL_U4;
  p[lane] = make_uint4(w[0], w[1], w[2], w[3]);
  p[COEF_ROWB_U4 + lane] = make_uint4(w[4], w[5], w[6], w[7]);
  ((g_uint2*)(p + COEF_ROWC_U4))[lane] = make_uint2(w[8], w[9]);
}
// The measurement share as the FLP kernels read it: the interleaved staging (element e of the lane's
// report at p[e * IL]) or, for the leader, its explicit input share in place (p[e], report-major).
struct MeasView {
  const uint4* p;
  uint32_t es;  // element stride in uint4
  __device__ __forceinline__ const uint4& operator[](uint64_t e) const { return p[e * es]; }
};
__device__ __forceinline__ MeasView meas_view(const Cfg& c, const Bufs& b, uint64_t blk, uint32_t lane) {
  if (b.meas_rs) {
    const uint64_t r0 = blk * 64 + lane, r = r0 < b.n ? r0 : b.n - 1;
    return MeasView{reinterpret_cast<const uint4*>(b.meas_src + r * b.meas_rs), 1u};
  }
  return MeasView{b.meas + il_idx(blk, c.meas_len, 0, lane), (uint32_t)IL};
}
__device__ __forceinline__ void load16(const uint8_t* p, uint32_t w[4]) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
}

// the verify key of report r: its row of the per-report keys of a coalesced launch, or the engine's
__device__ __forceinline__ void load_vk(const Cfg& c, const Bufs& b, uint64_t r, uint32_t vk[4]) {
  if (b.vkeys) {
    load16(b.vkeys + 16 * r, vk);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) vk[i] = c.vk[i];
  }
}

// 192-bit add of x << sh (sh < 64) into the accumulator
__device__ __forceinline__ void trunc_add(acc192& a, f128 x, uint32_t sh) {
  uint64_t w0 = x.lo << sh;
  uint64_t w1 = sh ? ((x.hi << sh) | (x.lo >> (64 - sh))) : x.hi;
  uint64_t w2 = sh ? (x.hi >> (64 - sh)) : 0;
  uint32_t cc = 0;
  a.w0 = addc64(a.w0, w0, cc);
  a.w1 = addc64(a.w1, w1, cc);
  a.w2 = a.w2 + w2 + cc;
}

// A value the optimizer cannot see through (no instruction is emitted): keeps x * 2^j a single
// v_mad_u64_u32 (x * 2^j + T) instead of the zero-extend + 64-bit shift + 64-bit add it would
// strength-reduce the multiply to.
__device__ __forceinline__ uint32_t opaque_u32(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Output-share truncation in the fast XOF kernel (SumVec / Sum):
//   out_i = sum_{j<bits} 2^j x_{bits*i+j} mod p.
// Word columns T_w = sum_j x_{j,w} 2^j (< 2^(32+bits) <= 2^64) cost one v_mad_u64_u32 per 32-bit
// word of each element; the <= 160-bit total is reduced once per output element.
struct TruncW {
  uint64_t T[4];
  uint32_t j, i;
};
__device__ __forceinline__ void truncw_zero(TruncW& t) {
#pragma unroll
  for (int w = 0; w < 4; w++) t.T[w] = 0;
}
// T_w += v_w * sh for the element v, sh = 2^j (or 0 for an element that does not count)
__device__ __forceinline__ void truncw_mac(TruncW& t, uint4 v, uint32_t sh) {
  t.T[0] += (uint64_t)v.x * sh;
  t.T[1] += (uint64_t)v.y * sh;
  t.T[2] += (uint64_t)v.z * sh;
  t.T[3] += (uint64_t)v.w * sh;
}
__device__ __forceinline__ f128 truncw_value(const TruncW& t) {
  // V = T0 + T1 2^32 + T2 2^64 + T3 2^96
  uint32_t c = 0;
  const uint64_t w0 = addc64(t.T[0], t.T[1] << 32, c);
  const uint64_t w1 = addc64(t.T[2], (t.T[1] >> 32) | (t.T[3] << 32), c);
  const uint64_t w2 = (t.T[3] >> 32) + c;
  return reduce192_small(w0, w1, w2);  // V < 2^(128 + bits), bits <= 32
}

// h * 2^32 mod p (the high half of a > 32-bit truncation)
__device__ __forceinline__ f128 shl32_mod(f128 h) {
  return reduce192(h.lo << 32, (h.hi << 32) | (h.lo >> 32), h.hi >> 32);
}

}  // namespace jx
#endif  // __HIPCC__
