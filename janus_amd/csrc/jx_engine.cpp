// jx_engine.cpp — host side of the C ABI in include/jx_prio3.h.
//
// Owns device staging, constant tables, resident prepared batches and per-segment batch
// aggregations; sequences the K1 (XOF) -> K1' (slow path) -> K3 (FLP) -> K4 (accumulate) launches
// on one HIP stream per engine. Every entry point takes the engine mutex for the duration of the
// call only, so concurrent aggregation jobs can share an engine (each holds a batch handle). There
// is no CPU compute path: if the device or the kernels are unavailable every entry point fails with
// an error status.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_field.h"
#include "jx_fused_plan.h"
#include "jx_ntt.h"
#include "jx_sha_aes.h"
#include "jx_shard.h"
#include "jx_upload.h"

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

// every entry point: the engine mutex for the call, and a fresh per-thread error message
#define LOCK(e)                                   \
  std::lock_guard<jxi::FairMutex> _lk((e)->mu);   \
  t_err.clear()


// ---------------------------------------------------------------------------- host field helpers

static f128 h_mpow(f128 aR, uint64_t e) {
  f128 r = make128(R1_128_LO, R1_128_HI);
  while (e) {
    if (e & 1) r = mont128(r, aR);
    aR = mont128(aR, aR);
    e >>= 1;
  }
  return r;
}
static f128 h_minv(f128 aR) {
  // exponent p - 2 = 0xFFFFFFFFFFFFFFE3_FFFFFFFFFFFFFFFF, square-and-multiply from the top bit
  const uint64_t ehi = 0xFFFFFFFFFFFFFFE3ull, elo = 0xFFFFFFFFFFFFFFFFull;
  f128 r = make128(R1_128_LO, R1_128_HI);
  for (int i = 127; i >= 0; i--) {
    r = mont128(r, r);
    uint64_t bit = i >= 64 ? (ehi >> (i - 64)) & 1 : (elo >> i) & 1;
    if (bit) r = mont128(r, aR);
  }
  return r;
}
static uint4 h_u4(f128 a) {
  uint4 v;
  v.x = lo32(a.lo);
  v.y = hi32(a.lo);
  v.z = lo32(a.hi);
  v.w = hi32(a.hi);
  return v;
}
static f128 h_from_u64(uint64_t v) { return make128(v, 0); }

static int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
static int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) l++;
  return l;
}
static uint32_t isqrt_floor(uint32_t v) {
  uint32_t r = 0;
  while ((uint64_t)(r + 1) * (r + 1) <= v) r++;
  return r < 1 ? 1 : r;
}

namespace jx {
int psum_ppw(uint32_t chunk);
}

// ---------------------------------------------------------------------------- configuration

// HMAC-SHA256 states after the key block for a 32-byte key (little-endian memory words)
static void host_hmac_pads(const uint8_t key[32], uint32_t ist[8], uint32_t ost[8]) {
  uint32_t kbe[8];
  for (int i = 0; i < 8; i++)
    kbe[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) | ((uint32_t)key[4 * i + 2] << 8) |
             key[4 * i + 3];
  hmac_pads(kbe, ist, ost);
}

// most gadget calls of a Field128 ParallelSum instance (see make_cfg)
constexpr uint32_t MAX_PSUM128_CALLS = 1u << 16;

static int32_t make_cfg(const jx_prio3_params* p, const uint8_t* vk, uint32_t vk_len, Cfg& c, std::string& why) {
  memset(&c, 0, sizeof c);
  const bool mp = p->algo_id == ALGO_SUMVEC_F64_MULTIPROOF;
  if (mp ? (p->num_proofs < 2 || p->num_proofs > MP_MAX_PROOFS) : p->num_proofs != 1) {
    why = mp ? "num_proofs must be in [2, 8]" : "num_proofs must be 1";
    return JX_E_UNSUPPORTED;
  }
  if (vk_len != (mp ? 32u : 16u)) {
    why = "verify key length must be 16 (32 for Prio3SumVecField64MultiproofHmacSha256Aes128)";
    return JX_E_INVALID;
  }
  c.algo = p->algo_id;
  c.np = p->num_proofs;
  c.seed = mp ? 32 : 16;
  c.dst_id = mp ? 0xFFFF1003u : p->algo_id;  // core/src/vdaf.rs:18-20
  c.bits = p->bits;
  c.length = p->length;
  c.chunk = p->chunk_length;
  uint32_t arity = 0;
  switch (p->algo_id) {
    case ALGO_COUNT:
      c.meas_len = 1;
      c.out_len = 1;
      c.jr_len = 0;
      c.calls = 1;
      arity = 2;
      break;
    case ALGO_SUM:
      if (p->bits < 1 || p->bits > 64) {
        why = "Prio3Sum bits must be in [1, 64]";
        return JX_E_UNSUPPORTED;
      }
      c.meas_len = p->bits;
      c.out_len = 1;
      c.jr_len = 1;
      c.calls = p->bits;
      arity = 1;
      break;
    case ALGO_SUMVEC:
    case ALGO_SUMVEC_F64_MULTIPROOF:
      if (p->bits < 1 || p->bits > (mp ? 32u : 64u) || p->length < 1 || p->chunk_length < 1) {
        why = mp ? "Prio3SumVecField64Multiproof needs 1 <= bits <= 32, length >= 1, chunk_length >= 1"
                 : "Prio3SumVec needs 1 <= bits <= 64, length >= 1, chunk_length >= 1";
        return JX_E_UNSUPPORTED;
      }
      c.meas_len = p->bits * p->length;
      c.out_len = p->length;
      c.jr_len = 1;
      c.calls = (c.meas_len + p->chunk_length - 1) / p->chunk_length;
      arity = 2 * p->chunk_length;
      break;
    case ALGO_HISTOGRAM:
      if (p->length < 1 || p->chunk_length < 1) {
        why = "Prio3Histogram needs length >= 1, chunk_length >= 1";
        return JX_E_UNSUPPORTED;
      }
      c.meas_len = p->length;
      c.out_len = p->length;
      c.jr_len = 2;
      c.calls = (p->length + p->chunk_length - 1) / p->chunk_length;
      arity = 2 * p->chunk_length;
      c.out_is_meas = 1;
      break;
    case ALGO_FIXEDPOINT_L2: {
      // FixedPointBoundedL2VecSum::new(entries) as prio 0.16.1 sizes it (restated in
      // oracle/prio3_oracle.c cfg_make): n-bit entries (n = 16 | 32, BitSize16 / BitSize32,
      // core/src/vdaf.rs:26-33), 2n-2 norm bits, chunk0 = floor(sqrt(n*entries + 2n-2)),
      // chunk1 = floor(sqrt(entries)); chunk_length is not a parameter of this VDAF.
      if ((p->bits != 16 && p->bits != 32) || p->length < 1 || p->length > (1u << 24)) {
        why = "Prio3FixedPointBoundedL2VecSum needs bits (bitsize) 16 or 32 and 1 <= length <= 2^24";
        return JX_E_UNSUPPORTED;
      }
      c.dst_id = 0xFFFF0000u;
      c.norm_bits = 2 * p->bits - 2;
      c.meas_len = p->bits * p->length + c.norm_bits;
      c.out_len = p->length;
      c.jr_len = 2;
      c.chunk = isqrt_floor(c.meas_len);
      c.calls = (c.meas_len + c.chunk - 1) / c.chunk;
      arity = 2 * c.chunk;
      c.chunk1 = isqrt_floor(p->length);
      c.calls1 = (p->length + c.chunk1 - 1) / c.chunk1;
      c.P1 = next_pow2(1 + c.calls1);
      c.logP1 = ilog2(c.P1);
      c.gpoly1_len = 2 * (c.P1 - 1) + 1;
      c.ppw1 = 2;
      c.ngroups1 = (c.chunk1 + c.ppw1 - 1) / c.ppw1;
      break;
    }
    default:
      why = "unknown algo_id";
      return JX_E_INVALID;
  }
  const bool fp = c.algo == ALGO_FIXEDPOINT_L2;
  if (c.algo == ALGO_SUMVEC || c.algo == ALGO_HISTOGRAM || mp || fp) {
    c.ppw = psum_ppw(c.chunk);
    c.ngroups = (c.chunk + c.ppw - 1) / c.ppw;
  }
  c.ngt = c.ngroups + c.ngroups1;
  c.qr_len = fp ? 2 : 1;
  c.trunc_len = fp ? p->bits * p->length : c.out_len * c.bits;
  // Field128 ParallelSum: a lazy wire sum holds one product < 2^256 per call and wacc_reduce (jx_field.h)
  // takes values < 2^272. FixedPoint stays far below (calls < 2^15, calls1 <= 2^12); the Field64 kernels
  // fold into add64 and have no such limit.
  if ((c.algo == ALGO_SUMVEC || c.algo == ALGO_HISTOGRAM) && c.calls > MAX_PSUM128_CALLS) {
    why = "more than 65536 gadget calls (ceil(measurement length / chunk_length)) in a Field128 ParallelSum";
    return JX_E_UNSUPPORTED;
  }
  c.P = next_pow2(1 + c.calls);
  if (mp && c.P > (1u << 30)) {
    why = "too many gadget calls for Field64";
    return JX_E_UNSUPPORTED;
  }
  c.logP = ilog2(c.P);
  c.gpoly_len = 2 * (c.P - 1) + 1;
  c.proof_len = arity + c.gpoly_len;
  c.ver_len = arity + 2;
  if (fp) {  // gadget 1's sub-proof [seeds || gadget poly] and verifier part [wires || G1(t1)]
    c.proof1_off = c.proof_len;
    c.proof_len += c.chunk1 + c.gpoly1_len;
    c.ver_len += c.chunk1 + 1;
  }
  const uint32_t fb = (c.algo == ALGO_COUNT || mp) ? 8 : 16;
  c.fb = fb;
  const bool jr = c.jr_len > 0;
  const uint32_t S = c.seed;
  c.ps_bytes = jr ? 2 * S : 0;
  c.his_bytes = jr ? 3 * S : 2 * S;
  c.lps_bytes = c.np * c.ver_len * fb + (jr ? S : 0);
  c.lis_bytes = (c.meas_len + c.np * c.proof_len) * fb + (jr ? S : 0);
  if (mp) {
    c.nco = MCOEF_K + 2 * c.calls;
    c.ncoef = 0;
    host_hmac_pads(vk, c.vk_ist, c.vk_ost);
    const uint8_t zero[32] = {0};
    host_hmac_pads(zero, c.zero_ist, c.zero_ost);
  } else if (c.algo == ALGO_COUNT)
    c.ncoef = 0;
  else if (c.algo == ALGO_SUM)
    c.ncoef = COEF_K + c.calls;
  else
    c.ncoef = COEF_K + coef_call_slots(c.calls);  // (c_k, d_k) as 26-bit limbs: 40 bytes per call
  if (c.algo == ALGO_SUMVEC || c.algo == ALGO_HISTOGRAM || fp) {  // gadget 0's power tables (jx_kernels.h)
    c.c_rpow = c.ncoef;
    c.ncoef += c.chunk;
    c.c_tpow = c.ncoef;
    c.ncoef += c.ngroups;
  }
  if (fp) {
    c.coef1 = c.ncoef;
    c.ncoef += G1_K + c.calls1;
  }
  for (int i = 0; i < 4; i++)
    c.vk[i] = (uint32_t)vk[4 * i] | ((uint32_t)vk[4 * i + 1] << 8) | ((uint32_t)vk[4 * i + 2] << 16) |
              ((uint32_t)vk[4 * i + 3] << 24);
  c.c_omega = 0;
  c.c_S = c.P;
  c.c_misc = c.P + c.gpoly_len;
  c.c_omega1 = c.c_misc + NMISC;
  c.c_S1 = c.c_omega1 + c.P1;
  return JX_OK;
}

// constant tables: w^k R (k < P), S_m R = (sum_{k=1..calls} w^{km}) R (m < gpoly_len), misc
static uint4 h_u4_64(uint64_t v) {
  uint4 r;
  r.x = lo32(v);
  r.y = hi32(v);
  r.z = r.w = 0;
  return r;
}

// w1^k R (k < P1) and S1_m R for gadget 1 of FixedPointBoundedL2VecSum
static void root_tables(f128 gen, uint32_t P, uint32_t logP, uint32_t calls, uint32_t glen, uint4* omega, uint4* S) {
  f128 w = gen;
  for (int i = 0; i < 66 - (int)logP; i++) w = mont128(w, w);
  f128 wk = make128(R1_128_LO, R1_128_HI);
  std::vector<f128> pw(P);
  for (uint32_t k = 0; k < P; k++) {
    pw[k] = wk;
    omega[k] = h_u4(wk);
    wk = mont128(wk, w);
  }
  // S_m = sum_{k=1..calls} z^k with z = w^m depends on m mod P only: calls where z = 1 (m = 0 mod P), else
  // z (z^calls - 1) / (z - 1), the P - 1 inverses out of one h_minv (Montgomery's trick). The plain double
  // sum is glen * calls additions: most of a minute at 65536 calls.
  const f128 R1 = make128(R1_128_LO, R1_128_HI);
  std::vector<f128> d(P), pre(P), Sp(P);  // d[m] = (w^m - 1) R, pre[m] = (d[1] ... d[m]) R
  pre[0] = R1;
  for (uint32_t m = 1; m < P; m++) {
    d[m] = sub128(pw[m], R1);
    pre[m] = mont128(pre[m - 1], d[m]);
  }
  f128 inv = h_minv(pre[P - 1]);  // (d[1] ... d[m])^-1 R, m going down
  Sp[0] = to_mont128(h_from_u64(calls));
  for (uint32_t m = P - 1; m >= 1; m--) {
    const f128 dinv = mont128(inv, pre[m - 1]);
    inv = mont128(inv, d[m]);
    const f128 zc = pw[((uint64_t)m * calls) % P];
    Sp[m] = mont128(mont128(pw[m], sub128(zc, R1)), dinv);
  }
  for (uint32_t m = 0; m < glen; m++) S[m] = h_u4(Sp[m % P]);
}

static std::vector<uint4> make_consts(const Cfg& c) {
  std::vector<uint4> t(c.P + c.gpoly_len + NMISC + c.P1 + c.gpoly1_len);
  if (c.algo == ALGO_COUNT) return t;
  if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF) {
    // Field64: GEN = 7^((p-1)/2^32) (order 2^32), w = GEN^(2^(32 - logP)); canonical values
    uint64_t w = pow64_h(pow64_h(7, (P64 - 1) >> 32), 1ull << (32 - c.logP));
    std::vector<uint64_t> pw(c.P);
    uint64_t wk = 1;
    for (uint32_t k = 0; k < c.P; k++) {
      pw[k] = wk;
      t[c.c_omega + k] = h_u4_64(wk);
      wk = mul64(wk, w);
    }
    for (uint32_t m = 0; m < c.gpoly_len; m++) {
      uint64_t s = 0;
      for (uint32_t k = 1; k <= c.calls; k++) s = add64(s, pw[(uint64_t)(k * m) % c.P]);
      t[c.c_S + m] = h_u4_64(s);
    }
    t[c.c_misc + 0] = h_u4_64(pow64_h(c.P, P64 - 2));  // 1/P
    t[c.c_misc + 1] = h_u4_64(pow64_h(2, P64 - 2));    // 1/2
    return t;
  }
  // GEN = 7^((p-1)/2^66), order 2^66; w = GEN^(2^(66 - logP))
  f128 gen = h_mpow(to_mont128(h_from_u64(7)), 4611686018427387897ull);
  root_tables(gen, c.P, c.logP, c.calls, c.gpoly_len, &t[c.c_omega], &t[c.c_S]);
  f128 invP = h_minv(to_mont128(h_from_u64(c.P)));
  f128 half_m = h_minv(to_mont128(h_from_u64(2)));
  t[c.c_misc + 0] = h_u4(invP);                     // (1/P) R
  t[c.c_misc + 1] = h_u4(from_mont128(half_m));     // 1/2 canonical
  t[c.c_misc + 2] = h_u4(make128(R1_128_LO, R1_128_HI));
  t[c.c_misc + 3] = h_u4(half_m);                   // (1/2) R
  if (c.algo == ALGO_FIXEDPOINT_L2) {
    const uint32_t n = c.bits;
    t[c.c_misc + 4] = h_u4(make128(n < 64 ? 1ull << n : 0, n >= 64 ? 1ull << (n - 64) : 0));  // 2^n
    const uint32_t e2 = 2 * n - 2;                                                           // 2^(2n-2) R^-1
    t[c.c_misc + 5] = h_u4(from_mont128(make128(e2 < 64 ? 1ull << e2 : 0, e2 >= 64 ? 1ull << (e2 - 64) : 0)));
    t[c.c_misc + 6] = h_u4(make128(1ull << (n - 2), 0));                                      // 2^(n-2)
    t[c.c_misc + 7] = h_u4(h_minv(to_mont128(h_from_u64(c.P1))));                            // (1/P1) R
    root_tables(gen, c.P1, c.logP1, c.calls1, c.gpoly1_len, &t[c.c_omega1], &t[c.c_S1]);
  }
  return t;
}

// ---------------------------------------------------------------------------- staging (per call, from the arena)

// staging element bytes: the multiproof Field64 kernels use 8-byte elements (outputs stay uint4)
static uint32_t stage_eb(const Cfg& c) { return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 8u : 16u; }
static uint64_t coef_elems(const Cfg& c) { return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? (uint64_t)c.np * c.nco : c.ncoef; }
static uint64_t part_bytes(const Cfg& c) {
  return c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 24ull * c.np * c.ngroups : 64ull * c.ngt;
}
// the output shares alias the measurement-share staging (Histogram: output = measurement share)
static bool outs_alias_meas(const Cfg& c) { return c.out_is_meas && c.algo != ALGO_COUNT; }
// The leader's FLP kernels read its explicit measurement share in place (Bufs::meas_rs) instead of a
// staged copy: every TurboSHAKE instance whose output is not the measurement share itself.
static bool leader_inplace(const Cfg& c) {
  return c.algo == ALGO_SUM || c.algo == ALGO_SUMVEC || c.algo == ALGO_FIXEDPOINT_L2;
}

namespace jxi {
size_t align256(size_t v) { return (v + 255) / 256 * 256; }
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
static uint32_t acc_nchunks(const jx_engine* e) {
  if (e->acc_chunks) return e->acc_chunks;
  const uint32_t want = (16384u + e->cfg.out_len - 1) / e->cfg.out_len;
  return want < 16u ? 16u : (want > 4096u ? 4096u : want);
}

// Lay the regions named by `fl` for `cap` reports out from `base` (nullptr: only size them).
static size_t stage_layout(jx_engine* e, uint64_t cap, uint32_t fl, uint8_t* base) {
  const Cfg& c = e->cfg;
  const uint64_t eb = stage_eb(c);
  size_t off = 0;
  auto take = [&](auto*& p, size_t bytes) {
    using T = std::remove_reference_t<decltype(p)>;
    if (base) p = reinterpret_cast<T>(base + off);
    off += align256(bytes ? bytes : 1);
  };
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
    take(e->d_ct, e->enc_ct_bytes);
    take(e->d_pt, e->enc_ct_bytes);
    take(e->d_status, cap);
  }
  if (fl & SG_ENCC) {
    take(e->d_ec_times, cap * 8);
    take(e->d_ec_eoff, (cap + 1) * 8);
    take(e->d_ec_poff, (cap + 1) * 8);
    take(e->d_ec_kidx, cap * 2);
  }
  return off;
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
size_t stage_bytes(const jx_engine* e, uint64_t cap, uint32_t flags) {
  return stage_layout(const_cast<jx_engine*>(e), (cap + 63) / 64 * 64, flags, nullptr);
}

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

int32_t stage_acquire(jx_engine* e, uint64_t n, uint32_t fl, Stage& st, bool may_wait) {
  st.release();
  const uint64_t cap = (n + 63) / 64 * 64;
  const size_t bytes = stage_layout(e, cap, fl, nullptr);
  hipError_t rc = arena_get(e->arena, bytes, e->stream, true, may_wait, st.slab);
  if (rc == hipErrorOutOfMemory) return nomem(e, "staging", bytes);
  HIPCHK(e, rc);
  st.e = e;
  stage_layout(e, cap, fl, (uint8_t*)st.slab.p);
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

// Per-call device scratch from the arena, handed back stream-ordered on the engine stream when it goes out of
// scope: no hipMalloc / hipFree / stream synchronize on a call path (hipFree waits for the device, and every
// engine's launches on it).
namespace {
struct Scratch {
  jx_engine* e = nullptr;
  Slab s;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    if (s.p) arena_put(e->arena, s, e->stream);
  }
  uint8_t* p() const { return (uint8_t*)s.p; }
};
}  // namespace

// may_wait: the caller holds no other staging (arena_get's rule)
static int32_t scratch_get(jx_engine* e, size_t bytes, Scratch& out, bool may_wait = false) {
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

static int32_t get_segment(jx_engine* e, uint32_t id, Segment** out) {
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
  const size_t o_outs = 0, o_ver = align256((size_t)cap * c.out_len * 16), o_msg = o_ver + align256(cap),
               o_non = o_msg + align256((size_t)cap * c.seed), bytes = o_non + align256(cap * 16);
  Batch b;
  b.n = n;
  b.leader = leader;
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
  uint8_t* m = (uint8_t*)b.slab.p;
  b.outs = (uint4*)(m + o_outs);
  b.verdicts = m + o_ver;
  b.msgs = m + o_msg;
  b.nonces = m + o_non;
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

static int32_t find_batch(jx_engine* e, uint64_t id, uint64_t n, const char* what, Batch** out) {
  auto it = e->batches.find(id);
  if (id == 0 || it == e->batches.end() || __atomic_load_n(&it->second.pending, __ATOMIC_ACQUIRE))
    return fail(e, JX_E_STATE, std::string(what) + ": batch id names no resident prepared batch (released or never made)");
  if (it->second.n != n)
    return fail(e, JX_E_INVALID, std::string(what) + ": report count differs from the batch's");
  *out = &it->second;
  return JX_OK;
}

static AccSrc batch_src(const Batch& b) { return AccSrc{b.n, b.outs, b.verdicts, b.nonces}; }

// ---------------------------------------------------------------------------- timing

static hipError_t stage_begin(jx_engine* e, hipEvent_t* ev) {
  if (!e->timing) return hipSuccess;
  hipError_t st = hipEventCreate(ev);
  if (st != hipSuccess) return st;
  return hipEventRecord(*ev, e->stream);
}
static hipError_t stage_end(jx_engine* e, int stage, hipEvent_t ev0) {
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

static bool use_inplace(const jx_engine* e) { return leader_inplace(e->cfg); }

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
  if (leader && use_inplace(e)) {
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
  const bool no_split = c.algo == ALGO_COUNT || c.algo == ALGO_SUMVEC_F64_MULTIPROOF;
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
static int32_t flush_acc(jx_engine* e) {
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
#define FLUSH_ACC(e)                 \
  do {                               \
    int32_t _fr = flush_acc(e);      \
    if (_fr) return _fr;             \
  } while (0)

// The device pointer table of a call's targets, [3][S]: aggs, counts, checksums. It owns the per-call scratch it
// lies in, which goes back to the arena (stream-ordered) with it.
struct PtrTable {
  Scratch mem;
  void** d() const { return (void**)mem.p(); }
};

// Upload the pointer table of `targets` into `tbl`. The pinned host copy is double-buffered and reused only once
// the upload that last read it has completed, so the host never waits for the call's own kernels.
static int32_t upload_targets(jx_engine* e, const std::vector<Segment>& targets, PtrTable& tbl) {
  const uint64_t S = targets.size();
  int32_t rc = scratch_get(e, 3 * S * sizeof(void*), tbl.mem);
  if (rc) return rc;
  const int k = e->ptrs_k;
  e->ptrs_k ^= 1;
  if (!e->ev_ptrs[k]) HIPCHK(e, hipEventCreateWithFlags(&e->ev_ptrs[k], hipEventDisableTiming));
  else HIPCHK(e, hipEventSynchronize(e->ev_ptrs[k]));
  if (e->h_ptrs_cap[k] < S) {
    if (e->h_ptrs[k]) (void)hipHostFree(e->h_ptrs[k]);
    e->h_ptrs[k] = nullptr;
    HIPCHK(e, hipHostMalloc((void**)&e->h_ptrs[k], 3 * S * sizeof(void*), hipHostMallocDefault));
    e->h_ptrs_cap[k] = S;
  }
  void** h = e->h_ptrs[k];
  for (uint64_t t = 0; t < S; t++) {
    h[t] = targets[t].agg;
    h[S + t] = targets[t].count;
    h[2 * S + t] = targets[t].checksum;
  }
  HIPCHK(e, hipMemcpyAsync(tbl.d(), h, 3 * S * sizeof(void*), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipEventRecord(e->ev_ptrs[k], e->stream));
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
  const size_t o_segx = 0, o_perm = align256((4 * SEG_MAX + 3) * sizeof(uint32_t)),
               o_items = o_perm + align256(n * sizeof(uint32_t)), o_spart = o_items + align256(wmax * sizeof(uint4)),
               wbytes = o_spart + align256(wmax * per_item);
  Scratch work;
  int32_t rc = scratch_get(e, wbytes, work);
  if (rc) return rc;
  // d_segx: cnt, off, cursor [SEG_MAX each], ioff [SEG_MAX + 1], nitems [2]
  uint32_t* const d_segx = (uint32_t*)(work.p() + o_segx);
  uint32_t* const d_perm = (uint32_t*)(work.p() + o_perm);
  uint4* const d_items = (uint4*)(work.p() + o_items);
  uint64_t* const d_spart = (uint64_t*)(work.p() + o_spart);
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
static int32_t segment_targets(jx_engine* e, const uint32_t* ids, uint64_t nids, std::vector<Segment>& out) {
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

// Accumulate src into targets[d_dense[r]] (d_dense nullable: all into targets[0]). One target takes the
// coalesced select/accumulate path; several go through their pointer table (tbl, or null: accumulate_many).
static int32_t accumulate_into(jx_engine* e, const AccSrc& src, const uint8_t* d_mask, const uint32_t* d_dense,
                               const std::vector<Segment>& targets, const PtrTable* tbl = nullptr) {
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

// ---------------------------------------------------------------------------- pipelines
// The launches of a fused call alternate over child engines (jx_fused_plan.h says how many and why).
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

// Staging for up to P pipelines: the first one may wait for the arena, the others take what is free
// now (so two calls never wait on each other holding half their pipelines). *got = pipelines staged.
static int32_t pipes_acquire(jx_engine* e, uint32_t P, uint64_t chunk, uint32_t flags, Stage* st, uint32_t* got) {
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
    q->enc_ct_bytes = e->enc_ct_bytes;
    int32_t rc = stage_acquire(q, chunk, flags, st[k], k == 0);
    if (rc) {
      if (k == 0) return rc;
      t_err.clear();  // run with the pipelines that fit (retried on the next call)
      break;
    }
    *got = k + 1;
  }
  return JX_OK;
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

// measurement staging for a helper prepare whose outputs go to a batch (Histogram writes its
// measurement share, which is its output share, straight into the batch)
static uint32_t helper_meas_flag(const Cfg& c) { return outs_alias_meas(c) ? 0u : SG_MEAS; }

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
    rc = pipes_acquire(e, plan.pipes, chunk, fused_stage_flags(call.host, true, call.sealed), pst, &P);
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
    rc = stage_acquire(e, chunk, fused_stage_flags(call.host, false, call.sealed), st);
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

// ---------------------------------------------------------------------------- C ABI

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
  for (int k = 0; k < 2; k++) {
    if (e->h_ptrs[k]) (void)hipHostFree(e->h_ptrs[k]);
    if (e->ev_ptrs[k]) (void)hipEventDestroy(e->ev_ptrs[k]);
  }
  if (e->h_acc) (void)hipHostFree(e->h_acc);
  if (e->ev_hacc) (void)hipEventDestroy(e->ev_hacc);
  if (e->h_enc) (void)hipHostFree(e->h_enc);
  if (e->ev_henc) (void)hipEventDestroy(e->ev_henc);
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

// Release batch `id` when a prepare call fails after creating it.
static int32_t drop_on_error(jx_engine* e, uint64_t id, int32_t rc) {
  if (rc) {
    auto it = e->batches.find(id);
    if (it != e->batches.end()) batch_free(e, it);
  }
  return rc;
}

static int32_t copy_out_shares(jx_engine* e, const uint4* outs, uint64_t n, uint8_t* dst) {
  const Cfg& c = e->cfg;
  Scratch tmp;
  int32_t rc = scratch_get(e, n * c.out_len * c.fb, tmp);
  if (rc) return rc;
  HIPCHK(e, launch_transpose_out(c, outs, n, tmp.p(), e->stream));
  HIPCHK(e, hipMemcpyAsync(dst, tmp.p(), n * c.out_len * c.fb, hipMemcpyDeviceToHost, e->stream));
  return JX_OK;
}

// What every call that takes sealed helper input shares checks before anything is queued (jx_helper_prep_encrypted_batch2
// and the two sealed fused calls), and the request as an EncJob. encs and payloads are only compared with null here:
// the device forms pass device pointers.
static int32_t enc_job_check(jx_engine* e, uint64_t n, const uint64_t* times, const uint8_t* task_id,
                             jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index, const uint8_t* encs,
                             const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                             uint32_t flags, EncJob& job) {
  if (nkeypairs > JX_ENC_MAX_KEYPAIRS || (nkeypairs && !keypairs) || (flags & ~JX_ENC_REQUIRE_TASKPROV))
    return fail(e, JX_E_INVALID, "encrypted prepare: at most JX_ENC_MAX_KEYPAIRS keypairs, flags JX_ENC_*");
  for (uint32_t k = 0; k < nkeypairs; k++)
    if (!keypairs[k] || hpke_device(keypairs[k]) != e->device)
      return fail(e, JX_E_INVALID, "encrypted prepare: every keypair must be an HPKE context on the engine's device");
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t k0 = key_index[2 * i], k1 = key_index[2 * i + 1];
    if ((k0 >= nkeypairs && k0 != JX_KEY_NONE && k0 != JX_KEY_MALFORMED) || (k1 >= nkeypairs && k1 != JX_KEY_NONE) ||
        payload_offsets[i + 1] < payload_offsets[i] || payload_offsets[i + 1] - payload_offsets[i] > 0xFFFFFFFFull)
      return fail(e, JX_E_INVALID, "encrypted prepare: key_index out of range or payload offsets decreasing");
  }
  if (n && payload_offsets[n] > payload_offsets[0] && !payloads) return JX_E_INVALID;
  for (uint64_t i = 0; enc_offsets && i < n; i++) {
    if (enc_offsets[i + 1] < enc_offsets[i])
      return fail(e, JX_E_INVALID, "encrypted prepare: encapsulated-key offsets decreasing");
    job.enc65 += enc_offsets[i + 1] - enc_offsets[i] == 65;
  }
  job.enc_offsets = enc_offsets;
  job.times = times;
  job.task_id = task_id;
  job.keypairs = keypairs;
  job.nkeys = nkeypairs;
  job.key_index = key_index;
  job.encs = encs;
  job.payloads = payloads;
  job.payload_offsets = payload_offsets;
  job.flags = flags;
  return JX_OK;
}

static int32_t helper_prep_batch_locked(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* ps,
                                        const uint8_t* his, const uint8_t* lps, uint8_t* out_msgs, uint8_t* out_verdicts,
                                        uint8_t* out_shares, Batch* B) {
  const Cfg& c = e->cfg;
  Stage st;
  int32_t rc = stage_acquire(e, n, SG_IN | SG_HIN | helper_meas_flag(c) | SG_PREP, st);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
  if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(e->d_ps, ps, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_his, his, n * c.his_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_lps, lps, n * c.lps_bytes, hipMemcpyHostToDevice, e->stream));
  rc = prep_core(e, n, B->nonces, e->d_ps, e->d_his, e->d_lps, B->verdicts, B->msgs, B->outs);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
  if (out_msgs && c.jr_len)
    HIPCHK(e, hipMemcpyAsync(out_msgs, B->msgs, n * c.seed, hipMemcpyDeviceToHost, e->stream));
  if (out_shares) {
    rc = copy_out_shares(e, B->outs, n, out_shares);
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return drain_timing(e);
}

// Coalesced prepares take jobs up to a quarter of a launch (larger ones fill the device by themselves) that fit
// one of the coalescer's lanes for their role (a leader's explicit input shares can be MBs per report); the
// rest take the direct path.
static bool coalescible(const jx_engine* e, uint64_t n, bool leader = false, bool encrypted = false,
                        uint64_t ct_bytes = 0) {
  return e->coalesce && n > 0 && n <= e->default_chunk / 4 && coalescer_accepts(e, leader, n, encrypted, ct_bytes);
}

int32_t jx_helper_prep_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                             const uint8_t* helper_input_shares, const uint8_t* leader_prep_shares,
                             uint8_t* out_prep_msgs, uint8_t* out_verdicts, uint8_t* out_output_shares,
                             uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !helper_input_shares || !leader_prep_shares || !out_verdicts))) return JX_E_INVALID;
  if (n && e->cfg.ps_bytes && !public_shares) return JX_E_INVALID;
  if (!out_output_shares && coalescible(e, n)) {
    t_err.clear();
    return coalesced_helper_prep(e, n, nonces, public_shares, helper_input_shares, leader_prep_shares, out_prep_msgs,
                                 out_verdicts, out_batch_id);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t id = 0;
  Batch* B = nullptr;
  int32_t rc = batch_new(e, n, false, &id, &B);
  if (rc) return rc;
  if (n) {
    rc = helper_prep_batch_locked(e, n, nonces, public_shares, helper_input_shares, leader_prep_shares, out_prep_msgs,
                                  out_verdicts, out_output_shares, B);
    if (rc) return drop_on_error(e, id, rc);
  }
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
}

int32_t jx_helper_prep_encrypted_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                       const uint8_t* public_shares, const uint8_t task_id[32],
                                       jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                       const uint8_t* encs, const uint8_t* payloads, const uint64_t* payload_offsets,
                                       uint32_t flags, const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs,
                                       uint8_t* out_verdicts, uint8_t* out_open_status, uint64_t* out_batch_id) {
  // the case of the call below in which every encapsulated key is 32 bytes
  return jx_helper_prep_encrypted_batch2(e, n, nonces, times, public_shares, task_id, keypairs, nkeypairs, key_index, encs,
                                         nullptr, payloads, payload_offsets, flags, leader_prep_shares, out_prep_msgs,
                                         out_verdicts, out_open_status, out_batch_id);
}

int32_t jx_helper_prep_encrypted_batch2(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                        const uint8_t* public_shares, const uint8_t task_id[32],
                                        jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                        const uint8_t* encs, const uint64_t* enc_offsets, const uint8_t* payloads,
                                        const uint64_t* payload_offsets, uint32_t flags,
                                        const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs, uint8_t* out_verdicts,
                                        uint8_t* out_open_status, uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !times || !task_id || !key_index || !encs || !payload_offsets || !leader_prep_shares ||
                   !out_verdicts)))
    return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !public_shares) return JX_E_INVALID;
  EncJob job;
  if (const int32_t rc = enc_job_check(e, n, times, task_id, keypairs, nkeypairs, key_index, encs, enc_offsets, payloads,
                                       payload_offsets, flags, job))
    return rc;
  const uint64_t ct = n ? job.ct_bytes(n) : 0;
  if (coalescible(e, n, false, true, ct)) {
    t_err.clear();
    return coalesced_helper_prep(e, n, nonces, public_shares, nullptr, leader_prep_shares, out_prep_msgs, out_verdicts,
                                 out_batch_id, &job, out_open_status);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t id = 0;
  Batch* B = nullptr;
  int32_t rc = batch_new(e, n, false, &id, &B);
  if (rc) return rc;
  if (n) {
    auto run = [&]() -> int32_t {
      // the job's rows in pageable host memory, uploaded with its inputs; they name their keypairs by their slots
      // of the device's key registry, where the keys have been since the contexts were created
      std::vector<EncRow> rows(n);
      bool suites = false;
      for (uint32_t k = 0; k < nkeypairs; k++) suites = suites || !hpke_default_suite(keypairs[k]);
      const HpkeKeyRow* reg = nullptr;
      uint32_t reg_cap = 0;
      hpke_registry(e->device, &reg, &reg_cap);
      // the 65-byte encapsulated keys follow the ciphertexts in the launch's ciphertext region
      std::vector<uint8_t> enc65(job.enc65 ? 65 * job.enc65 : 1);
      const uint64_t pb = job.payload_bytes(n), n65 = fill_enc_rows(job, n, rows.data(), 0, enc65.data());
      e->enc_ct_bytes = ct ? ct : 1;
      Stage st;
      int32_t r = stage_acquire(e, n, SG_IN | SG_HIN | SG_ENC | helper_meas_flag(c) | SG_PREP, st);
      if (r) return r;
      HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
      if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(e->d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
      HIPCHK(e, hipMemcpyAsync(e->d_lps, leader_prep_shares, n * c.lps_bytes, hipMemcpyHostToDevice, e->stream));
      HIPCHK(e, hipMemcpyAsync(e->d_encrows, rows.data(), n * sizeof(EncRow), hipMemcpyHostToDevice, e->stream));
      if (pb) HIPCHK(e, hipMemcpyAsync(e->d_ct, payloads + payload_offsets[0], pb, hipMemcpyHostToDevice, e->stream));
      if (n65) HIPCHK(e, hipMemcpyAsync(e->d_ct + pb, enc65.data(), 65 * n65, hipMemcpyHostToDevice, e->stream));
      HpkeRowsArgs ha{n, e->d_encrows, e->d_ct, e->d_pt, reg, reg ? reg_cap : 0, B->nonces, e->d_ps, c.ps_bytes,
                      e->d_his, c.his_bytes, e->d_status};
      HIPCHK(e, launch_hpke_rows(ha, suites, n65 != 0, e->stream));
      r = prep_core(e, n, B->nonces, e->d_ps, e->d_his, e->d_lps, B->verdicts, B->msgs, B->outs);
      if (r) return r;
      HIPCHK(e, launch_open_mask(e->d_status, B->verdicts, n, e->stream));
      HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
      if (out_prep_msgs && c.jr_len)
        HIPCHK(e, hipMemcpyAsync(out_prep_msgs, B->msgs, n * c.seed, hipMemcpyDeviceToHost, e->stream));
      if (out_open_status) HIPCHK(e, hipMemcpyAsync(out_open_status, e->d_status, n, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));  // the pageable rows and the caller's outputs
      return drain_timing(e);
    };
    rc = run();
    if (rc) return drop_on_error(e, id, rc);
  }
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
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

int32_t jx_engine_leader_sizes(const jx_engine* e, uint32_t* leader_input_share) {
  if (!e) return JX_E_INVALID;
  if (leader_input_share) *leader_input_share = e->cfg.lis_bytes;
  return JX_OK;
}

int32_t jx_leader_prep_init_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                  const uint8_t* leader_input_shares, uint8_t* out_prep_shares,
                                  uint8_t* out_verdicts, uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !leader_input_shares || !out_prep_shares || !out_verdicts))) return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !public_shares) return JX_E_INVALID;
  if (coalescible(e, n, true)) {
    t_err.clear();
    return coalesced_leader_init(e, n, nonces, public_shares, leader_input_shares, out_prep_shares, out_verdicts,
                                 out_batch_id);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t id = 0;
  Batch* B = nullptr;
  int32_t rc = batch_new(e, n, true, &id, &B);
  if (rc) return rc;
  if (n) {
    auto run = [&]() -> int32_t {
      Stage st;
      int32_t r = stage_acquire(e, n, SG_IN | SG_LEAD | SG_PREP | (use_inplace(e) ? 0u : SG_MEAS), st);
      if (r) return r;
      HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
      if (c.ps_bytes)
        HIPCHK(e, hipMemcpyAsync(e->d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
      if (e->lis_stride == c.lis_bytes)
        HIPCHK(e, hipMemcpyAsync(e->d_lis, leader_input_shares, n * c.lis_bytes, hipMemcpyHostToDevice, e->stream));
      else  // padded rows (aligned in-place reads of the measurement share)
        HIPCHK(e, hipMemcpy2DAsync(e->d_lis, e->lis_stride, leader_input_shares, c.lis_bytes, c.lis_bytes, n,
                                   hipMemcpyHostToDevice, e->stream));
      r = prep_core(e, n, B->nonces, e->d_ps, nullptr, nullptr, B->verdicts, B->msgs, B->outs, e->d_lis, e->d_lps_out,
                    e->lis_stride);
      if (r) return r;
      HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemcpyAsync(out_prep_shares, e->d_lps_out, n * c.lps_bytes, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
      return drain_timing(e);
    };
    rc = run();
    if (rc) return drop_on_error(e, id, rc);
  }
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
}

int32_t jx_leader_prep_init_device_ex(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                      const void* d_leader_input_shares, uint64_t lis_stride, void* d_out_prep_shares,
                                      void* d_out_verdicts, uint64_t* out_batch_id) {
  if (!out_batch_id) return JX_E_INVALID;
  *out_batch_id = 0;
  if (!e || (n && (!d_nonces || !d_leader_input_shares || !d_out_prep_shares))) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !d_public_shares) return JX_E_INVALID;
  if (lis_stride == 0) lis_stride = c.lis_bytes;
  if (lis_stride < c.lis_bytes || (lis_stride & 15u))
    return fail(e, JX_E_INVALID, "leader init: the row stride must be >= the leader input share and a multiple of 16");
  // the in-place FLP kernels read the measurement share in 16-byte vectors (header contract)
  if (n && use_inplace(e) && (reinterpret_cast<uintptr_t>(d_leader_input_shares) & 15u))
    return fail(e, JX_E_INVALID, "leader init: d_leader_input_shares must be 16-byte aligned");
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t id = 0;
  Batch* B = nullptr;
  int32_t rc = batch_new(e, n, true, &id, &B);
  if (rc) return rc;
  if (n) {
    auto run = [&]() -> int32_t {
      Stage st;
      int32_t r = stage_acquire(e, n, SG_PREP | (use_inplace(e) ? 0u : SG_MEAS), st);
      if (r) return r;
      HIPCHK(e, hipMemcpyAsync(B->nonces, d_nonces, n * 16, hipMemcpyDeviceToDevice, e->stream));
      r = prep_core(e, n, B->nonces, (const uint8_t*)d_public_shares, nullptr, nullptr, B->verdicts, B->msgs, B->outs,
                    (const uint8_t*)d_leader_input_shares, (uint8_t*)d_out_prep_shares, lis_stride);
      if (r) return r;
      if (d_out_verdicts) HIPCHK(e, hipMemcpyAsync(d_out_verdicts, B->verdicts, n, hipMemcpyDeviceToDevice, e->stream));
      return JX_OK;
    };
    rc = run();
    if (rc) return drop_on_error(e, id, rc);
  }
  *out_batch_id = id;
  return JX_OK;
}

int32_t jx_leader_prep_init_device(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                   const void* d_leader_input_shares, void* d_out_prep_shares, void* d_out_verdicts,
                                   uint64_t* out_batch_id) {
  return jx_leader_prep_init_device_ex(e, n, d_nonces, d_public_shares, d_leader_input_shares, 0, d_out_prep_shares,
                                       d_out_verdicts, out_batch_id);
}

// ---- the leader's upload path (kernels: jx_hpke_long.hip)

namespace {
// What both upload calls check before anything is queued, and the reports' rows: keypair indices become slots of
// the device's key registry, as fill_enc_rows does for the helper's rows; ciphertext and encapsulated-key offsets
// are the caller's own.
int32_t upload_rows(jx_engine* e, uint64_t n, const uint64_t* times, jx_hpke* const* keypairs, uint32_t nkeypairs,
                    const uint8_t* key_index, const uint64_t* enc_offsets, const uint64_t* payload_offsets,
                    uint64_t* lis_stride, std::vector<UpRow>& rows, bool* any_p256) {
  const Cfg& c = e->cfg;
  if (nkeypairs > JX_ENC_MAX_KEYPAIRS || (nkeypairs && !keypairs))
    return fail(e, JX_E_INVALID, "upload open: at most JX_ENC_MAX_KEYPAIRS keypairs");
  uint32_t klen[JX_ENC_MAX_KEYPAIRS];
  uint16_t slot[JX_ENC_MAX_KEYPAIRS];
  *any_p256 = false;
  for (uint32_t k = 0; k < nkeypairs; k++) {
    if (!keypairs[k] || hpke_device(keypairs[k]) != e->device)
      return fail(e, JX_E_INVALID, "upload open: every keypair must be an HPKE context on the engine's device");
    klen[k] = hpke_enc_len(keypairs[k]);
    slot[k] = hpke_slot(keypairs[k]);
    *any_p256 = *any_p256 || klen[k] == 65;
  }
  if (*lis_stride == 0) *lis_stride = c.lis_bytes;
  if (*lis_stride < c.lis_bytes || (*lis_stride != c.lis_bytes && (*lis_stride & 15u)))
    return fail(e, JX_E_INVALID, "upload open: the row stride must be 0, or >= the leader input share and a multiple of 16");
  rows.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t k0 = key_index[2 * i], k1 = key_index[2 * i + 1];
    if ((k0 >= nkeypairs && k0 != JX_KEY_NONE && k0 != JX_KEY_MALFORMED) || (k1 >= nkeypairs && k1 != JX_KEY_NONE) ||
        payload_offsets[i + 1] < payload_offsets[i] || payload_offsets[i + 1] - payload_offsets[i] > 0xFFFFFFFFull ||
        (enc_offsets && enc_offsets[i + 1] < enc_offsets[i]))
      return fail(e, JX_E_INVALID, "upload open: key_index out of range, offsets decreasing or a payload of 2^32 bytes or more");
    UpRow& w = rows[i];
    memset(&w, 0, sizeof w);
    w.ct_off = payload_offsets[i];
    w.ct_len = (uint32_t)(payload_offsets[i + 1] - payload_offsets[i]);
    w.enc_off = enc_offsets ? enc_offsets[i] : 32 * i;
    const uint64_t len = enc_offsets ? enc_offsets[i + 1] - enc_offsets[i] : 32;
    w.enc_len = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    // a trial can only succeed when the encapsulated key has the length of the keypair's KEM; a key that fits
    // neither keypair fails the report without an open
    const bool fits = (k0 < nkeypairs && klen[k0] == len) || (k1 < nkeypairs && klen[k1] == len);
    if (k0 == JX_KEY_MALFORMED || (k0 < nkeypairs && !fits)) w.flags |= UP_ROW_MALFORMED;
    w.key0 = k0 < nkeypairs ? slot[k0] : (k0 == JX_KEY_MALFORMED ? (uint16_t)0 : KEY_SLOT_NONE);
    w.key1 = k1 < nkeypairs ? slot[k1] : KEY_SLOT_NONE;
    for (int b = 0; b < 8; b++) w.time_be[b] = (uint8_t)(times[i] >> (56 - 8 * b));
  }
  return JX_OK;
}

// The launch, with everything on the device but the rows: d_rows / d_ctx / d_pts are scratch of n x sizeof(UpRow),
// n x UPLOAD_CTX_BYTES and the payloads' span. cts, pts and ext are indexed by the rows' absolute ct_off.
int32_t upload_launch(jx_engine* e, uint64_t n, const std::vector<UpRow>& rows, bool any_p256, const uint8_t task_id[32],
                      const uint8_t* d_ids, const uint8_t* d_ps, const uint8_t* d_encs, const uint8_t* cts, uint8_t* pts,
                      UpRow* d_rows, void* d_ctx, uint8_t* d_out_rows, uint64_t lis_stride, uint8_t* ext,
                      uint32_t* d_ext_len, uint8_t* d_status) {
  const Cfg& c = e->cfg;
  HIPCHK(e, hipMemcpyAsync(d_rows, rows.data(), n * sizeof(UpRow), hipMemcpyHostToDevice, e->stream));
  UploadArgs a{};
  a.n = n;
  a.rows = d_rows;
  uint32_t cap = 0;
  hpke_registry(e->device, &a.keys, &cap);
  a.nkeys = a.keys ? cap : 0;
  a.ps_bytes = c.ps_bytes;
  a.ids = d_ids;
  a.ps = d_ps;
  memcpy(a.task_id, task_id, 32);
  a.encs = d_encs;
  a.cts = cts;
  a.pts = pts;
  a.ctx = d_ctx;
  a.out_rows = d_out_rows;
  a.lis_stride = lis_stride;
  a.lis_bytes = c.lis_bytes;
  a.elem_bytes = c.lis_bytes - (c.jr_len ? c.seed : 0);
  a.fb = c.fb;
  a.out_ext = ext;
  a.out_ext_len = d_ext_len;
  a.out_status = d_status;
  HIPCHK(e, launch_upload_open(a, any_p256, e->stream));
  return JX_OK;
}
}  // namespace

int32_t jx_leader_upload_open_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                     const void* d_public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                     uint32_t nkeypairs, const uint8_t* key_index, const void* d_encs,
                                     const uint64_t* enc_offsets, const void* d_payloads, const uint64_t* payload_offsets,
                                     void* d_out_rows, uint64_t lis_stride, void* d_out_extensions, void* d_out_ext_len,
                                     void* d_out_status) {
  if (!e || (n && (!d_report_ids || !times || !task_id || !key_index || !d_encs || !payload_offsets || !d_out_rows ||
                   !d_out_extensions || !d_out_ext_len || !d_out_status)))
    return JX_E_INVALID;
  if (n == 0) return JX_OK;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !d_public_shares) return JX_E_INVALID;
  if (reinterpret_cast<uintptr_t>(d_out_rows) & 15u)
    return fail(e, JX_E_INVALID, "upload open: d_out_rows must be 16-byte aligned");
  std::vector<UpRow> rows;
  bool any_p256 = false;
  if (const int32_t rc = upload_rows(e, n, times, keypairs, nkeypairs, key_index, enc_offsets, payload_offsets,
                                     &lis_stride, rows, &any_p256))
    return rc;
  const uint64_t c0 = payload_offsets[0], span = payload_offsets[n] - c0;
  if (span && !d_payloads) return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  const size_t o_rows = 0, o_ctx = o_rows + align256(n * sizeof(UpRow)), o_pt = o_ctx + align256(n * UPLOAD_CTX_BYTES),
               bytes = o_pt + align256(span ? span : 1);
  Slab slab;
  HIPCHK(e, arena_get(e->arena, bytes, e->stream, true, true, slab));
  uint8_t* base = (uint8_t*)slab.p;
  int32_t rc = upload_launch(e, n, rows, any_p256, task_id, (const uint8_t*)d_report_ids, (const uint8_t*)d_public_shares,
                             (const uint8_t*)d_encs, (const uint8_t*)d_payloads, base + o_pt - c0, (UpRow*)(base + o_rows),
                             base + o_ctx, (uint8_t*)d_out_rows, lis_stride, (uint8_t*)d_out_extensions,
                             (uint32_t*)d_out_ext_len, (uint8_t*)d_out_status);
  // the rows leave pageable host memory before the call returns; the launch itself stays queued
  if (rc == JX_OK) {
    hipEvent_t ev = nullptr;
    hipError_t st = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (st == hipSuccess) st = hipEventRecord(ev, e->stream);
    arena_put(e->arena, slab, e->stream);
    if (st == hipSuccess) st = hipEventSynchronize(ev);
    if (ev) (void)hipEventDestroy(ev);
    HIPCHK(e, st);
    return JX_OK;
  }
  arena_put(e->arena, slab, e->stream);
  return rc;
}

int32_t jx_leader_upload_open_batch(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                                    const uint8_t* public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                    uint32_t nkeypairs, const uint8_t* key_index, const uint8_t* encs,
                                    const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                                    uint8_t* out_leader_input_shares, uint8_t* out_extensions, uint32_t* out_ext_len,
                                    uint8_t* out_status) {
  if (!e || (n && (!report_ids || !times || !task_id || !key_index || !encs || !payload_offsets ||
                   !out_leader_input_shares || !out_extensions || !out_ext_len || !out_status)))
    return JX_E_INVALID;
  if (n == 0) return JX_OK;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !public_shares) return JX_E_INVALID;
  std::vector<UpRow> rows;
  bool any_p256 = false;
  uint64_t lis_stride = (c.lis_bytes + 15u) & ~15ull;  // the device rows; the caller's are LIS apart
  if (const int32_t rc = upload_rows(e, n, times, keypairs, nkeypairs, key_index, enc_offsets, payload_offsets,
                                     &lis_stride, rows, &any_p256))
    return rc;
  const uint64_t c0 = payload_offsets[0], span = payload_offsets[n] - c0;
  if (span && !payloads) return JX_E_INVALID;
  const uint64_t e0 = enc_offsets ? enc_offsets[0] : 0, enc_bytes = (enc_offsets ? enc_offsets[n] : 32 * n) - e0;
  HIPCHK(e, hipSetDevice(e->device));
  const size_t sp = align256(span ? span : 1);
  const size_t o_rows = 0, o_ctx = o_rows + align256(n * sizeof(UpRow)), o_pt = o_ctx + align256(n * UPLOAD_CTX_BYTES),
               o_ct = o_pt + sp, o_ext = o_ct + sp, o_enc = o_ext + sp, o_ids = o_enc + align256(enc_bytes ? enc_bytes : 1),
               o_ps = o_ids + align256(n * 16), o_out = o_ps + align256(c.ps_bytes ? n * c.ps_bytes : 1),
               o_len = o_out + align256(n * lis_stride), o_st = o_len + align256(n * 4), bytes = o_st + align256(n);
  Slab slab;
  HIPCHK(e, arena_get(e->arena, bytes, e->stream, true, true, slab));
  uint8_t* base = (uint8_t*)slab.p;
  auto run = [&]() -> int32_t {
    HIPCHK(e, hipMemcpyAsync(base + o_ids, report_ids, n * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(base + o_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    if (enc_bytes) HIPCHK(e, hipMemcpyAsync(base + o_enc, encs + e0, enc_bytes, hipMemcpyHostToDevice, e->stream));
    if (span) HIPCHK(e, hipMemcpyAsync(base + o_ct, payloads + c0, span, hipMemcpyHostToDevice, e->stream));
    int32_t r = upload_launch(e, n, rows, any_p256, task_id, base + o_ids, base + o_ps, base + o_enc - e0, base + o_ct - c0,
                              base + o_pt - c0, (UpRow*)(base + o_rows), base + o_ctx, base + o_out, lis_stride,
                              base + o_ext - c0, (uint32_t*)(base + o_len), base + o_st);
    if (r) return r;
    HIPCHK(e, hipMemcpy2DAsync(out_leader_input_shares, c.lis_bytes, base + o_out, lis_stride, c.lis_bytes, n,
                               hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_ext_len, base + o_len, n * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_status, base + o_st, n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // the extension bytes: each report's own, where its payload was (most batches have none)
    bool any = false;
    for (uint64_t i = 0; i < n; i++) {
      if (!out_ext_len[i]) continue;
      any = true;
      HIPCHK(e, hipMemcpyAsync(out_extensions + payload_offsets[i], base + o_ext + (payload_offsets[i] - c0), out_ext_len[i],
                               hipMemcpyDeviceToHost, e->stream));
    }
    if (any) HIPCHK(e, hipStreamSynchronize(e->stream));
    return JX_OK;
  };
  const int32_t rc = run();
  arena_put(e->arena, slab, e->stream);
  return rc;
}

static int32_t leader_batch(jx_engine* e, uint64_t batch_id, uint64_t n, Batch** B) {
  int32_t rc = find_batch(e, batch_id, n, "leader finish", B);
  if (rc) return rc;
  if (!(*B)->leader) return fail(e, JX_E_STATE, "leader finish: the batch is a helper batch");
  if ((*B)->finished) return fail(e, JX_E_STATE, "leader finish: the batch was already finished");
  return JX_OK;
}

int32_t jx_leader_prep_finish_batch(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* prep_msgs,
                                    uint8_t* out_verdicts, uint8_t* out_output_shares) {
  if (!e || (n && !out_verdicts)) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  Batch* B = nullptr;
  int32_t rc = leader_batch(e, batch_id, n, &B);
  if (rc) return rc;
  if (n && c.jr_len && !prep_msgs) return JX_E_INVALID;
  if (n == 0) {
    B->finished = true;
    return JX_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  Stage st;
  if (c.jr_len) {
    rc = stage_acquire(e, n, SG_LMSG, st);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_in_msgs, prep_msgs, n * c.seed, hipMemcpyHostToDevice, e->stream));
    Bufs b{};
    b.n = n;
    b.verdicts = B->verdicts;
    b.msgs = B->msgs;
    HIPCHK(e, launch_leader_finish(c, b, e->d_in_msgs, nullptr, e->stream));
  }
  // finished once prepare_next is queued: a failure above leaves the batch finishable (or releasable)
  B->finished = true;
  HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
  if (out_output_shares) {
    rc = copy_out_shares(e, B->outs, n, out_output_shares);
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

int32_t jx_leader_prep_finish_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_prep_msgs,
                                     const void* d_peer_verdicts, void* d_out_verdicts) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  Batch* B = nullptr;
  int32_t rc = leader_batch(e, batch_id, n, &B);
  if (rc) return rc;
  if (n && c.jr_len && !d_prep_msgs) return JX_E_INVALID;
  if (n == 0) {
    B->finished = true;
    return JX_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  Bufs b{};
  b.n = n;
  b.verdicts = B->verdicts;
  b.msgs = B->msgs;
  HIPCHK(e, launch_leader_finish(c, b, (const uint8_t*)d_prep_msgs, (const uint8_t*)d_peer_verdicts, e->stream));
  B->finished = true;
  if (d_out_verdicts) HIPCHK(e, hipMemcpyAsync(d_out_verdicts, B->verdicts, n, hipMemcpyDeviceToDevice, e->stream));
  return JX_OK;
}

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
  if (!e->ev_hacc) HIPCHK(e, hipEventCreateWithFlags(&e->ev_hacc, hipEventDisableTiming));
  else HIPCHK(e, hipEventSynchronize(e->ev_hacc));
  if (e->h_acc_cap < total) {
    if (e->h_acc) (void)hipHostFree(e->h_acc);
    e->h_acc = nullptr;
    e->h_acc_cap = 0;
    HIPCHK(e, hipHostMalloc((void**)&e->h_acc, total, hipHostMallocDefault));
    e->h_acc_cap = total;
  }
  size_t off = 0;
  for (size_t i = 0; i < src.size(); i++) {
    memcpy(e->h_acc + off, src[i].first, src[i].second);
    HIPCHK(e, hipMemcpyAsync(dst[i], e->h_acc + off, src[i].second, hipMemcpyHostToDevice, e->stream));
    off += align256(src[i].second);
  }
  HIPCHK(e, hipEventRecord(e->ev_hacc, e->stream));
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

// Whether the engine's algorithm pipelines its fused calls at all (jx_fused_plan.h).
static bool fused_pipelines(const Cfg& c) { return c.algo != ALGO_COUNT && c.algo != ALGO_SUMVEC_F64_MULTIPROOF; }

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
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, fused_pipelines(c), false, true);
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
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, fused_pipelines(c), many, false);
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

// Fill `sc` from its checked job and return the lanes' enc_ct_bytes: the largest ciphertext region any launch of
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
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, fused_pipelines(c), false, true);
  e->enc_ct_bytes = sealed_setup(e, n, plan, true, sc);
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
      fused_plan(n, e->default_chunk, e->round_reports, e->npipes, fused_pipelines(c), many, false);
  e->enc_ct_bytes = sealed_setup(e, n, plan, false, sc);
  // The compact arrays leave the caller's memory here, into pinned memory that the launches' uploads read after
  // the call has returned: times | payload offsets | encapsulated-key offsets (when given) | key-index pairs.
  const size_t o_tm = 0, o_po = o_tm + n * 8, o_eo = o_po + (n + 1) * 8, o_ki = o_eo + (enc_offsets ? (n + 1) * 8 : 0),
               hbytes = o_ki + 2 * n;
  if (!e->ev_henc) HIPCHK(e, hipEventCreateWithFlags(&e->ev_henc, hipEventDisableTiming));
  else HIPCHK(e, hipEventSynchronize(e->ev_henc));
  if (e->h_enc_cap < hbytes) {
    if (e->h_enc) (void)hipHostFree(e->h_enc);
    e->h_enc = nullptr;
    e->h_enc_cap = 0;
    HIPCHK(e, hipHostMalloc((void**)&e->h_enc, hbytes, hipHostMallocDefault));
    e->h_enc_cap = hbytes;
  }
  uint8_t* const hb = e->h_enc;
  memcpy(hb + o_tm, times, n * 8);
  memcpy(hb + o_po, payload_offsets, (n + 1) * 8);
  if (enc_offsets) memcpy(hb + o_eo, enc_offsets, (n + 1) * 8);
  memcpy(hb + o_ki, key_index, 2 * n);
  const uint64_t* const po = (const uint64_t*)(hb + o_po);
  FusedCall call{};
  call.sealed = true;
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
  (void)hipEventRecord(e->ev_henc, e->stream);  // behind the join: every lane's uploads have read the pinned copy
  return rc;
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

// ---- the client: Prio3.shard (kernels: jx_shard.hip)

static_assert(JX_SHARD_MAX_P == jx::SHARD_MAX_P, "the header's cap is the prove kernel's");

namespace {
// Scratch of one launch at most (and at least 64 reports). The two XOF kernels run one report per lane and a
// launch's waves all run the same length, so a launch is as fast with one wave per SIMD as with one per device:
// the budget is what keeps the headline instance's 16,384-report call (133 KB of scratch per report) in one launch.
constexpr uint64_t SHARD_SCRATCH_BUDGET = 4ull << 30;

// the instance as the shard kernels take it; refuses what they do not cover
int32_t shard_args(jx_engine* e, ShardArgs& a) {
  const Cfg& c = e->cfg;
  if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF || c.algo == ALGO_FIXEDPOINT_L2)
    return fail(e, JX_E_UNSUPPORTED,
                "shard: Prio3SumVecField64MultiproofHmacSha256Aes128 (algo id 4) and Prio3FixedPointBoundedL2VecSum "
                "(algo id 5) are not sharded on the device (they need a second XOF and the PolyEval gadget)");
  if (c.P > JX_SHARD_MAX_P)
    return fail(e, JX_E_UNSUPPORTED,
                "shard: the gadget's transform size P = " + std::to_string(c.P) + " exceeds JX_SHARD_MAX_P = " +
                    std::to_string(JX_SHARD_MAX_P));
  memset(&a, 0, sizeof a);
  a.algo = c.algo;
  a.bits = c.bits;
  a.length = c.length;
  a.chunk = c.chunk;
  a.meas_len = c.meas_len;
  a.calls = c.calls;
  a.P = c.P;
  a.logP = c.logP;
  a.gpoly_len = c.gpoly_len;
  a.proof_len = c.proof_len;
  a.arity = c.proof_len - c.gpoly_len;
  a.dst_id = c.dst_id;
  a.ps_bytes = c.ps_bytes;
  a.his_bytes = c.his_bytes;
  a.lis_bytes = c.lis_bytes;
  a.jr = c.jr_len > 0;
  a.rand_bytes = c.seed * (3 + (a.jr ? 2 : 0));
  a.mstride = c.algo == ALGO_SUMVEC ? c.length : 1;
  a.waves = shard_waves(c.algo, c.P, c.chunk);
  return JX_OK;
}

// the transform table of the engine's P, made on the host once per engine
int32_t shard_table(jx_engine* e) {
  const Cfg& c = e->cfg;
  if (e->d_shard_tab || c.algo == ALGO_COUNT) return JX_OK;
  std::vector<f128> t(ntt_table_len(c.P));
  ntt_build_table(c.logP, t.data());
  static_assert(sizeof(f128) == sizeof(uint4), "table entries are 16 bytes");
  uint4* d = nullptr;
  HIPCHK(e, hipMalloc((void**)&d, t.size() * sizeof(f128)));
  // the vector is pageable: the copy has left it when this returns
  const hipError_t st = hipMemcpy(d, t.data(), t.size() * sizeof(f128), hipMemcpyHostToDevice);
  if (st != hipSuccess) {
    (void)hipFree(d);
    HIPCHK(e, st);
  }
  e->d_shard_tab = d;
  return JX_OK;
}

uint64_t shard_chunk(const jx_engine* e, const ShardArgs& a, uint64_t n, uint64_t extra_per_report) {
  uint64_t chunk = SHARD_SCRATCH_BUDGET / (shard_scratch_bytes(a) + extra_per_report);
  if (chunk < 64) chunk = 64;
  if (e->shard_chunk) chunk = e->shard_chunk;  // debug option 10
  return chunk < n ? chunk : n;
}
size_t shard_scratch_total(const ShardArgs& a, uint64_t m) {
  return align256(m) + align256(16 * m * a.meas_len) + align256(16 * m * a.arity) + align256(16 * m * a.P) +
         align256(16 * m);
}
// carve the scratch of a launch of m reports at `base`
void shard_carve(ShardArgs& a, uint8_t* base, uint64_t m) {
  a.status = base;
  base += align256(m);
  a.hmeas = (uint4*)base;
  base += align256(16 * m * a.meas_len);
  a.prand = (uint4*)base;
  base += align256(16 * m * a.arity);
  a.cpow = (uint4*)base;
  base += align256(16 * m * a.P);
  a.rjr = (uint4*)base;
}

// the launches of n reports, `chunk` at a time, over one scratch region
int32_t shard_launches(jx_engine* e, ShardArgs a, uint64_t n, uint64_t chunk, uint8_t* scratch, uint8_t* d_out_status) {
  a.tab = e->d_shard_tab;
  shard_carve(a, scratch, chunk);
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = n - off < chunk ? n - off : chunk;
    a.n = m;
    HIPCHK(e, launch_shard(a, e->stream));
    if (d_out_status) HIPCHK(e, hipMemcpyAsync(d_out_status + off, a.status, m, hipMemcpyDeviceToDevice, e->stream));
    a.meas += m * a.mstride;
    a.nonces += m * 16;
    a.rands += m * a.rand_bytes;
    if (a.ps) a.ps += m * a.ps_bytes;
    a.lis += m * a.lis_stride;
    a.his += m * a.his_bytes;
  }
  return JX_OK;
}
}  // namespace

int32_t jx_client_rand_bytes(const jx_engine* e, uint32_t* bytes) {
  if (!e) return JX_E_INVALID;
  if (bytes) *bytes = e->cfg.seed * (3 + (e->cfg.jr_len ? 2 : 0));
  return JX_OK;
}

int32_t jx_client_shard_device(jx_engine* e, uint64_t n, const void* d_measurements, const void* d_nonces,
                               const void* d_rands, void* d_out_public_shares, void* d_out_leader_input_shares,
                               uint64_t lis_stride, void* d_out_helper_input_shares, void* d_out_status) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  ShardArgs a;
  if (const int32_t rc = shard_args(e, a)) return rc;
  if (n == 0) return JX_OK;
  if (!d_measurements || !d_nonces || !d_rands || !d_out_leader_input_shares || !d_out_helper_input_shares ||
      (a.ps_bytes && !d_out_public_shares))
    return JX_E_INVALID;
  if (lis_stride == 0) lis_stride = a.lis_bytes;
  if (lis_stride < a.lis_bytes || (lis_stride != a.lis_bytes && (lis_stride & 15u)))
    return fail(e, JX_E_INVALID, "shard: the row stride must be 0, or >= the leader input share and a multiple of 16");
  if ((reinterpret_cast<uintptr_t>(d_out_leader_input_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_measurements) & 7u) ||
      ((reinterpret_cast<uintptr_t>(d_nonces) | reinterpret_cast<uintptr_t>(d_rands) |
        reinterpret_cast<uintptr_t>(d_out_public_shares) | reinterpret_cast<uintptr_t>(d_out_helper_input_shares)) & 3u))
    return fail(e, JX_E_INVALID,
                "shard: the leader input share rows must be 16-byte aligned, the measurements 8-byte, the rest 4-byte");
  HIPCHK(e, hipSetDevice(e->device));
  if (const int32_t rc = shard_table(e)) return rc;
  a.lis_stride = lis_stride;
  a.meas = (const uint64_t*)d_measurements;
  a.nonces = (const uint8_t*)d_nonces;
  a.rands = (const uint8_t*)d_rands;
  a.ps = (uint8_t*)d_out_public_shares;
  a.lis = (uint8_t*)d_out_leader_input_shares;
  a.his = (uint8_t*)d_out_helper_input_shares;
  const uint64_t chunk = shard_chunk(e, a, n, 0);
  Slab slab;
  HIPCHK(e, arena_get(e->arena, shard_scratch_total(a, chunk), e->stream, true, true, slab));
  const int32_t rc = shard_launches(e, a, n, chunk, (uint8_t*)slab.p, (uint8_t*)d_out_status);
  arena_put(e->arena, slab, e->stream);
  return rc;
}

int32_t jx_client_shard_batch(jx_engine* e, uint64_t n, const uint64_t* measurements, const uint8_t* nonces,
                              const uint8_t* rands, uint8_t* out_public_shares, uint8_t* out_leader_input_shares,
                              uint8_t* out_helper_input_shares, uint8_t* out_status) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  ShardArgs a;
  if (const int32_t rc = shard_args(e, a)) return rc;
  if (n == 0) return JX_OK;
  if (!measurements || !nonces || !rands || !out_leader_input_shares || !out_helper_input_shares ||
      (a.ps_bytes && !out_public_shares))
    return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  if (const int32_t rc = shard_table(e)) return rc;
  a.lis_stride = a.lis_bytes;  // a multiple of 16 for every Field128 instance; Prio3Count's 48 too
  const uint64_t mrow = 8ull * a.mstride;
  const uint64_t io = mrow + 16 + a.rand_bytes + a.ps_bytes + a.lis_stride + a.his_bytes + 6 * 256;
  const uint64_t chunk = shard_chunk(e, a, n, io);
  const size_t o_meas = 0, o_non = o_meas + align256(chunk * mrow), o_rand = o_non + align256(chunk * 16),
               o_ps = o_rand + align256(chunk * a.rand_bytes), o_lis = o_ps + align256(chunk * a.ps_bytes + 1),
               o_his = o_lis + align256(chunk * a.lis_stride), o_scr = o_his + align256(chunk * a.his_bytes);
  Slab slab;
  HIPCHK(e, arena_get(e->arena, o_scr + shard_scratch_total(a, chunk), e->stream, true, true, slab));
  uint8_t* base = (uint8_t*)slab.p;
  auto run = [&]() -> int32_t {
    for (uint64_t off = 0; off < n; off += chunk) {
      const uint64_t m = n - off < chunk ? n - off : chunk;
      HIPCHK(e, hipMemcpyAsync(base + o_meas, measurements + off * a.mstride, m * mrow, hipMemcpyHostToDevice, e->stream));
      HIPCHK(e, hipMemcpyAsync(base + o_non, nonces + off * 16, m * 16, hipMemcpyHostToDevice, e->stream));
      HIPCHK(e, hipMemcpyAsync(base + o_rand, rands + off * a.rand_bytes, m * a.rand_bytes, hipMemcpyHostToDevice, e->stream));
      ShardArgs b = a;
      b.meas = (const uint64_t*)(base + o_meas);
      b.nonces = base + o_non;
      b.rands = base + o_rand;
      b.ps = base + o_ps;
      b.lis = base + o_lis;
      b.his = base + o_his;
      if (const int32_t rc = shard_launches(e, b, m, chunk, base + o_scr, nullptr)) return rc;
      if (a.ps_bytes)
        HIPCHK(e, hipMemcpyAsync(out_public_shares + off * a.ps_bytes, base + o_ps, m * a.ps_bytes, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemcpyAsync(out_leader_input_shares + off * a.lis_bytes, base + o_lis, m * a.lis_bytes, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemcpyAsync(out_helper_input_shares + off * a.his_bytes, base + o_his, m * a.his_bytes, hipMemcpyDeviceToHost, e->stream));
      if (out_status)  // the launch's status bytes are the first region of its scratch
        HIPCHK(e, hipMemcpyAsync(out_status + off, base + o_scr, m, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    return JX_OK;
  };
  const int32_t rc = run();
  arena_put(e->arena, slab, e->stream);
  return rc;
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
