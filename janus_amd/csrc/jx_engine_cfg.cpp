// jx_engine_cfg.cpp — a Prio3 instance as the kernels take it: parameter validation (make_cfg) and the constant
// tables an engine uploads once (make_consts), with the host field arithmetic they need.
#include <cstring>
#include <string>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_field.h"
#include "jx_sha_aes.h"

using namespace jx;
using namespace jxi;

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

int32_t jxi::make_cfg(const jx_prio3_params* p, const uint8_t* vk, uint32_t vk_len, Cfg& c, std::string& why) {
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

std::vector<uint4> jxi::make_consts(const Cfg& c) {
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

