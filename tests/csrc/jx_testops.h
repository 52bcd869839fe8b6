// What each arithmetic test operation computes, once, for both builds of the device arithmetic headers
// (janus_amd/csrc/jx_*.h): the g++ host libraries (tests/csrc/hosttest*.cpp) and the gfx950 harness
// (tests/csrc/devtest.hip). Thin callers of the product headers: no arithmetic of its own. Test-only.
//
// Sections: the jx_field.h operations are always there; for the others the includer includes the product headers
// first and names the sections it wants: JX_TESTOPS_BASE (jx_keccak.h, jx_sha256.h, jx_sha_aes.h, jx_hpke.h),
// JX_TESTOPS_SAMPLE (jx_sample.h; needs BASE), JX_TESTOPS_P256 (jx_p256.h), JX_TESTOPS_CHAPOLY (jx_chapoly_lanes.h).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_field.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JXT __device__ inline
#else
#define JXT static inline
#endif

namespace jxt {
using namespace jx;

JXT f128 ld(const uint8_t* p) {
  uint64_t lo, hi;
  memcpy(&lo, p, 8);
  memcpy(&hi, p + 8, 8);
  return make128(lo, hi);
}
JXT void st(uint8_t* p, f128 v) {
  memcpy(p, &v.lo, 8);
  memcpy(p + 8, &v.hi, 8);
}

// ---- jx_field.h
// op: 0 add, 1 sub, 2 mont, 3 to_mont, 4 from_mont, 5 neg (b may be null for the one-operand forms)
JXT void t_f128(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  f128 x = ld(a), y = b ? ld(b) : make128(0, 0), r;
  switch (op) {
    case 0: r = add128(x, y); break;
    case 1: r = sub128(x, y); break;
    case 2: r = mont128(x, y); break;
    case 3: r = to_mont128(x); break;
    case 4: r = from_mont128(x); break;
    default: r = neg128(x); break;
  }
  st(out, r);
}
JXT void t_reduce192(const uint64_t w[3], uint8_t* out) { st(out, reduce192(w[0], w[1], w[2])); }
JXT void t_reduce192_small(const uint64_t w[3], uint8_t* out) { st(out, reduce192_small(w[0], w[1], w[2])); }
JXT void t_mont_lazy(const uint8_t* a, const uint8_t* b, uint64_t out[3]) {
  uint64_t lo, hi;
  uint32_t top;
  mont128_lazy(ld(a), ld(b), lo, hi, top);
  out[0] = lo;
  out[1] = hi;
  out[2] = top;
}
// wacc_reduce of nine raw column sums (each < 2^63, the wire-sum bound)
JXT void t_wacc_reduce(const uint64_t cols[9], uint8_t* out) {
  wacc26 a;
  for (int s = 0; s < 9; s++) a.col[s] = cols[s];
  st(out, wacc_reduce(a));
}
JXT void t_wacc_normalize(const uint64_t cols[9], uint64_t out[9]) {
  wacc26 a;
  for (int s = 0; s < 9; s++) a.col[s] = cols[s];
  wacc_normalize(a);
  for (int s = 0; s < 9; s++) out[s] = a.col[s];
}
// sum_k xs[k] * cs[k] mod p through the 26-bit-limb column accumulator, normalising every
// `norm_every` terms (the FLP kernel normalises every 512 calls)
JXT void t_wide_dot(const uint8_t* xs, const uint8_t* cs, int n, int norm_every, uint8_t* out) {
  wacc26 a;
  wacc_zero(a);
  for (int k = 0; k < n; k++) {
    wacc_mac(a, to_limbs26(ld(xs + 16 * k)), to_limbs26(ld(cs + 16 * k)));
    if (norm_every > 0 && (k + 1) % norm_every == 0) wacc_normalize(a);
  }
  st(out, wacc_reduce(a));
}
// op: 0 add, 1 sub, 2 mul
JXT uint64_t t_f64(int op, uint64_t a, uint64_t b) {
  switch (op) {
    case 0: return add64(a, b);
    case 1: return sub64(a, b);
    default: return mul64(a, b);
  }
}
// sum_k xs[k] * cs[k] mod p64 through the Field64 limb column accumulator (folding every 1024 terms)
JXT uint64_t t_wacc64_dot(const uint64_t* xs, const uint64_t* cs, int n) {
  wacc64 a;
  wacc64_zero(a);
  uint64_t acc = 0;
  for (int k = 0; k < n; k++) {
    wacc64_mac(a, xs[k], to_c64limbs(cs[k]));
    if ((k + 1) % (int)WACC64_MAX_TERMS == 0) {
      acc = add64(acc, wacc64_reduce(a));
      wacc64_zero(a);
    }
  }
  return add64(acc, wacc64_reduce(a));
}
JXT uint64_t t_reduce192_p64(const uint64_t w[3]) { return reduce192_p64(w[0], w[1], w[2]); }
JXT int t_ge_p128(const uint8_t* a) { return ge_p128(ld(a)) ? 1 : 0; }
JXT int t_ge_p64(uint32_t lo, uint32_t hi) { return ge_p64(lo, hi) ? 1 : 0; }

// the staged coefficient limbs (pack_cd26 / unpack_cd26)
JXT void t_cl_to_limbs(const uint8_t* a, uint32_t l[5]) {
  const limbs26 r = to_limbs26(ld(a));
  for (int i = 0; i < 5; i++) l[i] = r.l[i];
}
JXT void t_cl_pack(const uint8_t* c, const uint8_t* d, uint32_t* w) { pack_cd26(ld(c), ld(d), w); }
JXT void t_cl_unpack(const uint32_t* w, uint32_t cl[5], uint32_t dl[5]) {
  limbs26 c, d;
  unpack_cd26(w, c, d);
  for (int i = 0; i < 5; i++) {
    cl[i] = c.l[i];
    dl[i] = d.l[i];
  }
}
// The ring's accumulation over n calls of one slot: ae += x_k * d_k, ao += x_k * c_k, as raw column sums.
// packed = 0: the coefficient limbs split from the 16-byte values at every use; 1: from the staged words.
JXT void t_cl_mac(const uint8_t* xs, const uint8_t* cs, const uint8_t* ds, int n, int packed, uint64_t cole[9],
                  uint64_t colo[9]) {
  wacc26 ae, ao;
  wacc_zero(ae);
  wacc_zero(ao);
  for (int k = 0; k < n; k++) {
    const limbs26 xl = to_limbs26(ld(xs + 16 * k));
    limbs26 ck, dk;
    if (packed) {
      uint32_t w[CD26_WORDS];
      pack_cd26(ld(cs + 16 * k), ld(ds + 16 * k), w);
      unpack_cd26(w, ck, dk);
    } else {
      ck = to_limbs26(ld(cs + 16 * k));
      dk = to_limbs26(ld(ds + 16 * k));
    }
    wacc_mac(ae, xl, dk);
    wacc_mac(ao, xl, ck);
  }
  for (int s = 0; s < 9; s++) {
    cole[s] = ae.col[s];
    colo[s] = ao.col[s];
  }
}

#ifdef JX_TESTOPS_BASE
// ---- jx_keccak.h, jx_sha256.h, jx_sha_aes.h, jx_hpke.h (the includer has included them)
JXT void st_to_words(const uint64_t st64[25], uint32_t s[50]) {
  for (int i = 0; i < 25; i++) {
    s[2 * i] = (uint32_t)st64[i];
    s[2 * i + 1] = (uint32_t)(st64[i] >> 32);
  }
}
JXT void st_from_words(const uint32_t s[50], uint64_t st64[25]) {
  for (int i = 0; i < 25; i++) st64[i] = (uint64_t)s[2 * i] | ((uint64_t)s[2 * i + 1] << 32);
}
JXT void t_keccak_p12(uint64_t st64[25]) {
  uint32_t s[50];
  st_to_words(st64, s);
  keccak_p12(s);
  st_from_words(s, st64);
}
JXT void t_sha256_16(const uint8_t id[16], uint8_t out[32]) {
  uint32_t w[4], d[8];
  memcpy(w, id, 16);
  sha256_16(w, d);
  memcpy(out, d, 32);
}
JXT void t_x25519(const uint8_t k[32], const uint8_t u[32], uint8_t out[32]) {
  uint8_t kc[32];
  memcpy(kc, k, 32);
  kc[0] &= 248;
  kc[31] &= 127;
  kc[31] |= 64;
  uint32_t kw[8], uw[8], ow[8];
  memcpy(kw, kc, 32);
  memcpy(uw, u, 32);
  x25519_ladder(ow, kw, uw);
  memcpy(out, ow, 32);
}
// op: 0 mul, 1 sq, 2 sub, 3 invert, 4 mul_small(121665); inputs/outputs canonical 32-byte LE
JXT void t_fe(int op, const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  uint32_t aw[8], bw[8], ow[8];
  memcpy(aw, a, 32);
  memcpy(bw, b, 32);
  fe x, y, r;
  fe_from_bytes(x, aw);
  fe_from_bytes(y, bw);
  switch (op) {
    case 0: fe_mul(r, x, y); break;
    case 1: fe_sq(r, x); break;
    case 2: fe_sub(r, x, y); break;
    case 3: fe_invert(r, x); break;
    default: fe_mul_small(r, x, 121665); break;
  }
  fe_to_bytes(ow, r);
  memcpy(out, ow, 32);
}
// op 0 mul, 1 sq, 4 mul_small(121665) on raw limbs (loosely reduced inputs up to 2^28 - 1, as fe_sub / fe_add
// produce them inside the ladder); the output limbs as the reduction leaves them (bounds checked by the test)
JXT void t_fe_limbs(int op, const uint32_t a[10], const uint32_t b[10], uint32_t out[10]) {
  fe x, y, r;
  for (int i = 0; i < 10; i++) {
    x.v[i] = a[i];
    y.v[i] = b[i];
  }
  switch (op) {
    case 0: fe_mul(r, x, y); break;
    case 1: fe_sq(r, x); break;
    default: fe_mul_small(r, x, 121665); break;
  }
  for (int i = 0; i < 10; i++) out[i] = r.v[i];
}
// x, h: 16-byte blocks; out = x * h in GF(2^128) (GCM bit order)
JXT void t_ghash_mul(const uint8_t x[16], const uint8_t h[16], uint8_t out[16]) {
  uint32_t xw[4], hw[4];
  for (int i = 0; i < 4; i++) {
    xw[i] = (uint32_t)x[4 * i] << 24 | (uint32_t)x[4 * i + 1] << 16 | (uint32_t)x[4 * i + 2] << 8 | x[4 * i + 3];
    hw[i] = (uint32_t)h[4 * i] << 24 | (uint32_t)h[4 * i + 1] << 16 | (uint32_t)h[4 * i + 2] << 8 | h[4 * i + 3];
  }
  ghash_mul(xw, hw);
  for (int i = 0; i < 4; i++)
    for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(xw[i] >> (24 - 8 * k));
}
// HMAC-SHA256 with a 32-byte key over msg (len <= 119) through hmac_pads/sha256_finish64/hmac_outer
JXT void t_hmac32(const uint8_t key[32], const uint8_t* msg, int len, uint8_t out[32]) {
  uint32_t kb[8], ist[8], ost[8], inner[8], o[8];
  for (int i = 0; i < 8; i++)
    kb[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
  hmac_pads(kb, ist, ost);
  Msg128 m;
  m_zero(m);
  for (int i = 0; i < len; i++) m_byte(m, i, msg[i]);
  sha256_finish64(inner, ist, m, len);
  hmac_outer(o, ost, inner);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(o[i] >> (24 - 8 * k));
}
// T-table AES of the XofHmacSha256Aes128 kernels (jx_sha_aes.h) over the table t0[x] = aes_t0_entry(sbox[x]):
// otf = 0 expands the 44-word schedule first, otf = 1 computes it on the fly
JXT void t_aes128_t(int otf, const uint32_t* t0, const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  auto T = [&](uint32_t x) { return t0[x]; };
  uint32_t k[4], rk[44], i4[4], o4[4];
  memcpy(k, key, 16);
  memcpy(i4, in, 16);
  if (otf) {
    aes128_encrypt_t_otf(T, k, i4, o4);
  } else {
    aes128_expand_key_t(T, k, rk);
    aes128_encrypt_t(T, rk, i4, o4);
  }
  memcpy(out, o4, 16);
}
#endif  // JX_TESTOPS_BASE

#ifdef JX_TESTOPS_SAMPLE
// ---- jx_sample.h: exact ">= p" on a loaded element and rejection sampling
JXT int t_ge_exact(const uint8_t* a) {
  uint4 v;
  memcpy(&v, a, 16);
  return ge_exact(v) ? 1 : 0;
}
// the running max of ge_screen over n 16-byte elements, as the XOF kernels keep it per block
JXT uint32_t t_ge_screen_max(const uint8_t* a, int n) {
  uint32_t gmax = 0;
  for (int i = 0; i < n; i++) {
    uint4 v;
    memcpy(&v, a + 16 * i, 16);
    gmax = gmax > ge_screen(v) ? gmax : ge_screen(v);
  }
  return gmax;
}
// sample64<N> (N = 1 | 5) on a Keccak state whose first block is ready; the state is left as sampling left it
JXT void t_sample64(int n, uint64_t st64[25], uint64_t* out) {
  uint32_t s[50];
  st_to_words(st64, s);
  if (n == 1) {
    sample64<1>(s, out);
  } else {
    sample64<5>(s, out);
  }
  st_from_words(s, st64);
}
JXT void t_sample2_f128(uint64_t st64[25], uint32_t cnt, int slow, uint8_t out[32], uint32_t* flags) {
  uint32_t s[50];
  st_to_words(st64, s);
  f128 o[2] = {make128(0, 0), make128(0, 0)};
  sample2_f128(s, o, cnt, slow != 0, *flags);
  st(out, o[0]);
  st(out + 16, o[1]);
  st_from_words(s, st64);
}
// n elements from the byte stream that starts at byte `pos` of the block in st64; returns the final position
JXT uint32_t t_bx_sample128(uint64_t st64[25], uint32_t pos, int n, uint8_t* out) {
  ByteXof x;
  st_to_words(st64, x.s);
  x.pos = pos;
  for (int i = 0; i < n; i++) st(out + 16 * i, bx_sample128(x));
  st_from_words(x.s, st64);
  return x.pos;
}
// xof_stream128 for n elements on a Keccak state whose first block is ready: value k of emit(k, v) to out[16 k]
// (k < n only). Returns the number of emit calls when call i came with k == i, else that number | 2^31.
JXT uint32_t t_xof_stream128(const uint64_t st64[25], uint32_t n, uint8_t* out) {
  uint32_t s[50], calls = 0, disorder = 0;
  st_to_words(st64, s);
  xof_stream128(s, n, [&](uint32_t k, f128 v) {
    if (k != calls) disorder = 0x80000000u;
    if (k < n) st(out + 16 * k, v);
    calls++;
  });
  return calls | disorder;
}
#endif  // JX_TESTOPS_SAMPLE

#ifdef JX_TESTOPS_P256
// ---- jx_p256.h
// a op b mod p on canonical integers (32 big-endian bytes each), through the Montgomery form the kernels use.
// op: 0 mul, 1 square (of a), 2 inverse (of a; 0 for 0), 3 add, 4 sub. Returns 0 when an operand is >= p.
JXT int t_p256_fe_op(int op, const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  p256_fe x, y, r;
  if (!p256_from_bytes(x, a) || !p256_from_bytes(y, b)) return 0;
  switch (op) {
    case 0: p256_mul(r, x, y); break;
    case 1: p256_sq(r, x); break;
    case 2: p256_invert(r, x); break;
    case 3: p256_add(r, x, y); break;
    default: p256_sub(r, x, y); break;
  }
  p256_to_bytes(out, r);
  return 1;
}
// 1: pt (65 bytes) is a valid encoding of a point of the curve
JXT int t_p256_point_valid(const uint8_t pt[65]) {
  p256_fe x, y;
  return p256_point_from_bytes(x, y, pt) ? 1 : 0;
}
// sk (32 big-endian bytes) * pt -> x || y (64 bytes). 0 for an invalid point or the point at infinity.
JXT int t_p256_scalar_mul(const uint8_t sk[32], const uint8_t pt[65], uint8_t out[64]) {
  uint32_t k[8];
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = sk + 4 * (7 - i);
    k[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  p256_fe x, y;
  if (!p256_point_from_bytes(x, y, pt)) return 0;
  uint8_t x_only[32];
  const int ok = p256_scalar_mul_xy(out, k, x, y) ? 1 : 0;
  const int ok_x = p256_scalar_mul_x(x_only, k, x, y) ? 1 : 0;  // what a lane calls
  int same = 1;
  for (int i = 0; i < 32; i++) same &= x_only[i] == out[i];
  return ok && ok_x && same;
}
#endif  // JX_TESTOPS_P256

#ifdef JX_TESTOPS_CHAPOLY
// ---- jx_chapoly_lanes.h
// out = h m mod 2^130 - 5 by pl_mul, limbs in and out as they are (the caller checks the ranges)
JXT void t_pl_mul(const uint32_t h[5], const uint32_t m[5], uint32_t out[5]) {
  for (int i = 0; i < 5; i++) out[i] = h[i];
  pl_mul(out, m);
}
#endif  // JX_TESTOPS_CHAPOLY

}  // namespace jxt
