// jx_p256.h — NIST P-256 for DHKEM(P-256, HKDF-SHA256) (RFC 9180 §7.1, KEM 0x0010; core/src/hpke.rs opens under
// it beside the X25519 KEM): validation of an encapsulated key and the x-coordinate of sk * P. One report per
// lane; __host__ __device__, so tests/csrc/hosttest_hpke_p256.cpp runs the same code on the CPU and
// jx_hpke_create_key computes sk * G with it.
//
// Representation. p = 2^256 - 2^224 + 2^192 + 2^96 - 1 has no small fold constant in 26-bit limbs (jx_hpke.h's
// 2^260 == 608 trick needs one), but p == -1 mod 2^32, so Montgomery's -p^-1 mod 2^32 is 1 and the reduction
// multiplier of a step is the low word itself; five of p's eight 32-bit words are 0 or 1. So: eight 32-bit limbs,
// little-endian, elements in Montgomery form a * 2^256 mod p, ALWAYS fully reduced (< p). Every function below
// takes operands < p and returns a value < p; there is no lazy range to track between operations.
//
// Bounds inside p256_mul (CIOS, one word of b per step, t of 8 words + hi < 2):
//   row:     t[j] + a[j] * b[i] + c <= (2^32 - 1) + (2^32 - 1)^2 + (2^32 - 1) = 2^64 - 1, so each column's sum fits
//            a v_mad_u64_u32 and its carry c < 2^32;
//   reduce:  m = t[0]; t[j] + m * p[j] + c fits the same way; t[0] + m * p[0] = t[0] * 2^32 is dropped;
//   value:   with a, b < p the running value stays < 2p after every step ((t + a b_i + m p) / 2^32 with t < 2p,
//            a < p, b_i, m < 2^32 gives < (2p + 2^32 p + 2^32 p) / 2^32 < 2p + 1), so hi is 0 or 1 and ONE masked
//            subtraction of p brings it below p.
//
// Scalar multiplication. Complete projective formulas for a = -3 (Renes, Costello, Batina, "Complete addition
// formulas for prime order elliptic curves", EUROCRYPT 2016, algorithms 4 and 6): valid for EVERY pair of inputs
// on a curve of odd order, the point at infinity (0 : 1 : 0), P = Q and P = -Q included, so the double-and-add-
// always loop from R = infinity has no exceptional case to rule out. It takes sk four bits at a time, most
// significant first: R = 16 R, then R = R + d P with d P from a table of 0 P .. 15 P (0 P = infinity). Under
// leading zero digits R stays infinity (2 * infinity, infinity + infinity); the first non-zero digit meets
// infinity + d P; a zero digit meets R + infinity; and whatever multiples R and d P are, equal or opposite
// included, their sum is covered. Every sk takes the same instructions: 256 doublings and 64 + 14 additions,
// ~3,900 field multiplications against ~6,400 bit by bit. P-256's order n is prime, so a valid P != infinity has
// order n and sk * P with sk in [1, n - 1] is never infinity: Z != 0 at the end (checked all the same: Z = 0 is a
// failed open). The digit of sk picks its table entry by word masks over ALL sixteen entries (1.5 KB of private
// memory per lane, read at addresses that depend on the loop counters alone); no branch and no address depends on
// sk.
#pragma once
#include <stdint.h>

#include "jx_field.h"

namespace jx {

struct p256_fe {
  uint32_t v[8];  // Montgomery form, little-endian words, value < p
};
struct p256_pt {
  p256_fe X, Y, Z;  // projective: (X/Z, Y/Z); infinity is (0 : 1 : 0)
};

// p and the group order n, little-endian words
#define JX_P256_P(i) ((i) < 3 ? 0xFFFFFFFFu : (i) < 6 ? 0u : (i) == 6 ? 1u : 0xFFFFFFFFu)
JX_HD uint32_t p256_n_word(int i) {
  const uint32_t n[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
  return n[i];
}

// r = t - p if t >= p else t, for t = hi * 2^256 + t[0..7] < 2p
JX_HD void p256_cond_sub_p(p256_fe& r, const uint32_t t[8], uint32_t hi) {
  uint32_t d[8];
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t x = (uint64_t)t[i] - JX_P256_P(i) - bw;
    d[i] = (uint32_t)x;
    bw = (x >> 63) & 1u;
  }
  // t >= p  <=>  no borrow out of the 9-word subtraction
  const uint32_t keep = 0u - (uint32_t)(bw > hi);  // all ones: t < p, keep t
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (t[i] & keep) | (d[i] & ~keep);
}

JX_HD void p256_add(p256_fe& r, const p256_fe& a, const p256_fe& b) {
  uint32_t t[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  p256_cond_sub_p(r, t, (uint32_t)c);
}

JX_HD void p256_sub(p256_fe& r, const p256_fe& a, const p256_fe& b) {
  uint32_t d[8];
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t x = (uint64_t)a.v[i] - b.v[i] - bw;
    d[i] = (uint32_t)x;
    bw = (x >> 63) & 1u;
  }
  const uint32_t m = 0u - (uint32_t)bw;  // a < b: add p back
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)d[i] + (JX_P256_P(i) & m);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
}

// Montgomery product a b 2^-256 mod p (bounds in the header comment)
JX_HD void p256_mul(p256_fe& r, const p256_fe& a, const p256_fe& b) {
  uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t hi = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a.v[j] * b.v[i] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += hi;  // < 2^32 + 1
    const uint32_t t8 = (uint32_t)c;
    const uint32_t t9 = (uint32_t)(c >> 32);
    const uint32_t m = t[0];
    c = ((uint64_t)m * JX_P256_P(0) + t[0]) >> 32;  // the low word is zero by construction
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * JX_P256_P(j) + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t8;
    t[7] = (uint32_t)c;
    hi = t9 + (uint32_t)(c >> 32);  // the value is < 2p < 2^257: 0 or 1
  }
  p256_cond_sub_p(r, t, hi);
}
JX_HD void p256_sq(p256_fe& r, const p256_fe& a) { p256_mul(r, a, a); }

JX_HD p256_fe p256_const(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6,
                         uint32_t w7) {
  p256_fe r;
  r.v[0] = w0, r.v[1] = w1, r.v[2] = w2, r.v[3] = w3, r.v[4] = w4, r.v[5] = w5, r.v[6] = w6, r.v[7] = w7;
  return r;
}
// 2^512 mod p (to Montgomery form), 2^256 mod p (one), b 2^256 mod p
JX_HD p256_fe p256_r2() {
  return p256_const(0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u);
}
JX_HD p256_fe p256_one() {
  return p256_const(0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u);
}
JX_HD p256_fe p256_b() {
  return p256_const(0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu, 0xf7212ed6u, 0xe5a220abu, 0x04874834u, 0xdc30061du);
}
JX_HD p256_fe p256_zero() { return p256_const(0, 0, 0, 0, 0, 0, 0, 0); }

// 32 big-endian bytes -> Montgomery form. False when the integer is >= p (the element is then not to be used).
JX_HD bool p256_from_bytes(p256_fe& r, const uint8_t* b) {
  p256_fe a;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 4 * (7 - i);
    a.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) bw = (((uint64_t)a.v[i] - JX_P256_P(i) - bw) >> 63) & 1u;
  const bool below = bw != 0;  // a - p borrows  <=>  a < p
  if (!below) a = p256_zero();
  p256_mul(r, a, p256_r2());
  return below;
}
// Montgomery form -> the canonical integer as 32 big-endian bytes
JX_HD void p256_to_bytes(uint8_t* b, const p256_fe& a) {
  p256_fe one = p256_zero(), c;
  one.v[0] = 1;
  p256_mul(c, a, one);  // a 2^-256, < p
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint8_t* q = b + 4 * (7 - i);
    q[0] = (uint8_t)(c.v[i] >> 24), q[1] = (uint8_t)(c.v[i] >> 16), q[2] = (uint8_t)(c.v[i] >> 8), q[3] = (uint8_t)c.v[i];
  }
}

JX_HD bool p256_eq(const p256_fe& a, const p256_fe& b) {  // both < p: equal values have equal words
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= a.v[i] ^ b.v[i];
  return d == 0;
}

// z^(p - 2): square and multiply over the PUBLIC exponent p - 2 = ffffffff 00000001 00000000 00000000 00000000
// ffffffff ffffffff fffffffd (256 squarings, 127 multiplications; once per open, against ~6,900 in the ladder).
// z = 0 gives 0.
JX_HD void p256_invert(p256_fe& r, const p256_fe& z) {
  p256_fe acc = p256_one();
#pragma unroll 1
  for (int pos = 255; pos >= 0; pos--) {
    const int w = pos >> 5;
    const uint32_t ew = w == 0 ? 0xFFFFFFFDu : (w < 3 || w == 7) ? 0xFFFFFFFFu : w == 6 ? 1u : 0u;
    p256_sq(acc, acc);
    if ((ew >> (pos & 31)) & 1u) p256_mul(acc, acc, z);
  }
  r = acc;
}

// Renes-Costello-Batina algorithm 4: complete addition on y^2 = x^3 - 3x + b (12 M + 2 m_b)
JX_HD void p256_pt_add(p256_pt& R, const p256_pt& P, const p256_pt& Q) {
  const p256_fe b = p256_b();
  p256_fe t0, t1, t2, t3, t4, X3, Y3, Z3;
  p256_mul(t0, P.X, Q.X);
  p256_mul(t1, P.Y, Q.Y);
  p256_mul(t2, P.Z, Q.Z);
  p256_add(t3, P.X, P.Y);
  p256_add(t4, Q.X, Q.Y);
  p256_mul(t3, t3, t4);
  p256_add(t4, t0, t1);
  p256_sub(t3, t3, t4);
  p256_add(t4, P.Y, P.Z);
  p256_add(X3, Q.Y, Q.Z);
  p256_mul(t4, t4, X3);
  p256_add(X3, t1, t2);
  p256_sub(t4, t4, X3);
  p256_add(X3, P.X, P.Z);
  p256_add(Y3, Q.X, Q.Z);
  p256_mul(X3, X3, Y3);
  p256_add(Y3, t0, t2);
  p256_sub(Y3, X3, Y3);
  p256_mul(Z3, b, t2);
  p256_sub(X3, Y3, Z3);
  p256_add(Z3, X3, X3);
  p256_add(X3, X3, Z3);
  p256_sub(Z3, t1, X3);
  p256_add(X3, t1, X3);
  p256_mul(Y3, b, Y3);
  p256_add(t1, t2, t2);
  p256_add(t2, t1, t2);
  p256_sub(Y3, Y3, t2);
  p256_sub(Y3, Y3, t0);
  p256_add(t1, Y3, Y3);
  p256_add(Y3, t1, Y3);
  p256_add(t1, t0, t0);
  p256_add(t0, t1, t0);
  p256_sub(t0, t0, t2);
  p256_mul(t1, t4, Y3);
  p256_mul(t2, t0, Y3);
  p256_mul(Y3, X3, Z3);
  p256_add(Y3, Y3, t2);
  p256_mul(X3, t3, X3);
  p256_sub(X3, X3, t1);
  p256_mul(Z3, t4, Z3);
  p256_mul(t1, t3, t0);
  p256_add(Z3, Z3, t1);
  R.X = X3, R.Y = Y3, R.Z = Z3;
}

// Renes-Costello-Batina algorithm 6: complete doubling for a = -3 (8 M + 3 S + 2 m_b)
JX_HD void p256_pt_dbl(p256_pt& R, const p256_pt& P) {
  const p256_fe b = p256_b();
  p256_fe t0, t1, t2, t3, X3, Y3, Z3;
  p256_sq(t0, P.X);
  p256_sq(t1, P.Y);
  p256_sq(t2, P.Z);
  p256_mul(t3, P.X, P.Y);
  p256_add(t3, t3, t3);
  p256_mul(Z3, P.X, P.Z);
  p256_add(Z3, Z3, Z3);
  p256_mul(Y3, b, t2);
  p256_sub(Y3, Y3, Z3);
  p256_add(X3, Y3, Y3);
  p256_add(Y3, X3, Y3);
  p256_sub(X3, t1, Y3);
  p256_add(Y3, t1, Y3);
  p256_mul(Y3, X3, Y3);
  p256_mul(X3, X3, t3);
  p256_add(t3, t2, t2);
  p256_add(t2, t2, t3);
  p256_mul(Z3, b, Z3);
  p256_sub(Z3, Z3, t2);
  p256_sub(Z3, Z3, t0);
  p256_add(t3, Z3, Z3);
  p256_add(Z3, Z3, t3);
  p256_add(t3, t0, t0);
  p256_add(t0, t3, t0);
  p256_sub(t0, t0, t2);
  p256_mul(t0, t0, Z3);
  p256_add(Y3, Y3, t0);
  p256_mul(t0, P.Y, P.Z);
  p256_add(t0, t0, t0);
  p256_mul(Z3, t0, Z3);
  p256_sub(X3, X3, Z3);
  p256_mul(Z3, t0, t1);
  p256_add(Z3, Z3, Z3);
  p256_add(Z3, Z3, Z3);
  R.X = X3, R.Y = Y3, R.Z = Z3;
}

// Validation of an uncompressed SEC 1 point (the caller has checked that there are 65 bytes): first byte 0x04,
// x < p, y < p, y^2 = x^3 - 3x + b. A point of another curve y^2 = x^3 - 3x + b' fails the last test, so the
// ladder never runs on a curve of smooth order (the invalid-curve attack). The point at infinity has no such
// encoding. All of it is public data. Out: the affine point in Montgomery form.
JX_HD bool p256_point_from_bytes(p256_fe& x, p256_fe& y, const uint8_t* enc) {
  bool ok = enc[0] == 0x04;
  ok = p256_from_bytes(x, enc + 1) && ok;
  ok = p256_from_bytes(y, enc + 33) && ok;
  p256_fe l, r, t;
  p256_sq(l, y);
  p256_sq(r, x);
  p256_mul(r, r, x);
  p256_add(t, x, x);
  p256_add(t, t, x);
  p256_sub(r, r, t);
  p256_add(r, r, p256_b());
  return ok && p256_eq(l, r);
}

// sk as 8 little-endian words (sk[0] the least significant): 1 <= sk < n
JX_HD bool p256_scalar_valid(const uint32_t sk[8]) {
  uint32_t nz = 0;
  uint64_t bw = 0;
  for (int i = 0; i < 8; i++) {
    nz |= sk[i];
    bw = (((uint64_t)sk[i] - p256_n_word(i) - bw) >> 63) & 1u;
  }
  return nz != 0 && bw != 0;
}

// sk * (x, y) in affine coordinates, x || y as 32 big-endian bytes each (WITH_Y) or x alone, for a valid point and
// sk in [1, n - 1] (8 little-endian words). False (and zeros) for the point at infinity, which those inputs
// cannot give.
template <bool WITH_Y>
JX_HD bool p256_scalar_mul_affine(uint8_t* out, const uint32_t sk[8], const p256_fe& x, const p256_fe& y) {
  // tab[j] = j * (x, y), j = 0..15 (tab[0] the point at infinity): 14 additions
  p256_pt tab[16], R, T;
  tab[0].X = p256_zero(), tab[0].Y = p256_one(), tab[0].Z = p256_zero();
  tab[1].X = x, tab[1].Y = y, tab[1].Z = p256_one();
#pragma unroll 1
  for (int j = 2; j < 16; j++) p256_pt_add(tab[j], tab[j - 1], tab[1]);
  R = tab[0];
#pragma unroll 1
  for (int w = 63; w >= 0; w--) {
#pragma unroll 1
    for (int k = 0; k < 4; k++) p256_pt_dbl(R, R);
    const uint32_t d = (sk[w >> 3] >> (4 * (w & 7))) & 15u;  // the index is the loop counter, not a key bit
    // T = tab[d] without an address that depends on d: every entry is read, one is kept
#pragma unroll
    for (int i = 0; i < 8; i++) T.X.v[i] = T.Y.v[i] = T.Z.v[i] = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t m = 0u - (((d ^ j) - 1u) >> 31);  // all ones iff j == d
#pragma unroll
      for (int i = 0; i < 8; i++) {
        T.X.v[i] |= tab[j].X.v[i] & m;
        T.Y.v[i] |= tab[j].Y.v[i] & m;
        T.Z.v[i] |= tab[j].Z.v[i] & m;
      }
    }
    p256_pt_add(R, R, T);
  }
  p256_fe zi, ax;
  const bool finite = !p256_eq(R.Z, p256_zero());
  p256_invert(zi, R.Z);
  p256_mul(ax, R.X, zi);
  p256_to_bytes(out, ax);
  if (WITH_Y) {
    p256_mul(ax, R.Y, zi);
    p256_to_bytes(out + 32, ax);
  }
  return finite;
}
// what DHKEM's DH needs: the x-coordinate
JX_HD bool p256_scalar_mul_x(uint8_t out[32], const uint32_t sk[8], const p256_fe& x, const p256_fe& y) {
  return p256_scalar_mul_affine<false>(out, sk, x, y);
}
// both coordinates: the public key of a private one (jx_hpke_create_key, on the host)
JX_HD bool p256_scalar_mul_xy(uint8_t out[64], const uint32_t sk[8], const p256_fe& x, const p256_fe& y) {
  return p256_scalar_mul_affine<true>(out, sk, x, y);
}

}  // namespace jx
