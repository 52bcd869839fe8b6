// jx_ghash_lanes.h — GHASH of one long message split over the 64 lanes of a wave (jx_hpke_long.hip), and the
// table form of the multiplication by a fixed element that the split needs. __host__ __device__: tests/csrc/
// hosttest_hpke_long.cpp runs the same code on the CPU, one loop iteration per lane.
//
// GHASH over blocks X_0 .. X_{N-1} (the AAD's blocks, then the ciphertext's, each zero padded) and the length
// block L is S = (X_0 H^N + X_1 H^(N-1) + ... + X_{N-1} H + L) H. Lane j owns blocks j, j + 64, ...: with c_j of them
// its last one is k_j = j + 64 (c_j - 1), and Horner in H^64 gives
//   P_j = X_j (H^64)^(c_j - 1) + X_(j+64) (H^64)^(c_j - 2) + ... + X_(k_j),
// so S = (sum_j P_j H^(d_j) + L) H with d_j = N - k_j in [1, 64]: the exponent depends on N and j alone, never on
// which lane holds the last or a partial block. A lane without blocks contributes zero.
//
// The per-block product P H^64 has a fixed right operand, so it runs over a 16-entry table M[n] = n H^64 (n: the
// four coefficients of one nibble), four bits of P per step (Shoup): 31 shifts by x^4 with the 16-bit reduction
// computed from the nibble that falls off, 32 table reads. The table is the caller's: TL is any callable
// (nibble, uint32_t out[4]).
#pragma once
#include "jx_hpke.h"

namespace jx {

constexpr uint32_t GL_LANES = 64;

// how many of N blocks lane j owns
JX_HD uint64_t gl_lane_blocks(uint64_t N, uint32_t j) { return N > j ? (N - j + GL_LANES - 1) / GL_LANES : 0; }
// d_j: the power of H that lane j's Horner partial is multiplied by (1..64); 0 for a lane without blocks
JX_HD uint32_t gl_lane_exponent(uint64_t N, uint32_t j) {
  const uint64_t c = gl_lane_blocks(N, j);
  return c ? (uint32_t)(N - (j + GL_LANES * (c - 1))) : 0u;
}

// entry n of the table of the fixed element h: (n's four bits as the coefficients of x^0..x^3, bit 3 first) h
JX_HD void gl_tab4_entry(uint32_t n, const uint32_t h[4], uint32_t out[4]) {
  out[0] = n << 28;
  out[1] = out[2] = out[3] = 0;
  ghash_mul(out, h);
}

// x = x h, h given by its table
template <class TL>
JX_HD void ghash_mul_tab4(uint32_t x[4], const TL& M) {
  uint32_t e[4];
  M(x[3] & 0xfu, e);
  uint32_t z0 = e[0], z1 = e[1], z2 = e[2], z3 = e[3];
#pragma unroll
  for (int i = 30; i >= 0; i--) {
    // z x^4: the four coefficients that leave at the low end come back as rem (x^128 = 1 + x + x^2 + x^7)
    const uint32_t rem = z3 & 0xfu;
    z3 = (z3 >> 4) | (z2 << 28);
    z2 = (z2 >> 4) | (z1 << 28);
    z1 = (z1 >> 4) | (z0 << 28);
    z0 = (z0 >> 4) ^ (((rem << 5) ^ (rem << 10) ^ (rem << 11) ^ (rem << 12)) << 16);
    M((x[i >> 3] >> (28 - 4 * (i & 7))) & 0xfu, e);
    z0 ^= e[0];
    z1 ^= e[1];
    z2 ^= e[2];
    z3 ^= e[3];
  }
  x[0] = z0;
  x[1] = z1;
  x[2] = z2;
  x[3] = z3;
}

// Lane j's Horner partial P_j over its blocks of N. Block: (k, uint32_t x[4]) -> block k as 4 big-endian words;
// M64: the table of H^64.
template <class Block, class TL>
JX_HD void gl_lane_partial(uint64_t N, uint32_t j, Block block, const TL& M64, uint32_t p[4]) {
  p[0] = p[1] = p[2] = p[3] = 0;
  for (uint64_t k = j; k < N; k += GL_LANES) {
    if (k != j) ghash_mul_tab4(p, M64);
    uint32_t x[4];
    block(k, x);
    for (int w = 0; w < 4; w++) p[w] ^= x[w];
  }
}

// One step of the powers H^1 .. H^64 by doubling: before step s (0..5) lane l < 2^s holds H^(l+1); lane l in
// [2^s, 2^(s+1)) takes H^(2^s) from lane 2^s - 1 and H^(l+1-2^s) from lane l - 2^s. The sources of lane l at step s
// (the caller shuffles, or indexes an array):
JX_HD uint32_t gl_pow_src_base(int s) { return (1u << s) - 1; }
JX_HD uint32_t gl_pow_src_other(int s, uint32_t l) { return (l - (1u << s)) & (GL_LANES - 1); }
JX_HD bool gl_pow_active(int s, uint32_t l) { return l >= (1u << s) && l < (2u << s); }

// S from the XOR over the lanes of P_j H^(d_j)
JX_HD void gl_finish(uint32_t y[4], uint64_t alen, uint64_t clen, const uint32_t h[4]) {
  y[0] ^= (uint32_t)((8 * alen) >> 32);
  y[1] ^= (uint32_t)(8 * alen);
  y[2] ^= (uint32_t)((8 * clen) >> 32);
  y[3] ^= (uint32_t)(8 * clen);
  ghash_mul(y, h);
}

// ---- AES with either key length over the T-table of jx_sha_aes.h (TL: x -> T0[x]); NK key words, NK + 6 rounds
template <int NK, class TL>
JX_HD void aes_expand_key_t(const TL& T, const uint32_t* key, uint32_t* rk) {
#pragma unroll
  for (int i = 0; i < NK; i++) rk[i] = key[i];
  uint32_t rcon = 1;
#pragma unroll
  for (int i = NK; i < 4 * (NK + 7); i++) {
    uint32_t t = rk[i - 1];
    if (i % NK == 0) {
      t = aes_sub_word_t(T, (t >> 8) | (t << 24)) ^ rcon;
      rcon = aes_xtime(rcon);
    } else if (NK == 8 && i % 8 == 4) {
      t = aes_sub_word_t(T, t);
    }
    rk[i] = rk[i - NK] ^ t;
  }
}
template <int NK, class TL>
JX_HD void aes_encrypt_t_nk(const TL& T, const uint32_t* rk, const uint32_t in[4], uint32_t out[4]) {
  constexpr int NR = NK + 6;
  uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
#pragma unroll
  for (int r = 1; r < NR; r++) {
    const uint32_t t0 = T(s0 & 0xffu) ^ rotl32(T((s1 >> 8) & 0xffu), 8) ^ rotl32(T((s2 >> 16) & 0xffu), 16) ^
                        rotl32(T(s3 >> 24), 24) ^ rk[4 * r];
    const uint32_t t1 = T(s1 & 0xffu) ^ rotl32(T((s2 >> 8) & 0xffu), 8) ^ rotl32(T((s3 >> 16) & 0xffu), 16) ^
                        rotl32(T(s0 >> 24), 24) ^ rk[4 * r + 1];
    const uint32_t t2 = T(s2 & 0xffu) ^ rotl32(T((s3 >> 8) & 0xffu), 8) ^ rotl32(T((s0 >> 16) & 0xffu), 16) ^
                        rotl32(T(s1 >> 24), 24) ^ rk[4 * r + 2];
    const uint32_t t3 = T(s3 & 0xffu) ^ rotl32(T((s0 >> 8) & 0xffu), 8) ^ rotl32(T((s1 >> 16) & 0xffu), 16) ^
                        rotl32(T(s2 >> 24), 24) ^ rk[4 * r + 3];
    s0 = t0;
    s1 = t1;
    s2 = t2;
    s3 = t3;
  }
  // last round: SubBytes + ShiftRows only; S[x] is byte 1 of T0[x]
  out[0] = (((T(s0 & 0xffu) >> 8) & 0xffu) | (T((s1 >> 8) & 0xffu) & 0xff00u) |
            ((T((s2 >> 16) & 0xffu) & 0xff00u) << 8) | ((T(s3 >> 24) & 0xff00u) << 16)) ^ rk[4 * NR];
  out[1] = (((T(s1 & 0xffu) >> 8) & 0xffu) | (T((s2 >> 8) & 0xffu) & 0xff00u) |
            ((T((s3 >> 16) & 0xffu) & 0xff00u) << 8) | ((T(s0 >> 24) & 0xff00u) << 16)) ^ rk[4 * NR + 1];
  out[2] = (((T(s2 & 0xffu) >> 8) & 0xffu) | (T((s3 >> 8) & 0xffu) & 0xff00u) |
            ((T((s0 >> 16) & 0xffu) & 0xff00u) << 8) | ((T(s1 >> 24) & 0xff00u) << 16)) ^ rk[4 * NR + 2];
  out[3] = (((T(s3 & 0xffu) >> 8) & 0xffu) | (T((s0 >> 8) & 0xffu) & 0xff00u) |
            ((T((s1 >> 16) & 0xffu) & 0xff00u) << 8) | ((T(s2 >> 24) & 0xff00u) << 16)) ^ rk[4 * NR + 3];
}

}  // namespace jx
