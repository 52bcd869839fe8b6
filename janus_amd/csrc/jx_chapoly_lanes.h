// jx_chapoly_lanes.h — ChaCha20-Poly1305 of one long message split over the 64 lanes of a wave (jx_hpke_long.hip):
// Poly1305 as 64 Horner chains in r^64, and the lane -> keystream block map of the decryption. __host__ __device__:
// tests/csrc/hosttest_chapoly_lanes.cpp runs the same code on the CPU, one loop iteration per lane.
//
// The AEAD's MAC input is aad || pad16 || ct || pad16 || le64(alen) || le64(clen): N = ceil(alen / 16) +
// ceil(clen / 16) + 1 blocks of 16 bytes, the length block being block N - 1, an ordinary last block. Every block
// carries the 2^128 bit (chapoly_tag_ok of jx_chapoly.h passes hibit = 1 throughout). With c_k the block values,
//   h = sum_k c_k r^(N - k)  mod 2^130 - 5.
// Lane j owns blocks j, j + 64, ...: with n_j of them its last one is k_j = j + 64 (n_j - 1), and Horner in r^64 gives
//   P_j = c_j (r^64)^(n_j - 1) + c_(j+64) (r^64)^(n_j - 2) + ... + c_(k_j),
// so h = sum_j P_j r^(d_j) with d_j = N - k_j = gl_lane_exponent(N, j) in [1, 64] (jx_ghash_lanes.h, whose lane
// arithmetic and doubling steps are used unchanged). A lane without blocks contributes zero. The tag is
// poly1305_finish of the sum: the full reduction, then + s mod 2^128.
//
// Limbs. Values mod 2^130 - 5 are five 26-bit limbs, as in jx_chapoly.h. Two ranges occur:
//   carried: every limb < 2^26 + 2^10    (what pl_mul returns; the clamped r is carried too)
//   loose:   every limb < 2^27           (a carried value plus one block: what pl_mul accepts as the accumulator)
// pl_mul accepts a loose accumulator and any multiplier with limbs < PL_MUL_MAX = 2^26 + 2^25, so 5 m < 2^29 and a
// column of five products stays under 5 * 2^27 * 2^29 < 2^59 (the column bound of jx_chapoly.h). The powers of r are
// products, not clamped values: they are carried, which is well inside that range.
#pragma once
#include "jx_chapoly.h"
#include "jx_ghash_lanes.h"

namespace jx {

constexpr uint32_t PL_M26 = 0x3ffffffu;
constexpr uint32_t PL_MUL_MAX = (1u << 26) + (1u << 25);  // exclusive bound of a multiplier's limbs

// The block m (16 bytes as 4 little-endian words) + 2^128 in limbs: c[0..3] < 2^26, c[4] < 2^25.
JX_HD void pl_block_limbs(const uint32_t m[4], uint32_t c[5]) {
  c[0] = m[0] & PL_M26;
  c[1] = ((m[0] >> 26) | (m[1] << 6)) & PL_M26;
  c[2] = ((m[1] >> 20) | (m[2] << 12)) & PL_M26;
  c[3] = ((m[2] >> 14) | (m[3] << 18)) & PL_M26;
  c[4] = (m[3] >> 8) | (1u << 24);
}

// h = h m mod 2^130 - 5, partially reduced. In: h loose (limbs < 2^27), m limbs < PL_MUL_MAX. Out: h carried:
// h[0], h[2], h[3], h[4] < 2^26 and h[1] < 2^26 + 2^10. (d4 < 5 * 2^56 + 2^33, so 5 (d4 >> 26) < 2^35 and the
// carry out of limb 0 is < 2^9 + 1.) The same columns and carry pass as poly1305_block.
JX_HD void pl_mul(uint32_t h[5], const uint32_t m[5]) {
  const uint64_t h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4];
  const uint64_t r0 = m[0], r1 = m[1], r2 = m[2], r3 = m[3], r4 = m[4];
  const uint64_t s1 = 5 * r1, s2 = 5 * r2, s3 = 5 * r3, s4 = 5 * r4;  // 2^130 == 5; each < 2^29
  uint64_t d0 = h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
  uint64_t d1 = h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
  uint64_t d2 = h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
  uint64_t d3 = h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
  uint64_t d4 = h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  const uint64_t c0 = (d0 & PL_M26) + 5 * (d4 >> 26);
  h[0] = (uint32_t)(c0 & PL_M26);
  h[1] = (uint32_t)((d1 & PL_M26) + (c0 >> 26));
  h[2] = (uint32_t)(d2 & PL_M26);
  h[3] = (uint32_t)(d3 & PL_M26);
  h[4] = (uint32_t)(d4 & PL_M26);
}

// Lane j's Horner partial P_j over its blocks of N. Block: (k, uint32_t m[4]) -> block k as 4 little-endian words,
// zero padded (the 2^128 bit is added here). r64: r^64, carried. Out: p loose (a carried product plus the last
// block), or all zero for a lane without blocks.
template <class Block>
JX_HD void pl_lane_partial(uint64_t N, uint32_t j, Block block, const uint32_t r64[5], uint32_t p[5]) {
  p[0] = p[1] = p[2] = p[3] = p[4] = 0;
  for (uint64_t k = j; k < N; k += GL_LANES) {
    if (k != j) pl_mul(p, r64);
    uint32_t m[4], c[5];
    block(k, m);
    pl_block_limbs(m, c);
#pragma unroll
    for (int i = 0; i < 5; i++) p[i] += c[i];  // < 2^26 + 2^10 + 2^26 < 2^27
  }
}

// Lane j's term P_j r^(d_j), ready for the sum over the wave. In: p loose, rd carried (the value is not used by a
// lane without blocks, whose p is zero). Out: every limb < 2^26 exactly (pl_mul, then the two carry passes of
// poly1305_carry), so that 64 of them add up to at most 64 (2^26 - 1) = 2^32 - 64 per limb: the wave sums the
// terms limb-wise in plain 32-bit words, in any order, and cannot overflow.
JX_HD void pl_lane_term(uint32_t p[5], const uint32_t rd[5]) {
  pl_mul(p, rd);
  Poly1305 t;
#pragma unroll
  for (int i = 0; i < 5; i++) t.h[i] = p[i];
  poly1305_carry(t);
#pragma unroll
  for (int i = 0; i < 5; i++) p[i] = t.h[i];
}

// The tag from the limb-wise sum of the 64 terms. In: sum limbs <= 2^32 - 64. The carry pass runs in 64 bits
// (a limb plus the carry from below may pass 2^32); what leaves limb 4 is at most 64 and comes back as 5 * 64
// into limb 0, so poly1305_finish gets limbs < 2^26 + 2^9, inside the < 2^27 its carry passes accept.
// st: r and s of the one-time key (poly1305_init); its accumulator is overwritten.
JX_HD void pl_finish(Poly1305& st, const uint32_t sum[5], uint32_t tag[4]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    c += sum[i];
    st.h[i] = (uint32_t)(c & PL_M26);
    c >>= 26;
  }
  st.h[0] += 5 * (uint32_t)c;
  poly1305_finish(st, tag);
}

// How many MAC blocks the AEAD input has, the length block included
JX_HD uint64_t pl_mac_blocks(uint64_t alen, uint64_t clen) { return (alen + 15) / 16 + (clen + 15) / 16 + 1; }
// The length block as 4 little-endian words
JX_HD void pl_len_block(uint64_t alen, uint64_t clen, uint32_t m[4]) {
  m[0] = (uint32_t)alen;
  m[1] = (uint32_t)(alen >> 32);
  m[2] = (uint32_t)clen;
  m[3] = (uint32_t)(clen >> 32);
}

// ---- ChaCha20 over the wave: one 64-byte keystream block per lane and stride. Lane j decrypts blocks j, j + 64, ...
// of the cl_blocks(clen) blocks; block b is keystream block counter 1 + b and bytes [64 b, 64 b + 64) of the
// ciphertext, moved as four 16-byte pieces q = 0..3 with the last block's pieces clipped to the ciphertext's end.
// (The counter stays below 2^32: the entry points refuse ciphertexts of 2^32 bytes.)
JX_HD uint64_t cl_blocks(uint64_t clen) { return (clen + 63) / 64; }
JX_HD uint32_t cl_counter(uint64_t b) { return (uint32_t)(1 + b); }
JX_HD uint64_t cl_piece_offset(uint64_t b, uint32_t q) { return 64 * b + 16 * q; }
// bytes of piece q of block b that lie inside the ciphertext: 0..16
JX_HD uint32_t cl_piece_len(uint64_t clen, uint64_t b, uint32_t q) {
  const uint64_t o = cl_piece_offset(b, q);
  return o >= clen ? 0u : (clen - o < 16 ? (uint32_t)(clen - o) : 16u);
}

}  // namespace jx
