// jx_chapoly.h — ChaCha20-Poly1305 (RFC 8439) open, one ciphertext per lane: HPKE AEAD 0x0003.
// __host__ __device__: tests/csrc/hosttest_hpke_suites.cpp runs the same code on the CPU.
//
//  * ChaCha20: the 20-round block function; key as 8 and nonce as 3 little-endian words.
//  * Poly1305: the accumulator and r in five 26-bit limbs, products in 64-bit columns (as fe_mul of jx_hpke.h:
//    limbs < 2^27 and 5 r < 2^29, so a column of five products stays under 2^59), one carry pass per block
//    and a full reduction mod 2^130 - 5 at the end, before s is added. Carries are plain 64-bit C++.
//  * The AEAD: the one-time Poly1305 key is the first 32 bytes of block 0; the MAC covers aad || pad16 || ct ||
//    pad16 || len(aad) || len(ct) (lengths as little-endian u64); the plaintext is ct ^ blocks 1, 2, ...
#pragma once
#include "jx_sha_aes.h"

namespace jx {

#define JX_CHACHA_QR(a, b, c, d) \
  a += b;                        \
  d = rotl32(d ^ a, 16);         \
  c += d;                        \
  b = rotl32(b ^ c, 12);         \
  a += b;                        \
  d = rotl32(d ^ a, 8);          \
  c += d;                        \
  b = rotl32(b ^ c, 7);

// RFC 8439 §2.3: out = 16 little-endian keystream words of block `counter`
JX_HD void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
  uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
  uint32_t x12 = counter, x13 = nonce[0], x14 = nonce[1], x15 = nonce[2];
#pragma unroll 1
  for (int i = 0; i < 10; i++) {
    JX_CHACHA_QR(x0, x4, x8, x12)
    JX_CHACHA_QR(x1, x5, x9, x13)
    JX_CHACHA_QR(x2, x6, x10, x14)
    JX_CHACHA_QR(x3, x7, x11, x15)
    JX_CHACHA_QR(x0, x5, x10, x15)
    JX_CHACHA_QR(x1, x6, x11, x12)
    JX_CHACHA_QR(x2, x7, x8, x13)
    JX_CHACHA_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + 0x61707865u;
  out[1] = x1 + 0x3320646eu;
  out[2] = x2 + 0x79622d32u;
  out[3] = x3 + 0x6b206574u;
  out[4] = x4 + key[0];
  out[5] = x5 + key[1];
  out[6] = x6 + key[2];
  out[7] = x7 + key[3];
  out[8] = x8 + key[4];
  out[9] = x9 + key[5];
  out[10] = x10 + key[6];
  out[11] = x11 + key[7];
  out[12] = x12 + counter;
  out[13] = x13 + nonce[0];
  out[14] = x14 + nonce[1];
  out[15] = x15 + nonce[2];
}
#undef JX_CHACHA_QR

struct Poly1305 {
  uint32_t r[5];  // clamped r, 26-bit limbs
  uint32_t h[5];  // accumulator, limbs < 2^26 + small between blocks
  uint32_t s[4];  // added to the reduced accumulator mod 2^128
};

// key: 32 bytes as 8 little-endian words (r || s); r is clamped (RFC 8439 §2.5.1)
JX_HD void poly1305_init(Poly1305& p, const uint32_t key[8]) {
  p.r[0] = key[0] & 0x3ffffffu;
  p.r[1] = ((key[0] >> 26) | (key[1] << 6)) & 0x3ffff03u;
  p.r[2] = ((key[1] >> 20) | (key[2] << 12)) & 0x3ffc0ffu;
  p.r[3] = ((key[2] >> 14) | (key[3] << 18)) & 0x3f03fffu;
  p.r[4] = (key[3] >> 8) & 0x00fffffu;
#pragma unroll
  for (int i = 0; i < 5; i++) p.h[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) p.s[i] = key[4 + i];
}

// h = (h + m + hibit 2^128) r mod 2^130 - 5, partially reduced. m: 16 bytes as 4 little-endian words; hibit is
// 1 for a full block (and for every block of the AEAD's padded input), 0 for a final partial block, whose
// 0x01 byte the caller has put into m.
JX_HD void poly1305_block(Poly1305& p, const uint32_t m[4], uint32_t hibit) {
  const uint32_t M = 0x3ffffffu;
  const uint64_t h0 = p.h[0] + (m[0] & M), h1 = p.h[1] + (((m[0] >> 26) | (m[1] << 6)) & M),
                 h2 = p.h[2] + (((m[1] >> 20) | (m[2] << 12)) & M), h3 = p.h[3] + (((m[2] >> 14) | (m[3] << 18)) & M),
                 h4 = p.h[4] + ((m[3] >> 8) | (hibit << 24));
  const uint64_t r0 = p.r[0], r1 = p.r[1], r2 = p.r[2], r3 = p.r[3], r4 = p.r[4];
  const uint64_t s1 = 5 * r1, s2 = 5 * r2, s3 = 5 * r3, s4 = 5 * r4;  // 2^130 == 5
  uint64_t d0 = h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
  uint64_t d1 = h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
  uint64_t d2 = h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
  uint64_t d3 = h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
  uint64_t d4 = h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  uint64_t c0 = (d0 & M) + 5 * (d4 >> 26);  // < 2^26 + 5 * 2^34
  p.h[0] = (uint32_t)(c0 & M);
  p.h[1] = (uint32_t)((d1 & M) + (c0 >> 26));
  p.h[2] = (uint32_t)(d2 & M);
  p.h[3] = (uint32_t)(d3 & M);
  p.h[4] = (uint32_t)(d4 & M);
}

// The accumulator fully carried: every limb < 2^26, the value < 2^130 (it may still be >= 2^130 - 5).
JX_HD void poly1305_carry(Poly1305& p) {
  const uint32_t M = 0x3ffffffu;
  // Two passes. The first leaves limbs 1..4 < 2^26 and limb 0 < 2^26 + 5 * 4 (the limbs come in < 2^27, so at
  // most 3 leaves limb 4): a value < 2^130 + 20. If the second pass carries out of limb 4 again, what stays is
  // < 20, and 5 more cannot carry.
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      p.h[i + 1] += p.h[i] >> 26;
      p.h[i] &= M;
    }
    p.h[0] += 5 * (p.h[4] >> 26);
    p.h[4] &= M;
  }
}

// tag = ((h mod 2^130 - 5) + s) mod 2^128, as 4 little-endian words
JX_HD void poly1305_finish(Poly1305& p, uint32_t tag[4]) {
  const uint32_t M = 0x3ffffffu;
  poly1305_carry(p);
  // g = h + 5 - 2^130: not negative exactly when h >= 2^130 - 5, and then g is h reduced
  uint32_t g[5], c = 5;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    g[i] = p.h[i] + c;
    c = g[i] >> 26;
    if (i < 4) g[i] &= M;
  }
  const uint32_t take_g = 0u - (g[4] >> 26);  // bit 130 of h + 5
  g[4] &= M;
  uint32_t h[5];
#pragma unroll
  for (int i = 0; i < 5; i++) h[i] = (p.h[i] & ~take_g) | (g[i] & take_g);
  const uint32_t w0 = h[0] | (h[1] << 26), w1 = (h[1] >> 6) | (h[2] << 20), w2 = (h[2] >> 12) | (h[3] << 14),
                 w3 = (h[3] >> 18) | (h[4] << 8);
  uint64_t f = (uint64_t)w0 + p.s[0];
  tag[0] = (uint32_t)f;
  f = (uint64_t)w1 + p.s[1] + (f >> 32);
  tag[1] = (uint32_t)f;
  f = (uint64_t)w2 + p.s[2] + (f >> 32);
  tag[2] = (uint32_t)f;
  f = (uint64_t)w3 + p.s[3] + (f >> 32);
  tag[3] = (uint32_t)f;
}

// Poly1305 of a byte message (RFC 8439 §2.5): full blocks, then a final partial block closed with 0x01.
// Byte: any callable i -> byte i of the message.
template <class Byte>
JX_HD void poly1305_absorb(Poly1305& p, uint64_t len, Byte byte) {
  for (uint64_t i = 0; i < len; i += 16) {
    uint32_t m[4] = {0, 0, 0, 0};
    const uint32_t n = len - i < 16 ? (uint32_t)(len - i) : 16u;
    for (uint32_t k = 0; k < n; k++) m[k >> 2] |= (uint32_t)byte(i + k) << (8 * (k & 3));
    if (n < 16) m[n >> 2] |= 1u << (8 * (n & 3));
    poly1305_block(p, m, n == 16);
  }
}
template <class Byte>
JX_HD void poly1305_mac(const uint32_t key[8], uint64_t len, Byte byte, uint32_t tag[4]) {
  Poly1305 p;
  poly1305_init(p, key);
  poly1305_absorb(p, len, byte);
  poly1305_finish(p, tag);
}

// 16 bytes of p[0, n) from offset i as 4 little-endian words, zero padded
JX_HD void ld_block_le(const uint8_t* p, uint64_t i, uint64_t n, uint32_t m[4]) {
#pragma unroll
  for (int w = 0; w < 4; w++) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t j = i + 4 * w + k;
      v |= (uint32_t)(j < n ? p[j] : 0) << (8 * k);
    }
    m[w] = v;
  }
}

// RFC 8439 §2.8 tag check of ct[0, clen) with tag ct[clen, clen + 16) under associated data of alen bytes
// (AadByte: i -> byte i). True when the tag matches.
template <class AadByte>
JX_HD bool chapoly_tag_ok(const uint32_t key[8], const uint32_t nonce[3], uint64_t alen, AadByte aad_byte,
                          const uint8_t* ct, uint64_t clen) {
  uint32_t ks[16];
  chacha20_block(key, 0, nonce, ks);
  Poly1305 p;
  poly1305_init(p, ks);
  for (uint64_t i = 0; i < alen; i += 16) {
    uint32_t m[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16 && i + k < alen; k++) m[k >> 2] |= (uint32_t)aad_byte(i + k) << (8 * (k & 3));
    poly1305_block(p, m, 1);
  }
  for (uint64_t i = 0; i < clen; i += 16) {
    uint32_t m[4];
    ld_block_le(ct, i, clen, m);
    poly1305_block(p, m, 1);
  }
  const uint32_t lens[4] = {(uint32_t)alen, (uint32_t)(alen >> 32), (uint32_t)clen, (uint32_t)(clen >> 32)};
  poly1305_block(p, lens, 1);
  uint32_t tag[4], want[4];
  poly1305_finish(p, tag);
  ld_block_le(ct + clen, 0, 16, want);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) diff |= tag[k] ^ want[k];
  return diff == 0;
}

// pt = ct ^ keystream of blocks 1, 2, ...
JX_HD void chapoly_decrypt(const uint32_t key[8], const uint32_t nonce[3], const uint8_t* ct, uint64_t clen,
                           uint8_t* pt) {
  for (uint64_t i = 0; i < clen; i += 64) {
    uint32_t ks[16];
    chacha20_block(key, (uint32_t)(1 + i / 64), nonce, ks);
    for (uint64_t j = 0; j < 64 && i + j < clen; j++) pt[i + j] = ct[i + j] ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3)));
  }
}

}  // namespace jx
