// jx_sha512.h — SHA-512 / SHA-384 (FIPS 180-4) and HMAC / hashing over byte messages, generic in the hash:
// the HKDF-SHA384 and HKDF-SHA512 key schedules of the HPKE suites beside the default one (jx_hpke_suites.h).
// __host__ __device__: tests/csrc/hosttest_hpke_suites.cpp runs the same code on the CPU against hashlib.
//
// Unlike the SHA-256 helpers of jx_sha_aes.h (messages of a fixed layout held in registers), messages here
// are byte arrays of any length: a LabeledExpand message with a 97- or 129-byte key_schedule_context does not
// fit one 128-byte block, and the host hashes an application info of any length with the same code.
#pragma once
#include "jx_sha_aes.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JX_HDM __host__ __device__ __forceinline__
#else
#define JX_HDM inline
#endif

namespace jx {

constexpr uint64_t SHA512_K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
constexpr uint64_t SHA512_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                   0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                   0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint64_t SHA384_IV[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                                   0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                                   0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};

JX_HD uint64_t ror64(uint64_t v, int n) { return (v >> n) | (v << (64 - n)); }

// One 128-byte block (16 big-endian words). The message schedule is a rolling window of 16 words: rounds go in
// five groups of 16, unrolled within a group so that every index into the window is a constant.
JX_HD void sha512_compress(uint64_t st[8], const uint64_t* blk) {
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = blk[i];
  uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
  for (int t = 0; t < 80; t += 16) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (t) {
        const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
        const uint64_t s0 = ror64(w15, 1) ^ ror64(w15, 8) ^ (w15 >> 7);
        const uint64_t s1 = ror64(w2, 19) ^ ror64(w2, 61) ^ (w2 >> 6);
        w[j] += s0 + w[(j + 9) & 15] + s1;
      }
      const uint64_t S1 = ror64(e, 14) ^ ror64(e, 18) ^ ror64(e, 41);
      const uint64_t ch = (e & f) ^ (~e & g);
      const uint64_t t1 = h + S1 + ch + SHA512_K[t + j] + w[j];
      const uint64_t S0 = ror64(a, 28) ^ ror64(a, 34) ^ ror64(a, 39);
      const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
      h = g;
      g = f;
      f = e;
      e = d + t1;
      d = c;
      c = b;
      b = a;
      a = t1 + S0 + mj;
    }
  }
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
  st[5] += f;
  st[6] += g;
  st[7] += h;
}

// The three hashes of the HPKE KDFs: word type, digest bytes NH, block bytes BLK.
struct HashSha256 {
  typedef uint32_t W;
  static constexpr uint32_t NH = 32, BLK = 64;
  JX_HDM static void init(W st[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = SHA256_IV[i];
  }
  JX_HDM static void compress(W st[8], const W* blk) { sha256_compress(st, blk); }
};
struct HashSha512 {
  typedef uint64_t W;
  static constexpr uint32_t NH = 64, BLK = 128;
  JX_HDM static void init(W st[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = SHA512_IV[i];
  }
  JX_HDM static void compress(W st[8], const W* blk) { sha512_compress(st, blk); }
};
struct HashSha384 {  // SHA-512 with its own initial state, truncated to 48 bytes
  typedef uint64_t W;
  static constexpr uint32_t NH = 48, BLK = 128;
  JX_HDM static void init(W st[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = SHA384_IV[i];
  }
  JX_HDM static void compress(W st[8], const W* blk) { sha512_compress(st, blk); }
};

// Finish a hash whose state st absorbed `prefix` bytes (a multiple of BLK) already: the message msg[0, len),
// the padding and the bit length of prefix + len, over as many blocks as that takes. out: NH digest bytes.
template <class H>
JX_HD void hash_finish(uint8_t* out, typename H::W st[8], uint64_t prefix, const uint8_t* msg, uint32_t len) {
  typedef typename H::W W;
  constexpr uint32_t WB = sizeof(W);
  const uint32_t nblk = (len + 1 + 2 * WB + H::BLK - 1) / H::BLK;
  const uint64_t bits = 8 * (prefix + len);
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; b++) {
    W blk[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      W v = 0;
#pragma unroll
      for (uint32_t k = 0; k < WB; k++) {
        const uint32_t pos = b * H::BLK + i * WB + k;
        v = (W)(v << 8) | (W)(pos < len ? msg[pos] : pos == len ? 0x80 : 0);
      }
      blk[i] = v;
    }
    if (b == nblk - 1) {  // the length field: 2 words, big-endian (the high word of SHA-512's is zero)
      blk[14] = WB == 4 ? (W)(bits >> 32) : (W)0;
      blk[15] = (W)bits;
    }
    H::compress(st, blk);
  }
  for (uint32_t i = 0; i < H::NH; i++) out[i] = (uint8_t)(st[i / WB] >> (8 * (WB - 1 - i % WB)));
}

template <class H>
JX_HD void hash_bytes(uint8_t* out, const uint8_t* msg, uint32_t len) {
  typename H::W st[8];
  H::init(st);
  hash_finish<H>(out, st, 0, msg, len);
}

// HMAC (RFC 2104) key pads for a key of klen <= BLK bytes. A longer key would have to be hashed first; the
// HKDF keys of the HPKE key schedule are a 32-byte shared secret, an Nh-byte (<= 64) secret or the empty salt,
// so that case does not exist here.
template <class H>
JX_HD void hmac_pads_t(const uint8_t* key, uint32_t klen, typename H::W ist[8], typename H::W ost[8]) {
  typedef typename H::W W;
  constexpr uint32_t WB = sizeof(W);
#pragma unroll 1
  for (int p = 0; p < 2; p++) {
    const uint32_t pad = p ? 0x5cu : 0x36u;
    W blk[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      W v = 0;
#pragma unroll
      for (uint32_t k = 0; k < WB; k++) {
        const uint32_t pos = i * WB + k;
        v = (W)(v << 8) | (W)((pos < klen ? key[pos] : 0u) ^ pad);
      }
      blk[i] = v;
    }
    W* st = p ? ost : ist;
    H::init(st);
    H::compress(st, blk);
  }
}
// HMAC of msg[0, len) from the pads: the inner hash, then the outer hash over the inner digest. out: NH bytes.
template <class H>
JX_HD void hmac_finish_t(uint8_t* out, const typename H::W ist[8], const typename H::W ost[8], const uint8_t* msg,
                         uint32_t len) {
  typename H::W st[8];
  uint8_t inner[H::NH];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = ist[i];
  hash_finish<H>(inner, st, H::BLK, msg, len);
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = ost[i];
  hash_finish<H>(out, st, H::BLK, inner, H::NH);
}

}  // namespace jx
