// jx_sample.h — rejection sampling of field elements from a TurboSHAKE128 stream, as the XOF kernels of
// jx_kernels.hip inline it: an encoding >= p is skipped and the stream moves on (VDAF-08 §6.2.1 next_vec).
// A rejection is a 2^-32 event per Field64 element and a 2^-59 one per Field128 element, so this header also
// builds for the host, where tests/csrc/hosttest.cpp runs it on hand-built Keccak states
// (tests/test_device_math_host.py). xof_stream128, at the end, is the sampler of Prio3.shard's streams
// (jx_shard.hip). The exact ">= p" predicates on f128 / word pairs, ge_p128 / ge_p64, are in jx_field.h; the one
// on an explicit element as loaded (uint4), ge_exact, is here.
#pragma once
#include <stdint.h>

#include "jx_field.h"
#include "jx_flags.h"
#include "jx_keccak.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JX_DEV __device__
#define JX_DEVI __device__ __forceinline__
#else
#define JX_DEV static inline
#define JX_DEVI static inline
#endif

namespace jx {

#if !(defined(__HIPCC__) || defined(__HIP__))
struct uint4 {  // HIP's, for the host build
  uint32_t x, y, z, w;
};
#endif

// first N accepted Field64 samples from a stream whose first block is in S
template <int N>
JX_DEV void sample64(uint32_t* S, uint64_t out[N]) {
  int cnt = 0;
#pragma unroll 1
  for (int guard = 0; guard < 64; guard++) {
#pragma unroll
    for (int ci = 0; ci < 21; ci++) {
      uint64_t x = (uint64_t)S[2 * ci] | ((uint64_t)S[2 * ci + 1] << 32);
      bool acc = x < P64;
#pragma unroll
      for (int i = 0; i < N; i++)
        if (acc && cnt == i) out[i] = x;
      cnt += acc ? 1 : 0;
    }
    if (cnt >= N) break;
    keccak_p12(S);
  }
}

// Conservative ">= p" screen for a sampled Field128 element: true for every x >= p (and for
// the 2^-59-probable x in [2^128 - 2^69, p), which the slow kernel then redoes exactly).
// Tracked as a running max so that one compare per block decides.
JX_DEVI uint32_t ge_screen(uint4 v) { return v.w & (v.z | 0x1Fu); }

// Exact ">= p" test (decoding an explicit Field128 element, VDAF-08 decode rejects x >= p).
JX_DEVI bool ge_exact(uint4 v) {
  return v.w == 0xFFFFFFFFu && (v.z > 0xFFFFFFE4u || (v.z == 0xFFFFFFE4u && (v.x | v.y) != 0u));
}

// `cnt` (<= 2) Field128 samples from an XOF stream whose first block is in S. Fast path: the first
// two 16-byte chunks, FLAG_SLOW if one is >= p; slow path: rejection sampling (a rejection stays in
// the first block except with probability ~2^-600, beyond which chunks straddling blocks are skipped).
// Every index is static (the chunks are unrolled and a sample lands in out[0] / out[1] by select), so
// the state and the samples stay in registers: a data-dependent index would put both in scratch.
JX_DEVI void sample2_f128(uint32_t* S, f128 out[2], uint32_t cnt, bool slow, uint32_t& flags) {
  if (!slow) {
    out[0] = w4_to_f(S[0], S[1], S[2], S[3]);
    out[1] = w4_to_f(S[4], S[5], S[6], S[7]);
    if (ge_p128(out[0]) || (cnt > 1 && ge_p128(out[1]))) flags |= FLAG_SLOW;
    return;
  }
  f128 o0 = make128(0, 0), o1 = make128(0, 0);
  uint32_t k = 0;
  for (int guard = 0; guard < 64 && k < cnt; guard++) {
#pragma unroll
    for (int ci = 0; ci < 10; ci++) {
      const f128 v = w4_to_f(S[4 * ci], S[4 * ci + 1], S[4 * ci + 2], S[4 * ci + 3]);
      const bool take = k < cnt && !ge_p128(v);
      if (take && k == 0) o0 = v;
      if (take && k == 1) o1 = v;
      k += take ? 1u : 0u;
    }
    if (k < cnt) keccak_p12(S);
  }
  out[0] = o0;
  out[1] = o1;
}

// The slow XOF path's byte stream: rejection sampling at any position
struct ByteXof {
  uint32_t s[50];
  uint32_t pos;
};
JX_DEV uint32_t bx_byte(ByteXof& x) {
  if (x.pos == 168) {
    keccak_p12(x.s);
    x.pos = 0;
  }
  uint32_t v = (x.s[x.pos >> 2] >> (8 * (x.pos & 3))) & 0xffu;
  x.pos++;
  return v;
}
JX_DEV f128 bx_elem128(ByteXof& x) {
  uint32_t w[4];
  for (int i = 0; i < 4; i++) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= bx_byte(x) << (8 * k);
    w[i] = v;
  }
  return w4_to_f(w[0], w[1], w[2], w[3]);
}
JX_DEV f128 bx_sample128(ByteXof& x) {
  for (;;) {
    f128 v = bx_elem128(x);
    if (!ge_p128(v)) return v;
  }
}

// XOF.next_vec for Field128: emit(k, v) for the first n accepted 16-byte chunks of the stream whose first block
// is in S. 21 chunks span two blocks (the eleventh straddles them), so every state index is static.
template <class Emit>
JX_DEVI void xof_stream128(uint32_t* S, uint32_t n, Emit emit) {
  uint32_t k = 0;
  auto take = [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) __attribute__((always_inline)) {
    const f128 v = w4_to_f(w0, w1, w2, w3);
    if (k < n && !ge_p128(v)) {
      emit(k, v);
      k++;
    }
  };
#pragma unroll 1
  while (k < n) {
#pragma unroll
    for (int ci = 0; ci < 10; ci++) take(S[4 * ci], S[4 * ci + 1], S[4 * ci + 2], S[4 * ci + 3]);
    if (k >= n) break;
    const uint32_t c0 = S[40], c1 = S[41];
    keccak_p12(S);
    take(c0, c1, S[0], S[1]);
#pragma unroll
    for (int ci = 0; ci < 10; ci++) take(S[2 + 4 * ci], S[3 + 4 * ci], S[4 + 4 * ci], S[5 + 4 * ci]);
    if (k < n) keccak_p12(S);
  }
}

}  // namespace jx

#undef JX_DEV
#undef JX_DEVI
