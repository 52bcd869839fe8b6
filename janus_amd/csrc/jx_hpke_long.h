// jx_hpke_long.h — what jx_hpke_long.hip (the wave-per-report open of long payloads) shares with the unit that
// holds the C ABI (jx_hpke.hip).
#pragma once
#include "jx_chapoly_lanes.h"
#include "jx_ghash_lanes.h"
#include "jx_hpke_open.h"
#include "jx_keyreg.h"

namespace jx {

// What stage A leaves for stage B, one row per report: the AEAD's key and base nonce as little-endian words (Nk
// bytes of key, the rest zero), its id, and whether the KEM gave a usable secret (DH output non-zero / the
// encapsulated key a point of the curve).
struct LongCtxRow {
  uint32_t kw[8];
  uint32_t nw[3];
  uint32_t aead;
  uint32_t ok;
  uint32_t pad[3];
};
static_assert(sizeof(LongCtxRow) == 64, "LongCtxRow layout");

struct LongCtxArgs {
  uint64_t n;
  const HpkeKeyRow* keys;  // the device's key registry
  uint32_t slot;           // the recipient key's row
  const uint8_t* encs;     // n x 32 (X25519) or n x 65 (P-256)
  LongCtxRow* out;
  uint32_t zero_ist[8], zero_ost[8];  // HMAC-SHA256 pads of the empty salt
};

// Both stages on `s`: the context kernel of the key's KEM, then the open. b.n == ca.n.
hipError_t launch_hpke_long_open(const LongCtxArgs& ca, bool p256, const HpkeBufs& b, hipStream_t s);

#ifdef __HIPCC__
// ---- device code the wave-per-report kernels share: the open's (jx_hpke_long.hip) and the seal's
// (jx_hpke_seal.hip). Internal linkage: each unit instantiates its own.
namespace {

constexpr uint32_t WAVES = 4;  // per workgroup

__device__ __forceinline__ void write_ctx(LongCtxRow& o, uint32_t aead, const uint8_t kb[32], const uint8_t nb[12],
                                          bool ok) {
  for (int i = 0; i < 8; i++)
    o.kw[i] = (uint32_t)kb[4 * i] | ((uint32_t)kb[4 * i + 1] << 8) | ((uint32_t)kb[4 * i + 2] << 16) |
              ((uint32_t)kb[4 * i + 3] << 24);
  for (int i = 0; i < 3; i++)
    o.nw[i] = (uint32_t)nb[4 * i] | ((uint32_t)nb[4 * i + 1] << 8) | ((uint32_t)nb[4 * i + 2] << 16) |
              ((uint32_t)nb[4 * i + 3] << 24);
  o.aead = aead;
  o.ok = ok ? 1u : 0u;
  o.pad[0] = o.pad[1] = o.pad[2] = 0;
}

// len (1..16) bytes at p as 4 little-endian words, zero padded: the aligned 16 bytes that hold p[0] and, when the
// block goes past them, the next aligned 16 (which then hold p[len - 1]), so no load leaves the 16-byte lines of
// the block's own bytes
__device__ __forceinline__ void ld16(const uint8_t* p, uint32_t len, uint32_t w[4]) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t sh = (uint32_t)(a & 15);
  const uint4* q = reinterpret_cast<const uint4*>(a - sh);
  const uint4 lo = q[0];
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (sh + len > 16) hi = q[1];
  uint32_t v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y, v6 = hi.z, v7 = hi.w;
  if (sh & 8) {
    v0 = v2, v1 = v3, v2 = v4, v3 = v5, v4 = v6, v5 = v7;
  }
  if (sh & 4) {
    v0 = v1, v1 = v2, v2 = v3, v3 = v4, v4 = v5;
  }
  const uint32_t b = 8 * (sh & 3);
  w[0] = __funnelshift_r(v0, v1, b);
  w[1] = __funnelshift_r(v1, v2, b);
  w[2] = __funnelshift_r(v2, v3, b);
  w[3] = __funnelshift_r(v3, v4, b);
  if (len < 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t nb = len > 4u * i ? len - 4u * i : 0u;
      w[i] &= nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
    }
  }
}

__device__ __forceinline__ void st16(uint8_t* p, uint32_t len, const uint32_t w[4]) {
  const uintptr_t a = (uintptr_t)p;
  if (len == 16 && (a & 15) == 0) {
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else if (len == 16 && (a & 3) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = w[0], q[1] = w[1], q[2] = w[2], q[3] = w[3];
  } else {
    for (uint32_t j = 0; j < len; j++) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

__device__ __forceinline__ void shfl4(uint32_t out[4], const uint32_t in[4], uint32_t src) {
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = __shfl(in[k], (int)src);
}
__device__ __forceinline__ void shfl5(uint32_t out[5], const uint32_t in[5], uint32_t src) {
#pragma unroll
  for (int k = 0; k < 5; k++) out[k] = __shfl(in[k], (int)src);
}

__device__ __forceinline__ void fill_ttable(uint32_t* tt) {
  for (uint32_t i = threadIdx.x; i < 256 * 32; i += blockDim.x) tt[i] = aes_t0_entry(AES_SBOX[i >> 5]);
}

// What AES-GCM by the whole wave starts with, open or seal: the round keys, H = E(0) as 4 big-endian words, lane l's
// power H^(l+1) in pw, and the 4-bit table of H^64 in the wave's 16 x 4 words of LDS, m4. T: the T-table.
template <int NK, class TL>
__device__ __forceinline__ void gcm_wave_setup(const TL& T, uint32_t* m4, uint32_t lane, const uint32_t* kw,
                                               uint32_t* rk, uint32_t h[4], uint32_t pw[4]) {
  aes_expand_key_t<NK>(T, kw, rk);
  {
    const uint32_t zero4[4] = {0, 0, 0, 0};
    uint32_t hb[4];
    aes_encrypt_t_nk<NK>(T, rk, zero4, hb);
    for (int i = 0; i < 4; i++) h[i] = bswap32(hb[i]);
  }
  // lane l: H^(l+1), by doubling
  for (int k = 0; k < 4; k++) pw[k] = h[k];
#pragma unroll 1
  for (int s = 0; s < 6; s++) {
    uint32_t base[4], other[4];
    shfl4(base, pw, gl_pow_src_base(s));
    shfl4(other, pw, gl_pow_src_other(s, lane));
    ghash_mul(other, base);
    if (gl_pow_active(s, lane))
      for (int k = 0; k < 4; k++) pw[k] = other[k];
  }
  // the table of H^64 (lane 63's power): entry n by lane n
  {
    uint32_t h64[4], e[4];
    shfl4(h64, pw, 63);
    gl_tab4_entry(lane & 15u, h64, e);
    if (lane < 16) {
      uint4* dst = reinterpret_cast<uint4*>(m4) + lane;
      *dst = make_uint4(e[0], e[1], e[2], e[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// lane l: r^(l+1) of the Poly1305 key's r, by doubling (the steps of jx_ghash_lanes.h)
__device__ __forceinline__ void poly_wave_powers(uint32_t lane, const uint32_t r[5], uint32_t pw[5]) {
  for (int k = 0; k < 5; k++) pw[k] = r[k];
#pragma unroll 1
  for (int s = 0; s < 6; s++) {
    uint32_t base[5], other[5];
    shfl5(base, pw, gl_pow_src_base(s));
    shfl5(other, pw, gl_pow_src_other(s, lane));
    pl_mul(other, base);
    if (gl_pow_active(s, lane))
      for (int k = 0; k < 5; k++) pw[k] = other[k];
  }
}

}  // namespace
#endif  // __HIPCC__

}  // namespace jx
