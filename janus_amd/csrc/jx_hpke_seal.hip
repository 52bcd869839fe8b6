// jx_hpke_seal.hip — HPKE seal on the GPU (jx_hpke_seal_batch / _long_batch of include/jx_hpke.h) and the client's
// second half built on it (jx_client_seal_* of include/jx_prio3.h): the two hpke::seal calls of the reference
// client's prepare_report (client/src/lib.rs:339-383; core/src/hpke.rs:167). jx_hpke_seal.h has the algorithm and the
// serial pieces.
//
//  A. hpke_seal_ctx_kernel / client_seal_ctx_kernel, one lane per (seal, point): lane 2s runs X25519(skE, 9), lane
//     2s + 1 runs X25519(skE, pkR); the pair exchanges the results by __shfl_xor(.., 1) and the even lane runs
//     ExtractAndExpand and the suite's key schedule, so a seal's chain is one ladder long, as an open's is. The
//     recipient key and its key_schedule_context are read from the device's key registry by slot. The short form
//     (payloads such as the helper's 54-byte plaintext) seals in that same lane, with no second launch; the long
//     form leaves a LongCtxRow per seal.
//  B. hpke_seal_long_kernel / client_seal_long_kernel, one wave per seal, four waves per workgroup sharing the LDS
//     AES T-table: the shape of hpke_long_open_kernel with the order reversed. A lane encrypts its CTR blocks
//     (AES-GCM: counter block k to the lane that owns GHASH block na + k) or its ChaCha20 blocks (and owns the four
//     Poly1305 blocks of each: sl_lane_partial of jx_hpke_seal.h) and folds what it has just made into its MAC
//     partial in the same pass. Plaintext and associated data come through loader functors.
#include <hip/hip_runtime.h>

#include "jx_hpke_long.h"
#include "jx_hpke_seal.h"

namespace jx {
namespace {

__device__ __forceinline__ void load_words8(const uint8_t* p, uint32_t w[8]) {
  for (int i = 0; i < 8; i++)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
           ((uint32_t)p[4 * i + 3] << 24);
}
__device__ __forceinline__ void store_words8(uint8_t* p, const uint32_t w[8]) {
  for (int i = 0; i < 32; i++) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// Both lanes of a pair call this together (t: the lane's parity). The ephemeral key at skp is clamped here. The
// even lane gets enc and, in kb / nb, the AEAD key and base nonce, and returns whether the DH output was non-zero;
// the odd lane returns false. The point is chosen by the lane's parity alone, and the scalar reaches nothing but
// x25519_ladder.
__device__ __forceinline__ bool seal_pair_context(const HpkeKeyRow& key, const uint8_t* skp, uint32_t t,
                                                  const uint32_t zist[8], const uint32_t zost[8], uint32_t enc[8],
                                                  uint8_t kb[32], uint8_t nb[12]) {
  uint32_t k[8], u[8], dh[8];
  load_words8(skp, k);
  x25519_clamp(k);
  x25519_base_point(u);
  if (t)
    for (int i = 0; i < 8; i++) u[i] = key.pk[i];
  x25519_ladder(enc, k, u);
  for (int i = 0; i < 8; i++) dh[i] = __shfl_xor(enc[i], 1);
  if (t) return false;
  return hpke_seal_context(enc, dh, key.pk, key.ksc, key.kdf, key.aead, zist, zost, kb, nb);
}

// byte i of the InputShareAad (messages/src/lib.rs:1854-1858) of report r
__device__ __forceinline__ uint8_t client_aad_byte(const ClientSealArgs& a, uint64_t r, uint64_t time, uint64_t i) {
  if (i < 32) return a.task_id[i];
  if (i < 48) return a.ids[16 * r + (i - 32)];
  if (i < 56) return (uint8_t)(time >> (8 * (55 - i)));
  if (i < 60) return (uint8_t)(a.ps_bytes >> (8 * (59 - i)));
  return a.ps[(uint64_t)a.ps_bytes * r + (i - 60)];
}
// byte i of PlaintextInputShare (messages/src/lib.rs:1323-1326) with no extensions: u16 0 || u32 len || payload
__device__ __forceinline__ uint8_t plaintext_share_byte(const uint8_t* payload, uint32_t len, uint64_t i) {
  if (i < 2) return 0;
  if (i < 6) return (uint8_t)(len >> (8 * (5 - i)));
  return payload[i - 6];
}

template <bool SHORT>
__global__ __launch_bounds__(64) void hpke_seal_ctx_kernel(SealArgs a) {
  __shared__ uint8_t sbox[256];
  if (SHORT) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
    __syncthreads();
  }
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * a.n) return;  // (both lanes of a pair, or neither)
  const uint64_t r = idx >> 1;
  const uint32_t t = (uint32_t)(idx & 1);
  const HpkeKeyRow& key = a.keys[a.slot];
  uint32_t enc[8];
  uint8_t kb[32], nb[12];
  const bool nz = seal_pair_context(key, a.sks + 32 * r, t, a.zero_ist, a.zero_ost, enc, kb, nb);
  if (t) return;
  if (!nz)
    for (int i = 0; i < 8; i++) enc[i] = 0;
  store_words8(a.encs + 32 * r, enc);
  if constexpr (SHORT) {
    const uint64_t p0 = a.pt_off[r], p1 = a.pt_off[r + 1];
    const uint64_t a0 = a.aad_off[r], a1 = a.aad_off[r + 1];
    // (offsets the host entry refuses; the device entry cannot read them, so the kernel fails that seal)
    const bool fits = p1 >= p0 && a1 >= a0 && p1 - p0 < (1ull << 32) - 16;
    if (fits) {
      const uint8_t* pt = a.pts + p0;
      const uint8_t* aad = a.aads + a0;
      uint8_t* ct = a.cts + p0 + 16 * r;
      if (nz)
        suite_aead_seal(sbox, key.aead, kb, nb, a1 - a0, [&](uint64_t i) { return aad[i]; }, p1 - p0,
                        [&](uint64_t i) { return pt[i]; }, ct);
      else
        for (uint64_t i = 0; i < p1 - p0 + 16; i++) ct[i] = 0;
    }
    a.ok[r] = (uint8_t)(nz && fits);
  } else {
    write_ctx(reinterpret_cast<LongCtxRow*>(a.ctx)[r], key.aead, kb, nb, nz);
  }
}

// the bytes of a 16-byte block past len, cleared
__device__ __forceinline__ void mask16(uint32_t w[4], uint32_t len) {
  if (len < 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t nb = len > 4u * i ? len - 4u * i : 0u;
      w[i] &= nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
    }
  }
}

// AES-GCM seal by the whole wave. pt_ld / aad_ld(o, len, x): len (1..16) bytes from offset o (a multiple of 16) as 4
// little-endian words, zero padded. ct gets plen + 16 bytes, at any alignment.
template <int NK, class AadLd, class PtLd>
__device__ void gcm_wave_seal(const uint32_t* tt, uint32_t* m4, uint32_t lane, const LongCtxRow& c, AadLd aad_ld,
                              uint64_t alen, PtLd pt_ld, uint64_t plen, uint8_t* ct) {
  const uint32_t* tl = tt + (lane & 31u);
  auto T = [tl](uint32_t x) { return tl[x << 5]; };
  uint32_t rk[4 * (NK + 7)], h[4], pw[4];
  gcm_wave_setup<NK>(T, m4, lane, c.kw, rk, h, pw);
  const uint4* m4v = reinterpret_cast<const uint4*>(m4);
  auto M = [m4v](uint32_t n, uint32_t e[4]) {
    const uint4 v = m4v[n];
    e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
  };
  const uint64_t na = (alen + 15) / 16, nc = (plen + 15) / 16, N = na + nc;
  // counter blocks: nonce (12 bytes) || BE32 counter; J0 has counter 1, data block k counter 2 + k
  uint32_t cb[4] = {c.nw[0], c.nw[1], c.nw[2], 0}, ks[4];
  uint32_t p[4];
  gl_lane_partial(
      N, lane,
      [&](uint64_t k, uint32_t x[4]) {
        if (k < na) {
          const uint64_t o = 16 * k;
          aad_ld(o, alen - o < 16 ? (uint32_t)(alen - o) : 16u, x);
        } else {
          const uint64_t o = 16 * (k - na);
          const uint32_t len = plen - o < 16 ? (uint32_t)(plen - o) : 16u;
          pt_ld(o, len, x);
          cb[3] = bswap32((uint32_t)(2 + (k - na)));
          aes_encrypt_t_nk<NK>(T, rk, cb, ks);
          for (int w = 0; w < 4; w++) x[w] ^= ks[w];
          mask16(x, len);
          st16(ct + o, len, x);
        }
        for (int w = 0; w < 4; w++) x[w] = bswap32(x[w]);
      },
      M, p);
  {
    const uint32_t d = gl_lane_exponent(N, lane);
    uint32_t hd[4];
    shfl4(hd, pw, d ? d - 1 : 0);  // (a lane without blocks holds p = 0)
    ghash_mul(p, hd);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 4; k++) p[k] ^= __shfl_xor(p[k], off);
  gl_finish(p, alen, plen, h);
  cb[3] = bswap32(1u);
  aes_encrypt_t_nk<NK>(T, rk, cb, ks);
  uint32_t tag[4];
  for (int k = 0; k < 4; k++) tag[k] = ks[k] ^ bswap32(p[k]);
  if (lane == 0) st16(ct + plen, 16, tag);
}

// ChaCha20-Poly1305 seal by the whole wave (sl_lane_partial of jx_hpke_seal.h). Every shuffle sits outside the
// per-lane block loops.
template <class AadLd, class PtLd>
__device__ void chapoly_wave_seal(uint32_t lane, const LongCtxRow& c, AadLd aad_ld, uint64_t alen, PtLd pt_ld,
                                  uint64_t plen, uint8_t* ct) {
  uint32_t ks[16];
  chacha20_block(c.kw, 0, c.nw, ks);  // every lane: the one-time key r || s is the first 32 bytes of block 0
  Poly1305 st;
  poly1305_init(st, ks);
  uint32_t pw[5], r64[5], rgap[5];
  poly_wave_powers(lane, st.r, pw);
  shfl5(r64, pw, 63);
  shfl5(rgap, pw, SL_GAP - 3 * GL_LANES - 1);  // r^61, then three times r^64: r^253
  for (int i = 0; i < 3; i++) pl_mul(rgap, r64);
  const uint64_t na = (alen + 15) / 16, nc = (plen + 15) / 16;
  uint32_t a0[5] = {0, 0, 0, 0, 0};
  if (na) {  // (the same in every lane) A, as the open's split makes it
    uint32_t pa[5], rd[5];
    pl_lane_partial(
        na, lane,
        [&](uint64_t k, uint32_t m[4]) {
          const uint64_t o = 16 * k;
          aad_ld(o, alen - o < 16 ? (uint32_t)(alen - o) : 16u, m);
        },
        r64, pa);
    const uint32_t d = gl_lane_exponent(na, lane);
    shfl5(rd, pw, d ? d - 1 : 0);
    pl_lane_term(pa, rd);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      for (int k = 0; k < 5; k++) pa[k] += __shfl_xor(pa[k], off);
    pl_sum_carry(pa, a0);
  }
  uint32_t p[5];
  const uint32_t d = sl_lane_partial(
      nc, lane,
      [&](uint64_t b) {
        if (64 * b < plen) chacha20_block(c.kw, cl_counter(b), c.nw, ks);
      },
      [&](uint64_t b, uint32_t q, uint32_t m[4]) {
        const uint64_t mi = 4 * b + q;
        if (mi == nc) {
          pl_len_block(alen, plen, m);
        } else {
          const uint64_t o = 16 * mi;
          const uint32_t len = plen - o < 16 ? (uint32_t)(plen - o) : 16u;
          pt_ld(o, len, m);
          for (int w = 0; w < 4; w++) m[w] ^= ks[4 * q + w];
          mask16(m, len);
          st16(ct + o, len, m);
        }
      },
      st.r, rgap, a0, p);
  {
    // r^d, d in [1, 253]: r^((d - 1) % 64 + 1) from its lane, times r^64 up to three times
    const uint32_t e = d ? d - 1 : 0;
    uint32_t rd[5];
    shfl5(rd, pw, e & (GL_LANES - 1));
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
      if (i < (e >> 6)) pl_mul(rd, r64);
    pl_lane_term(p, rd);  // (a lane without blocks holds p = 0)
  }
  // every limb < 2^26, so 64 of them fit a 32-bit word (pl_lane_term)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 5; k++) p[k] += __shfl_xor(p[k], off);
  uint32_t tag[4];
  pl_finish(st, p, tag);
  if (lane == 0) st16(ct + plen, 16, tag);
}

template <class AadLd, class PtLd>
__device__ __forceinline__ void aead_wave_seal(const uint32_t* tt, uint32_t* m4, uint32_t lane, const LongCtxRow& c,
                                               AadLd aad_ld, uint64_t alen, PtLd pt_ld, uint64_t plen, uint8_t* ct) {
  if (c.aead == HPKE_AEAD_AES128GCM)
    gcm_wave_seal<4>(tt, m4, lane, c, aad_ld, alen, pt_ld, plen, ct);
  else if (c.aead == HPKE_AEAD_AES256GCM)
    gcm_wave_seal<8>(tt, m4, lane, c, aad_ld, alen, pt_ld, plen, ct);
  else
    chapoly_wave_seal(lane, c, aad_ld, alen, pt_ld, plen, ct);
}

// n zero bytes at p, by the wave
__device__ __forceinline__ void wave_zero(uint8_t* p, uint64_t n, uint32_t lane) {
  const uint32_t z[4] = {0, 0, 0, 0};
  for (uint64_t o = 16ull * lane; o < n; o += 16 * GL_LANES) st16(p + o, n - o < 16 ? (uint32_t)(n - o) : 16u, z);
}

__global__ __launch_bounds__(64 * WAVES) void hpke_seal_long_kernel(SealArgs a) {
  __shared__ uint32_t tt[256 * 32];
  __shared__ __attribute__((aligned(16))) uint32_t m4[WAVES][64];
  fill_ttable(tt);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * WAVES + wave;
  if (r >= a.n) return;
  const LongCtxRow c = reinterpret_cast<const LongCtxRow*>(a.ctx)[r];
  const uint64_t p0 = a.pt_off[r], p1 = a.pt_off[r + 1];
  const uint64_t a0 = a.aad_off[r], a1 = a.aad_off[r + 1];
  // (a plaintext of 2^32 - 16 bytes or more is no report share: the host entry refuses it, this one fails it)
  const bool fits = p1 >= p0 && a1 >= a0 && p1 - p0 < (1ull << 32) - 16;
  if (fits) {
    const uint8_t* pt = a.pts + p0;
    const uint8_t* aad = a.aads + a0;
    uint8_t* ct = a.cts + p0 + 16 * r;
    if (c.ok)
      aead_wave_seal(
          tt, m4[wave], lane, c, [&](uint64_t o, uint32_t len, uint32_t x[4]) { ld16(aad + o, len, x); }, a1 - a0,
          [&](uint64_t o, uint32_t len, uint32_t x[4]) { ld16(pt + o, len, x); }, p1 - p0, ct);
    else
      wave_zero(ct, p1 - p0 + 16, lane);
  }
  if (lane == 0) a.ok[r] = (uint8_t)(c.ok != 0 && fits);
}

// ---------------------------------------------------------------------------- the client: both shares of a report

// Seal s of 2n: s < n the leader's share of report s (context only: client_seal_long_kernel seals it), s >= n the
// helper's share of report s - n, sealed here in the short form. So a wave holds seals of one kind, but for the one
// wave across the boundary. A report the shard refused is skipped by both lanes of its pairs.
__global__ __launch_bounds__(64) void client_seal_ctx_kernel(ClientSealArgs a) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 4 * a.n) return;  // (both lanes of a pair, or neither)
  const uint64_t s = idx >> 1;
  const uint32_t t = (uint32_t)(idx & 1);
  const bool helper = s >= a.n;
  const uint64_t r = helper ? s - a.n : s;
  LongCtxRow& row = reinterpret_cast<LongCtxRow*>(a.ctx)[s];
  uint8_t* enc_out = (helper ? a.helper_encs : a.leader_encs) + 32 * r;
  const uint64_t hct_len = 6ull + a.his_bytes + 16;
  uint8_t* hct = a.helper_cts + hct_len * r;
  uint32_t enc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint8_t kb[32] = {0}, nb[12] = {0};
  bool nz = false;
  const bool skip = a.shard_status && a.shard_status[r] != 0;
  const HpkeKeyRow& key = a.keys[helper ? a.slot_helper : a.slot_leader];
  if (!skip) {
    nz = seal_pair_context(key, a.sks + 64 * r + (helper ? 32 : 0), t, a.zero_ist, a.zero_ost, enc, kb, nb);
    if (!nz)
      for (int i = 0; i < 8; i++) enc[i] = 0;
  }
  if (t) return;
  store_words8(enc_out, enc);
  write_ctx(row, key.aead, kb, nb, nz);
  if (!helper) return;
  if (nz) {
    const uint64_t time = a.times[r];
    const uint8_t* his = a.his + (uint64_t)a.his_bytes * r;
    suite_aead_seal(sbox, key.aead, kb, nb, 60ull + a.ps_bytes,
                    [&](uint64_t i) { return client_aad_byte(a, r, time, i); }, 6ull + a.his_bytes,
                    [&](uint64_t i) { return plaintext_share_byte(his, a.his_bytes, i); }, hct);
  } else {
    for (uint64_t i = 0; i < hct_len; i++) hct[i] = 0;
  }
}

__global__ __launch_bounds__(64 * WAVES) void client_seal_long_kernel(ClientSealArgs a) {
  __shared__ uint32_t tt[256 * 32];
  __shared__ __attribute__((aligned(16))) uint32_t m4[WAVES][64];
  fill_ttable(tt);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * WAVES + wave;
  if (r >= a.n) return;
  const LongCtxRow* ctx = reinterpret_cast<const LongCtxRow*>(a.ctx);
  const LongCtxRow c = ctx[r];
  const uint64_t plen = 6ull + a.lis_bytes;
  uint8_t* ct = a.leader_cts + (plen + 16) * r;
  const bool skip = a.shard_status && a.shard_status[r] != 0;
  if (c.ok) {
    const uint64_t time = a.times[r];
    const uint8_t* lis = a.lis + a.lis_stride * r;
    auto aad_ld = [&](uint64_t o, uint32_t len, uint32_t x[4]) {
      x[0] = x[1] = x[2] = x[3] = 0;
      for (uint32_t k = 0; k < len; k++) x[k >> 2] |= (uint32_t)client_aad_byte(a, r, time, o + k) << (8 * (k & 3));
    };
    // the share's header and its first ten bytes a byte at a time; from offset 16 on, the row read in place
    auto pt_ld = [&](uint64_t o, uint32_t len, uint32_t x[4]) {
      if (o >= 16) {
        ld16(lis + (o - 6), len, x);
      } else {
        x[0] = x[1] = x[2] = x[3] = 0;
        for (uint32_t k = 0; k < len; k++)
          x[k >> 2] |= (uint32_t)plaintext_share_byte(lis, a.lis_bytes, k) << (8 * (k & 3));
      }
    };
    aead_wave_seal(tt, m4[wave], lane, c, aad_ld, 60ull + a.ps_bytes, pt_ld, plen, ct);
  } else {
    wave_zero(ct, plen + 16, lane);
  }
  if (lane == 0)
    a.status[r] = (uint8_t)(skip ? JX_SEAL_SKIPPED : (c.ok && ctx[a.n + r].ok) ? JX_SEAL_OK : JX_SEAL_ZERO_DH);
}

}  // namespace

hipError_t launch_hpke_seal(const SealArgs& a, bool long_form, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const dim3 g((uint32_t)((2 * a.n + 63) / 64));
  if (!long_form) {
    hipLaunchKernelGGL(hpke_seal_ctx_kernel<true>, g, dim3(64), 0, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(hpke_seal_ctx_kernel<false>, g, dim3(64), 0, s, a);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(hpke_seal_long_kernel, dim3((uint32_t)((a.n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_client_seal(const ClientSealArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(client_seal_ctx_kernel, dim3((uint32_t)((4 * a.n + 63) / 64)), dim3(64), 0, s, a);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(client_seal_long_kernel, dim3((uint32_t)((a.n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, a);
  return hipGetLastError();
}

}  // namespace jx
