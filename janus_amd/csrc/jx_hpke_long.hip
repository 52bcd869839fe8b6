// jx_hpke_long.hip — HPKE open of long payloads, one wave per report (jx_hpke_open_long_batch[_device]), and the
// leader's upload path built on it (jx_leader_upload_open_*; the second half of this file).
//
// The kernels of jx_hpke_default / _suite / _p256.hip open one report per lane, which suits the helper's 48-byte
// shares. A leader input share is the whole measurement and proof share (135 KB for Prio3SumVec 8x1000/88): one
// lane would chain thousands of AES blocks and GHASH products, and neighbouring lanes would read addresses a whole
// share apart. Here the open is two launches:
//
//  A. hpke_long_ctx_*_kernel, one report per lane: the decapsulation and key schedule of the existing families,
//     unchanged (hpke_suite_context, hpke_p256_context of jx_hpke_suites.h), stopping before the AEAD. One
//     LongCtxRow per report goes to scratch: AEAD id, key, base nonce, and whether the DH output was non-zero /
//     the point valid. The recipient key is read from the device's key registry by its row index.
//  B. hpke_long_open_kernel, one wave per report, four waves per workgroup sharing one 32-copy AES T-table in
//     LDS (32 KiB). AES-GCM: lane j owns GHASH blocks j, j + 64, ... of AAD blocks || ciphertext blocks, Horner in
//     H^64 over a 4-bit table of H^64 in LDS (256 bytes per wave, every entry in banks of its own), then one
//     product by H^(d_j) (jx_ghash_lanes.h); the wave XORs the partials by __shfl_xor, adds the length block and
//     compares with E(J0) ^ tag. Only then CTR: lane j decrypts counter blocks 2 + j, 2 + j + 64, .... A block is
//     read as one or two aligned 16-byte loads and shifted into place, so a payload at any byte offset costs the
//     same loads; it is stored as 16 bytes, four words or bytes, as the output's alignment allows.
//     ChaCha20Poly1305 has the same shape (jx_chapoly_lanes.h): every lane derives the one-time key from keystream
//     block 0; lane j owns Poly1305 blocks j, j + 64, ... of AAD blocks || ciphertext blocks || the length block,
//     Horner in r^64 with a plain five-limb product (no table), then one product by r^(d_j); the wave adds the
//     partials limb-wise by __shfl_xor, finishes the tag and compares. Only then ChaCha20: lane j decrypts the
//     64-byte blocks j, j + 64, ... under counters 1 + j, 1 + j + 64, ..., each as four 16-byte pieces.
#include <hip/hip_runtime.h>

#include "jx_chapoly_lanes.h"
#include "jx_ghash_lanes.h"
#include "jx_hpke_long.h"
#include "jx_hpke_suites.h"
#include "jx_upload.h"

namespace jx {
namespace {

__global__ __launch_bounds__(64) void hpke_long_ctx_x25519_kernel(LongCtxArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const HpkeKeyRow& key = a.keys[a.slot];
  uint32_t enc[8];
  const uint8_t* p = a.encs + 32 * r;
  for (int i = 0; i < 8; i++)
    enc[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
             ((uint32_t)p[4 * i + 3] << 24);
  uint8_t kb[32], nb[12];
  const bool nz = hpke_suite_context(key.sk, key.pk, key.ksc, key.kdf, key.aead, a.zero_ist, a.zero_ost, enc, kb, nb);
  write_ctx(a.out[r], key.aead, kb, nb, nz);
}

__global__ __launch_bounds__(64) void hpke_long_ctx_p256_kernel(LongCtxArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const HpkeKeyRow& key = a.keys[a.slot];
  uint8_t kb[32] = {0}, nb[12] = {0};
  const bool ok = hpke_p256_context(key.sk, (const uint8_t*)key.pk, key.pky, key.ksc, key.kdf, key.aead,
                                    a.encs + 65 * r, kb, nb);
  write_ctx(a.out[r], key.aead, kb, nb, ok);
}

// AES-GCM open by the whole wave; every lane returns the same verdict. tt: the T-table; m4: the wave's 16 x 4 words.
// aad_ld(o, len, x): len (1..16) bytes of the associated data from offset o as 4 little-endian words, zero padded.
template <int NK, class AadLd>
__device__ bool gcm_wave_open(const uint32_t* tt, uint32_t* m4, uint32_t lane, const LongCtxRow& c, AadLd aad_ld,
                              uint64_t alen, const uint8_t* ct, uint64_t clen, uint8_t* pt) {
  const uint32_t* tl = tt + (lane & 31u);
  auto T = [tl](uint32_t x) { return tl[x << 5]; };
  uint32_t rk[4 * (NK + 7)], h[4], pw[4];
  gcm_wave_setup<NK>(T, m4, lane, c.kw, rk, h, pw);
  const uint4* m4v = reinterpret_cast<const uint4*>(m4);
  auto M = [m4v](uint32_t n, uint32_t e[4]) {
    const uint4 v = m4v[n];
    e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
  };
  const uint64_t na = (alen + 15) / 16, nc = (clen + 15) / 16, N = na + nc;
  uint32_t p[4];
  gl_lane_partial(
      N, lane,
      [&](uint64_t k, uint32_t x[4]) {
        if (k < na) {
          const uint64_t o = 16 * k;
          aad_ld(o, alen - o < 16 ? (uint32_t)(alen - o) : 16u, x);
        } else {
          const uint64_t o = 16 * (k - na);
          ld16(ct + o, clen - o < 16 ? (uint32_t)(clen - o) : 16u, x);
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
  gl_finish(p, alen, clen, h);
  // E(J0) ^ S == tag; counter blocks: nonce (12 bytes) || BE32 counter, J0 has counter 1
  uint32_t cb[4] = {c.nw[0], c.nw[1], c.nw[2], bswap32(1u)}, ks[4], tag[4];
  aes_encrypt_t_nk<NK>(T, rk, cb, ks);
  ld16(ct + clen, 16, tag);
  uint32_t diff = 0;
  for (int k = 0; k < 4; k++) diff |= ks[k] ^ bswap32(p[k]) ^ tag[k];
  if (diff != 0) return false;
  for (uint64_t k = lane; k < nc; k += GL_LANES) {
    const uint64_t o = 16 * k;
    const uint32_t len = clen - o < 16 ? (uint32_t)(clen - o) : 16u;
    uint32_t x[4];
    ld16(ct + o, len, x);
    cb[3] = bswap32((uint32_t)(2 + k));
    aes_encrypt_t_nk<NK>(T, rk, cb, ks);
    for (int w = 0; w < 4; w++) x[w] ^= ks[w];
    st16(pt + o, len, x);
  }
  return true;
}

// ChaCha20-Poly1305 open by the whole wave; every lane returns the same verdict. aad_ld as for gcm_wave_open: its
// zero-padded little-endian words are Poly1305's byte order. Every shuffle sits outside the per-lane block loops.
template <class AadLd>
__device__ bool chapoly_wave_open(uint32_t lane, const LongCtxRow& c, AadLd aad_ld, uint64_t alen, const uint8_t* ct,
                                  uint64_t clen, uint8_t* pt) {
  uint32_t ks[16];
  chacha20_block(c.kw, 0, c.nw, ks);  // every lane: the one-time key r || s is the first 32 bytes of block 0
  Poly1305 st;
  poly1305_init(st, ks);
  uint32_t pw[5], r64[5];
  poly_wave_powers(lane, st.r, pw);
  shfl5(r64, pw, 63);
  const uint64_t na = (alen + 15) / 16, nc = (clen + 15) / 16, N = pl_mac_blocks(alen, clen);
  uint32_t p[5];
  pl_lane_partial(
      N, lane,
      [&](uint64_t k, uint32_t m[4]) {
        if (k < na) {
          const uint64_t o = 16 * k;
          aad_ld(o, alen - o < 16 ? (uint32_t)(alen - o) : 16u, m);
        } else if (k < na + nc) {
          const uint64_t o = 16 * (k - na);
          ld16(ct + o, clen - o < 16 ? (uint32_t)(clen - o) : 16u, m);
        } else {
          pl_len_block(alen, clen, m);
        }
      },
      r64, p);
  {
    const uint32_t d = gl_lane_exponent(N, lane);
    uint32_t rd[5];
    shfl5(rd, pw, d ? d - 1 : 0);  // (a lane without blocks holds p = 0)
    pl_lane_term(p, rd);
  }
  // every limb < 2^26, so 64 of them fit a 32-bit word (pl_lane_term)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 5; k++) p[k] += __shfl_xor(p[k], off);
  uint32_t tag[4], want[4];
  pl_finish(st, p, tag);
  ld16(ct + clen, 16, want);
  uint32_t diff = 0;
  for (int k = 0; k < 4; k++) diff |= tag[k] ^ want[k];
  if (diff != 0) return false;
  const uint64_t nb = cl_blocks(clen);
  for (uint64_t b = lane; b < nb; b += GL_LANES) {
    chacha20_block(c.kw, cl_counter(b), c.nw, ks);
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t len = cl_piece_len(clen, b, q);
      if (len == 0) break;
      const uint64_t o = cl_piece_offset(b, q);
      uint32_t x[4];
      ld16(ct + o, len, x);
      for (int w = 0; w < 4; w++) x[w] ^= ks[4 * q + w];
      st16(pt + o, len, x);
    }
  }
  return true;
}

// The AEAD of the context row by the whole wave; every lane returns the same verdict. (The row, and so the branch,
// is the same in every lane.)
template <class AadLd>
__device__ __forceinline__ bool aead_wave_open(const uint32_t* tt, uint32_t* m4, uint32_t lane, const LongCtxRow& c,
                                               AadLd aad_ld, uint64_t alen, const uint8_t* ct, uint64_t clen,
                                               uint8_t* pt) {
  if (c.aead == HPKE_AEAD_AES128GCM) return gcm_wave_open<4>(tt, m4, lane, c, aad_ld, alen, ct, clen, pt);
  if (c.aead == HPKE_AEAD_AES256GCM) return gcm_wave_open<8>(tt, m4, lane, c, aad_ld, alen, ct, clen, pt);
  return chapoly_wave_open(lane, c, aad_ld, alen, ct, clen, pt);
}

__global__ __launch_bounds__(64 * WAVES) void hpke_long_open_kernel(const LongCtxRow* ctx, HpkeBufs b) {
  __shared__ uint32_t tt[256 * 32];
  __shared__ __attribute__((aligned(16))) uint32_t m4[WAVES][64];
  fill_ttable(tt);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * WAVES + wave;
  if (r >= b.n) return;
  const LongCtxRow c = ctx[r];
  const uint64_t c0 = b.ct_off[r], c1 = b.ct_off[r + 1];
  const uint64_t a0 = b.aad_off[r], alen = b.aad_off[r + 1] - a0;
  const uint8_t* ct = b.cts + c0;
  const uint8_t* aad = b.aads + a0;
  uint8_t* pt = b.pts + c0 - 16 * r;
  // (a ciphertext of 2^32 bytes or more is no report share: the host entry refuses it, this one fails it)
  bool ok = c.ok != 0 && c1 >= c0 + 16 && c1 - c0 < (1ull << 32);
  const uint64_t clen = ok ? c1 - c0 - 16 : 0;
  if (ok)
    ok = aead_wave_open(
        tt, m4[wave], lane, c, [&](uint64_t o, uint32_t len, uint32_t x[4]) { ld16(aad + o, len, x); }, alen, ct,
        clen, pt);
  if (lane == 0) b.ok[r] = (uint8_t)ok;
}

// ---------------------------------------------------------------------------- the leader's upload path
// jx_leader_upload_open_* (include/jx_prio3.h): handle_upload_generic's per-report loop (aggregator/src/
// aggregator.rs:1513-1694). Stage A for both trials of every report (the task's keypair, then the global one, as
// rows_body of jx_hpke_open.h tries them), then one wave per report: open under the first trial's context and, only
// if that fails to decrypt, under the second's; decode the PlaintextInputShare; check the payload's length and, in
// parallel over the wave, every field element < p (ge_p128 / ge_p64 of jx_field.h); lay the payload out as the row
// jx_leader_prep_init_device_ex reads.

__device__ __forceinline__ void fail_ctx(LongCtxRow& o) {
  const uint8_t z[32] = {0};
  write_ctx(o, 0, z, z, false);
}

// lane (report r, trial t) = 2 r + t. P256 false: the X25519 keys' rows and every row without a usable key; true:
// the P-256 keys' rows (launched only when the call has such a keypair).
template <bool P256>
__global__ __launch_bounds__(64) void upload_ctx_kernel(UploadArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * a.n) return;
  const UpRow& row = a.rows[idx >> 1];
  const uint32_t kidx = (idx & 1) ? row.key1 : row.key0;
  LongCtxRow& o = reinterpret_cast<LongCtxRow*>(a.ctx)[idx];
  if (kidx >= a.nkeys || (row.flags & UP_ROW_MALFORMED) || row.ct_len < 16) {
    if (!P256) fail_ctx(o);
    return;
  }
  const HpkeKeyRow& key = a.keys[kidx];
  if ((key.kem == (uint8_t)HPKE_KEM_P256_SHA256) != P256) return;  // the other kernel's row
  // a trial whose KEM does not fit the encapsulated key's length fails without an open
  if (row.enc_len != (P256 ? 65u : 32u)) {
    fail_ctx(o);
    return;
  }
  const uint8_t* p = a.encs + row.enc_off;
  uint8_t kb[32] = {0}, nb[12] = {0};
  bool ok;
  if constexpr (P256) {
    ok = hpke_p256_context(key.sk, (const uint8_t*)key.pk, key.pky, key.ksc, key.kdf, key.aead, p, kb, nb);
  } else {
    uint32_t enc[8];
    for (int i = 0; i < 8; i++)
      enc[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
               ((uint32_t)p[4 * i + 3] << 24);
    ok = hpke_suite_context(key.sk, key.pk, key.ksc, key.kdf, key.aead, a.zero_ist, a.zero_ost, enc, kb, nb);
  }
  write_ctx(o, key.aead, kb, nb, ok);
}

__global__ __launch_bounds__(64 * WAVES) void upload_open_kernel(UploadArgs a) {
  __shared__ uint32_t tt[256 * 32];
  __shared__ __attribute__((aligned(16))) uint32_t m4[WAVES][64];
  fill_ttable(tt);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * WAVES + wave;
  if (r >= a.n) return;
  const UpRow row = a.rows[r];
  const uint8_t* ct = a.cts + row.ct_off;
  uint8_t* pt = a.pts + row.ct_off;
  const uint64_t clen = row.ct_len >= 16 ? row.ct_len - 16 : 0;
  uint32_t st = JX_OPEN_OK;
  if (row.key0 == KEY_SLOT_NONE) {
    st = JX_OPEN_UNKNOWN_CONFIG;  // OutdatedHpkeConfig: neither the task nor the global keys hold the config id
  } else if ((row.flags & UP_ROW_MALFORMED) || row.ct_len < 16) {
    st = JX_OPEN_HPKE_DECRYPT_ERROR;
  } else {
    // byte i of the InputShareAad (messages/src/lib.rs:1854-1858): task_id || report id || time || u32 length of
    // the public share || the public share
    const uint8_t* id = a.ids + 16 * r;
    const uint8_t* ps = a.ps + (uint64_t)a.ps_bytes * r;
    const uint64_t alen = 60 + a.ps_bytes;
    auto aad_byte = [&](uint64_t i) -> uint8_t {
      if (i < 32) return a.task_id[i];
      if (i < 48) return id[i - 32];
      if (i < 56) return row.time_be[i - 48];
      if (i < 60) return (uint8_t)(a.ps_bytes >> (8 * (59 - i)));
      return ps[i - 60];
    };
    auto aad_ld = [&](uint64_t o, uint32_t len, uint32_t x[4]) {
      x[0] = x[1] = x[2] = x[3] = 0;
      for (uint32_t k = 0; k < len; k++) x[k >> 2] |= (uint32_t)aad_byte(o + k) << (8 * (k & 3));
    };
    bool ok = false;
    const LongCtxRow* ctx = reinterpret_cast<const LongCtxRow*>(a.ctx) + 2 * r;
    // the task's keypair first, then the global one (aggregator.rs:1602-1637): a second open only when the first
    // fails to decrypt and there is a fallback
    for (int t = 0; t < 2 && !ok; t++) {
      const LongCtxRow c = ctx[t];
      if (!c.ok) continue;
      ok = aead_wave_open(tt, m4[wave], lane, c, aad_ld, alen, ct, clen, pt);
    }
    if (!ok) st = JX_OPEN_HPKE_DECRYPT_ERROR;
  }
  // the plaintext was written by all lanes of this wave and is read by all of them
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
  __builtin_amdgcn_wave_barrier();
  uint64_t pay = 0, ext_end = 2;
  if (st == JX_OPEN_OK) {
    // PlaintextInputShare (messages/src/lib.rs:1323-1326), the framing rows_body decodes: u16-prefixed extensions
    // (type u16: TBD 0x0000 or Taskprov 0xFF00, else a decode error; u16-prefixed data), u32-prefixed payload,
    // nothing after it. Every lane decodes it (the same few bytes).
    const uint64_t L = clen;
    uint64_t plen = 0;
    if (L < 2) {
      st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
    } else {
      ext_end = 2 + (((uint32_t)pt[0] << 8) | pt[1]);
      if (ext_end > L) st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
      for (uint64_t i = 2; st == JX_OPEN_OK && i < ext_end;) {  // advances >= 4 bytes per extension
        if (i + 4 > ext_end) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
          break;
        }
        const uint32_t t = ((uint32_t)pt[i] << 8) | pt[i + 1], dl = ((uint32_t)pt[i + 2] << 8) | pt[i + 3];
        if ((t != 0x0000u && t != 0xFF00u) || i + 4 + dl > ext_end) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
          break;
        }
        i += 4 + dl;
      }
      if (st == JX_OPEN_OK) {
        if (ext_end + 4 > L) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
        } else {
          plen = ((uint64_t)pt[ext_end] << 24) | ((uint64_t)pt[ext_end + 1] << 16) | ((uint64_t)pt[ext_end + 2] << 8) |
                 pt[ext_end + 3];
          pay = ext_end + 4;
          if (pay + plen != L) st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
        }
      }
    }
    // A::InputShare::get_decoded_with_param(&(&vdaf, 0), payload) (aggregator.rs:1659-1662): the exact length, every
    // element of the measurement share and of the proofs share < p; the blind is opaque
    if (st == JX_OPEN_OK && plen != a.lis_bytes) st = JX_OPEN_INPUT_SHARE_DECODE_FAILURE;
    if (st == JX_OPEN_OK) {
      int bad = 0;
      for (uint64_t o = 16ull * lane; o < a.elem_bytes; o += 16 * GL_LANES) {
        const uint32_t len = a.elem_bytes - o < 16 ? (uint32_t)(a.elem_bytes - o) : 16u;
        uint32_t w[4];
        ld16(pt + pay + o, len, w);
        if (a.fb == 16)
          bad |= ge_p128(make128((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32)));
        else
          bad |= ge_p64(w[0], w[1]) || (len == 16 && ge_p64(w[2], w[3]));
      }
      if (__any(bad)) st = JX_OPEN_INPUT_SHARE_DECODE_FAILURE;
    }
  }
  // the row: the payload, then zeros up to the stride; zeros for a rejected report
  uint8_t* out = a.out_rows + a.lis_stride * r;
  for (uint64_t o = 16ull * lane; o < a.lis_stride; o += 16 * GL_LANES) {
    const uint32_t len = a.lis_stride - o < 16 ? (uint32_t)(a.lis_stride - o) : 16u;
    uint32_t w[4] = {0, 0, 0, 0};
    if (st == JX_OPEN_OK && o < a.lis_bytes) ld16(pt + pay + o, a.lis_bytes - o < 16 ? (uint32_t)(a.lis_bytes - o) : 16u, w);
    st16(out + o, len, w);
  }
  // the extension list without its length prefix, where the report's ciphertext was
  const uint64_t ext_len = st == JX_OPEN_OK ? ext_end - 2 : 0;
  for (uint64_t i = lane; i < ext_len; i += GL_LANES) a.out_ext[row.ct_off + i] = pt[2 + i];
  if (lane == 0) {
    a.out_ext_len[r] = (uint32_t)ext_len;
    a.out_status[r] = (uint8_t)st;
  }
}

}  // namespace

hipError_t launch_upload_open(UploadArgs a, bool any_p256, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, a.zero_ist, a.zero_ost);
  const dim3 g((uint32_t)((2 * a.n + 63) / 64));
  hipLaunchKernelGGL(upload_ctx_kernel<false>, g, dim3(64), 0, s, a);
  if (any_p256) hipLaunchKernelGGL(upload_ctx_kernel<true>, g, dim3(64), 0, s, a);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(upload_open_kernel, dim3((uint32_t)((a.n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hpke_long_open(const LongCtxArgs& ca, bool p256, const HpkeBufs& b, hipStream_t s) {
  if (b.n == 0) return hipSuccess;
  const dim3 g((uint32_t)((b.n + 63) / 64));
  if (p256)
    hipLaunchKernelGGL(hpke_long_ctx_p256_kernel, g, dim3(64), 0, s, ca);
  else
    hipLaunchKernelGGL(hpke_long_ctx_x25519_kernel, g, dim3(64), 0, s, ca);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(hpke_long_open_kernel, dim3((uint32_t)((b.n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s,
                     (const LongCtxRow*)ca.out, b);
  return hipGetLastError();
}

}  // namespace jx
