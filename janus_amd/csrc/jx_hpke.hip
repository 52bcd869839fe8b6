// jx_hpke.hip — batched HPKE open of report shares on the GPU.
//
// Replaces the per-report `hpke::open(&helper_keypair, &HpkeApplicationInfo::new(
// &Label::InputShare, &Role::Client, &Role::Helper), encrypted_input_share, &input_share_aad)`
// of the helper's aggregate-init loop (aggregator/src/aggregator.rs:1772-1832; core/src/hpke.rs:
// 200-230): RFC 9180 base mode, DHKEM(X25519, HKDF-SHA256), HKDF-SHA256, AES-128-GCM. One
// report per lane: X25519 decapsulation, the HKDF key schedule, AES-128-GCM open.
// The other eight X25519 suites an HpkeConfig can name (HKDF-SHA256 / -SHA384 / -SHA512 with AES-128-GCM /
// AES-256-GCM / ChaCha20Poly1305; jx_hpke_suites.h) go through a second pair of kernels, hpke_open_suite_kernel
// and hpke_rows_suite_kernel, which read the suite from the key row and dispatch per lane. They are launched only
// for a context, or a launch with a job, that holds a key outside the default suite (then for every row of the
// launch), so the default suite's kernels and their register budget are what they were.
// The second KEM the reference opens under, DHKEM(P-256, HKDF-SHA256) (0x0010; jx_p256.h), has a third pair,
// hpke_open_p256_kernel and hpke_rows_p256_kernel: its encapsulated keys are 65 bytes, so the rows of a prepare
// launch partition by that length (a trial of a keypair of the other KEM fails without an open), the X25519 rows
// kernels skip the 65-byte rows, and the P-256 rows kernel, launched only when the launch holds one, takes them.
//
// Two kernels (each with its suite twin and its P-256 twin):
//  - hpke_open_kernel: the standalone batch open of include/jx_hpke.h (caller's ciphertexts and AADs);
//  - hpke_rows_kernel: the open INSIDE a helper prepare launch (jx_helper_prep_encrypted_batch, alone or
//    coalesced): per report it builds the InputShareAad from the report's task id, id, time and public share
//    rows, tries the task's and then the global keypair (aggregator.rs:1807-1820), decodes the
//    PlaintextInputShare and checks its extensions (:1834-1893) and writes the payload into the helper
//    input-share row K1 reads, with one status byte per report (include/jx_prio3.h, JX_OPEN_*).
// C ABI in include/jx_hpke.h; the rows kernel's launcher is internal (jx_engine_internal.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/jx_hpke.h"
#include "jx_engine_internal.h"
#include "jx_hpke_suites.h"
#include "jx_keyreg.h"

using namespace jx;

namespace {

struct HpkeCfg {
  HpkeKeyRow key;          // clamped recipient scalar, public key, key_schedule_context, suite
  uint32_t zero_ist[8];    // HMAC-SHA256 pads of the empty salt (LabeledExtract with salt "")
  uint32_t zero_ost[8];
};
// What hpke_open_kernel takes: a default-suite key with its 65-byte key_schedule_context alone (the kernel keeps
// its argument in private memory, so the longer contexts of the other suites would cost it scratch).
struct HpkeDefaultCfg {
  uint32_t sk[8];
  uint32_t pk[8];
  uint8_t ksc[68];
  uint8_t pad[4];
  uint32_t zero_ist[8];
  uint32_t zero_ost[8];
};

struct HpkeBufs {
  uint64_t n;
  const uint8_t* encs;
  const uint8_t* cts;
  const uint64_t* ct_off;
  const uint8_t* aads;
  const uint64_t* aad_off;
  uint8_t* pts;
  uint8_t* ok;
};

// the default suite's id: "HPKE" || 0x0020 || 0x0001 || 0x0001
JX_HD int m_suite(Msg128& m, int pos) {
  pos = m_str(m, pos, "HPKE");
  const uint8_t ids[6] = {0x00, 0x20, 0x00, 0x01, 0x00, 0x01};
  for (int i = 0; i < 6; i++) m_byte(m, pos + i, ids[i]);
  return pos + 6;
}

// LabeledExpand(secret, label, ksc, L) for L <= 32: HMAC(secret, I2OSP(L,2) || "HPKE-v1" ||
// suite || label || ksc || 0x01)
JX_HD void expand_ksc(uint32_t out[8], const uint32_t ist[8], const uint32_t ost[8], int L, const char* label,
                      const uint8_t* ksc) {
  Msg128 m;
  m_zero(m);
  m_byte(m, 0, 0);
  m_byte(m, 1, L);
  int pos = m_str(m, 2, "HPKE-v1");
  pos = m_suite(m, pos);
  pos = m_str(m, pos, label);
  for (int i = 0; i < 65; i++) m_byte(m, pos + i, ksc[i]);
  pos += 65;
  m_byte(m, pos, 1);
  uint32_t inner[8];
  sha256_finish64(inner, ist, m, pos + 1);
  hmac_outer(out, ost, inner);
}

JX_HD uint8_t ld_byte(const uint8_t* p, uint64_t i, uint64_t n) { return i < n ? p[i] : 0; }
JX_HD void ld_block_be(const uint8_t* p, uint64_t n, uint32_t b[4]) {  // up to 16 bytes, zero padded
  for (int w = 0; w < 4; w++) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v = (v << 8) | ld_byte(p, 4 * w + k, n);
    b[w] = v;
  }
}

// The AES-128-GCM context of one recipient key for encapsulated key `enc` (8 LE words): DHKEM decap
// (RFC 9180 §4.1), the mode_base key schedule (§5.1), the round keys, the hash key H (4 BE words) and the
// base nonce (3 BE words). False when the DH output is all zero (a low-order point: the open fails).
// Key: anything with sk, pk and ksc (HpkeKeyRow, HpkeDefaultCfg).
template <class Key>
__device__ bool hpke_context(const uint8_t* sbox, const Key& key, const uint32_t zist[8], const uint32_t zost[8],
                             const uint32_t enc[8], uint32_t rk[44], uint32_t h[4], uint32_t nonce3[3]) {
  uint32_t ss[8], secret[8], kk[8], nonce[8];
  const bool nz = hpke_decap(ss, key.sk, key.pk, zist, zost, enc);
  {
    uint32_t ist[8], ost[8];
    hmac_pads(ss, ist, ost);
    Msg128 m;
    m_zero(m);
    int pos = m_str(m, 0, "HPKE-v1");
    pos = m_suite(m, pos);
    pos = m_str(m, pos, "secret");
    uint32_t inner[8];
    sha256_finish64(inner, ist, m, pos);
    hmac_outer(secret, ost, inner);
  }
  {
    uint32_t ist[8], ost[8];
    hmac_pads(secret, ist, ost);
    expand_ksc(kk, ist, ost, 16, "key", key.ksc);
    expand_ksc(nonce, ist, ost, 12, "base_nonce", key.ksc);
  }
  uint32_t kw[4], hblk[4], zero4[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; i++) kw[i] = bswap32(kk[i]);  // digest bytes 0..15 as LE words
  aes128_expand_key(sbox, kw, rk);
  aes128_encrypt(sbox, rk, zero4, hblk);
  for (int i = 0; i < 4; i++) h[i] = bswap32(hblk[i]);
  for (int i = 0; i < 3; i++) nonce3[i] = bswap32(nonce[i]);
  return nz;
}

// GCM tag check of ciphertext ct[0, clen) with tag ct[clen, clen + 16) and associated data produced 16
// bytes at a time by aad_block(i, w) (alen bytes): GHASH, then E(J0) ^ S == tag. NR: the cipher's rounds (10
// with AES-128's 44 round-key words, 14 with AES-256's 60).
template <int NR, class AadBlock>
__device__ bool gcm_tag_ok(const uint8_t* sbox, const uint32_t* rk, const uint32_t h[4], const uint32_t nonce3[3],
                           uint64_t alen, AadBlock aad_block, const uint8_t* ct, uint64_t clen) {
  uint32_t y[4] = {0, 0, 0, 0};
  for (uint64_t i = 0; i < alen; i += 16) {
    uint32_t x[4];
    aad_block(i, x);
    for (int k = 0; k < 4; k++) y[k] ^= x[k];
    ghash_mul(y, h);
  }
  for (uint64_t i = 0; i < clen; i += 16) {
    uint32_t x[4];
    ld_block_be(ct + i, clen - i, x);
    for (int k = 0; k < 4; k++) y[k] ^= x[k];
    ghash_mul(y, h);
  }
  y[0] ^= (uint32_t)((8 * alen) >> 32);
  y[1] ^= (uint32_t)(8 * alen);
  y[2] ^= (uint32_t)((8 * clen) >> 32);
  y[3] ^= (uint32_t)(8 * clen);
  ghash_mul(y, h);
  // counter blocks: nonce (12 bytes) || BE32 counter; J0 has counter 1
  uint32_t cb[4] = {nonce3[0], nonce3[1], nonce3[2], bswap32(1u)}, ks[4];
  aes_encrypt_nr<NR>(sbox, rk, cb, ks);
  uint32_t diff = 0;
  for (int k = 0; k < 4; k++) {
    uint32_t tag_w = 0;
    for (int q = 0; q < 4; q++) tag_w = (tag_w << 8) | ld_byte(ct + clen, 4 * k + q, 16);
    diff |= (bswap32(ks[k]) ^ y[k]) ^ tag_w;
  }
  return diff == 0;
}

// CTR decryption of ct[0, clen) into pt (counter blocks from 2)
template <int NR>
__device__ void gcm_decrypt(const uint8_t* sbox, const uint32_t* rk, const uint32_t nonce3[3], const uint8_t* ct,
                            uint64_t clen, uint8_t* pt) {
  uint32_t cb[4] = {nonce3[0], nonce3[1], nonce3[2], 0}, ks[4];
  for (uint64_t i = 0; i < clen; i += 16) {
    cb[3] = bswap32((uint32_t)(2 + i / 16));
    aes_encrypt_nr<NR>(sbox, rk, cb, ks);
    for (uint64_t j = 0; j < 16 && i + j < clen; j++) pt[i + j] = ct[i + j] ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3)));
  }
}

__device__ void load_enc(const uint8_t* p, uint32_t enc[8]) {
  for (int i = 0; i < 8; i++)
    enc[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
             ((uint32_t)p[4 * i + 3] << 24);
}

// One open under the key's own suite (jx_hpke_suites.h): the context, then the suite's AEAD with sequence
// number 0 (the nonce is the base nonce). The associated data comes a byte at a time from aad_byte(i).
// (suite_aead_open: the AEAD of either KEM's context, inlined into both callers.)
template <class AadByte>
__device__ __forceinline__ bool suite_aead_open(const uint8_t* sbox, uint32_t aead, const uint8_t kb[32],
                                                const uint8_t nb[12], uint64_t alen, AadByte aad_byte, const uint8_t* ct,
                                                uint64_t clen, uint8_t* pt) {
  uint32_t kw[8], nw[3];  // little-endian words
  for (int i = 0; i < 8; i++)
    kw[i] = (uint32_t)kb[4 * i] | ((uint32_t)kb[4 * i + 1] << 8) | ((uint32_t)kb[4 * i + 2] << 16) |
            ((uint32_t)kb[4 * i + 3] << 24);
  for (int i = 0; i < 3; i++)
    nw[i] = (uint32_t)nb[4 * i] | ((uint32_t)nb[4 * i + 1] << 8) | ((uint32_t)nb[4 * i + 2] << 16) |
            ((uint32_t)nb[4 * i + 3] << 24);
  if (aead == HPKE_AEAD_CHACHA20POLY1305) {
    if (!chapoly_tag_ok(kw, nw, alen, aad_byte, ct, clen)) return false;
    chapoly_decrypt(kw, nw, ct, clen, pt);
    return true;
  }
  auto aad_block = [&](uint64_t i, uint32_t x[4]) {  // 16 bytes as 4 big-endian words, zero padded
    for (int w = 0; w < 4; w++) {
      uint32_t v = 0;
      for (int k = 0; k < 4; k++) {
        const uint64_t j = i + 4 * w + k;
        v = (v << 8) | (j < alen ? (uint32_t)aad_byte(j) : 0u);
      }
      x[w] = v;
    }
  };
  uint32_t rk[60], h[4], hblk[4], zero4[4] = {0, 0, 0, 0};
  bool ok;
  if (aead == HPKE_AEAD_AES128GCM) {
    aes128_expand_key(sbox, kw, rk);
    aes128_encrypt(sbox, rk, zero4, hblk);
    for (int i = 0; i < 4; i++) h[i] = bswap32(hblk[i]);
    ok = gcm_tag_ok<10>(sbox, rk, h, nw, alen, aad_block, ct, clen);
    if (ok) gcm_decrypt<10>(sbox, rk, nw, ct, clen, pt);
  } else {
    aes256_expand_key(sbox, kw, rk);
    aes256_encrypt(sbox, rk, zero4, hblk);
    for (int i = 0; i < 4; i++) h[i] = bswap32(hblk[i]);
    ok = gcm_tag_ok<14>(sbox, rk, h, nw, alen, aad_block, ct, clen);
    if (ok) gcm_decrypt<14>(sbox, rk, nw, ct, clen, pt);
  }
  return ok;
}
template <class AadByte>
__device__ bool suite_open(const uint8_t* sbox, const HpkeKeyRow& key, const uint32_t zist[8], const uint32_t zost[8],
                           const uint32_t enc[8], uint64_t alen, AadByte aad_byte, const uint8_t* ct, uint64_t clen,
                           uint8_t* pt) {
  uint8_t kb[32], nb[12];
  const uint32_t aead = key.aead;
  if (!hpke_suite_context(key.sk, key.pk, key.ksc, key.kdf, aead, zist, zost, enc, kb, nb)) return false;
  return suite_aead_open(sbox, aead, kb, nb, alen, aad_byte, ct, clen, pt);
}
// The same under DHKEM(P-256, HKDF-SHA256): enc is the 65-byte encapsulated key where it lies in device memory. An
// invalid point (jx_p256.h) is a failed open.
template <class AadByte>
__device__ bool p256_open(const uint8_t* sbox, const HpkeKeyRow& key, const uint8_t* enc, uint64_t alen,
                          AadByte aad_byte, const uint8_t* ct, uint64_t clen, uint8_t* pt) {
  uint8_t kb[32], nb[12];
  const uint32_t aead = key.aead;
  if (!hpke_p256_context(key.sk, (const uint8_t*)key.pk, key.pky, key.ksc, key.kdf, aead, enc, kb, nb)) return false;
  return suite_aead_open(sbox, aead, kb, nb, alen, aad_byte, ct, clen, pt);
}

// The standalone batch open. SUITE false: the default suite alone (register-resident context); true: the suite of
// cfg.key, whichever of the nine it is.
template <bool SUITE, class Cfg>
__device__ void open_body(const uint8_t* sbox, const Cfg& cfg, const HpkeBufs& b) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  uint32_t enc[8];
  load_enc(b.encs + 32 * r, enc);
  const uint64_t c0 = b.ct_off[r], c1 = b.ct_off[r + 1];
  const uint64_t a0 = b.aad_off[r], a1 = b.aad_off[r + 1];
  const uint64_t alen = a1 - a0;
  const uint8_t* ct = b.cts + c0;
  const uint8_t* aad = b.aads + a0;
  bool ok;
  if constexpr (!SUITE) {
    uint32_t rk[44], h[4], nonce3[3];
    const bool nz = hpke_context(sbox, cfg, cfg.zero_ist, cfg.zero_ost, enc, rk, h, nonce3);
    ok = nz && c1 - c0 >= 16;
    const uint64_t clen = ok ? c1 - c0 - 16 : 0;
    ok = ok && gcm_tag_ok<10>(sbox, rk, h, nonce3, alen,
                              [&](uint64_t i, uint32_t x[4]) { ld_block_be(aad + i, alen - i, x); }, ct, clen);
    if (ok) gcm_decrypt<10>(sbox, rk, nonce3, ct, clen, b.pts + c0 - 16 * r);
  } else {
    ok = c1 - c0 >= 16 && suite_open(sbox, cfg.key, cfg.zero_ist, cfg.zero_ost, enc, alen,
                                     [&](uint64_t i) { return aad[i]; }, ct, c1 - c0 - 16, b.pts + c0 - 16 * r);
  }
  b.ok[r] = (uint8_t)ok;
}

__global__ __launch_bounds__(64) void hpke_open_kernel(HpkeDefaultCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  open_body<false>(sbox, cfg, b);
}
__global__ __launch_bounds__(64) void hpke_open_suite_kernel(HpkeCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  open_body<true>(sbox, cfg, b);
}

// The standalone batch open of a P-256 context: encapsulated keys at a stride of 65 bytes.
__global__ __launch_bounds__(64) void hpke_open_p256_kernel(HpkeCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const uint64_t c0 = b.ct_off[r], c1 = b.ct_off[r + 1];
  const uint64_t a0 = b.aad_off[r], a1 = b.aad_off[r + 1];
  const uint8_t* aad = b.aads + a0;
  const bool ok = c1 - c0 >= 16 && p256_open(sbox, cfg.key, b.encs + 65 * r, a1 - a0, [&](uint64_t i) { return aad[i]; },
                                             b.cts + c0, c1 - c0 - 16, b.pts + c0 - 16 * r);
  b.ok[r] = (uint8_t)ok;
}

// ---------------------------------------------------------------------------- open inside a prepare launch

struct RowsArgs {
  HpkeRowsArgs a;
  uint32_t zero_ist[8], zero_ost[8];
};

// byte i of the InputShareAad (messages/src/lib.rs:1854-1858): task_id (32) || report id (16) || time (8, BE)
// || u32 BE length of the public share || the public share
__device__ uint8_t aad_byte(const EncRow& e, const uint8_t* nonce, const uint8_t* ps, uint32_t ps_bytes, uint64_t i) {
  if (i < 32) return e.task_id[i];
  if (i < 48) return nonce[i - 32];
  if (i < 56) return e.time_be[i - 48];
  if (i < 60) return (uint8_t)(ps_bytes >> (8 * (59 - i)));
  return i - 60 < ps_bytes ? ps[i - 60] : 0;
}

// The open inside a prepare launch. Keys come from the device's key registry (a.keys, jx_keyreg.h): a row names the
// slots of its two trials. SUITE false: every key of the launch's jobs is of the default suite; true: each
// key's own suite (lanes of one wave may hold different ones). What follows the open is the same code.
// (ra by value: by reference the kernel's argument costs hpke_rows_kernel four more spilled registers.)
// P256: the rows whose encapsulated key is 65 bytes (ENC_ROW_ENC65), which the other two skip; a trial with a key
// of the other KEM fails without an open, as the hpke crate's deserialisation of the encapsulated key does. Jobs
// of default-suite keys alone never come with such a row (fill_enc_rows), so that body knows neither.
template <bool SUITE, bool P256 = false>
__device__ __forceinline__ void rows_body(const uint8_t* sbox, const RowsArgs ra) {
  const HpkeRowsArgs& a = ra.a;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const EncRow& e = a.rows[r];
  if constexpr (P256) {
    if ((e.flags & (ENC_ROW_ENCRYPTED | ENC_ROW_ENC65)) != (ENC_ROW_ENCRYPTED | ENC_ROW_ENC65)) return;
  } else {
    if (!(e.flags & ENC_ROW_ENCRYPTED)) {  // a plain report of the launch: its helper input share was uploaded
      a.status[r] = JX_OPEN_OK;
      return;
    }
    if constexpr (SUITE) {
      if (e.flags & ENC_ROW_ENC65) return;  // hpke_rows_p256_kernel's
    }
  }
  uint8_t* his = a.his + (uint64_t)a.his_bytes * r;
  uint32_t st = JX_OPEN_OK;
  const uint64_t c0 = e.ct_off, clen_all = e.ct_len;
  const uint8_t* ct = a.cts + c0;
  uint8_t* pt = a.pts + c0;
  const uint64_t clen = clen_all >= 16 ? clen_all - 16 : 0;
  if (e.key0 == KEY_SLOT_NONE) {
    st = JX_OPEN_UNKNOWN_CONFIG;  // neither the task nor the global keys hold the config id
  } else if ((e.flags & ENC_ROW_MALFORMED) || clen_all < 16) {
    st = JX_OPEN_HPKE_DECRYPT_ERROR;  // an encapsulated key that fits neither keypair's KEM, a ciphertext without a tag
  } else {
    uint32_t enc[8];
    if constexpr (!P256) load_enc(e.enc, enc);
    const uint8_t* nonce = a.nonces + 16 * r;
    const uint8_t* ps = a.ps + (uint64_t)a.ps_bytes * r;
    const uint64_t alen = 60 + a.ps_bytes;
    bool ok = false;
    // the task's keypair first, then the global one (aggregator.rs:1807-1820): a second trial only when the
    // first fails to decrypt
    for (int t = 0; t < 2 && !ok; t++) {
      const uint32_t kidx = t == 0 ? e.key0 : e.key1;
      if (kidx >= a.nkeys) break;
      if constexpr (!SUITE) {
        uint32_t rk[44], h[4], nonce3[3];
        const bool nz = hpke_context(sbox, a.keys[kidx], ra.zero_ist, ra.zero_ost, enc, rk, h, nonce3);
        ok = nz && gcm_tag_ok<10>(sbox, rk, h, nonce3, alen,
                                  [&](uint64_t i, uint32_t x[4]) {
                                    for (int w = 0; w < 4; w++) {
                                      uint32_t v = 0;
                                      for (int k = 0; k < 4; k++) {
                                        const uint64_t j = i + 4 * w + k;
                                        v = (v << 8) | (j < alen ? aad_byte(e, nonce, ps, a.ps_bytes, j) : 0u);
                                      }
                                      x[w] = v;
                                    }
                                  },
                                  ct, clen);
        if (ok) gcm_decrypt<10>(sbox, rk, nonce3, ct, clen, pt);
      } else if constexpr (P256) {
        if (a.keys[kidx].kem != (uint8_t)HPKE_KEM_P256_SHA256) continue;
        ok = p256_open(sbox, a.keys[kidx], a.cts + e.enc65_off, alen,
                       [&](uint64_t i) { return aad_byte(e, nonce, ps, a.ps_bytes, i); }, ct, clen, pt);
      } else {
        if (a.keys[kidx].kem != (uint8_t)HPKE_KEM_X25519_SHA256) continue;
        ok = suite_open(sbox, a.keys[kidx], ra.zero_ist, ra.zero_ost, enc, alen,
                        [&](uint64_t i) { return aad_byte(e, nonce, ps, a.ps_bytes, i); }, ct, clen, pt);
      }
    }
    if (!ok) st = JX_OPEN_HPKE_DECRYPT_ERROR;
  }
  uint64_t pay = 0, plen = 0;
  if (st == JX_OPEN_OK) {
    // PlaintextInputShare (messages/src/lib.rs:1323-1326): u16-prefixed extensions, u32-prefixed payload,
    // nothing after it; an extension is type u16 (TBD 0x0000 or Taskprov 0xFF00, else a decode error) || u16-
    // prefixed data
    const uint64_t L = clen;
    if (L < 2) {
      st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
    } else {
      const uint64_t end = 2 + (((uint32_t)pt[0] << 8) | pt[1]);
      uint32_t n_tbd = 0, n_tp = 0, tp_len = 0;
      if (end > L) st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
      for (uint64_t i = 2; st == JX_OPEN_OK && i < end;) {  // advances >= 4 bytes per extension
        if (i + 4 > end) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
          break;
        }
        const uint32_t t = ((uint32_t)pt[i] << 8) | pt[i + 1], dl = ((uint32_t)pt[i + 2] << 8) | pt[i + 3];
        if ((t != 0x0000u && t != 0xFF00u) || i + 4 + dl > end) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
          break;
        }
        if (t == 0) {
          n_tbd++;
        } else {
          n_tp++;
          tp_len = dl;
        }
        i += 4 + dl;
      }
      if (st == JX_OPEN_OK) {
        if (end + 4 > L) {
          st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
        } else {
          plen = ((uint64_t)pt[end] << 24) | ((uint64_t)pt[end + 1] << 16) | ((uint64_t)pt[end + 2] << 8) | pt[end + 3];
          pay = end + 4;
          if (pay + plen != L) st = JX_OPEN_PLAINTEXT_DECODE_FAILURE;
        }
      }
      const bool req = (e.flags & ENC_ROW_REQUIRE_TASKPROV) != 0;
      if (st == JX_OPEN_OK && (n_tbd > 1 || n_tp > 1))
        st = JX_OPEN_DUPLICATE_EXTENSION;  // aggregator.rs:1852-1867
      else if (st == JX_OPEN_OK && req && !(n_tp == 1 && tp_len == 0))
        st = JX_OPEN_MISSING_TASKPROV;  // :1869-1879
      else if (st == JX_OPEN_OK && !req && n_tp)
        st = JX_OPEN_UNEXPECTED_TASKPROV;  // :1880-1890
      if (st == JX_OPEN_OK && plen != a.his_bytes) st = JX_OPEN_INPUT_SHARE_DECODE_FAILURE;  // :1895-1910
    }
  }
  // the helper input share K1 reads (zeros for a failed report: prepared, then masked by launch_open_mask)
  for (uint32_t i = 0; i < a.his_bytes; i++) his[i] = st == JX_OPEN_OK ? pt[pay + i] : 0;
  a.status[r] = (uint8_t)st;
}

__global__ __launch_bounds__(64) void hpke_rows_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<false>(sbox, ra);
}
__global__ __launch_bounds__(64) void hpke_rows_suite_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<true>(sbox, ra);
}

__global__ __launch_bounds__(64) void hpke_rows_p256_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<true, true>(sbox, ra);
}

__global__ __launch_bounds__(256) void open_mask_kernel(const uint8_t* status, uint8_t* verdicts, uint64_t n) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n && status[r] != JX_OPEN_OK) verdicts[r] = JX_OPEN_FAILURE;
}

}  // namespace

struct jx_hpke {
  HpkeCfg cfg{};
  bool default_suite = true;  // X25519 with (HKDF-SHA256, AES-128-GCM): opened by hpke_open_kernel / hpke_rows_kernel
  uint32_t kem = HPKE_KEM_X25519_SHA256;
  int device = 0;
  uint32_t slot = 0;            // the context's row of the device's key registry, for as long as it lives
  hipStream_t stream = nullptr;  // created at the first standalone open or jx_hpke_stream (ensure_stream)
  jxi::Arena* arena = nullptr;  // the device's arena: the host-buffer open's device buffers
  std::mutex mu;                // one call at a time per handle (its stream and staging)
};

// errors: per calling thread (jx_hpke_last_error)
static thread_local std::string t_hpke_err;

static int32_t hfail(int32_t code, const std::string& m) {
  t_hpke_err = m;
  return code;
}
#define HCHK(call)                                                                                   \
  do {                                                                                               \
    hipError_t _st = (call);                                                                         \
    if (_st != hipSuccess) return hfail(JX_HPKE_E_HIP, std::string(#call) + ": " + hipGetErrorString(_st)); \
  } while (0)

// The device's key registry: KEY_SLOTS rows of device memory of its own (not the arena's: a launch in flight must
// never see the table move), allocated at the first context creation on the device and kept for the life of the
// process; one stream for the rows' uploads.
namespace {
struct KeyRegistry {
  std::mutex mu;
  HpkeKeyRow* d_rows = nullptr;
  hipStream_t stream = nullptr;
  KeySlots slots;
};
std::mutex g_reg_mu;
std::vector<KeyRegistry*> g_regs;  // by device

KeyRegistry* registry_for(int device) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if ((size_t)device >= g_regs.size()) g_regs.resize(device + 1, nullptr);
  if (!g_regs[device]) g_regs[device] = new KeyRegistry();
  return g_regs[device];
}

// Take a slot and write the row, synchronously: the row is on the device when this returns.
int32_t registry_add(int device, const HpkeKeyRow& row, uint32_t* slot) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  HCHK(hipSetDevice(device));
  if (!R->d_rows) {
    HpkeKeyRow* p = nullptr;
    const hipError_t st = hipMalloc((void**)&p, (size_t)KEY_SLOTS * sizeof(HpkeKeyRow));
    if (st == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (HPKE key registry)");
    HCHK(st);
    if (!R->stream) HCHK(hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking));
    R->d_rows = p;
  }
  const int32_t s = R->slots.take();
  if (s < 0)
    return hfail(JX_HPKE_E_NOMEM, "the device's HPKE key registry is full: " + std::to_string(KEY_SLOTS) +
                                      " live contexts (jx_hpke_destroy frees a slot)");
  hipError_t st = hipMemcpyAsync(R->d_rows + s, &row, sizeof row, hipMemcpyHostToDevice, R->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(R->stream);
  if (st != hipSuccess) {
    R->slots.free((uint32_t)s);
    return hfail(JX_HPKE_E_HIP, std::string("HPKE key registry upload: ") + hipGetErrorString(st));
  }
  *slot = (uint32_t)s;
  return JX_HPKE_OK;
}

// Wipe the row (it held a private key) and free the slot for the next context.
void registry_remove(int device, uint32_t slot) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  const HpkeKeyRow zero{};
  if (hipSetDevice(device) == hipSuccess &&
      hipMemcpyAsync(R->d_rows + slot, &zero, sizeof zero, hipMemcpyHostToDevice, R->stream) == hipSuccess)
    (void)hipStreamSynchronize(R->stream);
  R->slots.free(slot);
}

// with h->mu held
int32_t ensure_stream(jx_hpke* h) {
  if (h->stream) return JX_HPKE_OK;
  HCHK(hipSetDevice(h->device));
  HCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  return JX_HPKE_OK;
}
}  // namespace

// the default suite keeps its own kernel; any other goes through the suite kernel of its KEM
static void launch_open(const jx_hpke* h, const HpkeBufs& b) {
  const dim3 grid((uint32_t)((b.n + 63) / 64)), block(64);
  if (h->kem == HPKE_KEM_P256_SHA256) {
    hipLaunchKernelGGL(hpke_open_p256_kernel, grid, block, 0, h->stream, h->cfg, b);
  } else if (h->default_suite) {
    HpkeDefaultCfg d{};
    memcpy(d.sk, h->cfg.key.sk, 32);
    memcpy(d.pk, h->cfg.key.pk, 32);
    memcpy(d.ksc, h->cfg.key.ksc, 65);
    memcpy(d.zero_ist, h->cfg.zero_ist, 32);
    memcpy(d.zero_ost, h->cfg.zero_ost, 32);
    hipLaunchKernelGGL(hpke_open_kernel, grid, block, 0, h->stream, d, b);
  } else
    hipLaunchKernelGGL(hpke_open_suite_kernel, grid, block, 0, h->stream, h->cfg, b);
}

namespace jxi {

int hpke_device(const jx_hpke* h) { return h->device; }
uint16_t hpke_slot(const jx_hpke* h) { return (uint16_t)h->slot; }
void hpke_registry(int device, const HpkeKeyRow** rows, uint32_t* capacity) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  *rows = R->d_rows;
  *capacity = KEY_SLOTS;
}
bool hpke_default_suite(const jx_hpke* h) { return h->default_suite; }
uint32_t hpke_enc_len(const jx_hpke* h) { return jx::hpke_enc_len(h->kem); }

hipError_t launch_hpke_rows(const HpkeRowsArgs& a, bool suites, bool p256_rows, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  RowsArgs ra;
  ra.a = a;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, ra.zero_ist, ra.zero_ost);
  // a key of another suite among the launch's jobs: every row of the launch goes through the suite kernel
  if (suites)
    hipLaunchKernelGGL(hpke_rows_suite_kernel, dim3((uint32_t)((a.n + 63) / 64)), dim3(64), 0, s, ra);
  else
    hipLaunchKernelGGL(hpke_rows_kernel, dim3((uint32_t)((a.n + 63) / 64)), dim3(64), 0, s, ra);
  // the rows with a 65-byte encapsulated key (the others' rows it skips; both write his / status of their own rows)
  if (p256_rows) hipLaunchKernelGGL(hpke_rows_p256_kernel, dim3((uint32_t)((a.n + 63) / 64)), dim3(64), 0, s, ra);
  return hipGetLastError();
}

hipError_t launch_open_mask(const uint8_t* status, uint8_t* verdicts, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(open_mask_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, status, verdicts, n);
  return hipGetLastError();
}

}  // namespace jxi

extern "C" {

int32_t jx_hpke_create(const uint8_t sk[32], const uint8_t pk[32], const uint8_t* info, uint32_t info_len,
                       int32_t device, jx_hpke** out) {
  return jx_hpke_create_suite(HPKE_KEM_X25519_SHA256, HPKE_KDF_SHA256, HPKE_AEAD_AES128GCM, sk, pk, info, info_len,
                              device, out);
}

int32_t jx_hpke_create_suite(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t sk[32],
                             const uint8_t pk[32], const uint8_t* info, uint32_t info_len, int32_t device,
                             jx_hpke** out) {
  if (!sk || !pk || !out || (info_len && !info)) return JX_HPKE_E_INVALID;
  *out = nullptr;
  if (!hpke_suite_supported(kem_id, kdf_id, aead_id))
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "unsupported HPKE suite (KEM " + std::to_string(kem_id) + ", KDF " + std::to_string(kdf_id) + ", AEAD " +
                     std::to_string(aead_id) + "): KEM 0x0020 (X25519) with 32-byte keys (KEM 0x0010, P-256, has 65-byte "
                     "public keys: jx_hpke_create_key), KDF 1..3 (HKDF-SHA256/384/512), AEAD 1..3 (AES-128-GCM, "
                     "AES-256-GCM, ChaCha20Poly1305)");
  return jx_hpke_create_key(kem_id, kdf_id, aead_id, sk, 32, pk, 32, info, info_len, device, out);
}

int32_t jx_hpke_create_key(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t* sk, uint32_t sk_len,
                           const uint8_t* pk, uint32_t pk_len, const uint8_t* info, uint32_t info_len, int32_t device,
                           jx_hpke** out) {
  if (!sk || !pk || !out || (info_len && !info)) return JX_HPKE_E_INVALID;
  *out = nullptr;
  if (!hpke_key_supported(kem_id, kdf_id, aead_id))
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "unsupported HPKE suite (KEM " + std::to_string(kem_id) + ", KDF " + std::to_string(kdf_id) + ", AEAD " +
                     std::to_string(aead_id) + "): KEM 0x0020 (X25519) or 0x0010 (P-256), KDF 1..3 (HKDF-SHA256/384/512), "
                     "AEAD 1..3 (AES-128-GCM, AES-256-GCM, ChaCha20Poly1305)");
  const bool p256 = kem_id == HPKE_KEM_P256_SHA256;
  if (sk_len != 32 || pk_len != hpke_enc_len(kem_id))
    return hfail(JX_HPKE_E_INVALID, p256 ? "P-256 keypair: the private key is 32 bytes, the public key 65"
                                         : "X25519 keypair: the private and the public key are 32 bytes each");
  HpkeKeyRow key{};
  if (p256) {  // the same code as the kernels', on the host (jx_p256.h)
    if (const char* why = hpke_p256_keypair(sk, pk, key.sk, (uint8_t*)key.pk, key.pky)) return hfail(JX_HPKE_E_INVALID, why);
  } else {
    uint8_t k[32];
    memcpy(k, sk, 32);
    k[0] &= 248;
    k[31] &= 127;
    k[31] |= 64;
    for (int i = 0; i < 8; i++) {
      memcpy(&key.sk[i], k + 4 * i, 4);
      memcpy(&key.pk[i], pk + 4 * i, 4);
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return JX_HPKE_E_NODEVICE;
  if (device < 0 || device >= ndev) return JX_HPKE_E_INVALID;
  jx_hpke* h = new jx_hpke();
  h->device = device;
  h->cfg.key = key;
  h->kem = kem_id;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, h->cfg.zero_ist, h->cfg.zero_ost);
  // the key_schedule_context under the key's own suite and hash (jx_hpke_suites.h)
  static_assert(sizeof(h->cfg.key.ksc) >= HPKE_KSC_MAX, "HpkeKeyRow holds the longest key_schedule_context");
  hpke_key_schedule_context(kdf_id, aead_id, info, info_len, h->cfg.key.ksc, kem_id);
  h->cfg.key.kdf = (uint8_t)kdf_id;
  h->cfg.key.aead = (uint8_t)aead_id;
  h->cfg.key.kem = (uint8_t)kem_id;
  h->default_suite = !p256 && kdf_id == HPKE_KDF_SHA256 && aead_id == HPKE_AEAD_AES128GCM;
  // the context's row of the device's key registry (full: JX_HPKE_E_NOMEM)
  if (const int32_t rc = registry_add(device, h->cfg.key, &h->slot)) {
    delete h;
    return rc;
  }
  h->arena = jxi::arena_for(device);
  *out = h;
  return JX_HPKE_OK;
}

int32_t jx_hpke_suite(const jx_hpke* h, uint32_t* kem_id, uint32_t* kdf_id, uint32_t* aead_id) {
  if (!h) return JX_HPKE_E_INVALID;
  if (kem_id) *kem_id = h->kem;
  if (kdf_id) *kdf_id = h->cfg.key.kdf;
  if (aead_id) *aead_id = h->cfg.key.aead;
  return JX_HPKE_OK;
}

int32_t jx_hpke_enc_len(const jx_hpke* h) { return h ? (int32_t)hpke_enc_len(h->kem) : 0; }

int32_t jx_hpke_stream(const jx_hpke* h, void** out_stream) {
  if (!h || !out_stream) return JX_HPKE_E_INVALID;
  jx_hpke* m = const_cast<jx_hpke*>(h);  // the stream is created at its first use
  std::lock_guard<std::mutex> lk(m->mu);
  if (const int32_t rc = ensure_stream(m)) return rc;
  *out_stream = (void*)h->stream;
  return JX_HPKE_OK;
}

void jx_hpke_destroy(jx_hpke* h) {
  if (!h) return;
  if (h->stream) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  registry_remove(h->device, h->slot);
  delete h;
}

int32_t jx_hpke_open_batch_device(jx_hpke* h, uint64_t n, const void* d_encs, const void* d_cts,
                                  const uint64_t* d_ct_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                  void* d_out_plaintexts, void* d_out_ok) {
  if (!h || (n && (!d_encs || !d_cts || !d_ct_offsets || !d_aad_offsets || !d_out_plaintexts || !d_out_ok))) {
    return JX_HPKE_E_INVALID;
  }
  if (n == 0) return JX_HPKE_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  HpkeBufs b{n,
             (const uint8_t*)d_encs,
             (const uint8_t*)d_cts,
             d_ct_offsets,
             (const uint8_t*)d_aads,
             d_aad_offsets,
             (uint8_t*)d_out_plaintexts,
             (uint8_t*)d_out_ok};
  launch_open(h, b);
  HCHK(hipGetLastError());
  return JX_HPKE_OK;
}

// Host buffers: one staging slab from the device's arena (no per-call hipMalloc / hipFree, which would wait
// for the whole device), handed back stream-ordered; only this handle's stream is synchronized.
int32_t jx_hpke_open_batch(jx_hpke* h, uint64_t n, const uint8_t* encs, const uint8_t* cts,
                           const uint64_t* ct_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                           uint8_t* out_plaintexts, uint8_t* out_ok) {
  if (!h || (n && (!encs || !cts || !ct_offsets || !aad_offsets || !out_plaintexts || !out_ok)))
    return JX_HPKE_E_INVALID;
  if (n == 0) return JX_HPKE_OK;
  for (uint64_t i = 0; i < n; i++)
    if (ct_offsets[i + 1] < ct_offsets[i] + 16 || aad_offsets[i + 1] < aad_offsets[i])
      return hfail(JX_HPKE_E_INVALID, "offsets must be non-decreasing and every ciphertext >= 16 bytes");
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  const uint64_t ct_bytes = ct_offsets[n], aad_bytes = aad_offsets[n], pt_bytes = ct_bytes - 16 * n;
  const uint64_t enc_bytes = n * hpke_enc_len(h->kem);
  const size_t o_enc = 0, o_ct = o_enc + jxi::align256(enc_bytes), o_aad = o_ct + jxi::align256(ct_bytes),
               o_pt = o_aad + jxi::align256(aad_bytes ? aad_bytes : 1), o_ok = o_pt + jxi::align256(pt_bytes ? pt_bytes : 1),
               o_co = o_ok + jxi::align256(n), o_ao = o_co + jxi::align256((n + 1) * 8), bytes = o_ao + jxi::align256((n + 1) * 8);
  jxi::Slab slab;
  const hipError_t ga = jxi::arena_get(h->arena, bytes, h->stream, true, true, slab);
  if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
  HCHK(ga);
  uint8_t* base = (uint8_t*)slab.p;
  int32_t rc = JX_HPKE_OK;
  do {
    if (hipMemcpyAsync(base + o_enc, encs, enc_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ct, cts, ct_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (aad_bytes && hipMemcpyAsync(base + o_aad, aads, aad_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        hipMemcpyAsync(base + o_co, ct_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ao, aad_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "host-to-device copy failed");
      break;
    }
    HpkeBufs b{n, base + o_enc, base + o_ct, (const uint64_t*)(base + o_co), base + o_aad, (const uint64_t*)(base + o_ao),
               base + o_pt, base + o_ok};
    launch_open(h, b);
    if (hipGetLastError() != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "kernel launch failed");
      break;
    }
    if ((pt_bytes && hipMemcpyAsync(out_plaintexts, base + o_pt, pt_bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
        hipMemcpyAsync(out_ok, base + o_ok, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "device-to-host copy failed");
      break;
    }
  } while (0);
  jxi::arena_put(h->arena, slab, h->stream);  // reused after this stream's work
  return rc;
}

const char* jx_hpke_last_error(const jx_hpke* h) {
  (void)h;
  return t_hpke_err.c_str();
}

}  // extern "C"
