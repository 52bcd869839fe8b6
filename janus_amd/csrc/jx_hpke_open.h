// jx_hpke_open.h — what the three HPKE kernel families share (device code; included by jx_hpke.hip and the
// family units jx_hpke_default.hip, jx_hpke_suite.hip and jx_hpke_p256.hip, each of which is one translation unit so
// that the three compile side by side).
//
// The kernels' argument structs and the launchers of the family units are the only names that cross units; the
// helpers and the two bodies, open_body and rows_body, keep internal linkage: every unit instantiates its own.
#pragma once
#include <hip/hip_runtime.h>

#include "jx_engine_internal.h"
#include "jx_hpke_suites.h"

namespace jx {

// (The four structs are named in the launchers' signatures, which cross units, so they have external linkage.)
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

struct RowsArgs {
  HpkeRowsArgs a;
  uint32_t zero_ist[8], zero_ost[8];
};

// One launcher per kernel, each in its family's unit: ceil(n / 64) blocks of 64 lanes on `s`; the caller reads
// hipGetLastError. launch_hpke_open_default takes the context's HpkeCfg and passes its first 65 context bytes on.
void launch_hpke_open_default(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s);
void launch_hpke_rows_default(const RowsArgs& ra, hipStream_t s);
void launch_hpke_open_suite(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s);
void launch_hpke_rows_suite(const RowsArgs& ra, hipStream_t s);
void launch_hpke_open_p256(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s);
void launch_hpke_rows_p256(const RowsArgs& ra, hipStream_t s);

namespace {

// The default suite's context (jx_hpke_default.hip): the one unit that instantiates open_body<false> and
// rows_body<false> defines it.
template <class Key>
__device__ bool hpke_context(const uint8_t* sbox, const Key& key, const uint32_t zist[8], const uint32_t zost[8],
                             const uint32_t enc[8], uint32_t rk[44], uint32_t h[4], uint32_t nonce3[3]);

JX_HD uint8_t ld_byte(const uint8_t* p, uint64_t i, uint64_t n) { return i < n ? p[i] : 0; }
JX_HD void ld_block_be(const uint8_t* p, uint64_t n, uint32_t b[4]) {  // up to 16 bytes, zero padded
  for (int w = 0; w < 4; w++) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v = (v << 8) | ld_byte(p, 4 * w + k, n);
    b[w] = v;
  }
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

}  // namespace
}  // namespace jx
