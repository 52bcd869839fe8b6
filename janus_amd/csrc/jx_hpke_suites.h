// jx_hpke_suites.h — the RFC 9180 base-mode key schedule for every suite Janus accepts (core/src/
// hpke.rs dispatches on HpkeConfig's kem_id, kdf_id and aead_id; messages/src/lib.rs:768-846):
// KEM 0x0020 (X25519) or 0x0010 (P-256, whose decapsulation is here too, over jx_p256.h) with KDF HKDF-SHA256 /
// -SHA384 / -SHA512 (1, 2, 3) and AEAD AES-128-GCM / AES-256-GCM / ChaCha20Poly1305 (1, 2, 3). The default suite (1, 1) keeps its own register-resident code in jx_hpke_default.hip; this
// is what the suite kernels run, one report per lane, each lane with the suite of ITS key.
// __host__ __device__: tests/csrc/hosttest_hpke_suites.cpp runs the same code on the CPU.
//
//   secret     = LabeledExtract(shared_secret, "secret", "")        (psk is empty in mode_base)
//   key        = LabeledExpand(secret, "key", key_schedule_context, Nk)
//   base_nonce = LabeledExpand(secret, "base_nonce", key_schedule_context, Nn)
// with suite_id = "HPKE" || kem || kdf || aead in every label. Nk (16 or 32) and Nn (12) are at most Nh (32, 48
// or 64), so HKDF-Expand is its first HMAC iteration alone: T(1) = HMAC(prk, info || 0x01).
#pragma once
#include <string.h>

#include <vector>

#include "jx_chapoly.h"
#include "jx_hpke.h"
#include "jx_p256.h"
#include "jx_sha512.h"

namespace jx {

enum : uint32_t {
  HPKE_KEM_X25519_SHA256 = 0x0020,
  HPKE_KEM_P256_SHA256 = 0x0010,
  HPKE_KDF_SHA256 = 1,
  HPKE_KDF_SHA384 = 2,
  HPKE_KDF_SHA512 = 3,
  HPKE_AEAD_AES128GCM = 1,
  HPKE_AEAD_AES256GCM = 2,
  HPKE_AEAD_CHACHA20POLY1305 = 3,
};
constexpr uint32_t HPKE_KSC_MAX = 129;  // mode || psk_id_hash || info_hash with Nh = 64

JX_HD bool hpke_suite_supported(uint32_t kem, uint32_t kdf, uint32_t aead) {
  return kem == HPKE_KEM_X25519_SHA256 && kdf >= 1 && kdf <= 3 && aead >= 1 && aead <= 3;
}
// what jx_hpke_create_key accepts: either KEM (the P-256 one has 65-byte public and encapsulated keys)
JX_HD bool hpke_key_supported(uint32_t kem, uint32_t kdf, uint32_t aead) {
  return (kem == HPKE_KEM_X25519_SHA256 || kem == HPKE_KEM_P256_SHA256) && kdf >= 1 && kdf <= 3 && aead >= 1 && aead <= 3;
}
JX_HD uint32_t hpke_enc_len(uint32_t kem) { return kem == HPKE_KEM_P256_SHA256 ? 65u : 32u; }
JX_HD uint32_t hpke_nh(uint32_t kdf) { return kdf == HPKE_KDF_SHA256 ? 32u : kdf == HPKE_KDF_SHA384 ? 48u : 64u; }
JX_HD uint32_t hpke_nk(uint32_t aead) { return aead == HPKE_AEAD_AES128GCM ? 16u : 32u; }

// a labeled message under construction: at most I2OSP(L, 2) || "HPKE-v1" || suite_id (10) || "base_nonce" ||
// key_schedule_context (129) || 0x01 = 159 bytes
struct LabeledMsg {
  uint8_t b[160];
  uint32_t n;
};
JX_HD void lm_str(LabeledMsg& m, const char* s) {
  for (int i = 0; s[i]; i++) m.b[m.n++] = (uint8_t)s[i];
}
JX_HD void lm_head(LabeledMsg& m, uint32_t kdf, uint32_t aead, uint32_t kem = HPKE_KEM_X25519_SHA256) {  // "HPKE-v1" || suite_id
  lm_str(m, "HPKE-v1HPKE");
  const uint8_t ids[6] = {0x00, (uint8_t)kem, 0x00, (uint8_t)kdf, 0x00, (uint8_t)aead};
  for (int i = 0; i < 6; i++) m.b[m.n++] = ids[i];
}

// (key, base_nonce) of one context from the KEM's shared secret and the recipient key's key_schedule_context
// (1 + 2 Nh bytes). key holds Nk bytes (the rest is zero).
template <class H>
JX_HD void hpke_key_schedule_t(const uint8_t ss[32], const uint8_t* ksc, uint32_t kdf, uint32_t aead, uint8_t key[32],
                               uint8_t nonce[12], uint32_t kem) {
  typename H::W ist[8], ost[8];
  uint8_t secret[H::NH], t1[H::NH];
  LabeledMsg m;
  hmac_pads_t<H>(ss, 32, ist, ost);
  m.n = 0;
  lm_head(m, kdf, aead, kem);
  lm_str(m, "secret");
  hmac_finish_t<H>(secret, ist, ost, m.b, m.n);
  hmac_pads_t<H>(secret, H::NH, ist, ost);
  const uint32_t nk = hpke_nk(aead);
#pragma unroll 1
  for (int which = 0; which < 2; which++) {
    const uint32_t L = which ? 12u : nk;
    m.n = 0;
    m.b[m.n++] = 0;
    m.b[m.n++] = (uint8_t)L;
    lm_head(m, kdf, aead, kem);
    if (which)
      lm_str(m, "base_nonce");
    else
      lm_str(m, "key");
    for (uint32_t i = 0; i < 1 + 2 * H::NH; i++) m.b[m.n++] = ksc[i];
    m.b[m.n++] = 1;
    hmac_finish_t<H>(t1, ist, ost, m.b, m.n);
    if (which) {
      for (uint32_t i = 0; i < 12; i++) nonce[i] = t1[i];
    } else {
      for (uint32_t i = 0; i < 32; i++) key[i] = i < nk ? t1[i] : 0;
    }
  }
}

JX_HD void hpke_key_schedule(const uint8_t ss[32], const uint8_t* ksc, uint32_t kdf, uint32_t aead, uint8_t key[32],
                             uint8_t nonce[12], uint32_t kem = HPKE_KEM_X25519_SHA256) {
  switch (kdf) {
    case HPKE_KDF_SHA256: hpke_key_schedule_t<HashSha256>(ss, ksc, kdf, aead, key, nonce, kem); break;
    case HPKE_KDF_SHA384: hpke_key_schedule_t<HashSha384>(ss, ksc, kdf, aead, key, nonce, kem); break;
    default: hpke_key_schedule_t<HashSha512>(ss, ksc, kdf, aead, key, nonce, kem); break;
  }
}

// The AEAD key and base nonce of one recipient key (sk clamped, pk: 8 LE words; ksc and the ids of its suite)
// for encapsulated key enc: DHKEM decap, then the suite's key schedule. False when the DH output is all zero.
JX_HD bool hpke_suite_context(const uint32_t sk[8], const uint32_t pk[8], const uint8_t* ksc, uint32_t kdf,
                              uint32_t aead, const uint32_t zist[8], const uint32_t zost[8], const uint32_t enc[8],
                              uint8_t key[32], uint8_t nonce[12]) {
  uint32_t ss[8];
  const bool nz = hpke_decap(ss, sk, pk, zist, zost, enc);
  uint8_t ssb[32];
  for (int i = 0; i < 32; i++) ssb[i] = (uint8_t)(ss[i >> 2] >> (24 - 8 * (i & 3)));
  hpke_key_schedule(ssb, ksc, kdf, aead, key, nonce);
  return nz;
}

// ---- DHKEM(P-256, HKDF-SHA256) (RFC 9180 §4.1, §7.1; jx_p256.h)

// Decap for the recipient key (sk: 8 little-endian words of an integer in [1, n - 1]; pkx, pky: the public point's
// coordinates, 32 big-endian bytes each) and the 65-byte encapsulated key enc: dh = the x-coordinate of sk * enc,
// eae_prk = LabeledExtract("", "eae_prk", dh), shared_secret = LabeledExpand(eae_prk, "shared_secret",
// enc || 0x04 || pkx || pky, 32), both with HKDF-SHA256 and suite id "KEM" || 0x0010. The expand message is 158
// bytes (LabeledMsg holds 160). False when enc is no valid point (public data): the open fails.
JX_HD bool hpke_p256_decap(uint8_t ss[32], const uint32_t sk[8], const uint8_t* pkx, const uint8_t* pky,
                           const uint8_t* enc) {
  p256_fe x, y;
  if (!p256_point_from_bytes(x, y, enc)) return false;
  uint8_t dh[32];
  if (!p256_scalar_mul_x(dh, sk, x, y)) return false;
  uint32_t ist[8], ost[8];
  uint8_t eae_prk[32];
  LabeledMsg m;
  hmac_pads_t<HashSha256>(nullptr, 0, ist, ost);
  m.n = 0;
  lm_str(m, "HPKE-v1KEM");
  m.b[m.n++] = 0x00;
  m.b[m.n++] = 0x10;
  lm_str(m, "eae_prk");
  for (int i = 0; i < 32; i++) m.b[m.n++] = dh[i];
  hmac_finish_t<HashSha256>(eae_prk, ist, ost, m.b, m.n);
  hmac_pads_t<HashSha256>(eae_prk, 32, ist, ost);
  m.n = 0;
  m.b[m.n++] = 0;
  m.b[m.n++] = 32;
  lm_str(m, "HPKE-v1KEM");
  m.b[m.n++] = 0x00;
  m.b[m.n++] = 0x10;
  lm_str(m, "shared_secret");
  for (int i = 0; i < 65; i++) m.b[m.n++] = enc[i];
  m.b[m.n++] = 0x04;
  for (int i = 0; i < 32; i++) m.b[m.n++] = pkx[i];
  for (int i = 0; i < 32; i++) m.b[m.n++] = pky[i];
  m.b[m.n++] = 1;  // 158 bytes
  hmac_finish_t<HashSha256>(ss, ist, ost, m.b, m.n);
  return true;
}

// The AEAD key and base nonce of one P-256 recipient key for the 65-byte encapsulated key enc: decap, then the
// suite's key schedule under suite id "HPKE" || 0x0010 || kdf || aead.
JX_HD bool hpke_p256_context(const uint32_t sk[8], const uint8_t* pkx, const uint8_t* pky, const uint8_t* ksc,
                             uint32_t kdf, uint32_t aead, const uint8_t* enc, uint8_t key[32], uint8_t nonce[12]) {
  uint8_t ss[32];
  if (!hpke_p256_decap(ss, sk, pkx, pky, enc)) return false;
  hpke_key_schedule(ss, ksc, kdf, aead, key, nonce, HPKE_KEM_P256_SHA256);
  return true;
}

// ---- host: a P-256 recipient keypair as HpkeKeyRow holds it

// sk: the private key, 32 big-endian bytes; pk: the public key, 65 bytes (SEC 1 uncompressed). nullptr and the
// row's fields (jx_kernels.h) when 1 <= sk < n, pk is a valid point and pk = sk * G (the reference derives the
// public key from the private one, so a pair that disagrees is a configuration error); else the reason.
inline const char* hpke_p256_keypair(const uint8_t* sk, const uint8_t* pk, uint32_t sk_words[8], uint8_t pkx[32],
                                     uint8_t pky[32]) {
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = sk + 4 * (7 - i);
    sk_words[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  if (!p256_scalar_valid(sk_words)) return "P-256 keypair: the private key is not in [1, n - 1]";
  p256_fe x, y;
  if (!p256_point_from_bytes(x, y, pk)) return "P-256 keypair: the public key is not a point of the curve";
  const uint8_t g[65] = {0x04, 0x6b, 0x17, 0xd1, 0xf2, 0xe1, 0x2c, 0x42, 0x47, 0xf8, 0xbc, 0xe6, 0xe5, 0x63, 0xa4, 0x40, 0xf2,
                         0x77, 0x03, 0x7d, 0x81, 0x2d, 0xeb, 0x33, 0xa0, 0xf4, 0xa1, 0x39, 0x45, 0xd8, 0x98, 0xc2, 0x96,
                         0x4f, 0xe3, 0x42, 0xe2, 0xfe, 0x1a, 0x7f, 0x9b, 0x8e, 0xe7, 0xeb, 0x4a, 0x7c, 0x0f, 0x9e, 0x16,
                         0x2b, 0xce, 0x33, 0x57, 0x6b, 0x31, 0x5e, 0xce, 0xcb, 0xb6, 0x40, 0x68, 0x37, 0xbf, 0x51, 0xf5};
  p256_fe gx, gy;
  uint8_t xy[64];
  if (!p256_point_from_bytes(gx, gy, g) || !p256_scalar_mul_xy(xy, sk_words, gx, gy) || memcmp(xy, pk + 1, 64) != 0)
    return "P-256 keypair: the public key is not the private key times the base point";
  memcpy(pkx, pk + 1, 32);
  memcpy(pky, pk + 33, 32);
  return nullptr;
}

// ---- host: the key_schedule_context of a recipient key, computed once when its context is created

// LabeledExtract("", label, ikm) with the suite's hash: HMAC under the empty salt
template <class H>
inline void hpke_labeled_extract_empty_salt(uint32_t kdf, uint32_t aead, const char* label, const uint8_t* ikm,
                                            size_t n, uint8_t* out, uint32_t kem = HPKE_KEM_X25519_SHA256) {
  LabeledMsg head;
  head.n = 0;
  lm_head(head, kdf, aead, kem);
  lm_str(head, label);
  std::vector<uint8_t> msg(head.b, head.b + head.n);
  msg.insert(msg.end(), ikm, ikm + n);
  typename H::W ist[8], ost[8];
  hmac_pads_t<H>(nullptr, 0, ist, ost);
  hmac_finish_t<H>(out, ist, ost, msg.data(), (uint32_t)msg.size());
}
// key_schedule_context = mode_base (0x00) || LabeledExtract("", "psk_id_hash", "") || LabeledExtract("",
// "info_hash", info). Returns its length, 1 + 2 Nh.
inline uint32_t hpke_key_schedule_context(uint32_t kdf, uint32_t aead, const uint8_t* info, size_t info_len,
                                          uint8_t ksc[HPKE_KSC_MAX], uint32_t kem = HPKE_KEM_X25519_SHA256) {
  const uint32_t nh = hpke_nh(kdf);
  ksc[0] = 0;
  switch (kdf) {
    case HPKE_KDF_SHA256:
      hpke_labeled_extract_empty_salt<HashSha256>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1, kem);
      hpke_labeled_extract_empty_salt<HashSha256>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh, kem);
      break;
    case HPKE_KDF_SHA384:
      hpke_labeled_extract_empty_salt<HashSha384>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1, kem);
      hpke_labeled_extract_empty_salt<HashSha384>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh, kem);
      break;
    default:
      hpke_labeled_extract_empty_salt<HashSha512>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1, kem);
      hpke_labeled_extract_empty_salt<HashSha512>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh, kem);
      break;
  }
  return 1 + 2 * nh;
}

}  // namespace jx
