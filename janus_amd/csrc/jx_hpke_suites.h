// jx_hpke_suites.h — the RFC 9180 base-mode key schedule for every X25519 suite Janus accepts (core/src/
// hpke.rs dispatches on HpkeConfig's kem_id, kdf_id and aead_id; messages/src/lib.rs:768-846):
// KEM 0x0020 with KDF HKDF-SHA256 / -SHA384 / -SHA512 (1, 2, 3) and AEAD AES-128-GCM / AES-256-GCM /
// ChaCha20Poly1305 (1, 2, 3). The default suite (1, 1) keeps its own register-resident code in jx_hpke.hip; this
// is what the suite kernels run, one report per lane, each lane with the suite of ITS key.
// __host__ __device__: tests/csrc/hosttest_hpke_suites.cpp runs the same code on the CPU.
//
//   secret     = LabeledExtract(shared_secret, "secret", "")        (psk is empty in mode_base)
//   key        = LabeledExpand(secret, "key", key_schedule_context, Nk)
//   base_nonce = LabeledExpand(secret, "base_nonce", key_schedule_context, Nn)
// with suite_id = "HPKE" || kem || kdf || aead in every label. Nk (16 or 32) and Nn (12) are at most Nh (32, 48
// or 64), so HKDF-Expand is its first HMAC iteration alone: T(1) = HMAC(prk, info || 0x01).
#pragma once
#include <vector>

#include "jx_chapoly.h"
#include "jx_hpke.h"
#include "jx_sha512.h"

namespace jx {

enum : uint32_t {
  HPKE_KEM_X25519_SHA256 = 0x0020,
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
JX_HD void lm_head(LabeledMsg& m, uint32_t kdf, uint32_t aead) {  // "HPKE-v1" || suite_id
  lm_str(m, "HPKE-v1HPKE");
  const uint8_t ids[6] = {0x00, 0x20, 0x00, (uint8_t)kdf, 0x00, (uint8_t)aead};
  for (int i = 0; i < 6; i++) m.b[m.n++] = ids[i];
}

// (key, base_nonce) of one context from the KEM's shared secret and the recipient key's key_schedule_context
// (1 + 2 Nh bytes). key holds Nk bytes (the rest is zero).
template <class H>
JX_HD void hpke_key_schedule_t(const uint8_t ss[32], const uint8_t* ksc, uint32_t kdf, uint32_t aead, uint8_t key[32],
                               uint8_t nonce[12]) {
  typename H::W ist[8], ost[8];
  uint8_t secret[H::NH], t1[H::NH];
  LabeledMsg m;
  hmac_pads_t<H>(ss, 32, ist, ost);
  m.n = 0;
  lm_head(m, kdf, aead);
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
    lm_head(m, kdf, aead);
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
                             uint8_t nonce[12]) {
  switch (kdf) {
    case HPKE_KDF_SHA256: hpke_key_schedule_t<HashSha256>(ss, ksc, kdf, aead, key, nonce); break;
    case HPKE_KDF_SHA384: hpke_key_schedule_t<HashSha384>(ss, ksc, kdf, aead, key, nonce); break;
    default: hpke_key_schedule_t<HashSha512>(ss, ksc, kdf, aead, key, nonce); break;
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

// ---- host: the key_schedule_context of a recipient key, computed once when its context is created

// LabeledExtract("", label, ikm) with the suite's hash: HMAC under the empty salt
template <class H>
inline void hpke_labeled_extract_empty_salt(uint32_t kdf, uint32_t aead, const char* label, const uint8_t* ikm,
                                            size_t n, uint8_t* out) {
  LabeledMsg head;
  head.n = 0;
  lm_head(head, kdf, aead);
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
                                          uint8_t ksc[HPKE_KSC_MAX]) {
  const uint32_t nh = hpke_nh(kdf);
  ksc[0] = 0;
  switch (kdf) {
    case HPKE_KDF_SHA256:
      hpke_labeled_extract_empty_salt<HashSha256>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1);
      hpke_labeled_extract_empty_salt<HashSha256>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh);
      break;
    case HPKE_KDF_SHA384:
      hpke_labeled_extract_empty_salt<HashSha384>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1);
      hpke_labeled_extract_empty_salt<HashSha384>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh);
      break;
    default:
      hpke_labeled_extract_empty_salt<HashSha512>(kdf, aead, "psk_id_hash", nullptr, 0, ksc + 1);
      hpke_labeled_extract_empty_salt<HashSha512>(kdf, aead, "info_hash", info, info_len, ksc + 1 + nh);
      break;
  }
  return 1 + 2 * nh;
}

}  // namespace jx
