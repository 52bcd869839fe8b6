// jx_hpke_default.hip — the default suite's pair of open kernels (jx_hpke.hip has the overview): DHKEM(X25519,
// HKDF-SHA256), HKDF-SHA256, AES-128-GCM, with the register-resident context that only this suite has.
#include "jx_hpke_open.h"

namespace jx {
namespace {

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

__global__ __launch_bounds__(64) void hpke_open_kernel(HpkeDefaultCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  open_body<false>(sbox, cfg, b);
}

__global__ __launch_bounds__(64) void hpke_rows_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<false>(sbox, ra);
}

}  // namespace

void launch_hpke_open_default(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s) {
  HpkeDefaultCfg d{};
  memcpy(d.sk, cfg.key.sk, 32);
  memcpy(d.pk, cfg.key.pk, 32);
  memcpy(d.ksc, cfg.key.ksc, 65);
  memcpy(d.zero_ist, cfg.zero_ist, 32);
  memcpy(d.zero_ost, cfg.zero_ost, 32);
  hipLaunchKernelGGL(hpke_open_kernel, dim3((uint32_t)((b.n + 63) / 64)), dim3(64), 0, s, d, b);
}

void launch_hpke_rows_default(const RowsArgs& ra, hipStream_t s) {
  hipLaunchKernelGGL(hpke_rows_kernel, dim3((uint32_t)((ra.a.n + 63) / 64)), dim3(64), 0, s, ra);
}

}  // namespace jx
