// Host AEAD sealing for tools/bench_upload.py: 138 MB of leader shares cannot be sealed by the Python references
// in useful time, so the benchmark's inputs (never a test's) are sealed by the kernels' own AES / GHASH / ChaCha20 /
// Poly1305 code built for the host. g++ -O2 -std=c++17 -shared -fPIC.
#include <stdint.h>
#include <string.h>

#include "../janus_amd/csrc/jx_chapoly.h"
#include "../janus_amd/csrc/jx_ghash_lanes.h"

using namespace jx;

namespace {
struct Tab4 {
  uint32_t m[16][4];
  void operator()(uint32_t n, uint32_t e[4]) const { memcpy(e, m[n], 16); }
};
void ld_be(const uint8_t* p, uint64_t n, uint32_t x[4]) {
  uint8_t b[16] = {0};
  memcpy(b, p, n < 16 ? n : 16);
  for (int i = 0; i < 4; i++)
    x[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
template <int NR>
void gcm_seal(const uint32_t* rk, const uint8_t* nonce, const uint8_t* aad, uint64_t alen, const uint8_t* pt,
              uint64_t n, uint8_t* out) {
  uint32_t zero4[4] = {0, 0, 0, 0}, hb[4], h[4], cb[4], ks[4];
  aes_encrypt_nr<NR>(AES_SBOX, rk, zero4, hb);
  for (int i = 0; i < 4; i++) h[i] = bswap32(hb[i]);
  Tab4 t;
  for (uint32_t k = 0; k < 16; k++) gl_tab4_entry(k, h, t.m[k]);
  memcpy(cb, nonce, 12);
  for (uint64_t i = 0; i < n; i += 16) {
    cb[3] = bswap32((uint32_t)(2 + i / 16));
    aes_encrypt_nr<NR>(AES_SBOX, rk, cb, ks);
    for (uint64_t j = 0; j < 16 && i + j < n; j++) out[i + j] = pt[i + j] ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3)));
  }
  uint32_t y[4] = {0, 0, 0, 0}, x[4];
  for (uint64_t i = 0; i < alen; i += 16) {
    ld_be(aad + i, alen - i, x);
    for (int k = 0; k < 4; k++) y[k] ^= x[k];
    ghash_mul_tab4(y, t);
  }
  for (uint64_t i = 0; i < n; i += 16) {
    ld_be(out + i, n - i, x);
    for (int k = 0; k < 4; k++) y[k] ^= x[k];
    ghash_mul_tab4(y, t);
  }
  gl_finish(y, alen, n, h);
  cb[3] = bswap32(1u);
  aes_encrypt_nr<NR>(AES_SBOX, rk, cb, ks);
  for (int k = 0; k < 4; k++) {
    const uint32_t w = bswap32(ks[k]) ^ y[k];
    for (int q = 0; q < 4; q++) out[n + 4 * k + q] = (uint8_t)(w >> (24 - 8 * q));
  }
}
}  // namespace

extern "C" {

// aead: 1 AES-128-GCM, 2 AES-256-GCM, 3 ChaCha20Poly1305 (key: 16 or 32 bytes; nonce: 12). out: n + 16 bytes.
void us_seal(uint32_t aead, const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, uint64_t alen,
             const uint8_t* pt, uint64_t n, uint8_t* out) {
  uint32_t kw[8] = {0}, rk[60];
  memcpy(kw, key, aead == 1 ? 16 : 32);
  if (aead == 1) {
    aes128_expand_key(AES_SBOX, kw, rk);
    gcm_seal<10>(rk, nonce, aad, alen, pt, n, out);
    return;
  }
  if (aead == 2) {
    aes256_expand_key(AES_SBOX, kw, rk);
    gcm_seal<14>(rk, nonce, aad, alen, pt, n, out);
    return;
  }
  uint32_t nw[3], ks[16];
  memcpy(nw, nonce, 12);
  for (uint64_t i = 0; i < n; i += 64) {
    chacha20_block(kw, (uint32_t)(1 + i / 64), nw, ks);
    for (uint64_t j = 0; j < 64 && i + j < n; j++) out[i + j] = pt[i + j] ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3)));
  }
  chacha20_block(kw, 0, nw, ks);
  Poly1305 p;
  poly1305_init(p, ks);
  uint32_t m[4];
  for (uint64_t i = 0; i < alen; i += 16) {
    ld_block_le(aad, i, alen, m);
    poly1305_block(p, m, 1);
  }
  for (uint64_t i = 0; i < n; i += 16) {
    ld_block_le(out, i, n, m);
    poly1305_block(p, m, 1);
  }
  const uint32_t lens[4] = {(uint32_t)alen, (uint32_t)(alen >> 32), (uint32_t)n, (uint32_t)(n >> 32)};
  poly1305_block(p, lens, 1);
  uint32_t tag[4];
  poly1305_finish(p, tag);
  memcpy(out + n, tag, 16);
}

}  // extern "C"
