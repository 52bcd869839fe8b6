// Host build of the device arithmetic headers (janus_amd/csrc/jx_*.h), so the exact
// field / Keccak / SHA-256 code the kernels inline is checked against the oracle on
// the CPU (tests/test_device_math_host.py). Test-only; not part of the product.
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_field.h"
#include "../../janus_amd/csrc/jx_keccak.h"
#include "../../janus_amd/csrc/jx_sha256.h"
#include "../../janus_amd/csrc/jx_hpke.h"
#include "../../janus_amd/csrc/jx_sha_aes.h"
#include "../../janus_amd/csrc/jx_sample.h"
#define JX_TESTOPS_BASE
#define JX_TESTOPS_SAMPLE
#include "jx_testops.h"  // what each operation computes, shared with the gfx950 harness (devtest.hip)

using namespace jx;
using namespace jxt;

extern "C" {
// op: 0 add, 1 sub, 2 mont, 3 to_mont, 4 from_mont, 5 neg
void ht_f128(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) { t_f128(op, a, b, out); }
void ht_reduce192(const uint64_t w[3], uint8_t* out) { t_reduce192(w, out); }
// wacc_reduce of nine raw column sums (each < 2^63, the wire-sum bound)
void ht_wacc_reduce(const uint64_t cols[9], uint8_t* out) { t_wacc_reduce(cols, out); }
void ht_reduce192_small(const uint64_t w[3], uint8_t* out) { t_reduce192_small(w, out); }
void ht_mont_lazy(const uint8_t* a, const uint8_t* b, uint64_t out[3]) { t_mont_lazy(a, b, out); }
// sum_k xs[k] * cs[k] mod p through the 26-bit-limb column accumulator, normalising every
// `norm_every` terms (the FLP kernel normalises every 512 calls)
void ht_wide_dot(const uint8_t* xs, const uint8_t* cs, int n, int norm_every, uint8_t* out) { t_wide_dot(xs, cs, n, norm_every, out); }
// ---- HPKE primitives (jx_hpke.h)
void ht_x25519(const uint8_t k[32], const uint8_t u[32], uint8_t out[32]) { t_x25519(k, u, out); }
// op: 0 mul, 1 sq, 2 sub, 3 invert, 4 mul_small(121665); inputs/outputs canonical 32-byte LE
void ht_fe(int op, const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) { t_fe(op, a, b, out); }
// op 0 mul, 1 sq, 4 mul_small(121665) on raw limbs (loosely reduced inputs up to 2^28 - 1, as fe_sub / fe_add
// produce them inside the ladder); the output limbs as the reduction leaves them (bounds checked by the test)
void ht_fe_limbs(int op, const uint32_t a[10], const uint32_t b[10], uint32_t out[10]) { t_fe_limbs(op, a, b, out); }
static uint8_t HT_SBOX[256];
static void ht_sbox_init() {
  // FIPS 197 S-box generated from GF(2^8) inverses (independent of the kernel's table)
  uint8_t inv[256] = {0};
  for (int x = 1; x < 256; x++)
    for (int y = 1; y < 256; y++) {
      int a = x, b = y, r = 0;
      for (int i = 0; i < 8; i++) {
        if (b & 1) r ^= a;
        int hi = a & 0x80;
        a = (a << 1) & 0xff;
        if (hi) a ^= 0x1b;
        b >>= 1;
      }
      if (r == 1) {
        inv[x] = (uint8_t)y;
        break;
      }
    }
  for (int x = 0; x < 256; x++) {
    int b = inv[x], s = b;
    for (int i = 1; i < 5; i++) s ^= ((b << i) | (b >> (8 - i))) & 0xff;
    HT_SBOX[x] = (uint8_t)(s ^ 0x63);
  }
}
void ht_aes128(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  ht_sbox_init();
  uint32_t k[4], rk[44], i4[4], o4[4];
  memcpy(k, key, 16);
  memcpy(i4, in, 16);
  aes128_expand_key(HT_SBOX, k, rk);
  aes128_encrypt(HT_SBOX, rk, i4, o4);
  memcpy(out, o4, 16);
}
// x, h: 16-byte blocks; out = x * h in GF(2^128) (GCM bit order)
void ht_ghash_mul(const uint8_t x[16], const uint8_t h[16], uint8_t out[16]) { t_ghash_mul(x, h, out); }
// HMAC-SHA256 with a 32-byte key over msg (len <= 119) through hmac_pads/sha256_finish64/hmac_outer
void ht_hmac32(const uint8_t key[32], const uint8_t* msg, int len, uint8_t out[32]) { t_hmac32(key, msg, len, out); }
// op: 0 add, 1 sub, 2 mul
uint64_t ht_f64(int op, uint64_t a, uint64_t b) { return t_f64(op, a, b); }
void ht_keccak_p12(uint64_t st64[25]) { t_keccak_p12(st64); }
void ht_sha256_16(const uint8_t id[16], uint8_t out[32]) { t_sha256_16(id, out); }
// XOF prefix block builder: returns the 42 words of a one-block message
// prefix(algo, usage, seed) || binder (<= 142 bytes), padded.
void ht_xof_block(uint32_t algo, uint32_t usage, const uint8_t seed[16], const uint8_t* binder, int blen,
                  uint32_t out[42]) {
  Block b;
  blk_zero(b);
  uint32_t sw[4];
  memcpy(sw, seed, 16);
  int pos = blk_xof_prefix(b, algo, usage, sw);
  for (int i = 0; i < blen; i++) blk_put_byte(b, pos + i, binder[i]);
  blk_pad(b, pos + blen);
  memcpy(out, b.w, sizeof b.w);
}
// T-table AES of the XofHmacSha256Aes128 kernels (jx_sha_aes.h): otf = 0 expands the 44-word
// schedule first, otf = 1 computes it on the fly
void ht_aes128_t(int otf, const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  ht_sbox_init();
  static uint32_t t0[256];
  for (int x = 0; x < 256; x++) t0[x] = aes_t0_entry(HT_SBOX[x]);
  t_aes128_t(otf, t0, key, in, out);
}
uint32_t ht_be_word_shift16(uint32_t lo, uint32_t hi) { return be_word_shift16(lo, hi); }
// sum_k xs[k] * cs[k] mod p64 through the Field64 limb column accumulator (folding every 1024 terms)
uint64_t ht_wacc64_dot(const uint64_t* xs, const uint64_t* cs, int n) { return t_wacc64_dot(xs, cs, n); }
uint64_t ht_reduce192_p64(const uint64_t w[3]) { return t_reduce192_p64(w); }
// ---- exact ">= p" predicates and rejection sampling (jx_field.h, jx_sample.h)
int ht_ge_p128(const uint8_t* a) { return t_ge_p128(a); }
int ht_ge_p64(uint32_t lo, uint32_t hi) { return t_ge_p64(lo, hi); }
int ht_ge_exact(const uint8_t* a) { return t_ge_exact(a); }
// the running max of ge_screen over n 16-byte elements, as the XOF kernels keep it per block
uint32_t ht_ge_screen_max(const uint8_t* a, int n) { return t_ge_screen_max(a, n); }
// sample64<N> (N = 1 | 5) on a Keccak state whose first block is ready; the state is left as sampling left it
void ht_sample64(int n, uint64_t st64[25], uint64_t* out) { t_sample64(n, st64, out); }
void ht_sample2_f128(uint64_t st64[25], uint32_t cnt, int slow, uint8_t out[32], uint32_t* flags) { t_sample2_f128(st64, cnt, slow, out, flags); }
// n elements from the byte stream that starts at byte `pos` of the block in st64; returns the final position
uint32_t ht_bx_sample128(uint64_t st64[25], uint32_t pos, int n, uint8_t* out) { return t_bx_sample128(st64, pos, n, out); }
// xof_stream128: n elements into out[16 n]; returns the number of emit calls, | 2^31 if their k was not 0, 1, 2, ...
uint32_t ht_xof_stream128(const uint64_t st64[25], uint32_t n, uint8_t* out) { return t_xof_stream128(st64, n, out); }
}
