// Host build of the device code behind the P-256 HPKE kernels (janus_amd/csrc/jx_p256.h and the DHKEM(P-256,
// HKDF-SHA256) part of jx_hpke_suites.h), as a shared library for tests/test_hpke_p256_host.py.
// With -DJX_HOSTTEST_MAIN it is a stand-alone program (the same checks against constants baked in below) for a run
// under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_hpke_suites.h"
#define JX_TESTOPS_P256
#include "jx_testops.h"  // what each operation computes, shared with the gfx950 harness (devtest.hip)

using namespace jx;

extern "C" {

// a op b mod p on canonical integers (32 big-endian bytes each), through the Montgomery form the kernels use.
// op: 0 mul, 1 square (of a), 2 inverse (of a; 0 for 0), 3 add, 4 sub. Returns 0 when an operand is >= p.
int hp_fe_op(int op, const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) { return jxt::t_p256_fe_op(op, a, b, out); }

// 1: pt (65 bytes) is a valid encoding of a point of the curve
int hp_point_valid(const uint8_t pt[65]) { return jxt::t_p256_point_valid(pt); }

// sk (32 big-endian bytes) * pt -> x || y (64 bytes). 0 for an invalid point or the point at infinity.
int hp_scalar_mul(const uint8_t sk[32], const uint8_t pt[65], uint8_t out[64]) { return jxt::t_p256_scalar_mul(sk, pt, out); }

// What jx_hpke_create_key checks of a P-256 keypair: 0 when it is accepted, else 1
int hp_keypair(const uint8_t sk[32], const uint8_t pk[65]) {
  uint32_t k[8];
  uint8_t x[32], y[32];
  return hpke_p256_keypair(sk, pk, k, x, y) ? 1 : 0;
}

// What jx_hpke_create_key computes on the host and a lane of the P-256 kernels on the device: the
// key_schedule_context of (kdf, aead, info) under KEM 0x0010 and, for the encapsulated key enc, the AEAD key (32
// bytes, Nk used) and the base nonce. Returns 1, 0 for an encapsulated key that is no point, -1 for a refused
// keypair; ksc_len gets 1 + 2 Nh.
int hp_context(uint32_t kdf, uint32_t aead, const uint8_t sk[32], const uint8_t pk[65], const uint8_t* info,
               uint32_t info_len, const uint8_t enc[65], uint8_t key[32], uint8_t nonce[12], uint8_t ksc[129],
               uint32_t* ksc_len) {
  uint32_t k[8];
  uint8_t x[32], y[32];
  if (hpke_p256_keypair(sk, pk, k, x, y)) return -1;
  *ksc_len = hpke_key_schedule_context(kdf, aead, info, info_len, ksc, HPKE_KEM_P256_SHA256);
  return hpke_p256_context(k, x, y, ksc, kdf, aead, enc, key, nonce) ? 1 : 0;
}

int hp_key_supported(uint32_t kem, uint32_t kdf, uint32_t aead) { return hpke_key_supported(kem, kdf, aead) ? 1 : 0; }

}  // extern "C"

#ifdef JX_HOSTTEST_MAIN
#include "hosttest_hpke_p256_vectors.h"

static int failures = 0;
static void hex(const char* s, uint8_t* out) {
  for (size_t i = 0; s[2 * i]; i++) {
    unsigned v;
    sscanf(s + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}
static void check(const char* what, bool ok) {
  printf("%-52s %s\n", what, ok ? "ok" : "MISMATCH");
  failures += !ok;
}

int main() {
  uint8_t a[32], b[32], want[32], got[64], pt[65], sk[32];
  // field operations: {op, a, b, result} rows
  bool ok = true;
  for (size_t i = 0; i < sizeof(FIELD_CASES) / sizeof(FIELD_CASES[0]); i++) {
    hex(FIELD_CASES[i].a, a), hex(FIELD_CASES[i].b, b), hex(FIELD_CASES[i].r, want);
    ok = ok && hp_fe_op(FIELD_CASES[i].op, a, b, got) == 1 && memcmp(got, want, 32) == 0;
  }
  check("field mul / sq / invert / add / sub", ok);
  hex(P_HEX, a);
  check("an operand >= p is refused", hp_fe_op(0, a, a, got) == 0);
  // scalar multiplications: {sk, point, x || y}
  ok = true;
  for (size_t i = 0; i < sizeof(MUL_CASES) / sizeof(MUL_CASES[0]); i++) {
    uint8_t w[64];
    hex(MUL_CASES[i].sk, sk), hex(MUL_CASES[i].pt, pt), hex(MUL_CASES[i].xy, w);
    ok = ok && hp_scalar_mul(sk, pt, got) == 1 && memcmp(got, w, 64) == 0;
  }
  check("sk * P: 1, 2, 3, n-1, n-2, (n-1)/2, (n+1)/2, 2^128, 2^255", ok);
  // point validation
  ok = true;
  for (size_t i = 0; i < sizeof(POINT_CASES) / sizeof(POINT_CASES[0]); i++) {
    hex(POINT_CASES[i].pt, pt);
    ok = ok && hp_point_valid(pt) == POINT_CASES[i].valid;
  }
  check("point validation (off-curve, x = p, y = p, tags, b')", ok);
  // keypairs
  ok = true;
  for (size_t i = 0; i < sizeof(KEYPAIR_CASES) / sizeof(KEYPAIR_CASES[0]); i++) {
    hex(KEYPAIR_CASES[i].sk, sk), hex(KEYPAIR_CASES[i].pk, pt);
    ok = ok && hp_keypair(sk, pt) == KEYPAIR_CASES[i].refused;
  }
  check("keypairs: sk = 0, sk = n, pk != sk * G refused", ok);
  // RFC 9180 A.3 / A.4-style contexts
  uint8_t info[200], enc[65], k32[32], n12[12], ksc[129], want_key[32], want_nonce[12];
  uint32_t ksc_len;
  ok = true;
  for (size_t i = 0; i < sizeof(CONTEXT_CASES) / sizeof(CONTEXT_CASES[0]); i++) {
    const ContextCase& c = CONTEXT_CASES[i];
    hex(c.sk, sk), hex(c.pk, pt), hex(c.enc, enc), hex(c.info, info), hex(c.key, want_key), hex(c.nonce, want_nonce);
    const uint32_t nk = hpke_nk(c.aead);
    ok = ok && hp_context(c.kdf, c.aead, sk, pt, info, (uint32_t)strlen(c.info) / 2, enc, k32, n12, ksc, &ksc_len) == 1 &&
         memcmp(k32, want_key, nk) == 0 && memcmp(n12, want_nonce, 12) == 0 && ksc_len == 1 + 2 * hpke_nh(c.kdf);
  }
  check("RFC 9180 P-256 vectors: key and base nonce, six suites", ok);
  // every suite at the info lengths on both sides of the hashes' padding boundaries; an off-curve enc fails
  unsigned acc = 0;
  const ContextCase& c0 = CONTEXT_CASES[0];
  hex(c0.sk, sk), hex(c0.pk, pt), hex(c0.enc, enc);
  for (uint32_t i = 0; i < 200; i++) info[i] = (uint8_t)(i * 5 + 1);
  const uint32_t info_lens[5] = {0, 20, 111, 112, 200};
  for (uint32_t kdf = 1; kdf <= 3; kdf++)
    for (uint32_t aead = 1; aead <= 3; aead++)
      for (int j = 0; j < 5; j++) {
        if (hp_context(kdf, aead, sk, pt, info, info_lens[j], enc, k32, n12, ksc, &ksc_len) != 1) failures++;
        acc += k32[0] + n12[0];
        if (ksc_len != 1 + 2 * hpke_nh(kdf)) failures++;
      }
  printf("%-52s ok (%u)\n", "contexts: nine suites x five info lengths", acc);
  enc[40] ^= 1;
  check("an off-curve encapsulated key opens nothing", hp_context(1, 1, sk, pt, info, 0, enc, k32, n12, ksc, &ksc_len) == 0);
  check("ids", hp_key_supported(0x10, 1, 1) && hp_key_supported(0x20, 3, 3) && !hp_key_supported(0x11, 1, 1) &&
                   !hp_key_supported(0x10, 4, 1) && !hp_key_supported(0x10, 1, 0));
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
#endif
