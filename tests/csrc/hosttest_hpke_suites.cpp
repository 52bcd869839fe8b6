// Host build of the device headers behind the HPKE suite kernels (janus_amd/csrc/jx_sha512.h, jx_chapoly.h,
// jx_hpke_suites.h, AES-256 of jx_sha_aes.h), as a shared library for tests/test_hpke_suites_host.py.
// With -DJX_HOSTTEST_MAIN it is a stand-alone program (known answers plus sweeps over lengths) for a run under
// -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_hpke_suites.h"

using namespace jx;

static void words_le(const uint8_t* p, int n, uint32_t* w) {
  for (int i = 0; i < n; i++)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
}
static void bytes_le(const uint32_t* w, int n, uint8_t* p) {
  for (int i = 0; i < 4 * n; i++) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

template <class H>
static int hmac_any(const uint8_t* key, uint32_t klen, const uint8_t* msg, uint32_t len, uint8_t* out) {
  typename H::W ist[8], ost[8];
  hmac_pads_t<H>(key, klen, ist, ost);
  hmac_finish_t<H>(out, ist, ost, msg, len);
  return H::NH;
}

extern "C" {

// kind: 1 SHA-256, 2 SHA-384, 3 SHA-512 (the HPKE KDF ids). Returns the digest length.
int hs_hash(int kind, const uint8_t* msg, uint32_t len, uint8_t* out) {
  switch (kind) {
    case 1: hash_bytes<HashSha256>(out, msg, len); return 32;
    case 2: hash_bytes<HashSha384>(out, msg, len); return 48;
    default: hash_bytes<HashSha512>(out, msg, len); return 64;
  }
}

int hs_hmac(int kind, const uint8_t* key, uint32_t klen, const uint8_t* msg, uint32_t len, uint8_t* out) {
  switch (kind) {
    case 1: return hmac_any<HashSha256>(key, klen, msg, len, out);
    case 2: return hmac_any<HashSha384>(key, klen, msg, len, out);
    default: return hmac_any<HashSha512>(key, klen, msg, len, out);
  }
}

void hs_aes256(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]) {
  uint32_t k[8], rk[60], i4[4], o4[4];
  words_le(key, 8, k);
  words_le(in, 4, i4);
  aes256_expand_key(AES_SBOX, k, rk);
  aes256_encrypt(AES_SBOX, rk, i4, o4);
  bytes_le(o4, 4, out);
}

void hs_chacha20_block(const uint8_t key[32], uint32_t counter, const uint8_t nonce[12], uint8_t out[64]) {
  uint32_t k[8], n[3], o[16];
  words_le(key, 8, k);
  words_le(nonce, 3, n);
  chacha20_block(k, counter, n, o);
  bytes_le(o, 16, out);
}

// tag of msg under the one-time key; h_pre: the accumulator's limbs after the last block and a full carry, before
// the final reduction mod 2^130 - 5
void hs_poly1305(const uint8_t key[32], const uint8_t* msg, uint64_t len, uint8_t tag[16], uint32_t h_pre[5]) {
  uint32_t k[8], t[4];
  words_le(key, 8, k);
  Poly1305 p;
  poly1305_init(p, k);
  poly1305_absorb(p, len, [&](uint64_t i) { return msg[i]; });
  Poly1305 q = p;
  poly1305_carry(q);
  for (int i = 0; i < 5; i++) h_pre[i] = q.h[i];
  poly1305_finish(p, t);
  bytes_le(t, 4, tag);
}

// ct: ciphertext || 16-byte tag (n >= 16 bytes). 1 and the plaintext in pt when the tag matches, else 0.
int hs_chapoly_open(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad, uint64_t alen, const uint8_t* ct,
                    uint64_t n, uint8_t* pt) {
  uint32_t k[8], nw[3];
  words_le(key, 8, k);
  words_le(nonce, 3, nw);
  if (!chapoly_tag_ok(k, nw, alen, [&](uint64_t i) { return aad[i]; }, ct, n - 16)) return 0;
  chapoly_decrypt(k, nw, ct, n - 16, pt);
  return 1;
}

// What jx_hpke_create_suite computes on the host and a lane of the suite kernels on the device: the
// key_schedule_context of (kdf, aead, info) and, for encapsulated key enc, the AEAD key (32 bytes, Nk used) and
// the base nonce. Returns 0 for an all-zero DH output, else 1; ksc_len gets 1 + 2 Nh.
int hs_context(uint32_t kdf, uint32_t aead, const uint8_t sk[32], const uint8_t pk[32], const uint8_t* info,
               uint32_t info_len, const uint8_t enc[32], uint8_t key[32], uint8_t nonce[12], uint8_t ksc[129],
               uint32_t* ksc_len) {
  uint8_t k[32];
  memcpy(k, sk, 32);
  k[0] &= 248;
  k[31] &= 127;
  k[31] |= 64;
  uint32_t skw[8], pkw[8], encw[8], zist[8], zost[8];
  words_le(k, 8, skw);
  words_le(pk, 8, pkw);
  words_le(enc, 8, encw);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, zist, zost);
  *ksc_len = hpke_key_schedule_context(kdf, aead, info, info_len, ksc);
  return hpke_suite_context(skw, pkw, ksc, kdf, aead, zist, zost, encw, key, nonce) ? 1 : 0;
}

int hs_supported(uint32_t kem, uint32_t kdf, uint32_t aead) { return hpke_suite_supported(kem, kdf, aead) ? 1 : 0; }

}  // extern "C"

#ifdef JX_HOSTTEST_MAIN
static int failures = 0;
static void hex(const char* s, uint8_t* out) {
  for (size_t i = 0; s[2 * i]; i++) {
    unsigned v;
    sscanf(s + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}
static void expect(const char* what, const uint8_t* got, const char* want_hex, size_t n) {
  uint8_t want[256];
  hex(want_hex, want);
  const bool ok = memcmp(got, want, n) == 0;
  printf("%-44s %s\n", what, ok ? "ok" : "MISMATCH");
  failures += !ok;
}

int main() {
  uint8_t out[64], buf[600];
  // FIPS 180-4 "abc"
  hs_hash(3, (const uint8_t*)"abc", 3, out);
  expect("SHA-512(abc)", out,
         "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e"
         "2a9ac94fa54ca49f",
         64);
  hs_hash(2, (const uint8_t*)"abc", 3, out);
  expect("SHA-384(abc)", out,
         "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7", 48);
  hs_hash(1, (const uint8_t*)"abc", 3, out);
  expect("SHA-256(abc), generic path", out, "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad", 32);
  // every length across three block boundaries, and HMAC with every key length up to the block
  for (uint32_t i = 0; i < sizeof(buf); i++) buf[i] = (uint8_t)(31 * i + 7);
  unsigned acc = 0;
  for (int kind = 1; kind <= 3; kind++)
    for (uint32_t len = 0; len <= 400; len++) {
      hs_hash(kind, buf, len, out);
      acc += out[0];
      if (len <= (kind == 1 ? 64u : 128u)) {
        hs_hmac(kind, buf + 1, len, buf, 400 - len, out);
        acc += out[1];
      }
    }
  printf("%-44s ok (%u)\n", "hash / HMAC sweeps over lengths 0..400", acc);
  // FIPS 197 C.3
  uint8_t key[32], blk[16], ct16[16];
  for (int i = 0; i < 32; i++) key[i] = (uint8_t)i;
  hex("00112233445566778899aabbccddeeff", blk);
  hs_aes256(key, blk, ct16);
  expect("AES-256 FIPS 197 C.3", ct16, "8ea2b7ca516745bfeafc49904b496089", 16);
  // RFC 8439 §2.3.2
  uint8_t nonce[12], ks[64];
  hex("000000090000004a00000000", nonce);
  hs_chacha20_block(key, 1, nonce, ks);
  expect("ChaCha20 block RFC 8439 2.3.2", ks,
         "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9"
         "cbd083e8a2503c4e",
         64);
  // RFC 8439 §2.5.2
  uint8_t pkey[32], tag[16];
  uint32_t hpre[5];
  hex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b", pkey);
  const char* m = "Cryptographic Forum Research Group";
  hs_poly1305(pkey, (const uint8_t*)m, strlen(m), tag, hpre);
  expect("Poly1305 RFC 8439 2.5.2", tag, "a8061dc1305136c6c22b8baf0c0127a9", 16);
  for (uint64_t len = 0; len <= 70; len++) {
    hs_poly1305(pkey, buf, len, tag, hpre);
    acc += tag[0];
  }
  // RFC 8439 §2.8.2
  uint8_t akey[32], aad[12], ct[130], pt[114];
  for (int i = 0; i < 32; i++) akey[i] = (uint8_t)(0x80 + i);
  hex("070000004041424344454647", nonce);
  hex("50515253c0c1c2c3c4c5c6c7", aad);
  hex("d31a8d34648e60db7b86afbc53ef7ec2a4aded51296e08fea9e2b5a736ee62d63dbea45e8ca9671282fafb69da92728b1a71de0a9e060b29"
      "05d6a5b67ecd3b3692ddbd7f2d778b8c9803aee328091b58fab324e4fad675945585808b4831d7bc3ff4def08e4b7a9de576d26586cec64b"
      "61161ae10b594f09e26a7e902ecbd0600691",
      ct);
  const int opened = hs_chapoly_open(akey, nonce, aad, 12, ct, 130, pt);
  const char* want_pt =
      "Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be it.";
  const bool aead_ok = opened == 1 && memcmp(pt, want_pt, 114) == 0;
  printf("%-44s %s\n", "ChaCha20-Poly1305 open RFC 8439 2.8.2", aead_ok ? "ok" : "MISMATCH");
  failures += !aead_ok;
  ct[3] ^= 1;
  const bool rejects = hs_chapoly_open(akey, nonce, aad, 12, ct, 130, pt) == 0;
  printf("%-44s %s\n", "ChaCha20-Poly1305 rejects a flipped bit", rejects ? "ok" : "MISMATCH");
  failures += !rejects;
  // RFC 9180 A.1.1 / A.2.1-style contexts: the vectors for (1, 1) and (3, 3) (base nonce), then every suite at
  // the info lengths on both sides of the SHA-512 block boundary
  uint8_t sk[32], pk[32], enc[32], info[200], k32[32], n12[12], ksc[129];
  uint32_t ksc_len;
  hex("4612c550263fc8ad58375df3f557aac531d26850903e55a9f23f21d8534e8ac8", sk);
  hex("3948cfe0ad1ddb695d780e59077195da6c56506b027329794ab02bca80815c4d", pk);
  hex("37fda3567bdbd628e88668c3c8d7e97d1d1253b6d4ea6d44c150f741f1bf4431", enc);
  hex("4f6465206f6e2061204772656369616e2055726e", info);
  hs_context(1, 1, sk, pk, info, 20, enc, k32, n12, ksc, &ksc_len);
  expect("RFC 9180 A.1.1 base nonce (SHA256, AES-128)", n12, "56d890e5accaaf011cff4b7d", 12);
  expect("RFC 9180 A.1.1 key", k32, "4531685d41d65f03dc48f6b8302c05b0", 16);
  for (uint32_t i = 0; i < 200; i++) info[i] = (uint8_t)(i * 5 + 1);
  const uint32_t info_lens[5] = {0, 20, 111, 112, 200};
  for (uint32_t kdf = 1; kdf <= 3; kdf++)
    for (uint32_t aead = 1; aead <= 3; aead++)
      for (int j = 0; j < 5; j++) {
        const int nz = hs_context(kdf, aead, sk, pk, info, info_lens[j], enc, k32, n12, ksc, &ksc_len);
        acc += k32[0] + n12[0] + nz;
        if (ksc_len != 1 + 2 * hpke_nh(kdf)) failures++;
      }
  printf("%-44s ok (%u)\n", "contexts: nine suites x five info lengths", acc);
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
#endif
