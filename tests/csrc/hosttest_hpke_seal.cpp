// Host build of the serial seal bodies behind the HPKE seal kernels (janus_amd/csrc/jx_hpke_seal.h): encapsulation
// and key schedule, the one-message-per-lane AEAD seals, and the ChaCha20-Poly1305 split of a long message over 64
// lanes, one loop iteration per lane. A shared library for tests/test_hpke_seal_host.py; with -DJX_HOSTTEST_MAIN a
// stand-alone program (RFC 9180 A.1.1 plus sweeps over lengths) for a run under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../janus_amd/csrc/jx_hpke_seal.h"

using namespace jx;

static void words_le(const uint8_t* p, int n, uint32_t* w) {
  for (int i = 0; i < n; i++)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
}
static void bytes_le(const uint32_t* w, int n, uint8_t* p) {
  for (int i = 0; i < 4 * n; i++) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

extern "C" {

// Encap and the key schedule as a lane pair computes them (here one ladder after the other): enc, the AEAD key (32
// bytes, Nk used) and the base nonce for ephemeral key ske (clamped here) and recipient key pk. 0 for an all-zero DH.
int hq_context(uint32_t kdf, uint32_t aead, const uint8_t ske[32], const uint8_t pk[32], const uint8_t* info,
               uint32_t info_len, uint8_t enc[32], uint8_t key[32], uint8_t nonce[12]) {
  uint32_t k[8], pkw[8], u[8], encw[8], dh[8], zist[8], zost[8];
  words_le(ske, 8, k);
  x25519_clamp(k);
  words_le(pk, 8, pkw);
  x25519_base_point(u);
  x25519_ladder(encw, k, u);
  x25519_ladder(dh, k, pkw);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, zist, zost);
  uint8_t ksc[HPKE_KSC_MAX];
  hpke_key_schedule_context(kdf, aead, info, info_len, ksc);
  const bool nz = hpke_seal_context(encw, dh, pkw, ksc, kdf, aead, zist, zost, key, nonce);
  bytes_le(encw, 8, enc);
  return nz ? 1 : 0;
}

// The AEAD of the suite, one message per lane: ct gets plen + 16 bytes. key: 32 bytes, Nk used.
void hq_aead_seal(uint32_t aead, const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad, uint64_t alen,
                  const uint8_t* pt, uint64_t plen, uint8_t* ct) {
  suite_aead_seal(AES_SBOX, aead, key, nonce, alen, [&](uint64_t i) { return aad[i]; }, plen,
                  [&](uint64_t i) { return pt[i]; }, ct);
}

// The whole short-form seal. 0 (and nothing written) for an all-zero DH.
int hq_seal(uint32_t kdf, uint32_t aead, const uint8_t ske[32], const uint8_t pk[32], const uint8_t* info,
            uint32_t info_len, const uint8_t* aad, uint64_t alen, const uint8_t* pt, uint64_t plen, uint8_t enc[32],
            uint8_t* ct) {
  uint8_t key[32], nonce[12];
  if (!hq_context(kdf, aead, ske, pk, info, info_len, enc, key, nonce)) return 0;
  hq_aead_seal(aead, key, nonce, aad, alen, pt, plen, ct);
  return 1;
}

// ChaCha20-Poly1305 seal of one message as the 64 lanes of a wave split it (chapoly_wave_seal of jx_hpke_seal.hip):
// the same per-lane functions, the shuffles replaced by arrays indexed by lane.
void hq_chapoly_lanes_seal(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad, uint64_t alen,
                           const uint8_t* pt, uint64_t plen, uint8_t* ct) {
  uint32_t kw[8], nw[3], ks0[16];
  words_le(key, 8, kw);
  words_le(nonce, 3, nw);
  chacha20_block(kw, 0, nw, ks0);
  Poly1305 st;
  poly1305_init(st, ks0);
  uint32_t pw[GL_LANES][5];  // lane l: r^(l+1)
  for (int k = 0; k < 5; k++) pw[0][k] = st.r[k];
  for (uint32_t l = 1; l < GL_LANES; l++) {
    for (int k = 0; k < 5; k++) pw[l][k] = pw[l - 1][k];
    pl_mul(pw[l], st.r);
  }
  uint32_t rgap[5];
  for (int k = 0; k < 5; k++) rgap[k] = pw[SL_GAP - 3 * GL_LANES - 1][k];
  for (int i = 0; i < 3; i++) pl_mul(rgap, pw[63]);
  const uint64_t na = (alen + 15) / 16, nc = (plen + 15) / 16;
  auto ld = [](const uint8_t* p, uint64_t o, uint32_t len, uint32_t m[4]) {
    m[0] = m[1] = m[2] = m[3] = 0;
    for (uint32_t k = 0; k < len; k++) m[k >> 2] |= (uint32_t)p[o + k] << (8 * (k & 3));
  };
  uint32_t a0[5] = {0, 0, 0, 0, 0};
  if (na) {
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (uint32_t lane = 0; lane < GL_LANES; lane++) {
      uint32_t pa[5];
      pl_lane_partial(
          na, lane,
          [&](uint64_t k, uint32_t m[4]) { ld(aad, 16 * k, alen - 16 * k < 16 ? (uint32_t)(alen - 16 * k) : 16u, m); },
          pw[63], pa);
      const uint32_t d = gl_lane_exponent(na, lane);
      pl_lane_term(pa, pw[d ? d - 1 : 0]);
      for (int k = 0; k < 5; k++) sum[k] += pa[k];
    }
    pl_sum_carry(sum, a0);
  }
  uint32_t sum[5] = {0, 0, 0, 0, 0};
  for (uint32_t lane = 0; lane < GL_LANES; lane++) {
    uint32_t p[5], ks[16];
    const uint32_t d = sl_lane_partial(
        nc, lane,
        [&](uint64_t b) {
          if (64 * b < plen) chacha20_block(kw, cl_counter(b), nw, ks);
        },
        [&](uint64_t b, uint32_t q, uint32_t m[4]) {
          const uint64_t mi = 4 * b + q;
          if (mi == nc) {
            pl_len_block(alen, plen, m);
            return;
          }
          const uint64_t o = 16 * mi;
          const uint32_t len = plen - o < 16 ? (uint32_t)(plen - o) : 16u;
          ld(pt, o, len, m);
          for (int w = 0; w < 4; w++) m[w] ^= ks[4 * q + w];
          for (uint32_t k = len; k < 16; k++) m[k >> 2] &= ~(0xffu << (8 * (k & 3)));
          for (uint32_t k = 0; k < len; k++) ct[o + k] = (uint8_t)(m[k >> 2] >> (8 * (k & 3)));
        },
        st.r, rgap, a0, p);
    const uint32_t e = d ? d - 1 : 0;
    uint32_t rd[5];
    for (int k = 0; k < 5; k++) rd[k] = pw[e & (GL_LANES - 1)][k];
    for (uint32_t i = 0; i < 3; i++)
      if (i < (e >> 6)) pl_mul(rd, pw[63]);
    pl_lane_term(p, rd);
    for (int k = 0; k < 5; k++) sum[k] += p[k];
  }
  uint32_t tag[4];
  pl_finish(st, sum, tag);
  bytes_le(tag, 4, ct + plen);
}

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
  printf("%-52s %s\n", what, ok ? "ok" : "MISMATCH");
  failures += !ok;
}

int main() {
  // RFC 9180 A.1.1: DHKEM(X25519, HKDF-SHA256), HKDF-SHA256, AES-128-GCM, sequence number 0
  uint8_t ske[32], pk[32], info[20], aad[8], enc[32], ct[29 + 16];
  hex("52c4a758a802cd8b936eceea314432798d5baf2d7e9235dc084ab1b9cfa2f736", ske);
  hex("3948cfe0ad1ddb695d780e59077195da6c56506b027329794ab02bca80815c4d", pk);
  hex("4f6465206f6e2061204772656369616e2055726e", info);
  hex("436f756e742d30", aad);
  const char* pt = "Beauty is truth, truth beauty";
  const int nz = hq_seal(1, 1, ske, pk, info, 20, aad, 7, (const uint8_t*)pt, 29, enc, ct);
  failures += nz != 1;
  expect("RFC 9180 A.1.1 enc", enc, "37fda3567bdbd628e88668c3c8d7e97d1d1253b6d4ea6d44c150f741f1bf4431", 32);
  expect("RFC 9180 A.1.1 ct (sequence number 0)", ct,
         "f938558b5d72f1a23810b4be2ab4f84331acc02fc97babc53a52ae8218a355a96d8770ac83d07bea87e13c512a", 45);
  // every suite at lengths on both sides of the AEADs' block sizes; the lanes' split against the serial seal
  std::vector<uint8_t> buf(9000 + 1025), c1(9000 + 16), c2(9000 + 16);
  for (size_t i = 0; i < buf.size(); i++) buf[i] = (uint8_t)(31 * i + 7);
  unsigned acc = 0;
  const uint64_t lens[] = {0, 1, 15, 16, 17, 54, 63, 64, 65, 255, 1023, 4095, 4096, 4097, 8191, 9000};
  for (uint32_t kdf = 1; kdf <= 3; kdf++)
    for (uint32_t aead = 1; aead <= 3; aead++)
      for (uint64_t len : lens) {
        if (len > 255 && kdf != 1) continue;
        failures += hq_seal(kdf, aead, ske, pk, info, 20, buf.data() + 1, len % 93, buf.data() + 3, len, enc, c1.data()) != 1;
        acc += c1[len];
      }
  uint8_t key[32], nonce[12];
  hq_context(1, 3, ske, pk, info, 20, enc, key, nonce);
  for (uint64_t len : lens)
    for (uint64_t alen : {0, 1, 16, 60, 92, 1025}) {
      hq_aead_seal(3, key, nonce, buf.data() + 1, alen, buf.data() + 3, len, c1.data());
      hq_chapoly_lanes_seal(key, nonce, buf.data() + 1, alen, buf.data() + 3, len, c2.data());
      if (memcmp(c1.data(), c2.data(), len + 16) != 0) {
        printf("lanes split differs at len %llu, aad %llu\n", (unsigned long long)len, (unsigned long long)alen);
        failures++;
      }
    }
  failures += hq_seal(1, 1, ske, (const uint8_t*)"\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0", info, 20, aad, 7,
                      (const uint8_t*)pt, 29, enc, ct) != 0;
  printf("%-52s ok (%u)\n", "sweeps: nine suites, the lanes' ChaCha20-Poly1305 split", acc);
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
#endif
