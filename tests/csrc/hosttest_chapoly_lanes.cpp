// Host build of janus_amd/csrc/jx_chapoly_lanes.h for tests/test_chapoly_lanes_host.py: the 64 lanes of the wave are
// a loop, a shuffle is an array index, and what the kernel of jx_hpke_long.hip indexes is what this indexes.
// g++ -O2 -std=c++17 -shared -fPIC. With -DJX_HOSTTEST_MAIN it is a stand-alone program (a fixed subset of the same
// cases against the serial code of jx_chapoly.h and two constants from tests/hpke_suites_ref.py) for a run under
// -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../janus_amd/csrc/jx_chapoly_lanes.h"
#define JX_TESTOPS_CHAPOLY
#include "jx_testops.h"  // what each operation computes, shared with the gfx950 harness (devtest.hip)

using namespace jx;

namespace {

void le_words(const uint8_t* b, int n, uint32_t* w) {
  for (int i = 0; i < n; i++)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
void le_bytes(const uint32_t* w, int n, uint8_t* b) {
  for (int i = 0; i < 4 * n; i++) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// The tag of the emulated wave under the one-time key in st. rot: the lane the emulation starts from (the lanes run
// and are summed from there on, which must not matter). exps: the exponent each lane used; sum_out: the limb-wise sum
// of the 64 terms. Returns false when a 32-bit limb sum wrapped (it is summed in 64 bits beside).
bool wave_tag(Poly1305& st, const uint8_t* aad, uint64_t alen, const uint8_t* ct, uint64_t clen, uint32_t rot,
              uint32_t tag[4], uint32_t* exps, uint32_t* sum_out) {
  uint32_t pw[GL_LANES][5];  // lane l: r^(l+1)
  for (uint32_t l = 0; l < GL_LANES; l++) memcpy(pw[l], st.r, 20);
  for (int s = 0; s < 6; s++) {
    uint32_t next[GL_LANES][5];
    memcpy(next, pw, sizeof pw);
    for (uint32_t l = 0; l < GL_LANES; l++) {
      uint32_t other[5];
      memcpy(other, pw[gl_pow_src_other(s, l)], 20);
      pl_mul(other, pw[gl_pow_src_base(s)]);
      if (gl_pow_active(s, l)) memcpy(next[l], other, 20);
    }
    memcpy(pw, next, sizeof pw);
  }
  const uint64_t na = (alen + 15) / 16, nc = (clen + 15) / 16, N = pl_mac_blocks(alen, clen);
  auto block = [&](uint64_t k, uint32_t m[4]) {
    if (k < na)
      ld_block_le(aad, 16 * k, alen, m);
    else if (k < na + nc)
      ld_block_le(ct, 16 * (k - na), clen, m);
    else
      pl_len_block(alen, clen, m);
  };
  uint32_t sum[5] = {0, 0, 0, 0, 0};
  uint64_t wide[5] = {0, 0, 0, 0, 0};
  for (uint32_t i = 0; i < GL_LANES; i++) {
    const uint32_t j = (i + rot) % GL_LANES;
    uint32_t p[5];
    pl_lane_partial(N, j, block, pw[63], p);
    const uint32_t d = gl_lane_exponent(N, j);
    if (exps) exps[j] = d;
    pl_lane_term(p, pw[d ? d - 1 : 0]);
    for (int k = 0; k < 5; k++) sum[k] += p[k], wide[k] += p[k];
  }
  bool fits = true;
  for (int k = 0; k < 5; k++) fits = fits && wide[k] == sum[k];
  if (sum_out) memcpy(sum_out, sum, 20);
  pl_finish(st, sum, tag);
  return fits;
}

// pt = ct ^ keystream, every lane taking the blocks and pieces the kernel's lane takes
void wave_decrypt(const uint32_t key[8], const uint32_t nonce[3], const uint8_t* ct, uint64_t clen, uint8_t* pt) {
  const uint64_t nb = cl_blocks(clen);
  for (uint32_t lane = 0; lane < GL_LANES; lane++)
    for (uint64_t b = lane; b < nb; b += GL_LANES) {
      uint32_t ks[16];
      chacha20_block(key, cl_counter(b), nonce, ks);
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t len = cl_piece_len(clen, b, q);
        if (len == 0) break;
        const uint64_t o = cl_piece_offset(b, q);
        uint32_t x[4];
        ld_block_le(ct, o, o + len, x);
        for (int w = 0; w < 4; w++) x[w] ^= ks[4 * q + w];
        for (uint32_t i = 0; i < len; i++) pt[o + i] = (uint8_t)(x[i >> 2] >> (8 * (i & 3)));
      }
    }
}

}  // namespace

extern "C" {

// out = h m mod 2^130 - 5 by pl_mul, limbs in and out as they are (the caller checks the ranges)
void cl_mul(const uint32_t h[5], const uint32_t m[5], uint32_t out[5]) { jxt::t_pl_mul(h, m, out); }

// The AEAD tag over (aad, ct) under the Poly1305 key `key` (r || s, 32 bytes; r is clamped as poly1305_init
// clamps it) as the wave computes it. Returns 1, or 0 when a 32-bit limb sum of the combine wrapped.
int cl_tag_lanes(const uint8_t key[32], const uint8_t* aad, uint64_t alen, const uint8_t* ct, uint64_t clen,
                 uint32_t rot, uint8_t tag_out[16], uint32_t* exps, uint32_t* sum_out) {
  uint32_t kw[8], tag[4];
  le_words(key, 8, kw);
  Poly1305 st;
  poly1305_init(st, kw);
  const bool fits = wave_tag(st, aad, alen, ct, clen, rot, tag, exps, sum_out);
  le_bytes(tag, 4, tag_out);
  return fits ? 1 : 0;
}

// pt = ChaCha20 of ct[0, clen) from counter 1 on, by the lane -> block map
void cl_chacha_lanes(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* ct, uint64_t clen, uint8_t* pt) {
  uint32_t kw[8], nw[3];
  le_words(key, 8, kw);
  le_words(nonce, 3, nw);
  wave_decrypt(kw, nw, ct, clen, pt);
}

// The whole open as chapoly_wave_open orders it: the one-time key from block 0, the tag, and the decryption only
// when the tag holds (pt is untouched otherwise). ct_tag: the ciphertext and its 16-byte tag, n >= 16 bytes.
int cl_open_lanes(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad, uint64_t alen,
                  const uint8_t* ct_tag, uint64_t n, uint32_t rot, uint8_t* pt) {
  uint32_t kw[8], nw[3], ks[16], tag[4], want[4];
  le_words(key, 8, kw);
  le_words(nonce, 3, nw);
  const uint64_t clen = n - 16;
  chacha20_block(kw, 0, nw, ks);
  Poly1305 st;
  poly1305_init(st, ks);
  if (!wave_tag(st, aad, alen, ct_tag, clen, rot, tag, nullptr, nullptr)) return -1;
  ld_block_le(ct_tag + clen, 0, 16, want);
  uint32_t diff = 0;
  for (int k = 0; k < 4; k++) diff |= tag[k] ^ want[k];
  if (diff) return 0;
  wave_decrypt(kw, nw, ct_tag, clen, pt);
  return 1;
}

}  // extern "C"

#ifdef JX_HOSTTEST_MAIN
static int failures = 0;
static void check(const char* what, bool ok) {
  printf("%-72s %s\n", what, ok ? "ok" : "MISMATCH");
  failures += !ok;
}
static uint32_t rng_state = 0x9e3779b9u;
static uint8_t rnd8() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (uint8_t)(rng_state >> 24);
}
static std::vector<uint8_t> rnd_bytes(size_t n) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = rnd8();
  return v;
}
// the serial tag of jx_chapoly.h under a Poly1305 key given directly
static void serial_tag(const uint8_t key[32], const uint8_t* aad, uint64_t alen, const uint8_t* ct, uint64_t clen,
                       uint8_t out[16]) {
  uint32_t kw[8], m[4], tag[4];
  le_words(key, 8, kw);
  Poly1305 p;
  poly1305_init(p, kw);
  for (uint64_t i = 0; i < alen; i += 16) ld_block_le(aad, i, alen, m), poly1305_block(p, m, 1);
  for (uint64_t i = 0; i < clen; i += 16) ld_block_le(ct, i, clen, m), poly1305_block(p, m, 1);
  pl_len_block(alen, clen, m);
  poly1305_block(p, m, 1);
  poly1305_finish(p, tag);
  le_bytes(tag, 4, out);
}
static bool tags_agree(const uint8_t key[32], const std::vector<uint8_t>& aad, const std::vector<uint8_t>& ct, uint32_t rot) {
  uint8_t got[16], want[16];
  uint32_t exps[64];
  // (vector::data() of an empty vector may be null: the code under test must not touch it)
  if (cl_tag_lanes(key, aad.data(), aad.size(), ct.data(), ct.size(), rot, got, exps, nullptr) != 1) return false;
  serial_tag(key, aad.data(), aad.size(), ct.data(), ct.size(), want);
  const uint64_t N = pl_mac_blocks(aad.size(), ct.size());
  for (uint32_t j = 0; j < 64; j++) {
    uint64_t last = j;
    while (last + 64 < N) last += 64;
    if (exps[j] != (j < N ? (uint32_t)(N - last) : 0u)) return false;
  }
  return memcmp(got, want, 16) == 0;
}

int main() {
  // lane-split tag == serial tag: splits of totals around one, two and three strides, tails 1 / 15 / 16
  bool ok = true;
  const int totals[] = {1, 2, 63, 64, 65, 128, 129, 200};
  const int tails[] = {1, 15, 16};
  for (int total : totals)
    for (int na = 0; na < total; na += (total > 8 ? 13 : 1)) {
      const int nc = total - 1 - na;
      for (int tail : tails) {
        const size_t alen = 16 * na - (na % 2 ? 3 : 0), clen = nc ? 16 * nc - (16 - tail) : 0;
        const auto key = rnd_bytes(32), aad = rnd_bytes(alen), ct = rnd_bytes(clen);
        ok = ok && tags_agree(key.data(), aad, ct, 0) && tags_agree(key.data(), aad, ct, 37);
      }
    }
  check("lane-split Poly1305 == serial, AAD / ciphertext splits, two lane orders", ok);
  // key edges with all-0xFF messages: the largest limbs in the lane sums and the combine
  ok = true;
  for (int rk = 0; rk < 3; rk++)
    for (int sk = 0; sk < 2; sk++)
      for (int nblk : {64, 65, 200}) {
        uint8_t key[32];
        memset(key, 0, 32);
        if (rk == 1) key[0] = 1;
        if (rk == 2) memset(key, 0xff, 16);  // the clamp leaves its maximum
        if (sk) memset(key + 16, 0xff, 16);
        const std::vector<uint8_t> aad(16 * 3, 0xff), ct(16 * (nblk - 4), 0xff);
        ok = ok && tags_agree(key, aad, ct, 0) && tags_agree(key, aad, ct, 5);
      }
  check("r = 0, 1, clamp maximum; s = 0, all ones; all-0xFF, 64 / 65 / 200 blocks", ok);
  // pl_mul at the top of its accepted ranges returns carried limbs
  {
    uint32_t h[5], m[5], out[5];
    for (int i = 0; i < 5; i++) h[i] = (1u << 27) - 1, m[i] = PL_MUL_MAX - 1;
    cl_mul(h, m, out);
    ok = out[1] < (1u << 26) + (1u << 10);
    for (int i : {0, 2, 3, 4}) ok = ok && out[i] < (1u << 26);
    check("pl_mul of the largest accepted limbs returns carried limbs", ok);
  }
  // the block map against the serial chapoly_decrypt
  ok = true;
  const size_t clens[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 4160, 8191, 8192, 8193, 8263};
  const auto key = rnd_bytes(32), nonce = rnd_bytes(12);
  uint32_t kw[8], nw[3];
  le_words(key.data(), 8, kw);
  le_words(nonce.data(), 3, nw);
  for (size_t clen : clens) {
    const auto ct = rnd_bytes(clen);
    std::vector<uint8_t> got(clen), want(clen);  // exact sizes: a byte past the end is the sanitizer's to find
    cl_chacha_lanes(key.data(), nonce.data(), ct.data(), clen, got.data());
    chapoly_decrypt(kw, nw, ct.data(), clen, want.data());
    ok = ok && got == want;
  }
  check("ChaCha20 lane -> block map == serial, 13 lengths up to 8263", ok);
  // the whole open: a fixed input sealed by tests/hpke_suites_ref.py (chapoly_seal(bytes(range(32)),
  // bytes(range(12)), aad, pt), aad[i] = 7 i + 1, pt[i] = 31 i + 5, 92 and 8263 bytes): its tag and first bytes
  {
    uint8_t k32[32], n12[12];
    for (int i = 0; i < 32; i++) k32[i] = (uint8_t)i;
    for (int i = 0; i < 12; i++) n12[i] = (uint8_t)i;
    std::vector<uint8_t> aad(92), pt(8263), sealed(8263 + 16), opened(8263);
    for (size_t i = 0; i < aad.size(); i++) aad[i] = (uint8_t)(7 * i + 1);
    for (size_t i = 0; i < pt.size(); i++) pt[i] = (uint8_t)(31 * i + 5);
    le_words(k32, 8, kw);
    le_words(n12, 3, nw);
    chapoly_decrypt(kw, nw, pt.data(), pt.size(), sealed.data());  // (the stream cipher is its own inverse)
    uint32_t ks[16];
    chacha20_block(kw, 0, nw, ks);
    uint8_t otk[32];
    le_bytes(ks, 8, otk);
    serial_tag(otk, aad.data(), aad.size(), sealed.data(), pt.size(), sealed.data() + pt.size());
    static const uint8_t WANT_TAG[16] = {0xd7, 0xc4, 0x06, 0x88, 0x89, 0x2c, 0xb9, 0x49,
                                         0xa2, 0xdc, 0xf9, 0xcc, 0x87, 0x7c, 0xbf, 0x5c};
    static const uint8_t WANT_CT8[8] = {0x8c, 0xdf, 0x4b, 0x62, 0xa8, 0xb7, 0x1a, 0x9e};
    check("the fixed input's ciphertext and tag are the Python reference's",
          memcmp(sealed.data() + pt.size(), WANT_TAG, 16) == 0 && memcmp(sealed.data(), WANT_CT8, 8) == 0);
    check("whole open of 8263 bytes under 92 bytes of AAD",
          cl_open_lanes(k32, n12, aad.data(), aad.size(), sealed.data(), sealed.size(), 0, opened.data()) == 1 && opened == pt);
    ok = true;
    const size_t flips[] = {0, 16 * (64 - 6) + 3, 4096 + 77, 8262, 8263, 8263 + 15};
    for (size_t f : flips) {
      auto bad = sealed;
      bad[f] ^= 0x20;
      std::vector<uint8_t> out(8263, 0xA5);
      ok = ok && cl_open_lanes(k32, n12, aad.data(), aad.size(), bad.data(), bad.size(), 0, out.data()) == 0 &&
           out == std::vector<uint8_t>(8263, 0xA5);
    }
    aad[91] ^= 1;
    ok = ok && cl_open_lanes(k32, n12, aad.data(), aad.size(), sealed.data(), sealed.size(), 0, opened.data()) == 0;
    check("tampered ciphertext, tag and AAD fail and write no plaintext", ok);
  }
  // the shortest inputs: no AAD, no ciphertext
  {
    uint8_t k32[32] = {9}, n12[12] = {4}, sealed[16], none = 0;
    le_words(k32, 8, kw);
    le_words(n12, 3, nw);
    uint32_t ks[16];
    chacha20_block(kw, 0, nw, ks);
    uint8_t otk[32];
    le_bytes(ks, 8, otk);
    serial_tag(otk, nullptr, 0, nullptr, 0, sealed);
    check("empty AAD and empty ciphertext open", cl_open_lanes(k32, n12, nullptr, 0, sealed, 16, 0, &none) == 1);
  }
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
#endif
