// Host build of janus_amd/csrc/jx_ghash_lanes.h for tests/test_hpke_long_host.py: the 64 lanes of the wave are a
// loop, a shuffle is an array index. g++ -O2 -std=c++17 -shared -fPIC.
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_ghash_lanes.h"

using namespace jx;

namespace {
void be_words(const uint8_t* b, uint32_t w[4]) {
  for (int i = 0; i < 4; i++)
    w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
void be_bytes(const uint32_t w[4], uint8_t* b) {
  for (int i = 0; i < 16; i++) b[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
}
struct Tab4 {
  uint32_t m[16][4];
  void operator()(uint32_t n, uint32_t e[4]) const { memcpy(e, m[n], 16); }
};
void make_tab(const uint32_t h[4], Tab4& t) {
  for (uint32_t n = 0; n < 16; n++) gl_tab4_entry(n, h, t.m[n]);
}
}  // namespace

extern "C" {

// out = x * h by the bit loop of jx_hpke.h (16 big-endian bytes each)
void hl_ghash_mul(const uint8_t* x, const uint8_t* h, uint8_t* out) {
  uint32_t xw[4], hw[4];
  be_words(x, xw);
  be_words(h, hw);
  ghash_mul(xw, hw);
  be_bytes(xw, out);
}

// out = x * h by the 4-bit table of h
void hl_ghash_mul_tab4(const uint8_t* x, const uint8_t* h, uint8_t* out) {
  uint32_t xw[4], hw[4];
  be_words(x, xw);
  be_words(h, hw);
  Tab4 t;
  make_tab(hw, t);
  ghash_mul_tab4(xw, t);
  be_bytes(xw, out);
}

// GHASH_H(aad, ct) as the wave computes it. rot only changes the order in which the emulated lanes run and are
// XORed (from lane rot on), which must not matter. exps (64 words, nullable): the exponent each lane used.
void hl_ghash_lanes(const uint8_t* h16, const uint8_t* aad, uint64_t alen, const uint8_t* ct, uint64_t clen,
                    uint32_t rot, uint8_t* out, uint32_t* exps) {
  uint32_t h[4];
  be_words(h16, h);
  uint32_t pw[GL_LANES][4];  // lane l: H^(l+1)
  memcpy(pw[0], h, 16);
  for (uint32_t l = 1; l < GL_LANES; l++) memcpy(pw[l], h, 16);
  for (int s = 0; s < 6; s++) {
    uint32_t next[GL_LANES][4];
    memcpy(next, pw, sizeof pw);
    for (uint32_t l = 0; l < GL_LANES; l++) {
      uint32_t other[4];
      memcpy(other, pw[gl_pow_src_other(s, l)], 16);
      ghash_mul(other, pw[gl_pow_src_base(s)]);
      if (gl_pow_active(s, l)) memcpy(next[l], other, 16);
    }
    memcpy(pw, next, sizeof pw);
  }
  Tab4 m64;
  make_tab(pw[63], m64);
  const uint64_t na = (alen + 15) / 16, nc = (clen + 15) / 16, N = na + nc;
  auto block = [&](uint64_t k, uint32_t x[4]) {
    uint8_t b[16] = {0};
    if (k < na) {
      const uint64_t o = 16 * k;
      memcpy(b, aad + o, alen - o < 16 ? alen - o : 16);
    } else {
      const uint64_t o = 16 * (k - na);
      memcpy(b, ct + o, clen - o < 16 ? clen - o : 16);
    }
    be_words(b, x);
  };
  uint32_t y[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < GL_LANES; i++) {
    const uint32_t j = (i + rot) % GL_LANES;
    uint32_t p[4];
    gl_lane_partial(N, j, block, m64, p);
    const uint32_t d = gl_lane_exponent(N, j);
    if (exps) exps[j] = d;
    ghash_mul(p, pw[d ? d - 1 : 0]);
    for (int w = 0; w < 4; w++) y[w] ^= p[w];
  }
  gl_finish(y, alen, clen, h);
  be_bytes(y, out);
}

// AES with the T-table form of either key length (key: 16 or 32 bytes; in/out: 16 bytes)
void hl_aes_t(const uint8_t* key, uint32_t key_len, const uint8_t* in, uint8_t* out) {
  uint32_t t0[256];
  for (int i = 0; i < 256; i++) t0[i] = aes_t0_entry(AES_SBOX[i]);
  auto T = [&](uint32_t x) { return t0[x]; };
  uint32_t kw[8], iw[4], ow[4], rk[60];
  memcpy(kw, key, key_len);
  memcpy(iw, in, 16);
  if (key_len == 16) {
    aes_expand_key_t<4>(T, kw, rk);
    aes_encrypt_t_nk<4>(T, rk, iw, ow);
  } else {
    aes_expand_key_t<8>(T, kw, rk);
    aes_encrypt_t_nk<8>(T, rk, iw, ow);
  }
  memcpy(out, ow, 16);
}

}  // extern "C"
