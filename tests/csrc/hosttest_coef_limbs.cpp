// Host build of the staged-coefficient helpers (pack_cd26 / unpack_cd26, janus_amd/csrc/jx_field.h): K1 stores a
// ParallelSum call's (c_k, d_k) as ten 26-bit limbs and the FLP kernels feed wacc_mac from them
// (tests/test_coef_limbs_host.py). Test-only; not part of the product.
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_field.h"

using namespace jx;

static f128 ld(const uint8_t* p) {
  uint64_t lo, hi;
  memcpy(&lo, p, 8);
  memcpy(&hi, p + 8, 8);
  return make128(lo, hi);
}

extern "C" {
int cl_words(void) { return CD26_WORDS; }
void cl_to_limbs(const uint8_t* a, uint32_t l[5]) {
  const limbs26 r = to_limbs26(ld(a));
  for (int i = 0; i < 5; i++) l[i] = r.l[i];
}
void cl_pack(const uint8_t* c, const uint8_t* d, uint32_t* w) { pack_cd26(ld(c), ld(d), w); }
void cl_unpack(const uint32_t* w, uint32_t cl[5], uint32_t dl[5]) {
  limbs26 c, d;
  unpack_cd26(w, c, d);
  for (int i = 0; i < 5; i++) {
    cl[i] = c.l[i];
    dl[i] = d.l[i];
  }
}
// The ring's accumulation over n calls of one slot: ae += x_k * d_k, ao += x_k * c_k, as raw column sums.
// packed = 0: the coefficient limbs split from the 16-byte values at every use; 1: from the staged words.
void cl_mac(const uint8_t* xs, const uint8_t* cs, const uint8_t* ds, int n, int packed, uint64_t cole[9],
            uint64_t colo[9]) {
  wacc26 ae, ao;
  wacc_zero(ae);
  wacc_zero(ao);
  for (int k = 0; k < n; k++) {
    const limbs26 xl = to_limbs26(ld(xs + 16 * k));
    limbs26 ck, dk;
    if (packed) {
      uint32_t w[CD26_WORDS];
      pack_cd26(ld(cs + 16 * k), ld(ds + 16 * k), w);
      unpack_cd26(w, ck, dk);
    } else {
      ck = to_limbs26(ld(cs + 16 * k));
      dk = to_limbs26(ld(ds + 16 * k));
    }
    wacc_mac(ae, xl, dk);
    wacc_mac(ao, xl, ck);
  }
  for (int s = 0; s < 9; s++) {
    cole[s] = ae.col[s];
    colo[s] = ao.col[s];
  }
}
}
