// Host build of the staged-coefficient helpers (pack_cd26 / unpack_cd26, janus_amd/csrc/jx_field.h): K1 stores a
// ParallelSum call's (c_k, d_k) as ten 26-bit limbs and the FLP kernels feed wacc_mac from them
// (tests/test_coef_limbs_host.py). Test-only; not part of the product.
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_field.h"
#include "jx_testops.h"  // what each operation computes, shared with the gfx950 harness (devtest.hip)

using namespace jx;
using namespace jxt;

extern "C" {
int cl_words(void) { return CD26_WORDS; }
void cl_to_limbs(const uint8_t* a, uint32_t l[5]) { t_cl_to_limbs(a, l); }
void cl_pack(const uint8_t* c, const uint8_t* d, uint32_t* w) { t_cl_pack(c, d, w); }
void cl_unpack(const uint32_t* w, uint32_t cl[5], uint32_t dl[5]) { t_cl_unpack(w, cl, dl); }
// The ring's accumulation over n calls of one slot: ae += x_k * d_k, ao += x_k * c_k, as raw column sums.
// packed = 0: the coefficient limbs split from the 16-byte values at every use; 1: from the staged words.
void cl_mac(const uint8_t* xs, const uint8_t* cs, const uint8_t* ds, int n, int packed, uint64_t cole[9],
            uint64_t colo[9]) {
  t_cl_mac(xs, cs, ds, n, packed, cole, colo);
}
}
