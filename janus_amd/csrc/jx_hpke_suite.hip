// jx_hpke_suite.hip — the pair of open kernels of the nine X25519 suites (jx_hpke.hip has the overview;
// jx_hpke_suites.h the suites): each lane reads the suite from its key.
#include "jx_hpke_open.h"

namespace jx {
namespace {

__global__ __launch_bounds__(64) void hpke_open_suite_kernel(HpkeCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  open_body<true>(sbox, cfg, b);
}

__global__ __launch_bounds__(64) void hpke_rows_suite_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<true>(sbox, ra);
}

}  // namespace

void launch_hpke_open_suite(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s) {
  hipLaunchKernelGGL(hpke_open_suite_kernel, dim3((uint32_t)((b.n + 63) / 64)), dim3(64), 0, s, cfg, b);
}

void launch_hpke_rows_suite(const RowsArgs& ra, hipStream_t s) {
  hipLaunchKernelGGL(hpke_rows_suite_kernel, dim3((uint32_t)((ra.a.n + 63) / 64)), dim3(64), 0, s, ra);
}

}  // namespace jx
