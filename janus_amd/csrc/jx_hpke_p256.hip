// jx_hpke_p256.hip — the pair of open kernels of DHKEM(P-256, HKDF-SHA256) (jx_hpke.hip has the overview;
// jx_p256.h the curve): 65-byte encapsulated keys, read where they lie in device memory.
#include "jx_hpke_open.h"

namespace jx {
namespace {

// The standalone batch open of a P-256 context: encapsulated keys at a stride of 65 bytes.
__global__ __launch_bounds__(64) void hpke_open_p256_kernel(HpkeCfg cfg, HpkeBufs b) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const uint64_t c0 = b.ct_off[r], c1 = b.ct_off[r + 1];
  const uint64_t a0 = b.aad_off[r], a1 = b.aad_off[r + 1];
  const uint8_t* aad = b.aads + a0;
  const bool ok = c1 - c0 >= 16 && p256_open(sbox, cfg.key, b.encs + 65 * r, a1 - a0, [&](uint64_t i) { return aad[i]; },
                                             b.cts + c0, c1 - c0 - 16, b.pts + c0 - 16 * r);
  b.ok[r] = (uint8_t)ok;
}

__global__ __launch_bounds__(64) void hpke_rows_p256_kernel(RowsArgs ra) {
  __shared__ uint8_t sbox[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = AES_SBOX[i];
  __syncthreads();
  rows_body<true, true>(sbox, ra);
}

}  // namespace

void launch_hpke_open_p256(const HpkeCfg& cfg, const HpkeBufs& b, hipStream_t s) {
  hipLaunchKernelGGL(hpke_open_p256_kernel, dim3((uint32_t)((b.n + 63) / 64)), dim3(64), 0, s, cfg, b);
}

void launch_hpke_rows_p256(const RowsArgs& ra, hipStream_t s) {
  hipLaunchKernelGGL(hpke_rows_p256_kernel, dim3((uint32_t)((ra.a.n + 63) / 64)), dim3(64), 0, s, ra);
}

}  // namespace jx
