// jx_wire_dev.h — the two device helpers the wire kernels share (jx_wire.hip, jx_wire_upload.hip): the exclusive scan
// of one workgroup of 1024 and the copy of one wave at any alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jx {

// ---- exclusive scan by one workgroup of 1024: out[i] = sum of load(j) for j < i, out[n] the total. Thread t stores
// out[i] for exactly the i = t (mod 1024), and thread 0 stores out[n].
template <class F>
__device__ void block_exclusive_scan(uint64_t n, F load, uint64_t* out) {
  __shared__ uint64_t wsum[16];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + t;
    const uint64_t v = i < n ? load(i) : 0;
    uint64_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = __shfl_up((unsigned long long)x, d);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint64_t pre = 0, total = 0;
    for (uint32_t k = 0; k < 16; k++) {
      if (k < w) pre += wsum[k];
      total += wsum[k];
    }
    if (i < n) out[i] = carry + pre + x - v;
    carry += total;
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

// len bytes from src (any alignment) to dst by one wave: bytes up to dst's 16-byte boundary, 16 bytes per lane, the tail
__device__ inline void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t lane) {
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  if (head > len) head = len;
  if (lane < head) dst[lane] = src[lane];
  dst += head;
  src += head;
  len -= head;
  const uint64_t nv = len / 16;
  for (uint64_t v = lane; v < nv; v += 64) {
    uint4 x;
    __builtin_memcpy(&x, src + 16 * v, 16);
    *reinterpret_cast<uint4*>(dst + 16 * v) = x;
  }
  const uint64_t t0 = nv * 16;
  if (lane < len - t0) dst[t0 + lane] = src[t0 + lane];
}

}  // namespace jx
