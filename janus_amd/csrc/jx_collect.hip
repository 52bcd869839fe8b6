// jx_collect.hip — the kernels of collection (jx_collect.h): the merge of many collection jobs' shard records in one
// launch, the decision per job, the zeroing of refused jobs' outputs, and the collector's check-and-add of two opened
// aggregate shares. The seal and the opens between them are the long seal and the long open (jx_hpke_seal.hip,
// jx_hpke_long.hip), launched by jx_engine_collect.cpp. No atomics: every output byte has one writer, and a tile
// that meets an element >= p raises its job's flag with a plain store of 1 (every such tile stores the same word).
#include <hip/hip_runtime.h>

#include "jx_collect.h"

namespace jx {
namespace {

constexpr uint32_t DECIDE_WAVES = 4;  // jobs per workgroup of the decision kernel, a wave each

// the 64-bit word w of a row whose start is 8-byte aligned
__device__ __forceinline__ uint64_t ld64(const uint8_t* row, uint64_t w) {
  return reinterpret_cast<const uint64_t*>(row)[w];
}
__device__ __forceinline__ void st64(uint8_t* row, uint64_t w, uint64_t v) { reinterpret_cast<uint64_t*>(row)[w] = v; }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// Workgroup (job, tile): lane i of the tile owns element tile * COLLECT_TILE + i of the job's share and walks the
// job's records. Linear grid: blockIdx.x = job * tiles + tile.
template <uint32_t FB>
__global__ __launch_bounds__(COLLECT_TILE) void collect_merge_kernel(CollectMergeArgs a, uint32_t tiles) {
  const uint32_t job = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const uint32_t i = tile * COLLECT_TILE + threadIdx.x;
  if (job >= a.njobs || i >= a.out_len) return;
  const uint64_t pt_bytes = (uint64_t)a.out_len * FB, stride = pt_bytes + 40;
  const uint64_t r0 = a.rec_off[job], r1 = a.rec_off[job + 1];
  bool bad = false;
  uint8_t* out = a.pts + job * pt_bytes;
  if (FB == 8) {
    uint64_t s = 0;
    for (uint64_t q = r0; q < r1; q++) {
      uint64_t v;
      const bool good = collect_decode64(ld64(a.records + a.rec_idx[q] * stride, i), v);
      bad |= !good;
      s = collect_add64(s, good ? v : 0);
    }
    st64(out, i, s);
  } else {
    f128 s = make128(0, 0);
    for (uint64_t q = r0; q < r1; q++) {
      const uint8_t* rec = a.records + a.rec_idx[q] * stride;
      f128 v;
      const bool good = collect_decode128(ld64(rec, 2ull * i), ld64(rec, 2ull * i + 1), v);
      bad |= !good;
      s = collect_add128(s, good ? v : make128(0, 0));
    }
    st64(out, 2ull * i, s.lo);
    st64(out, 2ull * i + 1, s.hi);
  }
  if (bad) a.bad[job] = 1u;
}

// A wave per job: lane l takes the job's records l, l + 64, ...: the sum of their counts and the XOR of their
// checksums, folded over the wave; lane 0 decides the status.
__global__ __launch_bounds__(64 * DECIDE_WAVES) void collect_decide_kernel(CollectMergeArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t job = blockIdx.x * DECIDE_WAVES + (threadIdx.x >> 6);
  if (job >= a.njobs) return;  // the whole wave
  const uint64_t pt_bytes = (uint64_t)a.out_len * a.fb, stride = pt_bytes + 40;
  const uint64_t r0 = a.rec_off[job], r1 = a.rec_off[job + 1];
  uint64_t count = 0, cs[4] = {0, 0, 0, 0};
  for (uint64_t q = r0 + lane; q < r1; q += 64) {
    const uint8_t* tail = a.records + a.rec_idx[q] * stride + pt_bytes;
    count += ld64(tail, 0);
#pragma unroll
    for (int k = 0; k < 4; k++) cs[k] ^= ld64(tail, 1 + k);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    count += shfl_xor64(count, m);
#pragma unroll
    for (int k = 0; k < 4; k++) cs[k] ^= shfl_xor64(cs[k], m);
  }
  if (lane != 0) return;
  uint8_t csb[32];
#pragma unroll
  for (int k = 0; k < 32; k++) csb[k] = (uint8_t)(cs[k >> 3] >> (8 * (k & 7)));
  const uint8_t* ecs = a.exp_checksums ? a.exp_checksums + 32ull * job : nullptr;
  a.status0[job] = (uint8_t)collect_status(r1 - r0, a.bad[job] != 0, count, csb, ecs ? a.exp_counts[job] : 0, ecs,
                                           a.min_batch_size, a.max_batch_size);
  a.counts[job] = count;
#pragma unroll
  for (int k = 0; k < 4; k++) st64(a.checksums + 32ull * job, k, cs[k]);
}

// Workgroup (job, tile of 64-bit words): the job's final status (tile 0 writes it), and for a job that is not OK
// zeros over its ciphertext row, its share and (tile 0) its enc.
__global__ __launch_bounds__(COLLECT_TILE) void collect_finish_kernel(CollectFinishArgs a, uint32_t tiles) {
  const uint32_t job = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  if (job >= a.njobs) return;
  const uint32_t st = collect_seal_status(a.status0[job], a.sealed[job] != 0);
  if (tile == 0 && threadIdx.x == 0) a.status[job] = (uint8_t)st;
  if (st == COLLECT_OK) return;
  const uint64_t w = (uint64_t)tile * COLLECT_TILE + threadIdx.x, pt_words = a.pt_bytes / 8;
  if (w < pt_words + 2) st64(a.cts + job * (a.pt_bytes + 16), w, 0);
  if (w < pt_words) st64(a.pts + job * a.pt_bytes, w, 0);
  if (tile == 0 && threadIdx.x < 4) st64(a.encs + 32ull * job, threadIdx.x, 0);
}

// Workgroup (opened collection, tile): lane i checks element i of both shares and writes their sum. A collection one
// of whose shares did not open is left alone (its row is zero already; the plaintext of a failed open is not read).
template <uint32_t FB>
__global__ __launch_bounds__(COLLECT_TILE) void collect_unshard_kernel(CollectUnshardArgs a, uint32_t tiles) {
  const uint32_t c = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const uint32_t i = tile * COLLECT_TILE + threadIdx.x;
  if (c >= a.n || i >= a.out_len) return;
  if (!a.leader_ok[c] || !a.helper_ok[c]) return;
  const uint64_t pt_bytes = (uint64_t)a.out_len * FB;
  const uint8_t *l = a.leader_pts + c * pt_bytes, *h = a.helper_pts + c * pt_bytes;
  uint8_t* out = a.out + a.row[c] * pt_bytes;
  bool lg, hg;
  if (FB == 8) {
    uint64_t x, y;
    lg = collect_decode64(ld64(l, i), x);
    hg = collect_decode64(ld64(h, i), y);
    st64(out, i, collect_add64(lg ? x : 0, hg ? y : 0));
  } else {
    f128 x, y;
    lg = collect_decode128(ld64(l, 2ull * i), ld64(l, 2ull * i + 1), x);
    hg = collect_decode128(ld64(h, 2ull * i), ld64(h, 2ull * i + 1), y);
    const f128 s = collect_add128(lg ? x : make128(0, 0), hg ? y : make128(0, 0));
    st64(out, 2ull * i, s.lo);
    st64(out, 2ull * i + 1, s.hi);
  }
  if (!lg) a.bad[2 * c] = 1u;
  if (!hg) a.bad[2 * c + 1] = 1u;
}

// After it, workgroup (opened collection, tile of words): the collection's status (tile 0), zeros over a failed row.
__global__ __launch_bounds__(COLLECT_TILE) void collect_open_finish_kernel(CollectUnshardArgs a, uint32_t tiles) {
  const uint32_t c = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  if (c >= a.n) return;
  const uint32_t st = collect_open_status(a.leader_ok[c] != 0, a.helper_ok[c] != 0, a.bad[2 * c] != 0, a.bad[2 * c + 1] != 0);
  if (tile == 0 && threadIdx.x == 0) a.status[a.row[c]] = (uint8_t)st;
  if (st == COLLECT_OPEN_OK) return;
  const uint64_t pt_bytes = (uint64_t)a.out_len * a.fb;
  const uint64_t w = (uint64_t)tile * COLLECT_TILE + threadIdx.x;
  if (w < pt_bytes / 8) st64(a.out + a.row[c] * pt_bytes, w, 0);
}

uint32_t tiles_of(uint64_t items) { return (uint32_t)((items + COLLECT_TILE - 1) / COLLECT_TILE); }

}  // namespace

hipError_t launch_collect_merge(const CollectMergeArgs& a, hipStream_t s) {
  if (a.njobs == 0) return hipSuccess;
  const uint32_t tiles = tiles_of(a.out_len);
  if (a.fb == 8)
    hipLaunchKernelGGL(collect_merge_kernel<8>, dim3(a.njobs * tiles), dim3(COLLECT_TILE), 0, s, a, tiles);
  else
    hipLaunchKernelGGL(collect_merge_kernel<16>, dim3(a.njobs * tiles), dim3(COLLECT_TILE), 0, s, a, tiles);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(collect_decide_kernel, dim3((a.njobs + DECIDE_WAVES - 1) / DECIDE_WAVES), dim3(64 * DECIDE_WAVES),
                     0, s, a);
  return hipGetLastError();
}

hipError_t launch_collect_finish(const CollectFinishArgs& a, hipStream_t s) {
  if (a.njobs == 0) return hipSuccess;
  const uint32_t tiles = tiles_of(a.pt_bytes / 8 + 2);
  hipLaunchKernelGGL(collect_finish_kernel, dim3(a.njobs * tiles), dim3(COLLECT_TILE), 0, s, a, tiles);
  return hipGetLastError();
}

hipError_t launch_collect_unshard(const CollectUnshardArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t tiles = tiles_of(a.out_len);
  if (a.fb == 8)
    hipLaunchKernelGGL(collect_unshard_kernel<8>, dim3(a.n * tiles), dim3(COLLECT_TILE), 0, s, a, tiles);
  else
    hipLaunchKernelGGL(collect_unshard_kernel<16>, dim3(a.n * tiles), dim3(COLLECT_TILE), 0, s, a, tiles);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  const uint32_t wtiles = tiles_of((uint64_t)a.out_len * a.fb / 8);
  hipLaunchKernelGGL(collect_open_finish_kernel, dim3(a.n * wtiles), dim3(COLLECT_TILE), 0, s, a, wtiles);
  return hipGetLastError();
}

}  // namespace jx
