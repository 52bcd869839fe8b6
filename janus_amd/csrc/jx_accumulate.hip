// jx_accumulate.hip — K4, the masked / segmented accumulation of output shares, and what follows it: combining
// and exporting aggregate shares and records, the transposes and scatters of a coalesced launch's outputs, and the
// host-signal and copy-regions kernels (the stages are described at the top of jx_kernels.hip).
#include "jx_field.h"
#include "jx_kernels.h"
#include "jx_sha256.h"

namespace jx {

// ---------------------------------------------------------------------------- K4: accumulate

// selection + count + checksum. Grid-stride over reports (grid capped at SELECT_WGS
// workgroups): each thread folds its reports' SHA-256(id) and selections in registers, the
// workgroup reduces through LDS, and only one set of atomics per workgroup reaches L2 (one
// set per wave serialised ~15k atomics on the same 40 bytes for 1M Count reports).
__global__ __launch_bounds__(256) void select_kernel(AccArgs a, uint8_t* sel) {
  const uint64_t padded = ((a.n + 63) / 64) * 64;
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t cnt = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < padded; r += (uint64_t)gridDim.x * blockDim.x) {
    bool s = false;
    if (r < a.n) s = a.verdicts[r] == 0 && (!a.mask || a.mask[r]) && (!a.seg || a.seg[r] == a.seg_id);
    sel[r] = s;
    if (s) {
      uint32_t id[4], h[8];
      load16(a.nonces + 16 * r, id);
      sha256_16(id, h);
#pragma unroll
      for (int k = 0; k < 8; k++) d[k] ^= h[k];
      cnt++;
    }
  }
  // wave XOR / sum reduce, then across the 4 waves of the workgroup in LDS
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t v = d[k];
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
    d[k] = v;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  __shared__ uint32_t red[4][9];
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) red[w][k] = d[k];
    red[w][8] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const uint32_t k = threadIdx.x;
    uint32_t v = 0;
    for (uint32_t q = 0; q < blockDim.x / 64; q++) v = k < 8 ? (v ^ red[q][k]) : (v + red[q][k]);
    if (v) {
      if (k < 8)
        atomicXor(&a.checksum[k], v);
      else
        atomicAdd(a.count, (unsigned long long)v);
    }
  }
}

__global__ __launch_bounds__(256) void accumulate_kernel(AccArgs a, const uint8_t* sel) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.out_len) return;
  const uint64_t nblk = (a.n + 63) / 64;
  const uint64_t b0 = (uint64_t)blockIdx.y * a.blocks_per_chunk;
  const uint64_t b1 = (b0 + a.blocks_per_chunk < nblk) ? b0 + a.blocks_per_chunk : nblk;
  acc192 acc;
  acc_zero(acc);
  // four blocks' loads in flight per iteration (one dependent load per trip left HBM idle)
  uint64_t bk = b0;
  for (; bk + 4 <= b1; bk += 4) {
    uint4 v[4];
    uint8_t s4[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      s4[u] = sel[(bk + u) * 64 + lane];
      v[u] = a.outs[il_idx(bk + u, a.out_len, i, lane)];
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (s4[u]) acc_add128(acc, u4_to_f(v[u]));
  }
  for (; bk < b1; bk++) {
    if (sel[bk * 64 + lane]) acc_add128(acc, u4_to_f(a.outs[il_idx(bk, a.out_len, i, lane)]));
  }
  // wave reduction of the 192-bit accumulators
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o0 = ((uint64_t)__shfl_xor((uint32_t)(acc.w0 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w0, off);
    uint64_t o1 = ((uint64_t)__shfl_xor((uint32_t)(acc.w1 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w1, off);
    uint64_t o2 = ((uint64_t)__shfl_xor((uint32_t)(acc.w2 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w2, off);
    uint32_t cc = 0;
    acc.w0 = addc64(acc.w0, o0, cc);
    acc.w1 = addc64(acc.w1, o1, cc);
    acc.w2 = acc.w2 + o2 + cc;
  }
  if (lane == 0) {
    uint64_t* p = a.partials + ((uint64_t)blockIdx.y * a.out_len + i) * 3;
    p[0] = acc.w0;
    p[1] = acc.w1;
    p[2] = acc.w2;
  }
}


// one wave per output element: lanes stride over the report chunks' partial sums, then a
// shuffle reduction (Count / Sum use up to 4096 chunks of a single element)
__global__ __launch_bounds__(256) void reduce_partials_kernel(Cfg c, const uint64_t* partials, uint32_t nchunks,
                                                              uint4* agg) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= c.out_len) return;
  acc192 acc;
  acc_zero(acc);
  for (uint32_t q = lane; q < nchunks; q += 64) {
    const uint64_t* p = partials + ((uint64_t)q * c.out_len + i) * 3;
    uint32_t cc = 0;
    acc.w0 = addc64(acc.w0, p[0], cc);
    acc.w1 = addc64(acc.w1, p[1], cc);
    acc.w2 = acc.w2 + p[2] + cc;
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o0 = ((uint64_t)__shfl_xor((uint32_t)(acc.w0 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w0, off);
    uint64_t o1 = ((uint64_t)__shfl_xor((uint32_t)(acc.w1 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w1, off);
    uint64_t o2 = ((uint64_t)__shfl_xor((uint32_t)(acc.w2 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w2, off);
    uint32_t cc = 0;
    acc.w0 = addc64(acc.w0, o0, cc);
    acc.w1 = addc64(acc.w1, o1, cc);
    acc.w2 = acc.w2 + o2 + cc;
  }
  if (lane != 0) return;
  acc_add128(acc, u4_to_f(agg[i]));
  if (c.fb == 8) {
    uint64_t v = reduce192_p64(acc.w0, acc.w1, acc.w2);
    agg[i] = make_uint4(lo32(v), hi32(v), 0, 0);
  } else {
    agg[i] = f_to_u4(acc_reduce(acc));
  }
}

// K4 for a small batch (<= ACC_SMALL reports, e.g. one Janus aggregation job): one kernel instead of select +
// accumulate + reduce_partials, nothing staged. Wave w of the grid sums output element w over the selected
// reports and adds it into the aggregation; every thread also folds a grid-stride share of the selected
// reports' SHA-256(id) and count, reduced per workgroup into one set of atomics (as select_kernel).
__device__ __forceinline__ bool acc_selected(const AccArgs& a, uint64_t r) {
  return a.verdicts[r] == 0 && (!a.mask || a.mask[r]) && (!a.seg || a.seg[r] == a.seg_id);
}
__global__ __launch_bounds__(256) void accumulate_small_kernel(Cfg c, AccArgs a, uint4* agg) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i < a.out_len) {
    acc192 acc;
    acc_zero(acc);
    const uint64_t nblk = (a.n + 63) / 64;
    for (uint64_t bk = 0; bk < nblk; bk++) {
      const uint64_t r = bk * 64 + lane;
      if (r < a.n && acc_selected(a, r)) acc_add128(acc, u4_to_f(a.outs[il_idx(bk, a.out_len, i, lane)]));
    }
    for (int off = 32; off > 0; off >>= 1) {
      uint64_t o0 = ((uint64_t)__shfl_xor((uint32_t)(acc.w0 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w0, off);
      uint64_t o1 = ((uint64_t)__shfl_xor((uint32_t)(acc.w1 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w1, off);
      uint64_t o2 = ((uint64_t)__shfl_xor((uint32_t)(acc.w2 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w2, off);
      uint32_t cc = 0;
      acc.w0 = addc64(acc.w0, o0, cc);
      acc.w1 = addc64(acc.w1, o1, cc);
      acc.w2 = acc.w2 + o2 + cc;
    }
    if (lane == 0) {
      acc_add128(acc, u4_to_f(agg[i]));
      if (c.fb == 8) {
        const uint64_t v = reduce192_p64(acc.w0, acc.w1, acc.w2);
        agg[i] = make_uint4(lo32(v), hi32(v), 0, 0);
      } else {
        agg[i] = f_to_u4(acc_reduce(acc));
      }
    }
  }
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t cnt = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * blockDim.x) {
    if (acc_selected(a, r)) {
      uint32_t id[4], h[8];
      load16(a.nonces + 16 * r, id);
      sha256_16(id, h);
#pragma unroll
      for (int k = 0; k < 8; k++) d[k] ^= h[k];
      cnt++;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t v = d[k];
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
    d[k] = v;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  __shared__ uint32_t red[4][9];
  const uint32_t w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) red[w][k] = d[k];
    red[w][8] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const uint32_t k = threadIdx.x;
    uint32_t v = 0;
    for (uint32_t q = 0; q < 4; q++) v = k < 8 ? (v ^ red[q][k]) : (v + red[q][k]);
    if (v) {
      if (k < 8)
        atomicXor(&a.checksum[k], v);
      else
        atomicAdd(a.count, (unsigned long long)v);
    }
  }
}

// K4 for up to ACC_MULTI_MAX small batches into one aggregation (the engine's deferred jx_accumulate calls,
// flushed together: one launch instead of one per aggregation job). Workgroup i < out_len sums output element
// i over every batch's finished reports, its wave w taking batches w, w + 4, ... (each 64-report block read
// as one coalesced 1 KiB row), the four waves' 192-bit sums reduced through LDS and added into the
// aggregation. Each workgroup past out_len folds one batch into the count and the ReportIdChecksum.
__global__ __launch_bounds__(256) void accumulate_multi_kernel(Cfg c, AccMultiArgs a) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (blockIdx.x < c.out_len) {
    const uint32_t i = blockIdx.x;
    acc192 acc;
    acc_zero(acc);
    for (uint32_t k = w; k < a.nb; k += 4) {
      const AccDesc d = a.d[k];
      const uint64_t nblk = (d.n + 63) / 64;
      for (uint64_t bk = 0; bk < nblk; bk++) {
        const uint64_t r = bk * 64 + lane;
        if (r < d.n && d.verdicts[r] == 0) acc_add128(acc, u4_to_f(d.outs[il_idx(bk, c.out_len, i, lane)]));
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      uint64_t o0 = ((uint64_t)__shfl_xor((uint32_t)(acc.w0 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w0, off);
      uint64_t o1 = ((uint64_t)__shfl_xor((uint32_t)(acc.w1 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w1, off);
      uint64_t o2 = ((uint64_t)__shfl_xor((uint32_t)(acc.w2 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w2, off);
      uint32_t cc = 0;
      acc.w0 = addc64(acc.w0, o0, cc);
      acc.w1 = addc64(acc.w1, o1, cc);
      acc.w2 = acc.w2 + o2 + cc;
    }
    __shared__ uint64_t red[4][3];
    if (lane == 0) {
      red[w][0] = acc.w0;
      red[w][1] = acc.w1;
      red[w][2] = acc.w2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < 4; q++) {
        uint32_t cc = 0;
        acc.w0 = addc64(acc.w0, red[q][0], cc);
        acc.w1 = addc64(acc.w1, red[q][1], cc);
        acc.w2 = acc.w2 + red[q][2] + cc;
      }
      acc_add128(acc, u4_to_f(a.agg[i]));
      if (c.fb == 8) {
        const uint64_t v = reduce192_p64(acc.w0, acc.w1, acc.w2);
        a.agg[i] = make_uint4(lo32(v), hi32(v), 0, 0);
      } else {
        a.agg[i] = f_to_u4(acc_reduce(acc));
      }
    }
    return;
  }
  const AccDesc d = a.d[blockIdx.x - c.out_len];
  uint32_t h8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t cnt = 0;
  for (uint64_t r = threadIdx.x; r < d.n; r += 256) {
    if (d.verdicts[r] == 0) {
      uint32_t id[4], h[8];
      load16(d.nonces + 16 * r, id);
      sha256_16(id, h);
#pragma unroll
      for (int k = 0; k < 8; k++) h8[k] ^= h[k];
      cnt++;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t v = h8[k];
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
    h8[k] = v;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  __shared__ uint32_t redc[4][9];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) redc[w][k] = h8[k];
    redc[w][8] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const uint32_t k = threadIdx.x;
    uint32_t v = 0;
    for (uint32_t q = 0; q < 4; q++) v = k < 8 ? (v ^ redc[q][k]) : (v + redc[q][k]);
    if (v) {
      if (k < 8)
        atomicXor(&a.checksum[k], v);
      else
        atomicAdd(a.count, (unsigned long long)v);
    }
  }
}

// ---------------------------------------------------------------------------- K4 segmented
// One pass for any number of batch aggregations: a device counting sort of the selected reports by
// segment (LDS histograms, one global atomic per (workgroup, segment)), work items of <= L sorted
// positions that never straddle a segment, per-item 192-bit partial sums, then one reduction per
// (segment, element). The gathered loads are coalesced whenever a segment's reports are contiguous
// (the usual case: Janus jobs group reports by batch), and cost 64-byte sectors per lane otherwise.
__device__ __forceinline__ bool seg_sel(const SegArgs& a, uint64_t r, uint32_t& d) {
  if (r >= a.n || a.verdicts[r] != 0 || (a.mask && !a.mask[r])) return false;
  d = a.seg[r] - a.s0;
  return d < a.ns;
}

__global__ __launch_bounds__(256) void seg_count_kernel(SegArgs a) {
  __shared__ uint32_t h[SEG_MAX];
  for (uint32_t t = threadIdx.x; t < a.ns; t += blockDim.x) h[t] = 0;
  __syncthreads();
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t d;
    if (seg_sel(a, r, d)) atomicAdd(&h[d], 1u);
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < a.ns; t += blockDim.x)
    if (h[t]) atomicAdd(&a.cnt[t], h[t]);
}

// one workgroup: segment offsets, scatter cursors and the work-item table
__global__ __launch_bounds__(1024) void seg_plan_kernel(SegArgs a) {
  __shared__ uint32_t items_base;
  if (threadIdx.x == 0) {
    uint32_t pos = 0, w = 0;
    for (uint32_t s = 0; s < a.ns; s++) {
      const uint32_t c = a.cnt[s];
      a.off[s] = pos;
      a.cursor[s] = pos;
      a.ioff[s] = w;
      pos += c;
      w += (c + a.L - 1) / a.L;
    }
    a.ioff[a.ns] = w;
    a.nitems[0] = w;
    a.nitems[1] = pos;  // selected reports = sorted positions in use
    items_base = w;
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < a.ns; s += blockDim.x) {
    const uint32_t c = a.cnt[s], p0 = a.off[s];
    uint32_t w = a.ioff[s];
    for (uint32_t q = 0; q < c; q += a.L, w++) a.items[w] = make_uint4(s, p0 + q, p0 + min(c, q + a.L), 0);
  }
}

__global__ __launch_bounds__(256) void seg_scatter_kernel(SegArgs a) {
  __shared__ uint32_t h[SEG_MAX];
  for (uint32_t t = threadIdx.x; t < a.ns; t += blockDim.x) h[t] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t r_first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t r = r_first; r < a.n; r += stride) {
    uint32_t d;
    if (seg_sel(a, r, d)) atomicAdd(&h[d], 1u);
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < a.ns; t += blockDim.x)
    if (h[t]) h[t] = atomicAdd(&a.cursor[t], h[t]);  // this workgroup's range of segment t
  __syncthreads();
  for (uint64_t r = r_first; r < a.n; r += stride) {
    uint32_t d;
    if (seg_sel(a, r, d)) a.perm[atomicAdd(&h[d], 1u)] = (uint32_t)r;
  }
}

__device__ __forceinline__ void acc192_wave_reduce(acc192& acc) {
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o0 = ((uint64_t)__shfl_xor((uint32_t)(acc.w0 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w0, off);
    uint64_t o1 = ((uint64_t)__shfl_xor((uint32_t)(acc.w1 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w1, off);
    uint64_t o2 = ((uint64_t)__shfl_xor((uint32_t)(acc.w2 >> 32), off) << 32) | __shfl_xor((uint32_t)acc.w2, off);
    uint32_t cc = 0;
    acc.w0 = addc64(acc.w0, o0, cc);
    acc.w1 = addc64(acc.w1, o1, cc);
    acc.w2 = acc.w2 + o2 + cc;
  }
}

// wave per (output element, work item): lanes walk the item's sorted positions
__global__ __launch_bounds__(256) void seg_accumulate_kernel(SegArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t w = blockIdx.y;
  if (i >= a.out_len || w >= *a.nitems) return;
  const uint4 it = a.items[w];
  acc192 acc;
  acc_zero(acc);
  uint32_t p = it.y + lane;
  for (; p + 192 < it.z; p += 256) {  // four gathers in flight
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t r = a.perm[p + 64 * u];
      v[u] = a.outs[il_idx(r >> 6, a.out_len, i, r & 63)];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) acc_add128(acc, u4_to_f(v[u]));
  }
  for (; p < it.z; p += 64) {
    const uint32_t r = a.perm[p];
    acc_add128(acc, u4_to_f(a.outs[il_idx(r >> 6, a.out_len, i, r & 63)]));
  }
  acc192_wave_reduce(acc);
  if (lane == 0) {
    uint64_t* q = a.partials + ((uint64_t)w * a.out_len + i) * 3;
    q[0] = acc.w0;
    q[1] = acc.w1;
    q[2] = acc.w2;
  }
}

// ReportIdChecksum per segment: thread per sorted position; a wave whose 64 positions share a
// segment (all but the boundary waves) folds them and issues one set of atomics
__global__ __launch_bounds__(256) void seg_checksum_kernel(SegArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = a.nitems[1];
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t d = 0xFFFFFFFFu;
  if (p < total) {
    const uint32_t r = a.perm[p];
    uint32_t id[4];
    load16(a.nonces + 16ull * r, id);
    sha256_16(id, h);
    d = a.seg[r] - a.s0;
  }
  const uint32_t d0 = __shfl(d, 0);
  const bool uniform = __all(d == d0);
  if (uniform) {
    if (d0 == 0xFFFFFFFFu) return;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      uint32_t v = h[k];
      for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
      h[k] = v;
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < 8; k++) atomicXor(&a.checksums[d0][k], h[k]);
  } else if (d != 0xFFFFFFFFu) {
#pragma unroll
    for (int k = 0; k < 8; k++) atomicXor(&a.checksums[d][k], h[k]);
  }
}

// wave per (output element, segment): sum the segment's work-item partials into its aggregate
__global__ __launch_bounds__(256) void seg_reduce_kernel(SegArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t s = blockIdx.y;
  if (i >= a.out_len || s >= a.ns) return;
  acc192 acc;
  acc_zero(acc);
  for (uint32_t w = a.ioff[s] + lane; w < a.ioff[s + 1]; w += 64) {
    const uint64_t* q = a.partials + ((uint64_t)w * a.out_len + i) * 3;
    uint32_t cc = 0;
    acc.w0 = addc64(acc.w0, q[0], cc);
    acc.w1 = addc64(acc.w1, q[1], cc);
    acc.w2 = acc.w2 + q[2] + cc;
  }
  acc192_wave_reduce(acc);
  if (lane != 0) return;
  uint4* agg = a.aggs[s];
  acc_add128(acc, u4_to_f(agg[i]));
  if (a.fb == 8) {
    const uint64_t v = reduce192_p64(acc.w0, acc.w1, acc.w2);
    agg[i] = make_uint4(lo32(v), hi32(v), 0, 0);
  } else {
    agg[i] = f_to_u4(acc_reduce(acc));
  }
  if (i == 0) *a.counts[s] += a.cnt[s];
}

// multi-GPU combine: sum nparts encoded aggregate shares (LE bytes) mod p
// err: set to 1 if an input element is not canonical (>= p): the host merge rejects such a share
// (Field decode, janus_amd/distributed.py merge_aggregate_shares); the engine reports it on sync.
__global__ void combine_kernel(Cfg c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.out_len) return;
  const uint32_t fb = c.fb;
  const uint64_t stride = (uint64_t)c.out_len * fb;
  if (fb == 8) {
    uint64_t s = 0;
    for (uint32_t q = 0; q < nparts; q++) {
      const uint8_t* p = parts + q * stride + (uint64_t)i * 8;
      uint64_t v = 0;
      for (int k = 7; k >= 0; k--) v = (v << 8) | p[k];
      if (v >= P64) {
        atomicOr(err, 1u);
        v -= P64;
      }
      s = add64(s, v);
    }
    for (int k = 0; k < 8; k++) out[(uint64_t)i * 8 + k] = (uint8_t)(s >> (8 * k));
  } else {
    f128 s = make128(0, 0);
    for (uint32_t q = 0; q < nparts; q++) {
      const uint8_t* p = parts + q * stride + (uint64_t)i * 16;
      uint64_t lo = 0, hi = 0;
      for (int k = 7; k >= 0; k--) lo = (lo << 8) | p[k];
      for (int k = 15; k >= 8; k--) hi = (hi << 8) | p[k];
      f128 v = make128(lo, hi);
      if (ge_p128(v)) {
        atomicOr(err, 1u);
        v = sub128(v, make128(P128_LO, P128_HI));
      }
      s = add128(s, v);
    }
    for (int k = 0; k < 8; k++) out[(uint64_t)i * 16 + k] = (uint8_t)(s.lo >> (8 * k));
    for (int k = 0; k < 8; k++) out[(uint64_t)i * 16 + 8 + k] = (uint8_t)(s.hi >> (8 * k));
  }
}

// shard record = encoded aggregate share || count (u64 LE) || checksum (32 B), see
// janus_amd/distributed.py. Thread i < out_len writes element i; thread out_len the tail.
// blockIdx.y = record: ns records from contiguous segment state (agg [ns][out_len], count [ns],
// checksum [ns][8]) to ns back-to-back records
__global__ void record_export_kernel(Cfg c, const uint4* agg, const unsigned long long* count,
                                     const uint32_t* checksum, uint8_t* dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t fb = c.fb, y = blockIdx.y;
  agg += (uint64_t)y * c.out_len;
  count += y;
  checksum += 8 * y;
  dst += (uint64_t)y * (c.out_len * fb + 40u);
  if (i < c.out_len) {
    uint4 v = agg[i];
    for (uint32_t k = 0; k < fb; k++) {
      uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
      dst[(uint64_t)i * fb + k] = (uint8_t)(w >> (8 * (k & 3)));
    }
  } else if (i == c.out_len) {
    uint8_t* t = dst + (uint64_t)c.out_len * fb;
    const unsigned long long n = *count;
    for (int k = 0; k < 8; k++) t[k] = (uint8_t)(n >> (8 * k));
    for (int k = 0; k < 32; k++) t[8 + k] = (uint8_t)(checksum[k >> 2] >> (8 * (k & 3)));
  }
}

// merge nparts shard records (compute_aggregate_share, aggregate_share.rs:87-95):
// mod-p sum of the aggregate shares, sum of the counts, XOR of the checksums.
__global__ void record_combine_kernel(Cfg c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t fb = c.fb;
  const uint64_t stride = (uint64_t)c.out_len * fb + 40;
  if (i < c.out_len) {
    if (fb == 8) {
      uint64_t s = 0;
      for (uint32_t q = 0; q < nparts; q++) {
        const uint8_t* p = parts + q * stride + (uint64_t)i * 8;
        uint64_t v = 0;
        for (int k = 7; k >= 0; k--) v = (v << 8) | p[k];
        if (v >= P64) {
          atomicOr(err, 1u);
          v -= P64;
        }
        s = add64(s, v);
      }
      for (int k = 0; k < 8; k++) out[(uint64_t)i * 8 + k] = (uint8_t)(s >> (8 * k));
    } else {
      f128 s = make128(0, 0);
      for (uint32_t q = 0; q < nparts; q++) {
        const uint8_t* p = parts + q * stride + (uint64_t)i * 16;
        uint64_t lo = 0, hi = 0;
        for (int k = 7; k >= 0; k--) lo = (lo << 8) | p[k];
        for (int k = 15; k >= 8; k--) hi = (hi << 8) | p[k];
        f128 v = make128(lo, hi);
        if (ge_p128(v)) {
          atomicOr(err, 1u);
          v = sub128(v, make128(P128_LO, P128_HI));
        }
        s = add128(s, v);
      }
      for (int k = 0; k < 8; k++) out[(uint64_t)i * 16 + k] = (uint8_t)(s.lo >> (8 * k));
      for (int k = 0; k < 8; k++) out[(uint64_t)i * 16 + 8 + k] = (uint8_t)(s.hi >> (8 * k));
    }
  } else if (i == c.out_len) {
    const uint64_t tail = (uint64_t)c.out_len * fb;
    uint64_t n = 0;
    uint8_t cs[32];
    for (int k = 0; k < 32; k++) cs[k] = 0;
    for (uint32_t q = 0; q < nparts; q++) {
      const uint8_t* p = parts + q * stride + tail;
      uint64_t v = 0;
      for (int k = 7; k >= 0; k--) v = (v << 8) | p[k];
      n += v;
      for (int k = 0; k < 32; k++) cs[k] ^= p[8 + k];
    }
    for (int k = 0; k < 8; k++) out[tail + k] = (uint8_t)(n >> (8 * k));
    for (int k = 0; k < 32; k++) out[tail + 8 + k] = cs[k];
  }
}

// interleaved output shares -> [r][i] LE bytes
__global__ void transpose_out_kernel(Cfg c, const uint4* outs, uint64_t n, uint8_t* dst) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = t / c.out_len;
  const uint32_t i = t % c.out_len;
  if (r >= n) return;
  uint4 v = outs[il_idx(r / 64, c.out_len, i, r % 64)];
  if (c.fb == 8) {
    *reinterpret_cast<uint2*>(dst + t * 8) = make_uint2(v.x, v.y);
  } else {
    *reinterpret_cast<uint4*>(dst + t * 16) = v;
  }
}

// Coalesced launches (jx_coalesce.cpp): copy job j's slice [first, first + n) of the launch's staging into
// the job's own resident batch, so every job keeps an independent batch (interleaved output shares
// re-based to lane 0, verdicts, prep messages / leader seeds, report ids). blockIdx.y = job; the threads of
// a job stride over its destination elements (coalesced writes, reads shifted by first % 64).
__global__ __launch_bounds__(256) void scatter_jobs_kernel(Cfg c, const JobSlice* jobs, const uint4* outs,
                                                           const uint8_t* verdicts, const uint8_t* msgs,
                                                           const uint8_t* nonces) {
  const JobSlice j = jobs[blockIdx.y];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nblk = (j.n + 63) / 64;
  const uint64_t total = nblk * c.out_len * 64;
  for (uint64_t t = t0; t < total; t += stride) {
    const uint64_t blk = t / ((uint64_t)c.out_len * 64);
    const uint32_t rem = (uint32_t)(t % ((uint64_t)c.out_len * 64));
    const uint32_t e = rem / 64, l = rem % 64;
    const uint64_t i = blk * 64 + l;
    if (i >= j.n) continue;
    const uint64_t r = j.first + i;
    j.outs[t] = outs[il_idx(r / 64, c.out_len, e, r % 64)];
  }
  const uint32_t mb = c.seed;  // prep message / seed bytes: 16 or 32
  for (uint64_t i = t0; i < j.n; i += stride) {
    const uint64_t r = j.first + i;
    j.verdicts[i] = verdicts[r];
    const uint4* sm = reinterpret_cast<const uint4*>(msgs + r * mb);
    uint4* dm = reinterpret_cast<uint4*>(j.msgs + i * mb);
    dm[0] = sm[0];
    if (mb == 32) dm[1] = sm[1];
    reinterpret_cast<uint4*>(j.nonces)[i] = reinterpret_cast<const uint4*>(nonces)[r];
  }
}

__global__ void agg_encode_kernel(Cfg c, const uint4* agg, uint8_t* dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.out_len) return;
  uint4 v = agg[i];
  if (c.fb == 8)
    *reinterpret_cast<uint2*>(dst + (uint64_t)i * 8) = make_uint2(v.x, v.y);
  else
    *reinterpret_cast<uint4*>(dst + (uint64_t)i * 16) = v;
}

// ---------------------------------------------------------------------------- launchers

hipError_t launch_accumulate(const Cfg& c, const AccArgs& a, uint4* agg, hipStream_t s) {
  // sel lives at the tail of the partials allocation (see engine)
  uint8_t* sel = reinterpret_cast<uint8_t*>(a.partials + (size_t)a.nchunks * c.out_len * 3);
  uint64_t nthreads = ((a.n + 63) / 64) * 64;
  uint64_t swg = (nthreads + 255) / 256;
  if (swg > SELECT_WGS) swg = SELECT_WGS;
  hipLaunchKernelGGL(select_kernel, dim3((uint32_t)swg), dim3(256), 0, s, a, sel);
  hipLaunchKernelGGL(accumulate_kernel, dim3((c.out_len + 3) / 4, a.nchunks), dim3(256), 0, s, a,
                     (const uint8_t*)sel);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((c.out_len + 3) / 4), dim3(256), 0, s, c,
                     (const uint64_t*)a.partials, a.nchunks, agg);
  return hipGetLastError();
}

hipError_t launch_accumulate_small(const Cfg& c, const AccArgs& a, uint4* agg, hipStream_t s) {
  hipLaunchKernelGGL(accumulate_small_kernel, dim3((c.out_len + 3) / 4), dim3(256), 0, s, c, a, agg);
  return hipGetLastError();
}

__global__ __launch_bounds__(64) void host_signal_kernel(uint32_t* flag, uint32_t seq) {
  if (threadIdx.x == 0) __hip_atomic_store(flag + threadIdx.x, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_host_signal(uint32_t* flag, uint32_t seq, hipStream_t s) {
  hipLaunchKernelGGL(host_signal_kernel, dim3(1), dim3(64), 0, s, flag, seq);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void copy_regions_kernel(CopyArgs a) {
  const CopyRegion g = a.r[blockIdx.y];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool vec = ((g.width | g.dst_stride | g.src_stride | (uint64_t)(uintptr_t)g.dst | (uint64_t)(uintptr_t)g.src) & 15) == 0;
  if (vec) {
    const uint64_t cpr = g.width / 16, total = cpr * g.rows;
    for (uint64_t t = t0; t < total; t += step) {
      const uint64_t row = t / cpr, ch = t - row * cpr;
      *reinterpret_cast<uint4*>(g.dst + row * g.dst_stride + 16 * ch) =
          *reinterpret_cast<const uint4*>(g.src + row * g.src_stride + 16 * ch);
    }
  } else if (g.rows == 1 && (((uint64_t)(uintptr_t)g.dst | (uint64_t)(uintptr_t)g.src) & 15) == 0) {
    // one flat run of a length that is not a multiple of 16 (a launch's verdicts, open statuses): 16-byte vectors
    // and a byte tail, not one PCIe write per byte
    const uint64_t nv = g.width / 16;
    for (uint64_t t = t0; t < nv; t += step)
      reinterpret_cast<uint4*>(g.dst)[t] = reinterpret_cast<const uint4*>(g.src)[t];
    if (t0 < g.width - 16 * nv) g.dst[16 * nv + t0] = g.src[16 * nv + t0];
  } else {
    const uint64_t total = g.width * g.rows;
    for (uint64_t t = t0; t < total; t += step) {
      const uint64_t row = t / g.width, bt = t - row * g.width;
      g.dst[row * g.dst_stride + bt] = g.src[row * g.src_stride + bt];
    }
  }
}
hipError_t launch_copy_regions(const CopyArgs& a, hipStream_t s) {
  if (a.nr == 0) return hipSuccess;
  if (a.nr > COPY_MAX_REGIONS) return hipErrorInvalidValue;
  uint64_t most = 0;
  for (uint32_t k = 0; k < a.nr; k++) {
    const CopyRegion& g = a.r[k];
    const bool vec = ((g.width | g.dst_stride | g.src_stride | (uint64_t)(uintptr_t)g.dst | (uint64_t)(uintptr_t)g.src) & 15) == 0;
    const bool flat16 = g.rows == 1 && (((uint64_t)(uintptr_t)g.dst | (uint64_t)(uintptr_t)g.src) & 15) == 0;
    const uint64_t items = vec ? g.width / 16 * g.rows : flat16 ? g.width / 16 + 16 : g.width * g.rows;
    if (items > most) most = items;
  }
  // PCIe-bound: a few hundred waves keep enough reads in flight, and a big launch's K1 keeps the rest of the
  // SIMDs (JX_COPY_WGS overrides the cap for measurement)
  static const uint64_t cap = [] {
    const char* e = getenv("JX_COPY_WGS");
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 4096 ? (uint64_t)v : (uint64_t)64;
  }();
  uint64_t gx = (most + 255) / 256;
  if (gx > cap) gx = cap;
  if (gx == 0) gx = 1;
  hipLaunchKernelGGL(copy_regions_kernel, dim3((uint32_t)gx, a.nr), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_accumulate_multi(const Cfg& c, const AccMultiArgs& a, hipStream_t s) {
  if (a.nb == 0) return hipSuccess;
  if (a.nb > ACC_MULTI_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(accumulate_multi_kernel, dim3(c.out_len + a.nb), dim3(256), 0, s, c, a);
  return hipGetLastError();
}

// grid: workgroups of the count/scatter passes (the same for both: each workgroup re-walks its reports)
hipError_t launch_accumulate_segmented(const Cfg& c, const SegArgs& a, uint32_t grid, hipStream_t s) {
  (void)c;
  hipLaunchKernelGGL(seg_count_kernel, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(seg_scatter_kernel, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(seg_accumulate_kernel, dim3((a.out_len + 3) / 4, a.wmax), dim3(256), 0, s, a);
  // one thread per possible sorted position (n bounds the selected count); the rest return at once
  hipLaunchKernelGGL(seg_checksum_kernel, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(seg_reduce_kernel, dim3((a.out_len + 3) / 4, a.ns), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_combine(const Cfg& c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err,
                          hipStream_t s) {
  hipLaunchKernelGGL(combine_kernel, dim3((c.out_len + 255) / 256), dim3(256), 0, s, c, parts, nparts, out, err);
  return hipGetLastError();
}
hipError_t launch_record_export(const Cfg& c, const uint4* agg, const unsigned long long* count,
                                const uint32_t* checksum, uint8_t* dst, hipStream_t s, uint32_t ns) {
  hipLaunchKernelGGL(record_export_kernel, dim3((c.out_len + 1 + 255) / 256, ns), dim3(256), 0, s, c, agg, count,
                     checksum, dst);
  return hipGetLastError();
}
hipError_t launch_record_combine(const Cfg& c, const uint8_t* parts, uint32_t nparts, uint8_t* out, uint32_t* err,
                                 hipStream_t s) {
  hipLaunchKernelGGL(record_combine_kernel, dim3((c.out_len + 1 + 255) / 256), dim3(256), 0, s, c, parts, nparts,
                     out, err);
  return hipGetLastError();
}
hipError_t launch_transpose_out(const Cfg& c, const uint4* outs, uint64_t n, uint8_t* dst, hipStream_t s) {
  uint64_t t = n * c.out_len;
  hipLaunchKernelGGL(transpose_out_kernel, dim3((uint32_t)((t + 255) / 256)), dim3(256), 0, s, c, outs, n, dst);
  return hipGetLastError();
}
hipError_t launch_scatter_jobs(const Cfg& c, const JobSlice* d_jobs, uint32_t njobs, uint64_t max_job_reports,
                               const uint4* outs, const uint8_t* verdicts, const uint8_t* msgs, const uint8_t* nonces,
                               hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  const uint64_t elems = (max_job_reports + 63) / 64 * 64 * c.out_len;
  uint64_t gx = (elems + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(scatter_jobs_kernel, dim3((uint32_t)gx, njobs), dim3(256), 0, s, c, d_jobs, outs, verdicts, msgs,
                     nonces);
  return hipGetLastError();
}
hipError_t launch_agg_encode(const Cfg& c, const uint4* agg, uint8_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(agg_encode_kernel, dim3((c.out_len + 255) / 256), dim3(256), 0, s, c, agg, dst);
  return hipGetLastError();
}

}  // namespace jx
