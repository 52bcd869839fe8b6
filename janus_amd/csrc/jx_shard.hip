// jx_shard.hip — Prio3.shard on the device (VDAF-08 §7.2.1; the oracle's jo_shard): the client side of Count, Sum,
// SumVec and Histogram. DESIGN.md §5.6 has the algorithm, the lane mapping and the resource table.
//
//   shard_check_kernel    a lane per report: the measurement's range (prio's encode_measurement refuses the rest)
//   shard_count_kernel    Prio3Count, a lane per report: Field64, P = 2, the gadget polynomial in closed form
//   shard_expand_kernel   a lane per (report, stream): the helper's measurement share and, in the same pass, the
//                         leader's share enc(meas) - helper share straight into the leader input share row; the
//                         prove randomness; the helper's proof share (into the row's proof area, which the prove
//                         kernel then turns into the leader's share in place)
//   shard_absorb_kernel   a lane per (report, aggregator): the joint-randomness part over the share just written,
//                         the two parts exchanged between neighbouring lanes, then the joint-rand seed, r =
//                         joint_rand[0] and the table r^(chunk k) the wires are built from
//   shard_prove_kernel    FlpGeneric.prove, a workgroup per report and a wave per wire pair (jx_ntt.h)
//
// Every stream is sampled exactly: xof_stream128 tests each 16-byte chunk against p and skips a rejected one, at
// any position of any stream (sample64 does the same for Field64).
#include <hip/hip_runtime.h>

#include "jx_field.h"
#include "jx_keccak.h"
#include "jx_ntt.h"
#include "jx_sample.h"
#include "jx_shard.h"

namespace jx {

namespace {

constexpr uint8_t SHARD_INVALID = 1;  // JX_SHARD_INVALID_MEASUREMENT

__device__ __forceinline__ void ld16(const uint8_t* p, uint32_t w[4]) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = q[i];
}
__device__ __forceinline__ void st16(uint8_t* p, const uint32_t w[4], bool keep) {
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = keep ? w[i] : 0u;
}

// bit idx of the encoded measurement (flp_encode): Sum and SumVec entries little-endian, Histogram one-hot
__device__ __forceinline__ uint32_t meas_bit(const ShardArgs& a, const uint64_t* m, uint64_t idx) {
  if (a.algo == ALGO_HISTOGRAM) return m[0] == idx;
  if (a.algo == ALGO_SUM) return (uint32_t)(m[0] >> idx) & 1u;
  const uint64_t e = idx / a.bits;
  return (uint32_t)(m[e] >> (idx - e * a.bits)) & 1u;
}

// XofTurboShake128(seed, dst(usage), binder of NB <= 2 bytes): the state holds the first output block
template <int NB>
__device__ __forceinline__ void xof_start(uint32_t* S, uint32_t dst_id, uint32_t usage, const uint32_t seed[4],
                                          uint32_t b0, uint32_t b1) {
  Block m;
  blk_zero(m);
  const int pos = blk_xof_prefix(m, dst_id, usage, seed);
  if (NB > 0) blk_put_byte(m, pos, b0);
  if (NB > 1) blk_put_byte(m, pos + 1, b1);
  blk_pad(m, pos + NB);
  sponge_oneblock(S, m);
}

}  // namespace

// ---------------------------------------------------------------------------- measurement range
__global__ __launch_bounds__(256) void shard_check_kernel(ShardArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const uint64_t* m = a.meas + r * a.mstride;
  bool ok = true;
  if (a.algo == ALGO_COUNT)
    ok = m[0] < 2;
  else if (a.algo == ALGO_SUM)
    ok = a.bits >= 64 || (m[0] >> a.bits) == 0;
  else if (a.algo == ALGO_HISTOGRAM)
    ok = m[0] < a.length;
  else if (a.bits < 64)
    for (uint32_t i = 0; i < a.length; i++) ok = ok && (m[i] >> a.bits) == 0;
  a.status[r] = ok ? 0 : SHARD_INVALID;
}

// ---------------------------------------------------------------------------- Prio3Count
// Wires (seed_0, x) and (seed_1, x) at the points 1 and -1: w_i(X) = (s_i + x)/2 + (s_i - x)/2 X, and the
// gadget polynomial w_0 w_1 has three coefficients. proof = s_0, s_1, c_0, c_1, c_2.
__global__ __launch_bounds__(64) void shard_count_kernel(ShardArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const bool ok = a.status[r] == 0;
  const uint8_t* rd = a.rands + r * a.rand_bytes;
  uint32_t km[4], kp[4], kr[4];
  ld16(rd, km);
  ld16(rd + 16, kp);
  ld16(rd + 32, kr);
  uint8_t* his = a.his + r * a.his_bytes;
  st16(his, km, ok);
  st16(his + 16, kp, ok);
  uint64_t* row = reinterpret_cast<uint64_t*>(a.lis + r * a.lis_stride);
  const uint32_t pad0 = a.lis_bytes / 8, pad1 = (uint32_t)(a.lis_stride / 8);
  for (uint32_t i = pad0; i < pad1; i++) row[i] = 0;
  if (!ok) {
    for (uint32_t i = 0; i < pad0; i++) row[i] = 0;
    return;
  }
  const uint64_t x = a.meas[r * a.mstride];
  uint32_t S[50];
  uint64_t hm[1], s[2], hp[5];
  xof_start<1>(S, a.dst_id, 1, km, 1, 0);
  sample64<1>(S, hm);
  xof_start<1>(S, a.dst_id, 4, kr, 1, 0);
  sample64<2>(S, s);
  xof_start<2>(S, a.dst_id, 2, kp, 1, 1);
  sample64<5>(S, hp);
  const uint64_t half = 0x7FFFFFFF80000001ull;  // (p + 1) / 2
  const uint64_t a0 = mul64(add64(s[0], x), half), a1 = mul64(sub64(s[0], x), half);
  const uint64_t b0 = mul64(add64(s[1], x), half), b1 = mul64(sub64(s[1], x), half);
  const uint64_t proof[5] = {s[0], s[1], mul64(a0, b0), add64(mul64(a0, b1), mul64(a1, b0)), mul64(a1, b1)};
  row[0] = sub64(x, hm[0]);
#pragma unroll
  for (int i = 0; i < 5; i++) row[1 + i] = sub64(proof[i], hp[i]);
}

// ---------------------------------------------------------------------------- the three expansions
// blockIdx.y: 0 the measurement shares, 1 the prove randomness, 2 the helper's proof share
__global__ __launch_bounds__(64) void shard_expand_kernel(ShardArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= a.n) return;
  const uint32_t role = blockIdx.y;
  const bool ok = a.status[r] == 0;
  const uint8_t* rd = a.rands + r * a.rand_bytes;
  uint4* row = reinterpret_cast<uint4*>(a.lis + r * a.lis_stride);
  const uint4 zero = make_uint4(0, 0, 0, 0);
  uint32_t S[50];
  if (role == 0) {
    uint32_t km[4], kp[4], bl[4], bh[4];
    ld16(rd, km);
    ld16(rd + 16, kp);
    uint8_t* his = a.his + r * a.his_bytes;
    st16(his, km, ok);
    st16(his + 16, kp, ok);
    if (a.jr) {
      ld16(rd + 48, bl);
      ld16(rd + 64, bh);
      st16(his + 32, bh, ok);
      row[a.meas_len + a.proof_len] = ok ? make_uint4(bl[0], bl[1], bl[2], bl[3]) : zero;
    }
    for (uint64_t i = a.lis_bytes / 16; i < a.lis_stride / 16; i++) row[i] = zero;
    if (!ok) {
      for (uint32_t k = 0; k < a.meas_len; k++) row[k] = zero;
      return;
    }
    const uint64_t* m = a.meas + r * a.mstride;
    uint4* hm = a.hmeas + r * a.meas_len;
    xof_start<1>(S, a.dst_id, 1, km, 1, 0);
    xof_stream128(S, a.meas_len, [&](uint32_t k, f128 v) __attribute__((always_inline)) {
      hm[k] = f_to_u4(v);
      row[k] = f_to_u4(sub128(make128(meas_bit(a, m, k), 0), v));
    });
  } else if (role == 1) {
    if (!ok) return;
    uint32_t kr[4];
    ld16(rd + 32, kr);
    uint4* pr = a.prand + r * a.arity;
    xof_start<1>(S, a.dst_id, 4, kr, 1, 0);
    xof_stream128(S, a.arity, [&](uint32_t k, f128 v) __attribute__((always_inline)) { pr[k] = f_to_u4(v); });
  } else {
    uint4* pp = row + a.meas_len;
    if (!ok) {
      for (uint32_t k = 0; k < a.proof_len; k++) pp[k] = zero;
      return;
    }
    uint32_t kp[4];
    ld16(rd + 16, kp);
    xof_start<2>(S, a.dst_id, 2, kp, 1, 1);
    xof_stream128(S, a.proof_len, [&](uint32_t k, f128 v) __attribute__((always_inline)) { pp[k] = f_to_u4(v); });
  }
}

// ---------------------------------------------------------------------------- joint randomness
// Lane 2r absorbs the leader's measurement share (from its row), lane 2r + 1 the helper's (from the scratch):
// joint_rand_part = XOF(blind, dst(7), agg_id || nonce || share)[0..16]. The message is a 42-byte header and
// then the share, so block m's words are the share's aligned words from byte 168 m - 44 on, shifted by 16 bits.
__global__ __launch_bounds__(64) void shard_absorb_kernel(ShardArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = t < 2 * a.n;
  const uint64_t r = live ? t >> 1 : a.n - 1;
  const uint32_t agg = (uint32_t)t & 1u;
  const bool ok = a.status[r] == 0;
  const uint8_t* src =
      agg ? reinterpret_cast<const uint8_t*>(a.hmeas + r * a.meas_len) : a.lis + r * a.lis_stride;
  const uint32_t MB = a.meas_len * 16, ML = 42 + MB, b_last = ML / 168;
  uint32_t hdr[11];
  {
    uint32_t nonce[4], blind[4];
    ld16(a.nonces + 16 * r, nonce);
    ld16(a.rands + r * a.rand_bytes + 48 + 16 * agg, blind);
    Block h;
    blk_zero(h);
    const int pos = blk_xof_prefix(h, a.dst_id, 7, blind);
    blk_put_byte(h, pos, agg);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(h, pos + 1 + 4 * i, nonce[i]);
#pragma unroll
    for (int w = 0; w < 11; w++) hdr[w] = h.w[w];
  }
  uint32_t J[50];
#pragma unroll
  for (int w = 0; w < 50; w++) J[w] = 0;
#pragma unroll 1
  for (uint32_t m = 0; m <= b_last; m++) {
    uint32_t L[43];
    const int64_t base = 168ll * m - 44;
#pragma unroll
    for (int i = 0; i < 43; i++) {
      const int64_t off = base + 4 * i;
      L[i] = (ok && off >= 0 && off < (int64_t)MB) ? *reinterpret_cast<const uint32_t*>(src + off) : 0u;
    }
    uint32_t jw[42];
#pragma unroll
    for (int w = 0; w < 42; w++) jw[w] = alignbit(L[w + 1], L[w], 16);
    if (m == 0) {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = hdr[w];
      jw[10] = (hdr[10] & 0xffffu) | (L[11] << 16);
    }
    if (m == b_last) {  // TurboSHAKE padding: D = 1 after the message's last byte, 0x80 in the block's last
      const uint32_t nb = ML - 168 * b_last;
#pragma unroll
      for (int w = 0; w < 42; w++)
        if ((uint32_t)w == (nb >> 2)) jw[w] ^= 1u << (8 * (nb & 3));
      jw[41] ^= 0x80000000u;
    }
#pragma unroll
    for (int w = 0; w < 42; w++) J[w] ^= jw[w];
    keccak_p12(J);
  }
  uint32_t mine[4] = {J[0], J[1], J[2], J[3]}, other[4];
#pragma unroll
  for (int i = 0; i < 4; i++) other[i] = __shfl_xor(mine[i], 1);
  if (live) st16(a.ps + r * a.ps_bytes + 16 * agg, mine, ok);
  if (a.algo == ALGO_SUM || agg || !live || !ok) return;  // Prio3Sum's wires are the bits: no joint randomness in them
  // joint-rand seed = XOF(0, dst(6), part_0 || part_1)[0..16]; joint_rand[0] = its stream's first element (dst(3), [1])
  uint32_t seed[4];
  {
    const uint32_t z[4] = {0, 0, 0, 0};
    Block b;
    blk_zero(b);
    const int pos = blk_xof_prefix(b, a.dst_id, 6, z);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(b, pos + 4 * i, mine[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(b, pos + 16 + 4 * i, other[i]);
    blk_pad(b, pos + 32);
    sponge_oneblock(J, b);
#pragma unroll
    for (int i = 0; i < 4; i++) seed[i] = J[i];
  }
  xof_start<1>(J, a.dst_id, 3, seed, 1, 0);
  f128 rr = make128(0, 0);
  xof_stream128(J, 1, [&](uint32_t, f128 v) __attribute__((always_inline)) { rr = v; });
  const f128 rR = to_mont128(rr);
  a.rjr[r] = f_to_u4(rR);
  const f128 rc = mpow(rR, a.chunk);
  f128 cur = make128(1, 0);
  uint4* cp = a.cpow + r * a.P;
  for (uint32_t k = 0; k < a.calls; k++) {
    cp[k] = f_to_u4(cur);
    cur = mont128(cur, rc);
  }
}

// ---------------------------------------------------------------------------- FlpGeneric.prove
// A workgroup per report; wave w takes the wire pairs (chunk slots) w, w + W, ... Per wave in LDS: the pair's
// values A, B (P each) and the accumulators E, O of G's values at the even and odd points. Point k of slot j's
// wires is call k's input pair: (r^(idx+1) x, x - 1) for measurement element idx = (k - 1) chunk + j, (0, -1) for a
// padded slot, the prove randomness at k = 0 and zero past the last call. Prio3Sum has the one wire of Range2.
__global__ __launch_bounds__(256) void shard_prove_kernel(ShardArgs a) {
  extern __shared__ uint4 lds_u4[];
  f128* const lds = reinterpret_cast<f128*>(lds_u4);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const uint64_t r = blockIdx.x;
  if (a.status[r]) return;  // the whole workgroup: the rows were zeroed by shard_expand_kernel
  const uint32_t P = a.P;
  f128 *const A = lds + (size_t)wave * 4 * P, *const B = A + P, *const E = B + P, *const O = E + P;
  const f128* tab = reinterpret_cast<const f128*>(a.tab);
  uint4* const row = reinterpret_cast<uint4*>(a.lis + r * a.lis_stride) + a.meas_len;  // the proof share
  const uint4* prand = a.prand + r * a.arity;
  const uint64_t* m = a.meas + r * a.mstride;
  const auto sync = [] { wave_sync(); };
  const f128 zero = make128(0, 0), one = make128(1, 0), minus1 = make128(P128_LO - 1, P128_HI);
  for (uint32_t k = lane; k < P; k += 64) E[k] = O[k] = zero;
  // the wire seeds: the leader's share of the proof's first `arity` elements
  for (uint32_t j = threadIdx.x; j < a.arity; j += blockDim.x)
    row[j] = f_to_u4(sub128(u4_to_f(prand[j]), u4_to_f(row[j])));
  if (a.algo == ALGO_SUM) {
    if (wave == 0) {
      for (uint32_t k = lane; k < P; k += 64) {
        f128 v = zero;
        if (k == 0)
          v = u4_to_f(prand[0]);
        else if (k <= a.calls)
          v = make128(meas_bit(a, m, k - 1), 0);
        A[k] = v;
        E[k] = mont128(v, sub128(v, one));
      }
      sync();
      ntt_odd_points(A, P, tab, lane, 64u, sync);
      for (uint32_t k = lane; k < P; k += 64) O[k] = mont128(A[k], sub128(A[k], one));
      sync();
    }
  } else {
    const f128 rR = u4_to_f(a.rjr[r]);
    const f128 rW = mpow(rR, W);
    f128 rj = mpow(rR, wave + 1);  // r^(j+1) R
    const uint4* cp = a.cpow + r * P;
    for (uint32_t j = wave; j < a.chunk; j += W) {
      for (uint32_t k = lane; k < P; k += 64) {
        f128 va = zero, vb = zero;
        if (k == 0) {
          va = u4_to_f(prand[2 * j]);
          vb = u4_to_f(prand[2 * j + 1]);
        } else if (k <= a.calls) {
          const uint64_t idx = (uint64_t)(k - 1) * a.chunk + j;
          vb = minus1;
          if (idx < a.meas_len && meas_bit(a, m, idx)) {
            va = mont128(u4_to_f(cp[k - 1]), rj);
            vb = zero;
          }
        }
        A[k] = va;
        B[k] = vb;
        E[k] = add128(E[k], mont128(va, vb));
      }
      sync();
      ntt_odd_points(A, P, tab, lane, 64u, sync);
      ntt_odd_points(B, P, tab, lane, 64u, sync);
      for (uint32_t k = lane; k < P; k += 64) O[k] = add128(O[k], mont128(A[k], B[k]));
      sync();
      rj = mont128(rj, rW);
    }
  }
  __syncthreads();
  if (wave != 0) return;
  for (uint32_t w = 1; w < W; w++) {
    const f128 *Ew = lds + (size_t)w * 4 * P + 2 * P, *Ow = Ew + P;
    for (uint32_t k = lane; k < P; k += 64) {
      E[k] = add128(E[k], Ew[k]);
      O[k] = add128(O[k], Ow[k]);
    }
  }
  sync();
  uint4* const gp = row + a.arity;
  const uint32_t glen = a.gpoly_len;
  ntt_gpoly_finish(E, O, P, a.logP, tab, lane, 64u, sync, [&](uint32_t j, f128 g) __attribute__((always_inline)) {
    if (j < glen) gp[j] = f_to_u4(sub128(g, u4_to_f(gp[j])));
  });
}

// ---------------------------------------------------------------------------- launch
uint32_t shard_waves(uint32_t algo, uint32_t P, uint32_t chunk) {
  if (algo == ALGO_SUM) return 1;
  uint32_t w = SHARD_WG_LDS / (64u * P);
  if (w > 4) w = 4;
  if (w > chunk) w = chunk;
  return w < 1 ? 1 : w;
}
uint64_t shard_scratch_bytes(const ShardArgs& a) {
  if (a.algo == ALGO_COUNT) return 1;
  return 16ull * ((uint64_t)a.meas_len + a.arity + a.P + 1) + 1;
}

hipError_t launch_shard(const ShardArgs& a, hipStream_t s) {
  if (a.n > 0x7FFFFFFFull / 2) return hipErrorInvalidValue;
  const uint32_t n = (uint32_t)a.n;
  hipLaunchKernelGGL(shard_check_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
  if (a.algo == ALGO_COUNT) {
    hipLaunchKernelGGL(shard_count_kernel, dim3((n + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(shard_expand_kernel, dim3((n + 63) / 64, 3), dim3(64), 0, s, a);
  hipLaunchKernelGGL(shard_absorb_kernel, dim3((2 * n + 63) / 64), dim3(64), 0, s, a);
  hipLaunchKernelGGL(shard_prove_kernel, dim3(n), dim3(64 * a.waves), (size_t)a.waves * 64 * a.P, s, a);
  return hipGetLastError();
}

}  // namespace jx
