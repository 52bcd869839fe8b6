// jx_flp.hip — K3, the FLP query + decide kernels of the Prio3 engine, and the leader's prepare_next (the stages
// are described at the top of jx_kernels.hip, which keeps K0 and K1; the staging layout is in jx_kernels.h).
#include <type_traits>

#include "jx_field.h"
#include "jx_kernels.h"

namespace jx {

// ---------------------------------------------------------------------------- K3: FLP query + decide

__device__ __forceinline__ f128 ld_lead(const Bufs& b, const Cfg& c, uint64_t r, uint32_t idx, bool& dfail) {
  uint4 v = *reinterpret_cast<const uint4*>(b.lps + (uint64_t)c.lps_bytes * r + 16u * idx);
  f128 x = u4_to_f(v);
  dfail |= ge_p128(x);
  return x;
}

// Prio3Sum: gadget PolyEval(x^2 - x), arity 1, `bits` calls; one report per lane.
// LEADER: writes the leader's verifier share [v, W0, G(t)] as its prep share.
template <bool LEADER>
__global__ __launch_bounds__(256) void flp_sum_kernel(Cfg c, Bufs b) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint32_t NC = c.ncoef, C = c.calls;
  const uint4* omega = b.consts + c.c_omega;
  f128 LR = ld_il(b.coef, blk, NC, COEF_L, lane), c0R = ld_il(b.coef, blk, NC, COEF_C0, lane);
  f128 tR = ld_il(b.coef, blk, NC, COEF_T, lane), rR = ld_il(b.coef, blk, NC, COEF_R, lane);
  acc192 ao;
  acc_zero(ao);
  const MeasView mv = meas_view(c, b, blk, lane);
  for (uint32_t k = 1; k <= C; k++) {
    f128 x = u4_to_f(mv[k - 1]);
    uint64_t lo, hi;
    uint32_t top;
    mont128_lazy(x, ld_il(b.coef, blk, NC, COEF_K + k - 1, lane), lo, hi, top);
    acc_add(ao, lo, hi, top);
  }
  f128 s0 = ld_il(b.proof, blk, c.proof_len, 0, lane);
  f128 W0 = mont128(add128(mont128(s0, c0R), acc_reduce(ao)), LR);
  // v = sum_{k=1..C} r^k g(w^k). The spec evaluates the gadget polynomial g (GL = 2P - 1
  // coefficients) at every w^k by Horner: C * GL products and proof-share reads. Since w^P = 1,
  // g(w^k) = sum_{j<P} g'_j w^{kj} with g'_j = g_j + g_{j+P}, so
  //   v = sum_{j<P} g'_j S_j,   S_j = sum_{k=1..C} q_j^k,   q_j = r w^j.
  // w^{P/2} = -1 gives q_{j+P/2} = -q_j, so with E_j / O_j the even / odd-power parts of S_j,
  // S_j = E + O and S_{j+P/2} = E - O. With Q = q^2 and s = sum_{m=1..n} Q^m, n = floor(C/2):
  // E = s, O = q (1 + s - [C even] Q^n); s and Q^n come from the bits of n by doubling
  // (s_2n = s_n + Q^n s_n, Q^2n = (Q^n)^2; s_n+1 = s_n + Q^n+1). ~2 log2(C) products per pair of
  // j (identity checked in Python for C = 1..91), every proof coefficient read once.
  const uint32_t GL = c.gpoly_len, P = c.P, H = c.P / 2, n = C / 2;
  const f128 R1 = make128(R1_128_LO, R1_128_HI);
  f128 v = make128(0, 0);
  const f128 w1 = u4_to_f(omega[1 % P]);
  f128 wj = u4_to_f(omega[0]);  // w^j R
  for (uint32_t j = 0; j < H; j++) {
    f128 ga = ld_il(b.proof, blk, c.proof_len, 1 + j, lane);
    if (j + P < GL) ga = add128(ga, ld_il(b.proof, blk, c.proof_len, 1 + j + P, lane));
    f128 gb = ld_il(b.proof, blk, c.proof_len, 1 + j + H, lane);
    if (j + H + P < GL) gb = add128(gb, ld_il(b.proof, blk, c.proof_len, 1 + j + H + P, lane));
    const f128 q = mont128(rR, wj);  // r w^j, Montgomery form
    f128 sq = make128(0, 0), pq = R1;  // s_n, Q^n
    if (n > 0) {
      const f128 Q = mont128(q, q);
      sq = Q;
      pq = Q;
      const uint32_t top = 31u - (uint32_t)__builtin_clz(n);
      for (int bit = (int)top - 1; bit >= 0; bit--) {
        sq = add128(sq, mont128(pq, sq));
        pq = mont128(pq, pq);
        if ((n >> bit) & 1u) {
          pq = mont128(pq, Q);
          sq = add128(sq, pq);
        }
      }
    }
    const f128 O = mont128(q, add128(R1, (C & 1u) ? sq : sub128(sq, pq)));
    v = add128(v, mont128(ga, add128(sq, O)));
    v = add128(v, mont128(gb, sub128(sq, O)));
    wj = mont128(wj, w1);
  }
  f128 G = make128(0, 0);
  for (uint32_t m = GL; m-- > 0;) G = add128(mont128(G, tR), ld_il(b.proof, blk, c.proof_len, 1 + m, lane));
  if (LEADER) {
    if (r0 < b.n) {
      uint4* o = reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r);
      o[0] = f_to_u4(v);
      o[1] = f_to_u4(W0);
      o[2] = f_to_u4(G);
      b.verdicts[r0] = (b.flags[r] & (FLAG_INIT_FAIL | FLAG_INPUT_FAIL)) ? 1 : 0;
    }
    return;
  }
  bool dfail = false;
  f128 lv = ld_lead(b, c, r, 0, dfail), lw = ld_lead(b, c, r, 1, dfail), lg = ld_lead(b, c, r, 2, dfail);
  const uint32_t flags = b.flags[r];
  uint32_t verdict = 0;
  if (flags & FLAG_INIT_FAIL)
    verdict = 1;
  else if (dfail)
    verdict = 2;
  else {
    f128 V0 = add128(v, lv), V1 = add128(W0, lw), VG = add128(G, lg);
    // (V1^2 - V1) == VG, compared in the R^-1 scaled domain
    f128 lhs = sub128(mont128(V1, V1), mont128(V1, make128(1, 0)));
    if (!is_zero128(V0) || !eq128(lhs, mont128(VG, make128(1, 0))))
      verdict = 3;
    else if (flags & FLAG_NEXT_FAIL)
      verdict = 4;
  }
  if (r0 < b.n) b.verdicts[r0] = (uint8_t)verdict;
}

// The part kernels' common end: the calls kf+1..C (the ragged last call, or every call of a padded
// group) with guarded direct loads, then the wires at t, the leader's verifier share and the gadget
// polynomial's share of v and G(t) for group g of block blk.
template <int PPW, bool HIST, bool LEADER>
__device__ __forceinline__ void psum_group_finish(const Cfg& c, const Bufs& b, uint64_t blk, uint32_t g, uint32_t lane,
                                                  const f128* E, const f128* O, f128 sxr);
template <int PPW, bool HIST, bool LEADER>
__device__ __forceinline__ void psum_part_finish(const Cfg& c, const Bufs& b, uint64_t blk, uint32_t g, uint32_t lane,
                                                 uint32_t kf, wacc26* ae, wacc26* ao, acc192& sx) {
  const uint32_t NG = c.ngroups;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint32_t NC = c.ncoef, C = c.calls, chunk = c.chunk, M = c.meas_len, A = 2 * chunk;
  const uint32_t j0 = g * PPW;
  const uint4* cblk = b.coef + il_idx(blk, NC, 0, 0);
  const MeasView measb = meas_view(c, b, blk, lane);
#pragma unroll 1
  for (uint32_t k = kf + 1; k <= C; k++) {  // the ragged last call(s), or every call of a padded group
    limbs26 ck, dk;
    coef_call_limbs(ld_coef_call(cblk, lane, k), ck, dk);
    const uint32_t nb = (k - 1) * chunk + j0;
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      if (j0 + i < chunk && nb + i < M) {
        const f128 x = u4_to_f(measb[nb + i]);
        const limbs26 xl = to_limbs26(x);
        wacc_mac(ae[i], xl, dk);
        wacc_mac(ao[i], xl, ck);
        if (HIST) acc_add128(sx, x);
      }
    }
    if (((k - kf) & 511u) == 0) {
#pragma unroll
      for (int i = 0; i < PPW; i++) {
        wacc_normalize(ae[i]);
        wacc_normalize(ao[i]);
      }
    }
  }
  f128 E[PPW], O[PPW];
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    E[i] = wacc_reduce(ae[i]);
    O[i] = wacc_reduce(ao[i]);
  }
  psum_group_finish<PPW, HIST, LEADER>(c, b, blk, g, lane, E, O, HIST ? acc_reduce(sx) : make128(0, 0));
}

// The group finish from the reduced wire sums E_i = (sum_k d_k x_{k,i}) R, O_i = (sum_k c_k x_{k,i}) R of
// its PPW slots: wires at t (plus the leader's verifier share), this group's share of v and G(t), written
// as the four partial sums of the group (Histogram: sxr = its sum of x).
template <int PPW, bool HIST, bool LEADER>
__device__ __forceinline__ void psum_group_finish(const Cfg& c, const Bufs& b, uint64_t blk, uint32_t g, uint32_t lane,
                                                  const f128* E, const f128* O, f128 sxr) {
  const uint32_t NG = c.ngroups;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint32_t NC = c.ncoef, chunk = c.chunk, A = 2 * chunk;
  const uint32_t j0 = g * PPW;
  const uint4* coefb = b.coef + il_idx(blk, NC, 0, lane);
  // ---- wires at t for this group's slots, plus the leader's verifier share. K1 scaled the constants by
  // L (xof_tail): Lc = L canonical, c0LR = c_0 L R, hsL = L (sum c_k)/2, rpowL_j = L r^(j+1), so
  //   wire_even(t) = L (c_0 se + r^(j+1) sum_k d_k x) = mont(se, c0LR) + mont(E, rpowL_j)
  //   wire_odd(t)  = L (c_0 so + sum_k c_k x - (sum c_k)/2) = mont(so, c0LR) + mont(O, Lc) - hsL
  // (E, O are R-scaled: c_k, d_k are stored in Montgomery form).
  const f128 Lc = u4_to_f(coefb[COEF_L * IL]), c0LR = u4_to_f(coefb[COEF_C0 * IL]);
  const f128 hsL = u4_to_f(coefb[COEF_HALFSUM * IL]);
  bool dfail = false;
  f128 prod = make128(0, 0);
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    const uint32_t j = j0 + i;
    if (j < chunk) {
      f128 se = ld_il(b.proof, blk, c.proof_len, 2 * j, lane);
      f128 so = ld_il(b.proof, blk, c.proof_len, 2 * j + 1, lane);
      const f128 rpowL = u4_to_f(coefb[(c.c_rpow + j) * IL]);
      const f128 We = add128(mont128(se, c0LR), mont128(E[i], rpowL));
      const f128 Wo = sub128(add128(mont128(so, c0LR), mont128(O[i], Lc)), hsL);
      if (LEADER) {  // the leader's verifier share: wire values at t
        if (r0 < b.n) {
          uint4* o = reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r);
          o[1 + 2 * j] = f_to_u4(We);
          o[2 + 2 * j] = f_to_u4(Wo);
        }
      } else {
        f128 Ve = add128(We, ld_lead(b, c, r, 1 + 2 * j, dfail));
        f128 Vo = add128(Wo, ld_lead(b, c, r, 2 + 2 * j, dfail));
        prod = add128(prod, mont128(Ve, Vo));
      }
    }
  }
  // ---- gadget polynomial: v-part = sum_m g_m * S_m and the G(t) part over this group's m-range
  const uint32_t GL = c.gpoly_len;
  const uint32_t per = (GL + NG - 1) / NG;
  const uint32_t m0 = g * per, m1 = min(GL, m0 + per);
  const uint4* Sm = b.consts + c.c_S;
  f128 vpart = make128(0, 0), gpart = make128(0, 0);
  if (m0 < m1) {
    const f128 tR = u4_to_f(coefb[COEF_T * IL]);
    for (uint32_t m = m1; m-- > m0;) {
      f128 gm = ld_il(b.proof, blk, c.proof_len, A + m, lane);
      vpart = add128(vpart, mont128(gm, u4_to_f(Sm[m])));
      gpart = add128(mont128(gpart, tR), gm);
    }
    gpart = mont128(gpart, u4_to_f(coefb[(c.c_tpow + g) * IL]));  // t^m0 R (K1's table)
  }
  uint4* pp = b.part + ((blk * c.ngt + g) * 4) * IL + lane;
  pp[0] = f_to_u4(prod);
  pp[IL] = f_to_u4(vpart);
  pp[2 * IL] = f_to_u4(gpart);
  if (HIST) pp[3 * IL] = f_to_u4(sxr);
  if (dfail && r0 < b.n) atomicOr(&b.flags[r0], FLAG_DFAIL);
}

// Prio3SumVec / Prio3Histogram: gadget ParallelSum(Mul, chunk), arity 2*chunk.
//
// Phase 1 (flp_psum_part_kernel): one wave per (64-report block, slot group). Lanes are
// reports (the interleaved staging makes every load a coalesced 1 KiB). Group g owns the
// chunk slots [g*PPW, (g+1)*PPW) -- 2*PPW lazy wire accumulators per lane, small enough to
// stay in registers at >= 3 waves/SIMD -- and the gadget-polynomial coefficients
// [g*per, (g+1)*per). It writes four partial sums per report: sum_i Ve_i*Vo_i over its
// slots, its share of v (sum_m g_m S_m), its share of G(t), and (Histogram) sum of x.
// Phase 2 (flp_psum_final_kernel): one report per lane; adds the partials, the leader's
// v and G(t), and decides.
// PF: calls whose loads are in flight ahead of the one being multiplied (1: deeper register
// prefetch measured no faster). Used for PPW = 1; PPW = 2 takes the LDS-DMA ring kernel below.
template <int PPW, bool HIST, bool LEADER, int PF = 1>
__global__ __launch_bounds__(64, 4) void flp_psum_part_kernel(Cfg c, Bufs b) {
  const uint32_t NG = c.ngroups;
  // Workgroup ids are dispatched round-robin over the 8 XCDs; map them so that the NG
  // groups of one block run back to back on one XCD and share its L2 (coefficients,
  // leader share).
  const uint32_t bid = blockIdx.x;
  const uint32_t xcd = bid & 7u, q = bid >> 3;
  const uint32_t g = q % NG;
  const uint64_t blk = (uint64_t)(q / NG) * 8 + xcd;
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t NC = c.ncoef, C = c.calls, chunk = c.chunk, M = c.meas_len;
  const uint32_t j0 = g * PPW;

  // wire sums over the calls: ae[i] = sum_k d_k x_{k,i} * R, ao[i] = sum_k c_k x_{k,i} * R
  // (c_k, d_k are stored in Montgomery form), as unreduced 26-bit-limb column sums.
  wacc26 ae[PPW], ao[PPW];
  acc192 sx;
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    wacc_zero(ae[i]);
    wacc_zero(ao[i]);
  }
  acc_zero(sx);
  const uint4* cblk = b.coef + il_idx(blk, NC, 0, 0);
  const MeasView measb = meas_view(c, b, blk, lane);
  // calls whose PPW slots of this group are all real measurement elements run branch-free;
  // the rest (the ragged last chunk, slots beyond chunk) take the guarded tail loop
  uint32_t kf = 0;
  if (j0 + PPW <= chunk && M >= j0 + PPW) kf = min(C, (M - j0 - PPW) / chunk + 1);
  for (uint32_t k0 = 1; k0 <= kf; k0 += 512) {  // <= 5 * 512 limb products (< 2^52) per column
    const uint32_t k1 = min(kf, k0 + 511);
    // software pipeline: the loads of calls k+1 .. k+PF are in flight while call k multiplies
    CoefCall cr[PF];
    uint4 xr[PF][PPW];
#pragma unroll
    for (int u = 0; u < PF; u++) {
      const uint32_t k = k0 + u;
      if (k <= k1) {
        cr[u] = ld_coef_call(cblk, lane, k);
#pragma unroll
        for (int i = 0; i < PPW; i++) xr[u][i] = measb[(uint64_t)((k - 1) * chunk + j0 + i)];
      }
    }
#pragma unroll 1
    for (uint32_t kb = k0; kb <= k1; kb += PF) {
#pragma unroll
      for (int u = 0; u < PF; u++) {
        const uint32_t k = kb + u;
        if (k <= k1) {
          limbs26 ck, dk;
          coef_call_limbs(cr[u], ck, dk);
          f128 x[PPW];
#pragma unroll
          for (int i = 0; i < PPW; i++) x[i] = u4_to_f(xr[u][i]);
          const uint32_t kn = k + PF;
          if (kn <= k1) {
            cr[u] = ld_coef_call(cblk, lane, kn);
#pragma unroll
            for (int i = 0; i < PPW; i++) xr[u][i] = measb[(uint64_t)((kn - 1) * chunk + j0 + i)];
          }
#pragma unroll
          for (int i = 0; i < PPW; i++) {
            const limbs26 xl = to_limbs26(x[i]);
            wacc_mac(ae[i], xl, dk);
            wacc_mac(ao[i], xl, ck);
            if (HIST) acc_add128(sx, x[i]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      wacc_normalize(ae[i]);
      wacc_normalize(ao[i]);
    }
  }
  psum_part_finish<PPW, HIST, LEADER>(c, b, blk, g, lane, kf, ae, ao, sx);
}

// s_waitcnt vmcnt(N) alone (expcnt / lgkmcnt left unconstrained)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt(0x3f70 | (N & 15) | ((N >> 4) << 14));
}
__device__ __forceinline__ void glds16(const uint4* src, uint4* lds_row) {
  __builtin_amdgcn_global_load_lds((const void*)src, (void*)lds_row, 16, 0, 0);
}

__device__ __forceinline__ void glds4(const uint32_t* src, uint32_t* lds_row) {
  __builtin_amdgcn_global_load_lds((const void*)src, (void*)lds_row, 4, 0, 0);
}

// K3 with two LDS-DMA rings. A workgroup is K3W waves = K3W consecutive slot groups of one 64-report
// block. Per call k every wave streams its own PPW measurement elements into slot (k-1) % D of the
// measurement ring (depth D = 4) and a quarter of the call's coefficient limbs (K1 staged them as the ten
// 26-bit limbs of (c_k, d_k), jx_kernels.h: 2.5 KiB per call and block) into slot (k-1) % (D-1) of the
// coefficient ring: wave 0 row A and wave 1 row B (one global_load_lds_dwordx4 each), waves 2 and 3 one
// half of half-row C (a global_load_lds_dword each). So the coefficients are fetched once per K3W groups
// and never split into limbs here, every wave issues 1 + PPW loads per call, and D-1 (D-2) calls stay in
// flight without holding VGPRs; 4 x 8 + 3 x 2.5 = 39.5 KiB keeps four workgroups per CU. One s_barrier
// per call: after it, every wave's loads of call k have landed (each waited for its own with vmcnt) and
// every wave has finished reading call k-1's slots, which the next issues overwrite. Every call runs in
// the rings: an element past the share (the ragged last call) or of a padded slot is loaded from a zero
// constant, so it adds nothing, and a padding group's wave only keeps the barriers and its share of the
// coefficient loads.
//
// The loads of one wave complete in issue order, and iteration k issues c(k+2), then x(k+3): when
// iteration k starts, the loads issued after c(k) are x(k+1), c(k+1), x(k+2) = 2 PPW + 1, so
// vmcnt(2 PPW + 1) proves that c(k) and x(k) (issued before it) have landed, as long as those three were
// issued at all (k + 2 <= calls; later iterations wait for everything).
//
// The call loop is unrolled by D, so a block's measurement slots are the constants 0..3, and three such
// blocks (one per phase of the depth-3 coefficient ring) make every LDS address an immediate offset and
// every wait a constant; calls near the end (the last call's range check, fewer loads in flight) take the
// generic loop after it. The 512-call normalisation falls on a block's last call.
constexpr uint32_t K3W = 4;
// LDS address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) uint8_t*)p;
}
// One call's LDS reads (coefficient rows A, B and half-row C, two measurement rows) and one wait, in asm:
// the compiler's LDS-DMA wait tracking cannot tell which ring slot a read touches and would otherwise
// drain every outstanding global_load_lds (vmcnt(0)) before each read, serialising the rings; the explicit
// wait_vmcnt + s_barrier order the reads here. ca / ce: the lane's address in rows A / C of coefficient
// slot 0, x0 / x1: of its measurement rows in slot 0; OC / OX: the slots' byte offsets (immediates).
template <uint32_t OC, uint32_t OX>
__device__ __forceinline__ void lds_read_call(uint32_t ca, uint32_t ce, uint32_t x0, uint32_t x1, CoefCall& cv,
                                              uint4& xv0, uint4& xv1) {
  static_assert(OC + COEF_ROWB_U4 * 16 < 65536 && OX < 65536, "ds offsets are 16 bits");
  asm volatile(
      "ds_read_b128 %0, %5 offset:%9\n\t"
      "ds_read_b128 %1, %5 offset:%10\n\t"
      "ds_read_b64 %2, %6 offset:%9\n\t"
      "ds_read_b128 %3, %7 offset:%11\n\t"
      "ds_read_b128 %4, %8 offset:%11\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(cv.a), "=&v"(cv.b), "=&v"(cv.e), "=&v"(xv0), "=&v"(xv1)
      : "v"(ca), "v"(ce), "v"(x0), "v"(x1), "n"(OC), "n"(OC + COEF_ROWB_U4 * 16), "n"(OX)
      : "memory");
}
// W: waves (slot groups) per workgroup
// RING_ONLY (a measurement variant, instantiated only by tools/kernel_probe.hip): the ring, then a hash of
// the column sums instead of the group finish (results wrong by design), to time the finish by difference.
template <int PPW, bool HIST, bool LEADER, int D, int W = K3W, bool RING_ONLY = false>
__global__ __launch_bounds__(64 * W, 4) void flp_psum_part_glds_kernel(Cfg c, Bufs b) {
  static_assert(PPW == 2, "lds_read_call reads two measurement rows");
  static_assert(W == 4, "one quarter of a call's coefficient limbs per wave");
  static_assert(D == 4, "the unrolled blocks assume measurement depth 4, coefficient depth 3");
  constexpr int XROWS = W * PPW;  // x[wave][i]
  constexpr int DC = D - 1;       // depth of the coefficient ring
  constexpr uint32_t ROW_BYTES = 64 * 16, XSLOT = XROWS * ROW_BYTES, XBYTES = D * XSLOT;
  constexpr uint32_t CSLOT = COEF_CALL_BYTES;
  // the measurement ring [D][XROWS][64] uint4, then the coefficient ring [DC][COEF_CALL_U4] uint4
  __shared__ uint4 ring[D * XROWS * 64 + DC * COEF_CALL_U4];
  static_assert(sizeof(ring) <= 40 * 1024, "four workgroups per CU");
  const uint32_t NG = c.ngroups, NW = (NG + W - 1) / W;
  const uint32_t bid = blockIdx.x, xcd = bid & 7u, q = bid >> 3;
  const uint32_t wg = q % NW;
  const uint64_t blk = (uint64_t)(q / NW) * 8 + xcd;
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;  // uniform over the workgroup
  // (the wave index is uniform: in an SGPR, the ring slots' LDS addresses are scalar arithmetic)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t g = wg * W + wave;
  const uint32_t C = c.calls, chunk = c.chunk, M = c.meas_len;
  const uint32_t j0 = g * PPW;
  const MeasView measb = meas_view(c, b, blk, lane);
  const uint4* zero = b.consts + c.c_misc + MISC_ZERO;
  bool real[PPW];  // slot j0 + i exists (a padding group's wave has none)
#pragma unroll
  for (int i = 0; i < PPW; i++) real[i] = g < NG && j0 + i < chunk;

  wacc26 ae[PPW], ao[PPW];
  acc192 sx;
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    wacc_zero(ae[i]);
    wacc_zero(ao[i]);
  }
  acc_zero(sx);
  // The leader reads its explicit measurement share in place (report-major rows, Bufs::meas_rs): per call
  // the workgroup needs the W*PPW = 8 consecutive elements (128 bytes) of its slots from each of the 64
  // rows. Loaded per lane as the staged layout is (one 16-byte element of 64 rows per instruction) every
  // instruction touches 64 lines for 16 bytes each, and the other waves' parts of those lines come back
  // from HBM once L1/L2 have dropped them (4.0 MB of traffic per FixedPoint 16 x 10000 report against
  // 2.67 MB for the helper's staged stream). Here instruction q (wave q / PPW) reads rows 8q..8q+7 whole:
  // lane l = 8 pp + a takes row 8q + a, part p = pp ^ (q & 1), so eight lanes cover one row's 128 bytes.
  // The part swap on odd q puts rows r and r + 8 in opposite halves of a 256-byte LDS bank window, so the
  // consumers' ds_read_b128 (16 lanes per pass, lane = row) stay conflict-free.
  const bool inpl = LEADER && !HIST && b.meas_rs != 0;
  static_assert(W * PPW == 8, "one 128-byte row segment per report per call");
  // ---- sources. Measurement load u of this lane: the element's first-call address and whether its slot
  // exists (in place: slot wg * 8 + p of row 8 q + a; staged: slot j0 + u of the lane's report)
  const uint8_t* xbase[PPW];
  bool xreal[PPW], xlast[PPW];  // the slot exists; its element of the last call does (is below meas_len)
#pragma unroll
  for (int u = 0; u < PPW; u++) {
    uint32_t xslot;
    if (inpl) {
      const uint32_t q = wave * PPW + u, a = lane & 7u, p = (lane >> 3) ^ (q & 1u);
      const uint64_t r0 = blk * 64 + 8 * q + a, r = r0 < b.n ? r0 : b.n - 1;
      xslot = wg * (W * PPW) + p;
      xreal[u] = xslot < chunk;
      xbase[u] = b.meas_src + r * b.meas_rs + 16ull * xslot;
    } else {
      xslot = j0 + u;
      xreal[u] = real[u];
      xbase[u] = reinterpret_cast<const uint8_t*>(&measb[xslot]);
    }
    xlast[u] = xreal[u] && (C - 1) * chunk + xslot < M;
  }
  const uint64_t xstep = (uint64_t)chunk * measb.es * 16u;  // bytes from a call's element to the next call's
  // this wave's quarter of a call's coefficient limbs: its byte offset in the call's region (global and
  // LDS alike) and this lane's part of it
  const uint32_t cq = wave < 2 ? wave * ROW_BYTES : COEF_ROWC_U4 * 16 + (wave - 2) * 256;
  const uint8_t* cbase = reinterpret_cast<const uint8_t*>(b.coef + il_idx(blk, c.ncoef, COEF_K, 0)) + cq +
                         (wave < 2 ? lane * 16 : lane * 4);
  uint8_t* const ringb = reinterpret_cast<uint8_t*>(ring);
  // loads of call k: the coefficient quarter into slot sc of its ring, the measurement elements into slot sx
  auto issue_c = [&](const uint8_t* src, uint32_t sc) {
    uint8_t* dst = ringb + XBYTES + sc * CSLOT + cq;
    if (wave < 2)
      glds16(reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst));
    else
      glds4(reinterpret_cast<const uint32_t*>(src), reinterpret_cast<uint32_t*>(dst));
  };
  auto issue_x = [&](const uint8_t* const* src, uint32_t sx_) {
#pragma unroll
    for (int u = 0; u < PPW; u++)
      glds16(reinterpret_cast<const uint4*>(src[u]),
             reinterpret_cast<uint4*>(ringb + sx_ * XSLOT + (wave * PPW + u) * ROW_BYTES));
  };
  // Calls are issued in order, so a source is a running pointer: xp[u], stepping xst[u] per call (a missing
  // slot: the zero constant, step 0), and cp. Only the last call can reach past the share (xlast).
  const uint8_t* xp[PPW];
  uint64_t xst[PPW];
#pragma unroll
  for (int u = 0; u < PPW; u++) {
    xp[u] = xreal[u] ? xbase[u] : reinterpret_cast<const uint8_t*>(zero);
    xst[u] = xreal[u] ? xstep : 0u;
  }
  const uint8_t* cp = cbase;
  // (the empty asm keeps each pointer one register pair stepped in place: left alone, the compiler holds
  // multiples of the steps in further pairs for the unrolled calls, and the kernel spills)
  auto step_x = [&]() {
#pragma unroll
    for (int u = 0; u < PPW; u++) {
      xp[u] += xst[u];
      asm volatile("" : "+v"(xp[u]));
    }
  };
  // any call, every check made (the prologue and the generic loop)
  auto issue_c_k = [&](uint32_t k) {
    issue_c(cp, (k - 1) % DC);
    cp += CSLOT;
  };
  auto issue_x_k = [&](uint32_t k) {
    const uint8_t* src[PPW];
#pragma unroll
    for (int u = 0; u < PPW; u++)
      src[u] = k < C || xlast[u] ? xp[u] : reinterpret_cast<const uint8_t*>(zero);
    issue_x(src, (k - 1) % D);
    step_x();
  };
  // in the order the steady state issues them: x(1) c(1) x(2) c(2) x(3)
  for (uint32_t k = 1; k < D && k <= C; k++) {
    issue_x_k(k);
    if (k < DC) issue_c_k(k);
  }
  // ---- this lane's LDS read addresses in slot 0 of each ring
  const uint32_t ring_base = lds_addr(ring) + lane * 16;
  uint32_t xa[PPW];
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    const uint32_t q = lane >> 3, p = wave * PPW + i;
    xa[i] = ring_base + (inpl ? q * ROW_BYTES + ((8 * (p ^ (q & 1u)) + (lane & 7u)) * 16) - lane * 16
                              : (wave * PPW + i) * ROW_BYTES);
  }
  const uint32_t ca = ring_base, ce = lds_addr(ring) + COEF_ROWC_U4 * 16 + lane * 8;  // (+ XBYTES: an immediate)
  auto mac_call = [&](const CoefCall& cv, const uint4* xv) {
    limbs26 ck, dk;
    coef_call_limbs(cv, ck, dk);
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      const f128 x = u4_to_f(xv[i]);
      const limbs26 xl = to_limbs26(x);
      wacc_mac(ae[i], xl, dk);
      wacc_mac(ao[i], xl, ck);
      if (HIST) acc_add128(sx, x);
    }
  };
  auto normalize = [&]() {  // <= 5 * 512 limb products (< 2^52) per column
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      wacc_normalize(ae[i]);
      wacc_normalize(ao[i]);
    }
  };
  uint32_t k = 1;
  // ---- whole blocks of D calls k..k+3 (k = 1 mod D) that issue only calls before the last one
  // (k + 2 D - 2 < C): no range check, and every slot and wait is a constant. PH: (k - 1) / D mod DC, the
  // coefficient ring's phase.
  {
    auto step = [&](auto uc, auto phc) {
      constexpr uint32_t U = decltype(uc)::value, PH = decltype(phc)::value;
      wait_vmcnt<2 * PPW + 1>();
      __builtin_amdgcn_s_barrier();
      issue_c(cp, (PH + U + DC - 1) % DC);
      issue_x(xp, (U + D - 1) % D);
      cp += CSLOT;
      step_x();
      if (g < NG) {
        CoefCall cv;
        uint4 xv[PPW];
        lds_read_call<XBYTES + ((PH + U) % DC) * CSLOT, U * XSLOT>(ca, ce, xa[0], xa[1], cv, xv[0], xv[1]);
        mac_call(cv, xv);
      }
    };
    auto block = [&](auto phc) {
      step(std::integral_constant<uint32_t, 0>{}, phc);
      step(std::integral_constant<uint32_t, 1>{}, phc);
      step(std::integral_constant<uint32_t, 2>{}, phc);
      step(std::integral_constant<uint32_t, 3>{}, phc);
      k += D;
      if (((k - 1) & 511u) == 0 && g < NG) normalize();  // after call 512, 1024, ...
    };
    // such blocks: 1 + D j + 2 D - 2 < C; they run three at a time (one loop exit: with one per block the
    // register allocation spilled at every exit edge)
    const uint32_t nblocks = C > 2 * D - 1 ? (C - (2 * D - 1) + D - 1) / D : 0;
#pragma unroll 1
    for (uint32_t t = nblocks / DC; t > 0; t--) {
      block(std::integral_constant<uint32_t, 0>{});
      block(std::integral_constant<uint32_t, 1>{});
      block(std::integral_constant<uint32_t, 2>{});
    }
  }
  // ---- the remaining calls
#pragma unroll 1
  for (; k <= C; k++) {
    if (k + 2 > C)  // near the end fewer calls are in flight: wait for all
      wait_vmcnt<0>();
    else
      wait_vmcnt<2 * PPW + 1>();
    __builtin_amdgcn_s_barrier();
    if (k + DC - 1 <= C) issue_c_k(k + DC - 1);
    if (k + D - 1 <= C) issue_x_k(k + D - 1);
    if (g < NG) {
      const uint32_t co = ((k - 1) % DC) * CSLOT, xo = ((k - 1) % D) * XSLOT;
      CoefCall cv;
      uint4 xv[PPW];
      lds_read_call<XBYTES, 0>(ca + co, ce + co, xa[0] + xo, xa[1] + xo, cv, xv[0], xv[1]);
      mac_call(cv, xv);
      if ((k & 511u) == 0) normalize();
    }
  }
  if (g >= NG) return;
  if constexpr (RING_ONLY) {
    uint64_t h = 0;
#pragma unroll
    for (int i = 0; i < PPW; i++)
#pragma unroll
      for (int q = 0; q < 9; q++) h ^= ae[i].col[q] ^ ao[i].col[q];
    b.part[((blk * c.ngt + g) * 4) * IL + lane] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), 0, 0);
    return;
  }
  psum_part_finish<PPW, HIST, LEADER>(c, b, blk, g, lane, C, ae, ao, sx);
}

template <bool HIST, bool LEADER>
__global__ __launch_bounds__(256) void flp_psum_final_kernel(Cfg c, Bufs b) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const uint64_t blk = r / 64;
  const uint32_t lane = r % 64, NG = c.ngroups, A = 2 * c.chunk;
  f128 P = make128(0, 0), V = make128(0, 0), G = make128(0, 0), SX = make128(0, 0);
  const uint4* pp = b.part + (blk * c.ngt * 4) * IL + lane;
  for (uint32_t g = 0; g < NG; g++, pp += 4 * IL) {
    P = add128(P, u4_to_f(pp[0]));
    V = add128(V, u4_to_f(pp[IL]));
    G = add128(G, u4_to_f(pp[2 * IL]));
    if (HIST) SX = add128(SX, u4_to_f(pp[3 * IL]));
  }
  f128 vh = V;
  if (HIST) {
    // v = jr1 * range_check + jr1^2 * (sum(x) - 1/2)
    const f128 r2R = ld_il(b.coef, blk, c.ncoef, COEF_R2, lane);
    const f128 half = u4_to_f(b.consts[c.c_misc + 1]);
    f128 sc = sub128(SX, half);
    vh = add128(mont128(V, r2R), mont128(sc, mont128(r2R, r2R)));
  }
  const uint32_t flags = b.flags[r];
  if (LEADER) {  // verifier share [v, wires(t)..., G(t)]; wires were written by the part kernel
    uint4* o = reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r);
    o[0] = f_to_u4(vh);
    o[A + 1] = f_to_u4(G);
    b.verdicts[r] = (flags & (FLAG_INIT_FAIL | FLAG_INPUT_FAIL)) ? 1 : 0;
    return;
  }
  bool df = (flags & FLAG_DFAIL) != 0;
  f128 lv = ld_lead(b, c, r, 0, df), lg = ld_lead(b, c, r, A + 1, df);
  uint32_t verdict = 0;
  if (flags & FLAG_INIT_FAIL)
    verdict = 1;
  else if (df)
    verdict = 2;
  else {
    f128 V0 = add128(vh, lv), VG = add128(G, lg);
    if (!is_zero128(V0) || !eq128(P, mont128(VG, make128(1, 0))))
      verdict = 3;
    else if (flags & FLAG_NEXT_FAIL)
      verdict = 4;
  }
  b.verdicts[r] = (uint8_t)verdict;
}

// Prio3FixedPointBoundedL2VecSum, gadget 1: ParallelSum(PolyEval(p), chunk1) over the decoded entries
// y (= the output share, already truncated by K1), p(y) = 2^(2n-2) - 2^n y + y^2. One wave per
// (64-report block, group of PPW slots). Wire j at t1 is the barycentric sum
//   W_j = L1 (c'_0 s_j + sum_k c'_k y_{(k-1) chunk1 + j} + [short last chunk] c'_last 2^(n-2)),
// the padding value 2^(n-2) being the share of the encoded 0.0 (2^(n-1) / num_shares). The group
// also writes its share of v's gadget-1 part (sum_m g_m S1_m) and of G1(t1), and (helper) the sum of
// p(V_j) over its slots, V_j = own + leader wire, in the R^-1 domain of the decide compare.
template <int PPW, bool LEADER>
__global__ __launch_bounds__(64, 4) void flp_norm_part_kernel(Cfg c, Bufs b) {
  const uint32_t NG = c.ngroups1;
  const uint32_t bid = blockIdx.x;
  const uint32_t xcd = bid & 7u, q = bid >> 3;
  const uint32_t g = q % NG;
  const uint64_t blk = (uint64_t)(q / NG) * 8 + xcd;
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint32_t NC = c.ncoef, C = c.calls1, ch = c.chunk1, E = c.out_len, B = c.coef1;
  const uint32_t j0 = g * PPW;
  const uint4* coefb = b.coef + il_idx(blk, NC, 0, lane);
  const uint4* outb = b.outs + il_idx(blk, E, 0, lane);
  wacc26 ao[PPW];
#pragma unroll
  for (int i = 0; i < PPW; i++) wacc_zero(ao[i]);
#pragma unroll 1
  for (uint32_t k = 1; k <= C; k++) {
    const limbs26 ck = to_limbs26(u4_to_f(coefb[(B + G1_K + k - 1) * IL]));
    const uint32_t nb = (k - 1) * ch + j0;
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      if (j0 + i < ch && nb + i < E) wacc_mac(ao[i], to_limbs26(u4_to_f(outb[(uint64_t)(nb + i) * IL])), ck);
    }
    if ((k & 511u) == 0) {
#pragma unroll
      for (int i = 0; i < PPW; i++) wacc_normalize(ao[i]);
    }
  }
  const uint4* misc = b.consts + c.c_misc;
  const f128 LR = u4_to_f(coefb[(B + G1_L) * IL]), c0R = u4_to_f(coefb[(B + G1_C0) * IL]);
  const f128 tR = u4_to_f(coefb[(B + G1_T) * IL]);
  const f128 cl = u4_to_f(coefb[(B + G1_K + C - 1) * IL]);  // c'_calls1 (the possibly short last call)
  const f128 pad = mont128(u4_to_f(misc[6]), cl);          // 2^(n-2) c'_last, canonical
  const f128 twon = u4_to_f(misc[4]), K = u4_to_f(misc[5]);
  const uint32_t A0 = 2 * c.chunk;  // gadget 0's arity: gadget 1's wires follow it in the verifier
  bool dfail = false;
  f128 prod = make128(0, 0);
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    const uint32_t j = j0 + i;
    if (j < ch) {
      const f128 s = ld_il(b.proof, blk, c.proof_len, c.proof1_off + j, lane);
      f128 O = mont128(wacc_reduce(ao[i]), make128(1, 0));  // sum_k c'_k y (canonical)
      if ((C - 1) * ch + j >= E) O = add128(O, pad);
      const f128 W = mont128(add128(mont128(s, c0R), O), LR);
      if (LEADER) {
        if (r0 < b.n) reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r)[A0 + 2 + j] = f_to_u4(W);
      } else {
        const f128 V = add128(W, ld_lead(b, c, r, A0 + 2 + j, dfail));
        // p(V) R^-1 = V^2 R^-1 - 2^n V R^-1 + 2^(2n-2) R^-1
        prod = add128(prod, add128(sub128(mont128(V, V), mont128(V, twon)), K));
      }
    }
  }
  const uint32_t GL = c.gpoly1_len;
  const uint32_t per = (GL + NG - 1) / NG;
  const uint32_t m0 = g * per, m1 = min(GL, m0 + per);
  const uint4* Sm = b.consts + c.c_S1;
  const uint32_t goff = c.proof1_off + ch;
  f128 vpart = make128(0, 0), gpart = make128(0, 0);
  if (m0 < m1) {
    for (uint32_t m = m1; m-- > m0;) {
      f128 gm = ld_il(b.proof, blk, c.proof_len, goff + m, lane);
      vpart = add128(vpart, mont128(gm, u4_to_f(Sm[m])));
      gpart = add128(mont128(gpart, tR), gm);
    }
    gpart = mont128(gpart, mpow(tR, m0));
  }
  uint4* pp = b.part + ((blk * c.ngt + c.ngroups + g) * 4) * IL + lane;
  pp[0] = f_to_u4(prod);
  pp[IL] = f_to_u4(vpart);
  pp[2 * IL] = f_to_u4(gpart);
  if (dfail && r0 < b.n) atomicOr(&b.flags[r0], FLAG_DFAIL);
}

// FixedPoint decide: v = jr1 * range_check + jr1^2 * (computed_norm - claimed_norm) where range_check
// = sum_m g0_m S0_m and computed_norm = sum_m g1_m S1_m (the circuit's gadget outputs, as shares) and
// claimed_norm = sum_b 2^b x[entries*n + b]; then both gadgets' G(wires(t_g)) == gadget_poly_g(t_g).
template <bool LEADER>
__global__ __launch_bounds__(256) void flp_fp_final_kernel(Cfg c, Bufs b) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const uint64_t blk = r / 64;
  const uint32_t lane = r % 64, NG0 = c.ngroups, NG1 = c.ngroups1, A0 = 2 * c.chunk, A1 = c.chunk1;
  f128 P0 = make128(0, 0), V0 = P0, G0 = P0, P1 = P0, V1 = P0, G1 = P0;
  const uint4* pp = b.part + (blk * c.ngt * 4) * IL + lane;
  for (uint32_t g = 0; g < NG0; g++, pp += 4 * IL) {
    P0 = add128(P0, u4_to_f(pp[0]));
    V0 = add128(V0, u4_to_f(pp[IL]));
    G0 = add128(G0, u4_to_f(pp[2 * IL]));
  }
  for (uint32_t g = 0; g < NG1; g++, pp += 4 * IL) {
    P1 = add128(P1, u4_to_f(pp[0]));
    V1 = add128(V1, u4_to_f(pp[IL]));
    G1 = add128(G1, u4_to_f(pp[2 * IL]));
  }
  // claimed squared norm: the trailing norm_bits measurement elements, LE bits
  acc192 cn;
  acc_zero(cn);
  const uint32_t nb0 = c.trunc_len;
  const MeasView mv = meas_view(c, b, blk, lane);
  for (uint32_t i = 0; i < c.norm_bits; i++) trunc_add(cn, u4_to_f(mv[nb0 + i]), i);
  const f128 claimed = acc_reduce(cn);
  const f128 r2R = ld_il(b.coef, blk, c.ncoef, COEF_R2, lane);
  const f128 vh = add128(mont128(V0, r2R), mont128(sub128(V1, claimed), mont128(r2R, r2R)));
  const uint32_t flags = b.flags[r];
  if (LEADER) {
    uint4* o = reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r);
    o[0] = f_to_u4(vh);
    o[A0 + 1] = f_to_u4(G0);
    o[A0 + 2 + A1] = f_to_u4(G1);
    b.verdicts[r] = (flags & (FLAG_INIT_FAIL | FLAG_INPUT_FAIL)) ? 1 : 0;
    return;
  }
  bool df = (flags & FLAG_DFAIL) != 0;
  const f128 lv = ld_lead(b, c, r, 0, df), lg0 = ld_lead(b, c, r, A0 + 1, df), lg1 = ld_lead(b, c, r, A0 + 2 + A1, df);
  uint32_t verdict = 0;
  if (flags & FLAG_INIT_FAIL)
    verdict = 1;
  else if (df)
    verdict = 2;
  else {
    const f128 one = make128(1, 0);
    if (!is_zero128(add128(vh, lv)) || !eq128(P0, mont128(add128(G0, lg0), one)) ||
        !eq128(P1, mont128(add128(G1, lg1), one)))
      verdict = 3;
    else if (flags & FLAG_NEXT_FAIL)
      verdict = 4;
  }
  b.verdicts[r] = (uint8_t)verdict;
}

// ---------------------------------------------------------------------------- leader prepare_next
// leader_continued on PingPongMessage::Finish{prep_msg} (aggregation_job_driver.rs:588-602):
// prio prepare_next fails unless prep_msg equals the corrected joint-rand seed of the state.
// peer (nullable): the helper's verdicts; a report the helper rejected (PrepareStepResult::Reject)
// fails on the leader too (helper_step_failure, aggregation_job_driver.rs:646-660).
__global__ __launch_bounds__(256) void leader_finish_kernel(Cfg c, Bufs b, const uint8_t* prep_msgs,
                                                            const uint8_t* peer) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  if (b.verdicts[r] != 0) return;
  if (peer && peer[r] != 0) {
    b.verdicts[r] = 5;  // JX_HELPER_STEP_FAILURE
    return;
  }
  if (c.jr_len == 0) return;
  for (uint32_t o = 0; o < c.seed; o += 16) {
    const uint4 m = *reinterpret_cast<const uint4*>(prep_msgs + c.seed * r + o);
    const uint4 k = *reinterpret_cast<const uint4*>(b.msgs + c.seed * r + o);
    if (m.x != k.x || m.y != k.y || m.z != k.z || m.w != k.w) b.verdicts[r] = 4;
  }
}

// ---------------------------------------------------------------------------- launchers

hipError_t launch_leader_finish(const Cfg& c, const Bufs& b, const uint8_t* prep_msgs, const uint8_t* peer,
                                hipStream_t s) {
  hipLaunchKernelGGL(leader_finish_kernel, dim3((uint32_t)((b.n + 255) / 256)), dim3(256), 0, s, c, b, prep_msgs,
                     peer);
  return hipGetLastError();
}

// Slots per FLP group. Each slot holds two 9-column wide accumulators (36 VGPRs); PPW = 2
// (152 VGPRs, 3 waves/SIMD) measured fastest on MI355X for SumVec(8x1000/88): K3 11.8 ms vs
// 13.6 (PPW 1) and 12.5 (PPW 4, spills) per 312,500 reports. PPW = 1 only when it wastes
// fewer padded slot-lanes (chunk_length 1). (4 and 8 slots per wave spill, 0.3-4 KB/lane: removed.)
int psum_ppw(uint32_t chunk) {
  const int cands[] = {2, 1};
  int best = 2, best_cost = 1 << 30;
  for (int p : cands) {
    int ng = (int)((chunk + p - 1) / p);
    int cost = ng * p + 3 * ng;
    if (cost < best_cost) {
      best = p;
      best_cost = cost;
    }
  }
  return best;
}

// K3 phase 1: the LDS-DMA rings (measurement rows four calls deep, coefficient limb rows three; K3W slot
// groups per workgroup) for PPW = 2; the per-wave register-prefetch kernel for PPW = 1 (chunk_length 1).
// Measured and removed: 2 / 3 calls of register prefetch, 3-waves/SIMD builds, a ring
// with the measurement rows three deep as well, 8 groups per workgroup.
template <int PPW, bool HIST, bool LEADER>
static void launch_psum_part(const Cfg& c, const Bufs& b, hipStream_t s, uint32_t grid) {
  if constexpr (PPW == 2) {
    const uint32_t g2 = grid / c.ngroups * ((c.ngroups + K3W - 1) / K3W);
    hipLaunchKernelGGL((flp_psum_part_glds_kernel<PPW, HIST, LEADER, 4>), dim3(g2), dim3(64 * K3W), 0, s, c, b);
  } else {
    hipLaunchKernelGGL((flp_psum_part_kernel<PPW, HIST, LEADER>), dim3(grid), dim3(64), 0, s, c, b);
  }
}
template <int PPW, bool HIST, bool LEADER>
static void launch_psum_r(const Cfg& c, const Bufs& b, hipStream_t s) {
  const uint32_t nb = nblk_of(b.n);
  launch_psum_part<PPW, HIST, LEADER>(c, b, s, ((nb + 7) / 8) * 8 * c.ngroups);
  hipLaunchKernelGGL((flp_psum_final_kernel<HIST, LEADER>), dim3((uint32_t)((b.n + 255) / 256)), dim3(256), 0, s,
                     c, b);
}
template <int PPW>
static hipError_t launch_psum_t(const Cfg& c, const Bufs& b, hipStream_t s) {
  const bool hist = c.algo == ALGO_HISTOGRAM;
  if (hist && b.leader)
    launch_psum_r<PPW, true, true>(c, b, s);
  else if (hist)
    launch_psum_r<PPW, true, false>(c, b, s);
  else if (b.leader)
    launch_psum_r<PPW, false, true>(c, b, s);
  else
    launch_psum_r<PPW, false, false>(c, b, s);
  return hipGetLastError();
}

template <int PPW, bool LEADER>
static void launch_fp_r(const Cfg& c, const Bufs& b, hipStream_t s) {
  const uint32_t nb = nblk_of(b.n);
  launch_psum_part<PPW, false, LEADER>(c, b, s, ((nb + 7) / 8) * 8 * c.ngroups);
  hipLaunchKernelGGL((flp_norm_part_kernel<2, LEADER>), dim3(((nb + 7) / 8) * 8 * c.ngroups1), dim3(64), 0, s, c,
                     b);
  hipLaunchKernelGGL((flp_fp_final_kernel<LEADER>), dim3((uint32_t)((b.n + 255) / 256)), dim3(256), 0, s, c, b);
}

hipError_t launch_flp(const Cfg& c, const Bufs& b, hipStream_t s) {
  if (c.algo == ALGO_FIXEDPOINT_L2) {
    // chunk = isqrt(meas_len) >= 6 here, so psum_ppw never picks the one-slot kernel for this instance
    if (c.ppw != 2) return hipErrorInvalidValue;
    if (b.leader)
      launch_fp_r<2, true>(c, b, s);
    else
      launch_fp_r<2, false>(c, b, s);
    return hipGetLastError();
  }
  if (c.algo == ALGO_SUM) {
    uint32_t nb = nblk_of(b.n);
    if (b.leader)
      hipLaunchKernelGGL(flp_sum_kernel<true>, dim3((nb + 3) / 4), dim3(256), 0, s, c, b);
    else
      hipLaunchKernelGGL(flp_sum_kernel<false>, dim3((nb + 3) / 4), dim3(256), 0, s, c, b);
    return hipGetLastError();
  }
  switch (c.ppw) {
    case 2:
      return launch_psum_t<2>(c, b, s);
    case 1:
      return launch_psum_t<1>(c, b, s);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace jx
