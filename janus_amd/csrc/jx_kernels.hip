// jx_kernels.hip — gfx950 kernels for batched Prio3 helper preparation + aggregation.
//
// The per-report work Janus does at aggregator/src/aggregator.rs:1945-1967
// (prio 0.16.1 ping-pong helper_initialized + evaluate) is split into three
// launches over a batch of reports:
//
//   K1 xof_kernel      one report per lane. TurboSHAKE128 expansion of the helper
//                      measurement share (fused with the joint_rand_part absorb of the
//                      same bytes) and proof share; joint_rand_seed, joint_rands,
//                      query_rands, the prepare-message seed; per-report FLP
//                      coefficients (barycentric weights, batch-inverted).
//   K3 flp_*_kernel    FLP query on the helper share + add the leader's verifier
//                      share + decide + prepare_next check -> verdict byte.
//   K4 accumulate      masked/segmented field sum of output shares (+count, +checksum),
//                      i.e. BatchAggregation::merged_with (models.rs:1275-1330).
//
// Prio3Count (Field64, 3 permutations) runs as one lane-per-report kernel.
//
// This unit holds K0 (Count) and K1; K3 is in jx_flp.hip and K4 with what follows it in jx_accumulate.hip, so that
// the three compile side by side. What they share: the field helpers of jx_field.h and the staging layout of
// jx_kernels.h.
// Algorithm: draft-irtf-cfrg-vdaf-08 as implemented by prio 0.16.1; see DESIGN.md.
#include <cstdlib>
#include <stdlib.h>

#include <type_traits>

#include "jx_field.h"
#include "jx_kernels.h"
#include "jx_keccak.h"
#include "jx_sample.h"
#include "jx_sha256.h"

namespace jx {

// ---------------------------------------------------------------------------- Field64 helpers (Count)

__device__ uint64_t pow64(uint64_t a, uint64_t e) {
  uint64_t r = 1;
  while (e) {
    if (e & 1) r = mul64(r, a);
    a = mul64(a, a);
    e >>= 1;
  }
  return r;
}

// ---------------------------------------------------------------------------- K0: Prio3Count

// LEADER: prepare_init with agg_id 0 on the explicit leader input share (meas || proofs, Field64);
// writes the leader's verifier share [v, W0, W1, G] as its prep share.
template <bool LEADER>
__global__ __launch_bounds__(256) void count_kernel(Cfg c, Bufs b) {
  const uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nblk = (b.n + 63) / 64;
  if (r0 >= nblk * 64) return;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint64_t blk = r0 / 64;
  const uint32_t lane = r0 % 64;
  uint32_t nonce[4], kmeas[4], kproof[4], S[50];
  load16(b.nonces + 16 * r, nonce);
  uint64_t x[1], proof[5], t[1];
  bool bad = false;
  if (LEADER) {
    const uint2* ls = reinterpret_cast<const uint2*>(b.lis + b.lis_rs * r);
    uint2 q = ls[0];
    x[0] = (uint64_t)q.x | ((uint64_t)q.y << 32);
    bad |= x[0] >= P64;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      q = ls[1 + i];
      proof[i] = (uint64_t)q.x | ((uint64_t)q.y << 32);
      bad |= proof[i] >= P64;
    }
  } else {
  load16(b.his + (uint64_t)c.his_bytes * r, kmeas);
  load16(b.his + (uint64_t)c.his_bytes * r + 16, kproof);
  {  // helper_meas_share: XOF(k_meas, DST(usage 1), [agg_id=1])
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, ALGO_COUNT, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock(S, m);
    sample64<1>(S, x);
  }
  {  // helper_proofs_share: XOF(k_proofs, DST(usage 2), [PROOFS=1, agg_id=1])
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, ALGO_COUNT, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    sponge_oneblock(S, m);
    sample64<5>(S, proof);
  }
  }
  {  // query_rands: XOF(verify_key, DST(usage 5), [PROOFS=1] || nonce)
    Block m;
    blk_zero(m);
    uint32_t vk[4];
    load_vk(c, b, r, vk);
    int pos = blk_xof_prefix(m, ALGO_COUNT, 5, vk);
    blk_put_byte(m, pos, 1);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 1 + 4 * i, nonce[i]);
    blk_pad(m, pos + 17);
    sponge_oneblock(S, m);
    sample64<1>(S, t);
  }
  // FLP query, gadget Mul (arity 2), 1 call, P = 2, alpha = -1
  const uint64_t one = 1, minus1 = P64 - 1;
  uint64_t tt = t[0];
  uint64_t t2 = mul64(tt, tt);
  uint32_t verdict = 0;
  if (t2 == one) verdict = 1;  // prepare_init_failure
  uint64_t dm = sub64(tt, one), dp = add64(tt, one);
  uint64_t inv = pow64(mul64(dm, dp), P64 - 2);
  uint64_t c0 = mul64(inv, dp);                  // 1/(t-1)
  uint64_t c1 = mul64(minus1, mul64(inv, dm));   // -1/(t+1) = alpha^1/(t - alpha^1)
  uint64_t inv2 = (P64 + 1) / 2;
  uint64_t L = mul64(sub64(t2, one), inv2);
  uint64_t xm = x[0];
  uint64_t W0 = mul64(L, add64(mul64(c0, proof[0]), mul64(c1, xm)));
  uint64_t W1 = mul64(L, add64(mul64(c0, proof[1]), mul64(c1, xm)));
  // circuit: Mul(x,x) - x with the gadget replaced by gadget_poly(alpha^1) = g0 - g1 + g2
  uint64_t v = sub64(add64(sub64(proof[2], proof[3]), proof[4]), xm);
  uint64_t G = add64(proof[2], mul64(tt, add64(proof[3], mul64(tt, proof[4]))));
  if (LEADER) {
    if (r0 < b.n) {
      uint2* o = reinterpret_cast<uint2*>(b.lps_out + (uint64_t)c.lps_bytes * r);
      o[0] = make_uint2(lo32(v), hi32(v));
      o[1] = make_uint2(lo32(W0), hi32(W0));
      o[2] = make_uint2(lo32(W1), hi32(W1));
      o[3] = make_uint2(lo32(G), hi32(G));
      b.verdicts[r0] = (uint8_t)((verdict || bad) ? 1 : 0);
    }
    b.outs[il_idx(blk, 1, 0, lane)] = make_uint4(lo32(xm), hi32(xm), 0, 0);
    return;
  }
  // leader verifier share: [v, W0, W1, G] as 4 x 8-byte LE
  const uint8_t* lp = b.lps + (uint64_t)c.lps_bytes * r;
  uint64_t lv[4];
  bool dfail = false;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint2 q = *reinterpret_cast<const uint2*>(lp + 8 * i);
    lv[i] = (uint64_t)q.x | ((uint64_t)q.y << 32);
    dfail |= lv[i] >= P64;
  }
  if (verdict == 0 && dfail) verdict = 2;
  if (verdict == 0) {
    uint64_t V0 = add64(v, lv[0]), V1 = add64(W0, lv[1]), V2 = add64(W1, lv[2]), VG = add64(G, lv[3]);
    if (V0 != 0 || mul64(V1, V2) != VG) verdict = 3;
  }
  if (r0 < b.n) b.verdicts[r0] = (uint8_t)verdict;
  b.outs[il_idx(blk, 1, 0, lane)] = make_uint4(lo32(xm), hi32(xm), 0, 0);
}

// ---------------------------------------------------------------------------- K1: XOF stage (Field128)

struct Trunc {
  acc192 a;
  uint32_t j, i;
};

// (opaque_u32, TruncW, truncw_zero / truncw_mac / truncw_value and shl32_mod: the output-share truncation's word
// columns, in the device section of jx_kernels.h, where the device tests reach them)

// one measurement element at static stream position e (fast path: no rejections)
// WIDE (bits in (32, 64], Sum / SumVec): the word columns of bits 0..31 are folded into `lo` at
// bit 32 and restart for the bits 32.. (weights 2^(j-32) < 2^32); out = lo + 2^32 * high.
template <bool WIDE, bool STORE = true>
__device__ __forceinline__ void emit_meas(const Cfg& c, uint4* mp, uint4* op, uint32_t e, uint4 v, uint32_t& gmax,
                                          TruncW& tr, f128& lo) {
  // e is uniform. Straight-line except for the store guard and the once-per-output-element finish:
  // elements past the share (last block) or not truncated (Histogram; FixedPoint's trailing norm
  // bits) add with weight 0 instead of branching around the column sums.
  const bool in = e < c.meas_len;
  if (STORE && in) mp[(uint64_t)e * IL] = v;
  gmax = max(gmax, in ? ge_screen(v) : 0u);
  const bool tin = !c.out_is_meas && e < c.trunc_len;
  const uint32_t sh = opaque_u32(tin ? 1u << (WIDE ? (tr.j & 31u) : tr.j) : 0u);
  truncw_mac(tr, v, sh);
  tr.j += tin ? 1u : 0u;
  if (WIDE && tin && tr.j == 32 && c.bits > 32) {
    lo = truncw_value(tr);
    truncw_zero(tr);
  }
  if (tin && tr.j == c.bits) {
    f128 val = truncw_value(tr);
    if (WIDE && c.bits > 32) val = add128(lo, shl32_mod(val));
    op[(uint64_t)tr.i * IL] = f_to_u4(val);
    truncw_zero(tr);
    tr.j = 0;
    tr.i++;
  }
}
__device__ __forceinline__ void emit_proof(const Cfg& c, uint4* pp, uint32_t e, uint4 v, uint32_t& gmax) {
  if (e >= c.proof_len) return;
  gmax = max(gmax, ge_screen(v));
  pp[(uint64_t)e * IL] = v;
}

// Barycentric weights of one gadget on the P-th roots of unity w^k (Montgomery form):
//   c_k = w^k / (t - w^k) for k = 1..C at slot sk + (k-1), c_0 = 1/(t - 1) at slot s0,
// by one batch inversion (prefix products parked in the c_k slots, then one inversion chain).
// With with_d (ParallelSum gadget 0, sk = COEF_K; rcR = r^chunk R): also d_k = c_k rc^(k-1), rc = r^chunk,
// in the same backward pass: rc joins the inverted product, so 1/rc costs two products, and the powers
// descend from rc^(C-1). The pair (c_k, d_k) is stored as its 26-bit limbs in call k's 40-byte region
// (jx_kernels.h, st_coef_call), whose row A parks the prefix product until then. The backward pass keeps
// four prefix-product loads in flight (a prefix in slot k-1 is overwritten only at step k-1, after its
// read). Returns sum_{k>=1} c_k.
__device__ f128 bary_coeffs(uint4* coef, uint64_t blk, uint32_t NC, uint32_t lane, f128 tR, const uint4* omega,
                            uint32_t C, uint32_t s0, uint32_t sk, bool with_d = false, f128 rcR = f128{0, 0}) {
  // where step k parks its prefix product (uint4 index into coef)
  auto slot = [&](uint32_t k) -> uint64_t {
    if (k == 0) return il_idx(blk, NC, s0, lane);
    return with_d ? il_idx(blk, NC, sk, lane) + (uint64_t)(k - 1) * COEF_CALL_U4 : il_idx(blk, NC, sk + (k - 1), lane);
  };
  g_uint4* gco = (g_uint4*)coef;
  const g_uint4* gom = (const g_uint4*)omega;
  f128 acc = sub128(tR, u4_to_f(gom[0]));
  gco[slot(0)] = f_to_u4(acc);
  for (uint32_t k = 1; k <= C; k++) {
    acc = mont128(acc, sub128(tR, u4_to_f(gom[k])));
    gco[slot(k)] = f_to_u4(acc);
  }
  f128 inv, rp = make128(R1_128_LO, R1_128_HI), rinv = rp;
  if (with_d) {
    const f128 ie = minv(mont128(acc, rcR));  // 1 / (prefix * rc)
    inv = mont128(ie, rcR);                     // 1 / prefix
    rinv = mont128(ie, acc);                    // 1 / rc
    rp = mpow(rcR, C - 1);                      // rc^(C-1)
  } else {
    inv = minv(acc);
  }
  f128 sumc = make128(0, 0);
  // step k needs the prefix of slot k-1 and w^k: both loaded four steps ahead (vmcnt counts in order, so a
  // load issued just before its use would also wait for every prefetch)
  auto pref = [&](int k) { return k >= 1 ? u4_to_f(gco[slot((uint32_t)k - 1)]) : make128(0, 0); };
  auto wk = [&](int k) { return k >= 1 ? u4_to_f(gom[k]) : make128(0, 0); };
  const int Ci = (int)C;
  f128 q0 = pref(Ci), q1 = pref(Ci - 1), q2 = pref(Ci - 2), q3 = pref(Ci - 3);
  f128 o0 = wk(Ci), o1 = wk(Ci - 1), o2 = wk(Ci - 2), o3 = wk(Ci - 3);
  for (uint32_t k = C; k >= 1; k--) {
    const f128 pre = q0, w = o0;
    q0 = q1;
    q1 = q2;
    q2 = q3;
    o0 = o1;
    o1 = o2;
    o2 = o3;
    // unconditional loads (a clamped index past the end: the value is never used) keep the loop
    // branch-free, so the wait before the first use counts only the older loads
    const uint32_t kn = k > 4 ? k - 4 : 1;
    q3 = u4_to_f(gco[slot(kn - 1)]);
    o3 = u4_to_f(gom[kn]);
    f128 invden = mont128(inv, pre);
    inv = mont128(inv, sub128(tR, w));
    f128 ck = mont128(w, invden);
    if (with_d) {
      st_coef_call(coef + il_idx(blk, NC, 0, 0), lane, k, ck, mont128(ck, rp));
      rp = mont128(rp, rinv);
    } else {
      gco[slot(k)] = f_to_u4(ck);
    }
    sumc = add128(sumc, ck);
  }
  st_il(coef, blk, NC, s0, lane, inv);  // c_0 = 1/(t - 1)
  return sumc;
}

// Tail of the XOF stage shared by the fast and slow kernels: joint randomness,
// prepare-message seed, query randomness, FLP coefficients.
// part_h: the helper's joint_rand_part. Writes msgs / flags / coef.
// Returns flags (with FLAG_SLOW set if a rejected sample was hit and slow == false).
// INL: the barycentric coefficient chains are inlined instead of called (the lane-split kernel, whose
// registers have room for them: a call's frame and the registers saved around it cost it 80 B of scratch)
template <bool INL = false>
__device__ uint32_t xof_tail(const Cfg& c, const Bufs& b, uint64_t blk, uint32_t lane, uint64_t r, bool write_msg,
                             const uint32_t nonce[4], const uint32_t part_l[4], const uint32_t lead_part[4],
                             const uint32_t part_h[4], uint32_t flags, bool slow) {
  uint32_t S[50];
  const uint32_t zero[4] = {0, 0, 0, 0};
  // corrected joint-rand seed = XOF(0^16, DST(6), part_L || part_H)[0:16]
  uint32_t corr[4];
  {
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 6, zero);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 4 * i, part_l[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 16 + 4 * i, part_h[i]);
    blk_pad(m, pos + 32);
    sponge_oneblock(S, m);
#pragma unroll
    for (int i = 0; i < 4; i++) corr[i] = S[i];
  }
  // joint_rands = expand(corrected, DST(3), [PROOFS=1], JR_LEN)
  f128 jr[2];
  {
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 3, corr);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock(S, m);
    sample2_f128(S, jr, c.jr_len, slow, flags);
  }
  // prepare message = XOF(0^16, DST(6), leader's part || part_H); equals corr when the
  // leader's part matches the public share.
  bool same = part_l[0] == lead_part[0] && part_l[1] == lead_part[1] && part_l[2] == lead_part[2] &&
              part_l[3] == lead_part[3];
  uint32_t msg[4] = {corr[0], corr[1], corr[2], corr[3]};
  if (!same) {
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 6, zero);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 4 * i, lead_part[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 16 + 4 * i, part_h[i]);
    blk_pad(m, pos + 32);
    sponge_oneblock(S, m);
#pragma unroll
    for (int i = 0; i < 4; i++) msg[i] = S[i];
    if (msg[0] != corr[0] || msg[1] != corr[1] || msg[2] != corr[2] || msg[3] != corr[3]) flags |= FLAG_NEXT_FAIL;
  }
  if (write_msg) *reinterpret_cast<uint4*>(b.msgs + 16 * r) = make_uint4(msg[0], msg[1], msg[2], msg[3]);
  // query_rands = expand(verify_key, DST(5), [PROOFS=1] || nonce, QR_LEN): one t per gadget
  f128 tq[2];
  {
    Block m;
    blk_zero(m);
    uint32_t vk[4];
    load_vk(c, b, r, vk);
    int pos = blk_xof_prefix(m, c.dst_id, 5, vk);
    blk_put_byte(m, pos, 1);
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(m, pos + 1 + 4 * i, nonce[i]);
    blk_pad(m, pos + 17);
    sponge_oneblock(S, m);
    sample2_f128(S, tq, c.qr_len, slow, flags);
  }
  const f128 t = tq[0];
  // ---- FLP coefficients (Montgomery form). Barycentric weights on the P-th roots:
  //   wire_j(t) = L * sum_k c_k * wire_j[k],  c_k = w^k / (t - w^k),  L = (t^P - 1)/P
  const uint4* omega = b.consts + c.c_omega;
  const uint4* misc = b.consts + c.c_misc;
  const f128 R1 = make128(R1_128_LO, R1_128_HI);
  f128 tR = to_mont128(t);
  f128 tp = tR;
  for (uint32_t i = 0; i < c.logP; i++) tp = mont128(tp, tp);
  if (eq128(tp, R1)) flags |= FLAG_INIT_FAIL;
  f128 LR = mont128(sub128(tp, R1), u4_to_f(misc[0]));
  uint4* coef = b.coef;
  const uint32_t NC = c.ncoef;
  st_il(coef, blk, NC, COEF_L, lane, LR);
  st_il(coef, blk, NC, COEF_T, lane, tR);
  f128 rR = to_mont128(jr[0]);
  st_il(coef, blk, NC, COEF_R, lane, rR);
  st_il(coef, blk, NC, COEF_R2, lane, to_mont128(jr[1]));
  // batch inversion of den_k = t - w^k, k = 0..calls
  const uint32_t C = c.calls;
  const f128 rcR = mpow(rR, c.chunk);  // r^chunk (ParallelSum's d_k = c_k r^((k-1) chunk))
  f128 sumc;
  if constexpr (INL) {
    [[clang::always_inline]] sumc =
        bary_coeffs(coef, blk, NC, lane, tR, omega, C, COEF_C0, COEF_K, c.algo != ALGO_SUM, rcR);
  } else {
    sumc = bary_coeffs(coef, blk, NC, lane, tR, omega, C, COEF_C0, COEF_K, c.algo != ALGO_SUM, rcR);
  }
  if (c.algo == ALGO_SUM) {
    // (1/2) * sum c_k, canonical: mont(sumc*R, 1/2) = sumc/2
    st_il(coef, blk, NC, COEF_HALFSUM, lane, mont128(sumc, u4_to_f(misc[1])));
  } else {
    // the ParallelSum group finish (psum_group_finish) takes its constants scaled by L, so a wire at t costs
    // two products instead of three: COEF_C0 <- c_0 L R, COEF_L <- L canonical, COEF_HALFSUM <- L (sum c_k)/2
    // canonical; below, its power table holds L r^(j+1) (the chain starts from L r: mont(L R, r) = L r)
    const f128 c0R = ld_il(coef, blk, NC, COEF_C0, lane);
    st_il(coef, blk, NC, COEF_C0, lane, mont128(c0R, LR));
    st_il(coef, blk, NC, COEF_L, lane, mont128(LR, make128(1, 0)));
    st_il(coef, blk, NC, COEF_HALFSUM, lane, mont128(mont128(sumc, LR), u4_to_f(misc[1])));
  }
  if (c.algo != ALGO_SUM) {
    // power tables of the ParallelSum group finish: L r^(j+1) canonical for the even wires of slot j (a chain
    // of mont products from L r), and t^(g * per) R for group g's share of G(t)
    f128 rj = mont128(LR, jr[0]);
    for (uint32_t j = 0; j < c.chunk; j++) {
      st_il(coef, blk, NC, c.c_rpow + j, lane, rj);
      rj = mont128(rj, rR);
    }
    const uint32_t per = (c.gpoly_len + c.ngroups - 1) / c.ngroups;
    const f128 tstep = mpow(tR, per);
    f128 tg = R1;
    for (uint32_t g = 0; g < c.ngroups; g++) {
      st_il(coef, blk, NC, c.c_tpow + g, lane, tg);
      tg = mont128(tg, tstep);
    }
  }
  if (c.algo == ALGO_FIXEDPOINT_L2) {
    // gadget 1 (the norm's ParallelSum(PolyEval)): its own query randomness t1 and P1-th roots
    const f128 t1R = to_mont128(tq[1]);
    f128 tp1 = t1R;
    for (uint32_t i = 0; i < c.logP1; i++) tp1 = mont128(tp1, tp1);
    if (eq128(tp1, R1)) flags |= FLAG_INIT_FAIL;
    const uint32_t B = c.coef1;
    st_il(coef, blk, NC, B + G1_L, lane, mont128(sub128(tp1, R1), u4_to_f(misc[7])));
    st_il(coef, blk, NC, B + G1_T, lane, t1R);
    if constexpr (INL) {
      [[clang::always_inline]] (void)bary_coeffs(coef, blk, NC, lane, t1R, b.consts + c.c_omega1, c.calls1, B + G1_C0,
                                                  B + G1_K);
    } else {
      (void)bary_coeffs(coef, blk, NC, lane, t1R, b.consts + c.c_omega1, c.calls1, B + G1_C0, B + G1_K);
    }
  }
  return flags;
}

// K1, helper (agg_id 1, aggregator.rs:1947), large launches: the measurement and proof shares are
// expanded from seeds by TurboSHAKE128 and the squeeze runs alongside the joint_rand_part absorb, one
// report per lane with both sponges in VGPRs (2 waves/SIMD). The leader (agg_id 0) has its own
// one-sponge kernel (xof_leader_kernel); launches under one fused wave per SIMD take the lane-split
// kernel (xof_lanes_kernel). Variants measured slower and removed: squeeze-only +
// absorb-only launches, sequential S/J permutations at 3 waves/SIMD.
constexpr uint32_t K1_WAVES = 4;  // waves (64-report blocks) per K1 workgroup
// PROBE (measurement variants, instantiated only by tools/kernel_probe.hip, never by the library):
// 1 = the measurement-share staging stores skipped at run time by a uniform branch the compiler cannot
// resolve (everything else as built), 2 = no per-block emission at all (stores, truncation, >= p screen),
// 3 = the stores without the truncation and the screen. The variants write a sink to flags so nothing is dead.
template <bool WIDE = false, int PROBE = 0>
__global__ __launch_bounds__(64 * K1_WAVES, 1) void xof_kernel(Cfg c, Bufs b) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6);
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;

  const uint8_t* hs = b.his + (uint64_t)c.his_bytes * r;
  uint32_t flags = 0;
  const uint32_t MB = c.meas_len * 16;
  const uint32_t ML = 42 + MB;
  const uint32_t NM = (MB + 167) / 168;  // measurement-share blocks of 168 bytes
  const uint32_t b_last = ML / 168;      // last absorbed block (b_last <= NM)

  // ---- measurement share fused with the joint_rand_part absorb --------------------
  // S: XOF(k_meas, DST(1), [1]) squeezed 168 bytes (block m of the measurement share) per block.
  // J: XOF(k_blind, DST(7), [agg_id] || nonce || enc(meas_share))   (absorbing those bytes)
  // J's message block m is meas bytes [168m - 42, 168m + 126): the 42-byte header makes it a
  // 16-bit funnel shift (v_alignbit_b32) of the words of blocks m-1 and m. After block m is
  // consumed S (-> block m+1) and J (absorb block m) permute together: two independent streams
  // (keccak_p12_x2).
  uint32_t S[50], J[50];
  {
    uint32_t kmeas[4];
    load16(hs, kmeas);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock(S, m);
  }
  uint32_t hdr[11];
  {
    uint32_t nonce[4], kblind[4];
    load16(b.nonces + 16 * r, nonce);
    load16(hs + 32, kblind);
    Block h;
    blk_zero(h);
    int pos = blk_xof_prefix(h, c.dst_id, 7, kblind);
    blk_put_byte(h, pos, 1);  // agg_id
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(h, pos + 1 + 4 * i, nonce[i]);
#pragma unroll
    for (int w = 0; w < 11; w++) hdr[w] = h.w[w];  // 42 header bytes
  }
  uint32_t prev[11];
  uint32_t carry0 = 0, carry1 = 0;
  uint32_t gmax = 0;  // running ge_screen over every sampled element
  TruncW tr;
  truncw_zero(tr);
  tr.j = 0;
  tr.i = 0;
  f128 trunc_lo = make128(0, 0);
  uint4* const mp = b.meas + il_idx(blk, c.meas_len, 0, lane);
  uint4* const op = b.outs + il_idx(blk, c.out_len, 0, lane);
  uint32_t sink = 0;
  auto emit = [&](uint32_t e, uint4 v) {
    if constexpr (PROBE == 1) {
      if (b.force_slow == 0x5EED5EEDu && e < c.meas_len) mp[(uint64_t)e * IL] = v;  // never true at run time
      emit_meas<WIDE, false>(c, mp, op, e, v, gmax, tr, trunc_lo);
    } else if constexpr (PROBE == 3) {
      if (e < c.meas_len) mp[(uint64_t)e * IL] = v;
    } else {
      emit_meas<WIDE>(c, mp, op, e, v, gmax, tr, trunc_lo);
    }
  };
  // emit the measurement elements of block m (10 or 11, by parity)
  auto emit_block = [&](uint32_t m) {
    if constexpr (PROBE == 2) {
      sink ^= S[0] ^ S[41];
      return;
    }
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit(e0 + ci, make_uint4(S[4 * ci], S[4 * ci + 1], S[4 * ci + 2], S[4 * ci + 3]));
      carry0 = S[40];
      carry1 = S[41];
    } else {
      const uint32_t c0 = carry0, c1 = carry1;
      emit(e0 + 10, make_uint4(c0, c1, S[0], S[1]));
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit(e0 + 11 + ci, make_uint4(S[2 + 4 * ci], S[3 + 4 * ci], S[4 + 4 * ci], S[5 + 4 * ci]));
    }
  };
  // J ^= message block m built from S (block m, if present) and prev (block m-1)
  auto absorb_block = [&](uint32_t m, bool have) {
    const uint32_t s0 = have ? S[0] : 0u;
    if (m == 0) {
#pragma unroll
      for (int w = 0; w < 10; w++) J[w] = hdr[w];
      J[10] = (hdr[10] & 0xffffu) | (s0 << 16);
#pragma unroll
      for (int w = 11; w < 50; w++) J[w] = 0;
    } else {
#pragma unroll
      for (int w = 0; w < 10; w++) J[w] ^= alignbit(prev[w + 1], prev[w], 16);
      J[10] ^= alignbit(s0, prev[10], 16);
    }
    if (have) {
#pragma unroll
      for (int w = 11; w < 42; w++) J[w] ^= alignbit(S[w - 10], S[w - 11], 16);
#pragma unroll
      for (int w = 0; w < 11; w++) prev[w] = S[31 + w];
    }
  };
  // last absorbed block m: only message bytes [168m, ML) are absorbed, then TurboSHAKE padding
  // (D = 0x01 after the message, 0x80 in byte 167)
  auto absorb_last = [&](uint32_t m, bool have) {
    const uint32_t nb = ML - 168 * m;  // message bytes in this block (< 168)
    uint32_t jw[42];
    const uint32_t s0 = have ? S[0] : 0u;
    if (m == 0) {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = hdr[w];
      jw[10] = (hdr[10] & 0xffffu) | (s0 << 16);
#pragma unroll
      for (int w = 0; w < 50; w++) J[w] = 0;
    } else {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = alignbit(prev[w + 1], prev[w], 16);
      jw[10] = alignbit(s0, prev[10], 16);
    }
#pragma unroll
    for (int w = 11; w < 42; w++) jw[w] = have ? alignbit(S[w - 10], S[w - 11], 16) : 0u;
#pragma unroll
    for (int w = 0; w < 42; w++) {
      const uint32_t lo_b = 4 * w;
      if (lo_b >= nb)
        jw[w] = 0;
      else if (lo_b + 4 > nb)
        jw[w] &= (1u << (8 * (nb - lo_b))) - 1u;
      if ((uint32_t)w == (nb >> 2)) jw[w] ^= 1u << (8 * (nb & 3));
    }
    jw[41] ^= 0x80000000u;
#pragma unroll
    for (int w = 0; w < 42; w++) J[w] ^= jw[w];
    keccak_p12(J);
  };
  // advance to block m+1: S squeezes together with J's permutation
  auto advance = [&](uint32_t m) {
    if (m + 1 < NM)
      keccak_p12_x2(S, J);
    else
      keccak_p12(J);
  };
  // blocks m = 0 .. b_last (b_last <= NM); blocks m < NM hold measurement bytes. Block 0 is
  // peeled so that the 42-byte header is dead inside the main loop.
  emit_block(0);
  if (b_last == 0) {
    absorb_last(0, true);
  } else {
    absorb_block(0, true);
    advance(0);
#pragma unroll 1
    for (uint32_t m = 1; m < b_last; m++) {  // m < b_last <= NM: block m holds measurement bytes
      emit_block(m);
      absorb_block(m, true);
      advance(m);
    }
    const bool have = b_last < NM;
    if (have) emit_block(b_last);
    absorb_last(b_last, have);
  }
  uint32_t own_part[4] = {J[0], J[1], J[2], J[3]};

  // ---- proof share: XOF(k_proofs, DST(2), [PROOFS=1, agg_id=1]) ----------------------
  uint4* const pp = b.proof + il_idx(blk, c.proof_len, 0, lane);
  {
    uint32_t kproof[4];
    load16(hs + 16, kproof);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    sponge_oneblock(S, m);
  }
  const uint32_t NP = (c.proof_len * 16 + 167) / 168;
#pragma unroll 1
  for (uint32_t m = 0; m < NP; m++) {
    if (m > 0) keccak_p12(S);
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit_proof(c, pp, e0 + ci, make_uint4(S[4 * ci], S[4 * ci + 1], S[4 * ci + 2], S[4 * ci + 3]), gmax);
      carry0 = S[40];
      carry1 = S[41];
    } else {
      emit_proof(c, pp, e0 + 10, make_uint4(carry0, carry1, S[0], S[1]), gmax);
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit_proof(c, pp, e0 + 11 + ci, make_uint4(S[2 + 4 * ci], S[3 + 4 * ci], S[4 + 4 * ci], S[5 + 4 * ci]), gmax);
    }
  }
  if (gmax == 0xFFFFFFFFu) flags |= FLAG_SLOW;

  uint32_t nonce[4];
  load16(b.nonces + 16 * r, nonce);
  uint32_t part_l[4], lead_part[4];
  load16(b.ps + (uint64_t)c.ps_bytes * r, part_l);
  load16(b.lps + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16, lead_part);
  flags = xof_tail(c, b, blk, lane, r, r0 < b.n, nonce, part_l, lead_part, own_part, flags, false);
  if constexpr (PROBE != 0) flags = (sink ^ gmax ^ (uint32_t)tr.T[0]) & ~FLAG_SLOW;
  if (b.force_slow) flags |= FLAG_SLOW;
  if (r0 < b.n) b.flags[r0] = flags;
}

// ---------------------------------------------------------------------------- K1, lane-split helper
// A wave holds 32 reports. Lanes 0..31 (the S half) run the measurement-share squeeze of report
// (lane & 31), lanes 32..63 (the J half) the joint_rand_part absorb of the same report: a lane
// carries ONE Keccak state (<= 128 VGPRs, 4 waves/SIMD, against 2 for the two-sponge fused kernel)
// and one keccak_p12 instruction stream advances both sponges. After each permutation the S half
// emits block m (stores, truncation, >= p screen) and forms J's message words of block m (the 16-bit
// funnel shift of blocks m-1 and m); v_permlane32_swap_b32 hands them to the J half,
// which XORs them into its state (the S half XORs the swap's zeros). The J half squeezes block 0
// itself (the same sponge) to build its first message block; after the measurement every lane runs
// the proof-share squeeze (emitted by the S half) and then the J half finishes the XOF tail.

// lanes 32..63 receive lanes 0..31's v; lanes 0..31 receive 0
__device__ __forceinline__ uint32_t lower_to_upper(uint32_t v) {
  const auto r = __builtin_amdgcn_permlane32_swap(0u, v, false, false);
  return r[0];
}

// Registers: the XOF tail is inlined (xof_tail<true>) and the kernel is built for two waves per SIMD, so
// nothing spills (no scratch); how many of its workgroups share a CU is capped at launch by dynamic LDS
// it does not use (K1Launch::lds, jx_engine_debug option 6), the placement the two-jobs shape wants
// (chain-latency-bound waves, at most two per SIMD).
template <bool WIDE>  // WIDE (bits > 32) carries 4 more truncation words
__global__ __launch_bounds__(64 * K1_WAVES, 2) void xof_lanes_kernel(Cfg c, Bufs b) {
  const uint32_t lane = threadIdx.x & 63;
  const bool jh = lane >= 32;
  const uint64_t gw = (uint64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6);  // 32 reports per wave
  const uint64_t blk = gw >> 1;
  const uint32_t il = ((uint32_t)gw & 1u) * 32u + (lane & 31u);  // this report's slot in its 64-report block
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint64_t r0 = blk * 64 + il;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint8_t* hs = b.his + (uint64_t)c.his_bytes * r;
  const uint32_t MB = c.meas_len * 16;
  const uint32_t ML = 42 + MB;
  const uint32_t NM = (MB + 167) / 168;
  const uint32_t b_last = ML / 168;

  uint32_t st[50];
  {  // squeeze block 0 = XOF(k_meas, DST(1), [1]) in both halves
    uint32_t kmeas[4];
    load16(hs, kmeas);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock(st, m);
  }
  uint32_t hdr[11];
  {
    uint32_t nonce[4], kblind[4];
    load16(b.nonces + 16 * r, nonce);
    load16(hs + 32, kblind);
    Block h;
    blk_zero(h);
    int pos = blk_xof_prefix(h, c.dst_id, 7, kblind);
    blk_put_byte(h, pos, 1);  // agg_id
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(h, pos + 1 + 4 * i, nonce[i]);
#pragma unroll
    for (int w = 0; w < 11; w++) hdr[w] = h.w[w];
  }
  // aux: the half-specific state carried across permutations, in the SAME registers for both halves.
  // S half: the truncation word columns T0..T3 (8 words), the element carry (2), the >= p screen
  // (1) [, WIDE: the low 32-bit truncation (4)]. J half: pv = the raw words 31..41 of the previous
  // squeezed block (the 16-bit funnel shift of J's message words 0..10 needs them).
  constexpr int NAUX = WIDE ? 15 : 11;
  uint32_t aux[NAUX];
#pragma unroll
  for (int w = 0; w < NAUX; w++) aux[w] = 0;
  uint4* const mp = b.meas + il_idx(blk, c.meas_len, 0, il);
  uint4* const op = b.outs + il_idx(blk, c.out_len, 0, il);
  // uniform truncation position (output element ti, bit tj) of the next measurement element
  uint32_t tj = 0, ti = 0;
  const uint32_t tlen = c.out_is_meas ? 0u : min(c.trunc_len, c.meas_len);
  // S half (call inside `if (!jh)`): store the elements of squeezed block m, screen them, and add
  // them into the truncation word columns; an output element is finished every `bits` elements
  auto s_emit_block = [&](uint32_t m) {
    TruncW tr;
#pragma unroll
    for (int w = 0; w < 4; w++) tr.T[w] = (uint64_t)aux[2 * w] | ((uint64_t)aux[2 * w + 1] << 32);
    tr.j = tj;
    tr.i = ti;
    uint32_t carry0 = aux[8], carry1 = aux[9], gmax = aux[10];
    f128 trunc_lo = make128(0, 0);
    if constexpr (WIDE) trunc_lo = make128((uint64_t)aux[11] | ((uint64_t)aux[12] << 32), (uint64_t)aux[13] | ((uint64_t)aux[14] << 32));
    auto emit = [&](uint32_t e, uint4 v) {
      if (e >= c.meas_len) return;
      gmax = max(gmax, ge_screen(v));
      mp[(uint64_t)e * IL] = v;
      if (e < tlen) {
        const uint32_t sh = opaque_u32(1u << (WIDE ? (tr.j & 31u) : tr.j));
        tr.T[0] += (uint64_t)v.x * sh;
        tr.T[1] += (uint64_t)v.y * sh;
        tr.T[2] += (uint64_t)v.z * sh;
        tr.T[3] += (uint64_t)v.w * sh;
        ++tr.j;
        if (WIDE && tr.j == 32 && c.bits > 32) {
          trunc_lo = truncw_value(tr);
          truncw_zero(tr);
        }
        if (tr.j == c.bits) {
          f128 val = truncw_value(tr);
          if (WIDE && c.bits > 32) val = add128(trunc_lo, shl32_mod(val));
          op[(uint64_t)tr.i * IL] = f_to_u4(val);
          truncw_zero(tr);
          tr.j = 0;
          tr.i++;
        }
      }
    };
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit(e0 + ci, make_uint4(st[4 * ci], st[4 * ci + 1], st[4 * ci + 2], st[4 * ci + 3]));
      carry0 = st[40];
      carry1 = st[41];
    } else {
      emit(e0 + 10, make_uint4(carry0, carry1, st[0], st[1]));
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit(e0 + 11 + ci, make_uint4(st[2 + 4 * ci], st[3 + 4 * ci], st[4 + 4 * ci], st[5 + 4 * ci]));
    }
#pragma unroll
    for (int w = 0; w < 4; w++) {
      aux[2 * w] = (uint32_t)tr.T[w];
      aux[2 * w + 1] = (uint32_t)(tr.T[w] >> 32);
    }
    aux[8] = carry0;
    aux[9] = carry1;
    aux[10] = gmax;
    if constexpr (WIDE) {
      aux[11] = (uint32_t)trunc_lo.lo;
      aux[12] = (uint32_t)(trunc_lo.lo >> 32);
      aux[13] = (uint32_t)trunc_lo.hi;
      aux[14] = (uint32_t)(trunc_lo.hi >> 32);
    }
  };
  // uniform: advance (ti, tj) past the truncated elements of block m
  auto advance_trunc = [&](uint32_t m) {
    const uint32_t e0 = 21 * (m >> 1) + ((m & 1) ? 10u : 0u);
    const uint32_t e1 = e0 + ((m & 1) ? 11u : 10u);
    const uint32_t cnt = e1 <= tlen ? e1 - e0 : (e0 < tlen ? tlen - e0 : 0u);
    tj += cnt;
    while (tj >= c.bits && cnt) {
      tj -= c.bits;
      ti++;
    }
  };
  // last absorbed block: message bytes [0, nb) of the block, then TurboSHAKE padding
  auto pad_last = [&](uint32_t* jw, uint32_t nb) {
#pragma unroll
    for (int w = 0; w < 42; w++) {
      const uint32_t lo_b = 4 * w;
      if (lo_b >= nb)
        jw[w] = 0;
      else if (lo_b + 4 > nb)
        jw[w] &= (1u << (8 * (nb - lo_b))) - 1u;
      if ((uint32_t)w == (nb >> 2)) jw[w] ^= 1u << (8 * (nb & 3));
    }
    jw[41] ^= 0x80000000u;
  };

  if (!jh) s_emit_block(0);
  advance_trunc(0);
  {
    // J's message block 0: the 42-byte header || S_0[0, 126) (the J half holds S_0 too)
    uint32_t jw[42];
#pragma unroll
    for (int w = 0; w < 10; w++) jw[w] = hdr[w];
    jw[10] = (hdr[10] & 0xffffu) | (st[0] << 16);
#pragma unroll
    for (int w = 11; w < 42; w++) jw[w] = alignbit(st[w - 10], st[w - 11], 16);
    if (b_last == 0) pad_last(jw, ML);
    if (jh) {
#pragma unroll
      for (int w = 0; w < 11; w++) aux[w] = st[31 + w];
#pragma unroll
      for (int w = 0; w < 42; w++) st[w] = jw[w];
#pragma unroll
      for (int w = 42; w < 50; w++) st[w] = 0;
    }
  }
#pragma unroll 1
  for (uint32_t m = 1; m <= b_last; m++) {
    keccak_p12(st);  // S: squeeze block m; J: absorb block m - 1 (unrolled: slower, see keccak_p12_unrolled)
    const bool have = m < NM;
    if (have) {
      if (!jh) s_emit_block(m);
      advance_trunc(m);
    }
    // S -> J: the shifted message words 11..41 of block m (formed by the S half) and the raw words 0 and
    // 31..41 (J's funnel shift of words 0..10 and its next pv). v_permlane32_swap moves lanes 0..31 of
    // its second operand into lanes 32..63 of the first; the first operand is any dead register (the
    // previous swap's clobbered source), so the shifted words cost one swap each.
    uint32_t jw[42], raw[12];
    uint32_t dead = st[0];
    if (have) {
#pragma unroll
      for (int w = 11; w < 42; w++) {
        const auto r2 = __builtin_amdgcn_permlane32_swap(dead, alignbit(st[w - 10], st[w - 11], 16), false, false);
        jw[w] = r2[0];
        dead = r2[1];
      }
      {
        const auto r2 = __builtin_amdgcn_permlane32_swap(dead, st[0], false, false);
        raw[0] = r2[0];
        dead = r2[1];
      }
#pragma unroll
      for (int k = 0; k < 11; k++) {
        const auto r2 = __builtin_amdgcn_permlane32_swap(dead, st[31 + k], false, false);
        raw[1 + k] = r2[0];
        dead = r2[1];
      }
    } else {
#pragma unroll
      for (int w = 11; w < 42; w++) jw[w] = 0;
#pragma unroll
      for (int k = 0; k < 12; k++) raw[k] = 0;
    }
    if (jh) {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = alignbit(aux[w + 1], aux[w], 16);
      jw[10] = alignbit(raw[0], aux[10], 16);
      if (m == b_last) pad_last(jw, ML - 168 * m);
#pragma unroll
      for (int w = 0; w < 42; w++) st[w] ^= jw[w];
#pragma unroll
      for (int k = 0; k < 11; k++) aux[k] = raw[1 + k];
    }
  }
  keccak_p12(st);  // J: absorb block b_last
  uint32_t own_part[4] = {st[0], st[1], st[2], st[3]};

  // proof share: XOF(k_proofs, DST(2), [PROOFS=1, agg_id=1]) in both halves, emitted by the S half
  uint4* const pp = b.proof + il_idx(blk, c.proof_len, 0, il);
  {
    uint32_t kproof[4];
    load16(hs + 16, kproof);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    sponge_oneblock(st, m);
  }
  uint32_t carry0 = 0, carry1 = 0, gmax = aux[10];  // S half: the measurement's screen so far
  auto emit_p = [&](uint32_t e, uint4 v) {
    if (e >= c.proof_len) return;
    gmax = max(gmax, ge_screen(v));
    if (!jh) pp[(uint64_t)e * IL] = v;
  };
  const uint32_t NP = (c.proof_len * 16 + 167) / 168;
#pragma unroll 1
  for (uint32_t m = 0; m < NP; m++) {
    if (m > 0) keccak_p12(st);
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit_p(e0 + ci, make_uint4(st[4 * ci], st[4 * ci + 1], st[4 * ci + 2], st[4 * ci + 3]));
      carry0 = st[40];
      carry1 = st[41];
    } else {
      emit_p(e0 + 10, make_uint4(carry0, carry1, st[0], st[1]));
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit_p(e0 + 11 + ci, make_uint4(st[2 + 4 * ci], st[3 + 4 * ci], st[4 + 4 * ci], st[5 + 4 * ci]));
    }
  }
  // the S half's screen (measurement + proof elements) goes to the J half, which finishes the report
  const uint32_t smax = lower_to_upper(gmax);
  if (jh) {
    uint32_t flags = smax == 0xFFFFFFFFu ? FLAG_SLOW : 0u;
    uint32_t nonce[4], part_l[4], lead_part[4];
    load16(b.nonces + 16 * r, nonce);
    load16(b.ps + (uint64_t)c.ps_bytes * r, part_l);
    load16(b.lps + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16, lead_part);
    [[clang::always_inline]] flags =
        xof_tail<true>(c, b, blk, il, r, r0 < b.n, nonce, part_l, lead_part, own_part, flags, false);
    if (b.force_slow) flags |= FLAG_SLOW;
    if (r0 < b.n) b.flags[r0] = flags;
  }
}

// ---------------------------------------------------------------------------- K1, lane-pair helper
// Launches that would give the lane-split kernel at most one wave per SIMD are bound by how fast ONE
// wave issues its own dependent chain (a lone wave64 issues a VALU op every ~4-6.5 cycles, against 2
// with a partner wave, MI355X_MICROARCH.md 'vector-instruction ISSUE cost'). This kernel halves each
// sponge's chain instead: a Keccak state is split over a lane PAIR, the even lane holding the low and
// the odd lane the high 32-bit halves of the 25 64-bit words (25 VGPRs each). A 64-bit rotation is
// then one v_alignbit_b32 per lane between its own half and its partner's (fetched by a DPP quad_perm
// [1,0,3,2] move): 124 instructions per round on each lane instead of 190 on one. Four lanes per
// report: lanes 2k / 2k+1 of the lower half squeeze the measurement share (S, low / high halves),
// lanes 32+2k / 33+2k absorb the joint_rand_part (J), 16 reports per wave, twice the waves of the
// lane-split kernel and 1.45x its instructions per report, so it is the choice only below one
// lane-split wave per SIMD (FixedPointBoundedL2VecSum 16 x 10000 at <= 32,768 reports per launch).
// The S lanes emit the elements (each lane two of an element's four words), keep the truncation
// word columns of their two words, and form J's message words from their own and their partner's
// halves; v_permlane32_swap hands them to the J lanes.

// the partner lane's value (lane ^ 1)
__device__ __forceinline__ uint32_t pswap(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1, 0, 3, 2]
}
__device__ __forceinline__ uint64_t pswap64(uint64_t v) {
  return (uint64_t)pswap((uint32_t)v) | ((uint64_t)pswap((uint32_t)(v >> 32)) << 32);
}
// this lane's half of rotl64(word, N) from its own and its partner's half (the same formula on both)
template <int N>
__device__ __forceinline__ uint32_t hrot(uint32_t own, uint32_t par) {
  if constexpr (N == 0)
    return own;
  else if constexpr (N < 32)
    return alignbit(own, par, 32 - N);
  else if constexpr (N == 32)
    return par;
  else
    return alignbit(par, own, 64 - N);
}
template <int I>
__device__ __forceinline__ void rho_pi_half_one(const uint32_t* s, uint32_t* B) {
  constexpr int R = RotOf<I>::value;
  if constexpr (R == 0)
    B[PiDst<I>::value] = s[I];
  else
    B[PiDst<I>::value] = hrot<R>(s[I], pswap(s[I]));
}
template <int... Is>
__device__ __forceinline__ void rho_pi_half_all(const uint32_t* s, uint32_t* B, IndexSeq<Is...>) {
  (rho_pi_half_one<Is>(s, B), ...);
}
// One Keccak-f[1600] round on this lane's half s[25]; rc = this lane's half of the round constant.
// theta parity 10 v_bitop3, partner parities 5 DPP moves, D 5 alignbit + 5 xor, D applied 25 xor,
// rho 24 DPP moves + 24 alignbit, chi 25 v_bitop3, iota 1: 124 VALU.
__device__ __forceinline__ void keccak_round_half(uint32_t* s, uint32_t rc) {
  uint32_t C[5], Cp[5], B[25];
#pragma unroll
  for (int x = 0; x < 5; x++) C[x] = xor3(xor3(s[x], s[x + 5], s[x + 10]), s[x + 15], s[x + 20]);
#pragma unroll
  for (int x = 0; x < 5; x++) Cp[x] = pswap(C[x]);
#pragma unroll
  for (int x = 0; x < 5; x++) {
    const uint32_t D = C[(x + 4) % 5] ^ hrot<1>(C[(x + 1) % 5], Cp[(x + 1) % 5]);
#pragma unroll
    for (int y = 0; y < 5; y++) s[x + 5 * y] ^= D;
  }
  rho_pi_half_all(s, B, typename MakeSeq<25>::type{});
#pragma unroll
  for (int y = 0; y < 5; y++) {
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const int i = x + 5 * y, i1 = (x + 1) % 5 + 5 * y, i2 = (x + 2) % 5 + 5 * y;
      s[i] = B[i] ^ (~B[i1] & B[i2]);
    }
  }
  s[0] ^= rc;
}
__device__ __forceinline__ void keccak_p12_half(uint32_t* s, bool hi) {
#pragma unroll 1
  for (int ir = 12; ir < 24; ir++) keccak_round_half(s, hi ? KECCAK_RC_HI[ir] : KECCAK_RC_LO[ir]);
}
// the same with the rounds unrolled (round constants as literals; see keccak_p12_unrolled)
__device__ __forceinline__ void keccak_p12_half_unrolled(uint32_t* s, bool hi) {
#pragma unroll
  for (int ir = 12; ir < 24; ir++) keccak_round_half(s, hi ? KECCAK_RC_HI[ir] : KECCAK_RC_LO[ir]);
}
// a ? x1 : x0 as bit operations on an opaque all-ones / zero mask: a select between two array elements
// written `a ? v[i + 1] : v[i]` becomes an indexed load v[i + a], which puts the array in scratch
__device__ __forceinline__ uint32_t msel(uint32_t m, uint32_t x0, uint32_t x1) { return x0 ^ ((x0 ^ x1) & m); }
// state := 0; absorb one final block (42 words, this lane takes words 2i + hi); permute
__device__ __forceinline__ void sponge_oneblock_half(uint32_t* s, const Block& m, bool hi) {
  const uint32_t hm = opaque_u32(hi ? 0xFFFFFFFFu : 0u);
#pragma unroll
  for (int i = 0; i < 21; i++) s[i] = msel(hm, m.w[2 * i], m.w[2 * i + 1]);
#pragma unroll
  for (int i = 21; i < 25; i++) s[i] = 0;
  keccak_p12_half(s, hi);
}

// UNR: the rounds of the block loop unrolled (round constants as literals): 4.03 -> 3.59 ms for launches of
// at most one pair-wave per SIMD, but slower with several waves per SIMD (64 x 1,000-report coalesced jobs:
// 12.5 -> 15.2 ms per launch), so the engine picks it only for the former (k1_plan, K1_PAIRS_UNROLLED).
template <bool UNR>
__global__ __launch_bounds__(64 * K1_WAVES, 2) void xof_pairs_kernel(Cfg c, Bufs b) {
  const uint32_t lane = threadIdx.x & 63;
  const bool jh = lane >= 32;     // J lanes
  const bool hi = (lane & 1u) != 0;  // high halves
  const uint32_t hm = opaque_u32(hi ? 0xFFFFFFFFu : 0u);
  const uint64_t gw = (uint64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6);  // 16 reports per wave
  const uint64_t blk = gw >> 2;
  const uint32_t il = ((uint32_t)gw & 3u) * 16u + ((lane & 31u) >> 1);  // this report's slot in its 64-report block
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint64_t r0 = blk * 64 + il;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint8_t* hs = b.his + (uint64_t)c.his_bytes * r;
  const uint32_t MB = c.meas_len * 16;
  const uint32_t ML = 42 + MB;
  const uint32_t NM = (MB + 167) / 168;
  const uint32_t b_last = ML / 168;

  uint32_t h[25];
  {  // squeeze block 0 = XOF(k_meas, DST(1), [1]) on every lane pair
    uint32_t kmeas[4];
    load16(hs, kmeas);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock_half(h, m, hi);
  }
  uint32_t hdr[11];
  {
    uint32_t nonce[4], kblind[4];
    load16(b.nonces + 16 * r, nonce);
    load16(hs + 32, kblind);
    Block hb;
    blk_zero(hb);
    int pos = blk_xof_prefix(hb, c.dst_id, 7, kblind);
    blk_put_byte(hb, pos, 1);  // agg_id
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(hb, pos + 1 + 4 * i, nonce[i]);
#pragma unroll
    for (int w = 0; w < 11; w++) hdr[w] = hb.w[w];
  }
  // S lanes: the truncation word columns of this lane's two words of an element (Ta: word 0 | 1, Tb:
  // word 2 | 3), the element carry, the >= p screen (meaningful on the high lane: w & (z | 0x1F)) and
  // the own halves 15..20 of the previous squeezed block (J's message words 0..10 need them)
  uint64_t Ta = 0, Tb = 0;
  uint32_t carry = 0, gmax = 0, pv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) pv[k] = 0;
  uint32_t* const mp32 = reinterpret_cast<uint32_t*>(b.meas + il_idx(blk, c.meas_len, 0, il)) + (hi ? 1u : 0u);
  uint4* const op = b.outs + il_idx(blk, c.out_len, 0, il);
  uint32_t tj = 0, ti = 0;  // uniform truncation position of the next measurement element
  const uint32_t tlen = c.out_is_meas ? 0u : min(c.trunc_len, c.meas_len);
  // S lanes: element e's words (a, bw) = (x, z) on the low lane, (y, w) on the high lane
  auto emit = [&](uint32_t e, uint32_t a, uint32_t bw, uint32_t& tjl, uint32_t& til) {
    if (e >= c.meas_len) return;
    const uint32_t pb = pswap(bw);
    gmax = max(gmax, bw & (pb | 0x1Fu));
    mp32[(uint64_t)e * IL * 4] = a;
    mp32[(uint64_t)e * IL * 4 + 2] = bw;
    if (e < tlen) {
      const uint32_t sh = opaque_u32(1u << tjl);
      Ta += (uint64_t)a * sh;
      Tb += (uint64_t)bw * sh;
      ++tjl;
      if (tjl == c.bits) {  // V = T0 + T1 2^32 + T2 2^64 + T3 2^96, finished on the low lane
        TruncW tr;
        tr.T[0] = Ta;
        tr.T[1] = pswap64(Ta);
        tr.T[2] = Tb;
        tr.T[3] = pswap64(Tb);
        const f128 val = truncw_value(tr);
        if (!hi) op[(uint64_t)til * IL] = f_to_u4(val);
        Ta = 0;
        Tb = 0;
        tjl = 0;
        til++;
      }
    }
  };
  auto s_emit_block = [&](uint32_t m) {
    uint32_t tjl = tj, til = ti;
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit(e0 + ci, h[2 * ci], h[2 * ci + 1], tjl, til);
      carry = h[20];
    } else {
      emit(e0 + 10, carry, h[0], tjl, til);
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit(e0 + 11 + ci, h[1 + 2 * ci], h[2 + 2 * ci], tjl, til);
    }
  };
  // uniform: advance (ti, tj) past the truncated elements of block m
  auto advance_trunc = [&](uint32_t m) {
    const uint32_t e0 = 21 * (m >> 1) + ((m & 1) ? 10u : 0u);
    const uint32_t e1 = e0 + ((m & 1) ? 11u : 10u);
    const uint32_t cnt = e1 <= tlen ? e1 - e0 : (e0 < tlen ? tlen - e0 : 0u);
    tj += cnt;
    while (tj >= c.bits && cnt) {
      tj -= c.bits;
      ti++;
    }
  };
  // last absorbed block: message bytes [0, nb) of the block, then TurboSHAKE padding; jw[i] is this
  // lane's word 2i + hi
  auto pad_last_half = [&](uint32_t* jw, uint32_t nb) {
#pragma unroll
    for (int i = 0; i < 21; i++) {
      const uint32_t w = 2 * i + (hi ? 1u : 0u);
      const uint32_t lo_b = 4 * w;
      if (lo_b >= nb)
        jw[i] = 0;
      else if (lo_b + 4 > nb)
        jw[i] &= (1u << (8 * (nb - lo_b))) - 1u;
      if (w == (nb >> 2)) jw[i] ^= 1u << (8 * (nb & 3));
      if (w == 41) jw[i] ^= 0x80000000u;
    }
  };
  // J's message words of a block from the S stream E (the previous block's halves 15..20, then the
  // current block's): J word 2i + hi = alignbit(E_own[i - 5], E_par[i - 6 + hi], 16). Past the share
  // (the block after the last squeezed one, m == b_last == NM) the current halves are a squeezed block
  // that is not part of the message: every word they reach lies at or past byte nb, which the padding
  // of that last block clears.
  auto message = [&](uint32_t* jw) {
    uint32_t Eo[21], Ep[22];
#pragma unroll
    for (int k = 0; k < 5; k++) Eo[k] = pv[k + 1];
#pragma unroll
    for (int k = 0; k < 16; k++) Eo[5 + k] = h[k];
#pragma unroll
    for (int k = 0; k < 6; k++) Ep[k] = pswap(pv[k]);
#pragma unroll
    for (int k = 0; k < 16; k++) Ep[6 + k] = pswap(h[k]);
#pragma unroll
    for (int i = 0; i < 21; i++) jw[i] = alignbit(Eo[i], msel(hm, Ep[i], Ep[i + 1]), 16);
  };

  if (!jh) s_emit_block(0);
  advance_trunc(0);
  {
    // J's message block 0: the 42-byte header || S_0[0, 126) (the J lanes hold S_0 too)
    uint32_t Hp[16];
#pragma unroll
    for (int k = 0; k < 16; k++) Hp[k] = pswap(h[k]);
    uint32_t jw[21];
#pragma unroll
    for (int i = 0; i < 5; i++) jw[i] = msel(hm, hdr[2 * i], hdr[2 * i + 1]);
    jw[5] = msel(hm, (hdr[10] & 0xffffu) | (h[0] << 16), alignbit(h[0], Hp[0], 16));
#pragma unroll
    for (int i = 6; i < 21; i++) jw[i] = alignbit(h[i - 5], msel(hm, Hp[i - 6], Hp[i - 5]), 16);
    if (b_last == 0) pad_last_half(jw, ML);
#pragma unroll
    for (int k = 0; k < 6; k++) pv[k] = h[15 + k];
    if (jh) {
#pragma unroll
      for (int i = 0; i < 21; i++) h[i] = jw[i];
#pragma unroll
      for (int i = 21; i < 25; i++) h[i] = 0;
    }
  }
#pragma unroll 1
  for (uint32_t m = 1; m <= b_last; m++) {
    if constexpr (UNR)
      keccak_p12_half_unrolled(h, hi);  // S: squeeze block m; J: absorb block m - 1
    else
      keccak_p12_half(h, hi);
    const bool have = m < NM;
    if (have) {
      if (!jh) s_emit_block(m);
      advance_trunc(m);
    }
    uint32_t msg[21], jw[21];
    message(msg);
#pragma unroll
    for (int k = 0; k < 6; k++) pv[k] = h[15 + k];
    uint32_t dead = h[0];
#pragma unroll
    for (int i = 0; i < 21; i++) {  // S lanes -> J lanes (lane l -> l + 32, the same half)
      const auto r2 = __builtin_amdgcn_permlane32_swap(dead, msg[i], false, false);
      jw[i] = r2[0];
      dead = r2[1];
    }
    if (jh) {
      if (m == b_last) pad_last_half(jw, ML - 168 * m);
#pragma unroll
      for (int i = 0; i < 21; i++) h[i] ^= jw[i];
    }
  }
  keccak_p12_half(h, hi);  // J: absorb block b_last
  // J state words 0..3: the low J lane holds words 0, 2 and gets 1, 3 from its partner
  const uint32_t p0 = pswap(h[0]), p1 = pswap(h[1]);
  uint32_t own_part[4] = {h[0], p0, h[1], p1};

  // proof share: XOF(k_proofs, DST(2), [PROOFS=1, agg_id=1]) on every lane pair, emitted by the S lanes
  uint32_t* const pp32 = reinterpret_cast<uint32_t*>(b.proof + il_idx(blk, c.proof_len, 0, il)) + (hi ? 1u : 0u);
  {
    uint32_t kproof[4];
    load16(hs + 16, kproof);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    sponge_oneblock_half(h, m, hi);
  }
  auto emit_p = [&](uint32_t e, uint32_t a, uint32_t bw) {
    if (e >= c.proof_len) return;
    const uint32_t pb = pswap(bw);
    gmax = max(gmax, bw & (pb | 0x1Fu));
    if (!jh) {
      pp32[(uint64_t)e * IL * 4] = a;
      pp32[(uint64_t)e * IL * 4 + 2] = bw;
    }
  };
  carry = 0;
  const uint32_t NP = (c.proof_len * 16 + 167) / 168;
#pragma unroll 1
  for (uint32_t m = 0; m < NP; m++) {
    if (m > 0) keccak_p12_half(h, hi);
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit_p(e0 + ci, h[2 * ci], h[2 * ci + 1]);
      carry = h[20];
    } else {
      emit_p(e0 + 10, carry, h[0]);
#pragma unroll
      for (int ci = 0; ci < 10; ci++) emit_p(e0 + 11 + ci, h[1 + 2 * ci], h[2 + 2 * ci]);
    }
  }
  // the high S lane's screen -> its low partner -> the low J lane, which finishes the report
  const uint32_t smax = lower_to_upper(pswap(gmax));
  if (jh && !hi) {
    uint32_t flags = smax == 0xFFFFFFFFu ? FLAG_SLOW : 0u;
    uint32_t nonce[4], part_l[4], lead_part[4];
    load16(b.nonces + 16 * r, nonce);
    load16(b.ps + (uint64_t)c.ps_bytes * r, part_l);
    load16(b.lps + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16, lead_part);
    flags = xof_tail(c, b, blk, il, r, r0 < b.n, nonce, part_l, lead_part, own_part, flags, false);
    if (b.force_slow) flags |= FLAG_SLOW;
    if (r0 < b.n) b.flags[r0] = flags;
  }
}

// ---------------------------------------------------------------------------- K1, small helper launches
// A launch of a thousand reports or fewer (Janus's 10-1,000-report aggregation jobs, one at a time or a few
// coalesced) leaves most SIMDs empty, so K1's time is ONE report's chain: 762 squeeze + 763 absorb blocks for
// SumVec 8x1000, each a Keccak-p[1600,12]. The lane-pair kernel runs that chain at 124 dependent VALU per
// round per lane (4.0 ms per launch, profiles/r05_small_launch_kernels.json). This kernel spreads each
// sponge over 25 lanes, one 64-bit word per lane (lane = x + 5y), one report per wave: lanes 0..24 squeeze
// the measurement share (S), lanes 32..56 absorb the joint_rand_part (J). A round is 26 VALU per lane and
// two exchanges through the wave's own LDS region (kw_sync at each hand-off: a wave's LDS operations complete in
// order, so no barrier instruction is needed, only a compiler fence):
//   theta: every lane writes its word into a column-major table whose columns are padded with wrap copies
//          (slot c + 1 holds column c, slot 0 column 4, slot 6 column 0), then reads columns x - 1 and
//          x + 1 as five ds_read2_b64 at offsets (k, k + 10) from one base;
//   rho:   a per-lane rotation, two v_alignbit_b32 on operands ordered once per lane;
//   pi + chi: every lane writes its rotated word at its pi destination into a row-major table with rows
//          padded by wrap copies (slots 5, 6 = 0, 1), then reads B[x], B[x+1], B[x+2] of its row.
// Measured (tools/kernel_probe sweep, profiles/r05_words_sweep.jsonl): 2.5-2.7 ms per launch up to 1,024
// reports against 3.6 ms for the lane pairs (2.7-2.9 with the rounds in a loop: the unrolled rounds take
// the round constants as literals); equal at 2,048; beyond, issue-bound and slower. One exchange
// per round instead (each lane reading columns x - 1 .. x + 3 of the chi table and computing the next
// round's parities itself, 54 VALU per round) measured 3.5-3.8 ms: a lone wave pays more for the doubled
// VALU chain than for the second LDS round trip.
// S hands each squeezed block to J through a 27-word message window in LDS (the previous block's words
// 15..20, then the block), from which J lane w forms its message word w as one 48-bit funnel shift; the
// 42-byte header sits in the window's prefix for block 0. The output-share truncation runs afterwards in
// trunc_kernel (it needs `bits` consecutive elements that lie on different lanes here).
constexpr uint32_t KW_WAVES = 4;  // waves (reports) per workgroup
// per-wave LDS region, in 8-byte words: theta tables S / J, chi tables S / J, message window, init block, sink
constexpr uint32_t KW_AS = 0, KW_AJ = 35, KW_BS = 70, KW_BJ = 105, KW_MSG = 140, KW_INIT = 167, KW_SINK = 188,
                   KW_WORDS = 189;
__constant__ uint8_t kw_rot_tab[25] = {JX_ROT_LIST};

struct KwLane {
  uint32_t aw1, aw2, ab;  // theta: write (own slot, wrap copy), read base (column x - 1)
  uint32_t bw1, bw2, bb;  // chi: write (pi destination, wrap copy), read base (B[x] of the lane's row)
  uint32_t pm, s;         // rho: operand order mask, v_alignbit amount
  uint32_t m0;            // iota: all-ones on word 0
};

// A hand-off between the lanes of one wave through its LDS region: every lane's earlier LDS writes are
// visible to every lane's later reads (and earlier reads complete before later writes). gfx950 completes a
// wave's LDS operations in order, so this emits no instruction; it forbids the compiler from moving LDS
// accesses across it, which it may otherwise do for pairs it proves distinct per thread (the C++ model does
// not order plain accesses of different lanes).
__device__ __forceinline__ void kw_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void kw_round(uint2* L, const KwLane& k, uint32_t& lo, uint32_t& hi, uint32_t rlo,
                                         uint32_t rhi) {
  L[k.aw1] = make_uint2(lo, hi);
  L[k.aw2] = make_uint2(lo, hi);
  kw_sync();  // theta table written -> read (the previous round's chi reads are behind the chi sync)
  uint2 cm[5], cp[5];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    cm[j] = L[k.ab + j];
    cp[j] = L[k.ab + j + 10];
  }
  const uint32_t cml = xor3(xor3(cm[0].x, cm[1].x, cm[2].x), cm[3].x, cm[4].x);
  const uint32_t cmh = xor3(xor3(cm[0].y, cm[1].y, cm[2].y), cm[3].y, cm[4].y);
  const uint32_t cpl = xor3(xor3(cp[0].x, cp[1].x, cp[2].x), cp[3].x, cp[4].x);
  const uint32_t cph = xor3(xor3(cp[0].y, cp[1].y, cp[2].y), cp[3].y, cp[4].y);
  // D[x] = C[x - 1] ^ rotl64(C[x + 1], 1)
  lo = xor3(lo, cml, alignbit(cpl, cph, 31));
  hi = xor3(hi, cmh, alignbit(cph, cpl, 31));
  // rho: (P, Q) = the halves in the order this lane's rotation needs (see xof_words_kernel)
  const uint32_t P = msel(k.pm, hi, lo);
  const uint32_t Q = xor3(lo, hi, P);
  const uint32_t nh = alignbit(P, Q, k.s), nl = alignbit(Q, P, k.s);
  L[k.bw1] = make_uint2(nl, nh);
  L[k.bw2] = make_uint2(nl, nh);
  kw_sync();  // chi table written -> read (this round's theta reads are behind the theta sync)
  const uint2 b0 = L[k.bb], b1 = L[k.bb + 1], b2 = L[k.bb + 2];
  lo = (b0.x ^ (~b1.x & b2.x)) ^ (rlo & k.m0);
  hi = (b0.y ^ (~b1.y & b2.y)) ^ (rhi & k.m0);
}
__device__ __forceinline__ void kw_p12(uint2* L, const KwLane& k, uint32_t& lo, uint32_t& hi) {
#pragma unroll
  for (int ir = 12; ir < 24; ir++) kw_round(L, k, lo, hi, KECCAK_RC_LO[ir], KECCAK_RC_HI[ir]);
}

__global__ __launch_bounds__(64 * KW_WAVES) void xof_words_kernel(Cfg c, Bufs b) {
  __shared__ uint2 lds[KW_WAVES][KW_WORDS];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t r = (uint64_t)blockIdx.x * KW_WAVES + wv;
  if (r >= b.n) return;
  uint2* L = lds[wv];
  const uint64_t blk = r >> 6;
  const uint32_t il = (uint32_t)r & 63u;
  const bool jg = lane >= 32;         // J lanes
  const uint32_t i = lane & 31u;      // this lane's word of its sponge
  const bool act = i < 25;
  const bool sw21 = !jg && i < 21;    // S lanes holding a rate word
  const bool jw21 = jg && i < 21;     // J lanes absorbing a message word
  const uint32_t ia = act ? i : 0u, x = ia % 5u, y = ia / 5u;
  KwLane k;
  {
    const uint32_t A0 = jg ? KW_AJ : KW_AS, B0 = jg ? KW_BJ : KW_BS;
    const uint32_t xp = y, yp = (2u * x + 3u * y) % 5u;  // pi destination (column, row)
    k.aw1 = act ? A0 + (x + 1u) * 5u + y : KW_SINK;
    k.aw2 = !act ? KW_SINK : x == 4u ? A0 + y : x == 0u ? A0 + 30u + y : k.aw1;
    k.ab = A0 + x * 5u;
    k.bw1 = act ? B0 + yp * 7u + xp : KW_SINK;
    k.bw2 = !act ? KW_SINK : xp < 2u ? k.bw1 + 5u : k.bw1;
    k.bb = B0 + y * 7u + x;
    // rotl64 by R: with sw = R >= 32 and M = R mod 32, new hi = alignbit(P, Q, (32 - M) mod 32) and new lo =
    // alignbit(Q, P, ...), where P is the low half iff sw != (M == 0) (alignbit by 0 returns its second operand)
    const uint32_t R = kw_rot_tab[ia], M = R & 31u;
    k.pm = ((R >= 32u) != (M == 0u)) ? 0xFFFFFFFFu : 0u;
    k.s = (32u - M) & 31u;
    k.m0 = act && ia == 0u ? 0xFFFFFFFFu : 0u;
  }
  const uint8_t* hs = b.his + (uint64_t)c.his_bytes * r;
  const uint32_t MB = c.meas_len * 16;
  const uint32_t ML = 42 + MB;
  const uint32_t NM = (MB + 167) / 168;
  const uint32_t b_last = ML / 168;
  uint32_t lo = 0, hi = 0, gmax = 0;

  // S := the permuted one-block sponge of `m` (block word i on S lane i); J keeps its state
  auto s_init = [&](const Block& m) {
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < 21; w++) L[KW_INIT + w] = make_uint2(m.w[2 * w], m.w[2 * w + 1]);
    }
    kw_sync();  // lane 0's init block -> every S lane
    const uint2 v = L[KW_INIT + (i < 21u ? i : 0u)];
    const uint32_t jlo = lo, jhi = hi;
    lo = sw21 ? v.x : 0u;
    hi = sw21 ? v.y : 0u;
    kw_p12(L, k, lo, hi);
    if (jg) {
      lo = jlo;
      hi = jhi;
    }
  };
  // S lanes: block m's word i is stream word q = 21 m + i, half q & 1 of element q >> 1
  auto s_emit = [&](uint4* base, uint32_t len, uint32_t m) {
    if (sw21) {
      const uint32_t q = 21u * m + i, e = q >> 1;
      if (e < len) {
        reinterpret_cast<uint2*>(base + il_idx(blk, len, e, il))[q & 1u] = make_uint2(lo, hi);
        if (q & 1u) gmax = max(gmax, hi & (lo | 0x1Fu));  // ge_screen on the element's (z, w)
      }
    }
  };
  // J lanes: message word w of a block = stream bytes [8 w - 42, 8 w - 34) relative to the block = window
  // words (w, w + 1) shifted by 48 bits; the last absorbed block keeps bytes [0, nb) and takes the padding
  auto j_absorb = [&](bool last, uint32_t nb) {
    if (jw21) {
      const uint2 v0 = L[KW_MSG + i], v1 = L[KW_MSG + i + 1];
      uint32_t wd[2] = {alignbit(v1.x, v0.y, 16), alignbit(v1.y, v1.x, 16)};
      if (last) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const uint32_t d = 2u * i + (uint32_t)h, lb = 4u * d;
          if (lb >= nb)
            wd[h] = 0;
          else if (lb + 4u > nb)
            wd[h] &= (1u << (8u * (nb - lb))) - 1u;
          if (d == (nb >> 2)) wd[h] ^= 1u << (8u * (nb & 3u));
          if (d == 41u) wd[h] ^= 0x80000000u;
        }
      }
      lo ^= wd[0];
      hi ^= wd[1];
    }
  };

  {  // S: XOF(k_meas, DST(1), [1]) -> measurement-share block 0
    uint32_t kmeas[4];
    load16(hs, kmeas);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    s_init(m);
  }
  {  // the window's prefix: J's 42-byte header [agg_id || nonce after the XOF prefix] at stream bytes [-42, 0)
    uint32_t nonce[4], kblind[4];
    load16(b.nonces + 16 * r, nonce);
    load16(hs + 32, kblind);
    Block h;
    blk_zero(h);
    int pos = blk_xof_prefix(h, c.dst_id, 7, kblind);
    blk_put_byte(h, pos, 1);  // agg_id
#pragma unroll
    for (int q = 0; q < 4; q++) blk_put_word(h, pos + 1 + 4 * q, nonce[q]);
    if (lane == 0) {
      // window word t covers stream bytes [8 t - 48, 8 t - 40): header bytes 8 t - 6 ..
      L[KW_MSG + 0] = make_uint2(0u, h.w[0] << 16);
#pragma unroll
      for (int t = 1; t < 6; t++)
        L[KW_MSG + t] = make_uint2(alignbit(h.w[2 * t - 1], h.w[2 * t - 2], 16), alignbit(h.w[2 * t], h.w[2 * t - 1], 16));
    }
  }
  s_emit(b.meas, c.meas_len, 0);
  if (sw21) L[KW_MSG + 6 + i] = make_uint2(lo, hi);
  kw_sync();  // the header (lane 0) and S's block -> J's message words
  j_absorb(b_last == 0, ML);  // J's state is zero: absorbing block 0 sets it
  kw_sync();  // J's window reads complete before S overwrites the window's prefix
  if (sw21 && i >= 15u) L[KW_MSG + i - 15u] = make_uint2(lo, hi);
#pragma unroll 1
  for (uint32_t m = 1; m <= b_last; m++) {
    kw_p12(L, k, lo, hi);  // S: squeeze block m; J: absorb block m - 1
    if (m < NM) s_emit(b.meas, c.meas_len, m);
    if (sw21) L[KW_MSG + 6 + i] = make_uint2(lo, hi);
    kw_sync();  // S's block -> J's message words
    j_absorb(m == b_last, ML - 168u * m);
    kw_sync();  // J's window reads complete before S overwrites the window's prefix
    if (sw21 && i >= 15u) L[KW_MSG + i - 15u] = make_uint2(lo, hi);
  }
  kw_p12(L, k, lo, hi);  // J: absorb block b_last
  // J's joint_rand_part = its state words 0, 1 (lanes 32, 33)
  uint32_t own_part[4] = {(uint32_t)__builtin_amdgcn_readlane((int)lo, 32), (uint32_t)__builtin_amdgcn_readlane((int)hi, 32),
                          (uint32_t)__builtin_amdgcn_readlane((int)lo, 33), (uint32_t)__builtin_amdgcn_readlane((int)hi, 33)};
  {  // proof share: XOF(k_proofs, DST(2), [PROOFS=1, agg_id=1])
    uint32_t kproof[4];
    load16(hs + 16, kproof);
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    s_init(m);
  }
  const uint32_t NP = (c.proof_len * 16 + 167) / 168;
  s_emit(b.proof, c.proof_len, 0);
#pragma unroll 1
  for (uint32_t m = 1; m < NP; m++) {
    kw_p12(L, k, lo, hi);
    s_emit(b.proof, c.proof_len, m);
  }
  const bool slow = __ballot(gmax == 0xFFFFFFFFu) != 0;
  if (lane == 0) {
    uint32_t flags = slow ? FLAG_SLOW : 0u;
    uint32_t nonce[4], part_l[4], lead_part[4];
    load16(b.nonces + 16 * r, nonce);
    load16(b.ps + (uint64_t)c.ps_bytes * r, part_l);
    load16(b.lps + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16, lead_part);
    flags = xof_tail(c, b, blk, il, r, true, nonce, part_l, lead_part, own_part, flags, false);
    if (b.force_slow) flags |= FLAG_SLOW;
    b.flags[r] = flags;
  }
}

// The output-share truncation of the small-launch kernel, one thread per (report, output element), the
// report fastest within its 64-report block: out_i = sum_{j < bits} 2^j x_{bits i + j} mod p over the staged
// measurement share (the same word-column sums as emit_meas). Reports the slow kernel redoes get their
// output share rewritten there.
__global__ __launch_bounds__(256) void trunc_kernel(Cfg c, Bufs b, uint32_t nout) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t il = (uint32_t)(t & 63u);
  const uint64_t gi = t >> 6;
  const uint32_t i = (uint32_t)(gi % nout);
  const uint64_t blk = gi / nout;
  const uint64_t r = blk * 64 + il;
  if (r >= b.n) return;
  TruncW tr;
  truncw_zero(tr);
  for (uint32_t j = 0; j < c.bits; j++) {
    const uint4 v = b.meas[il_idx(blk, c.meas_len, i * c.bits + j, il)];
    tr.T[0] += (uint64_t)v.x << j;
    tr.T[1] += (uint64_t)v.y << j;
    tr.T[2] += (uint64_t)v.z << j;
    tr.T[3] += (uint64_t)v.w << j;
  }
  b.outs[il_idx(blk, c.out_len, i, il)] = f_to_u4(truncw_value(tr));
}

// ---------------------------------------------------------------------------- K1, leader role
// leader_initialized (aggregation_job_driver.rs:345): prepare_init with agg_id 0 on the explicit leader
// input share [meas || proofs || k_blind], one report per lane. Only the joint_rand_part absorb runs
// through Keccak; block m+1 of the share (21 8-byte loads per lane) is fetched into the block buffer
// while J permutes block m, so the loads land under the permutation. Elements >= p fail the report
// (decode). One buffer, one sponge: no spills even when a launch holds a third of a wave per SIMD
// (FixedPointBoundedL2VecSum at length 10000), where every scratch access would be exposed.
// INPLACE: the FLP kernels read the explicit share where it lies (Bufs::meas_rs), so K1 stages nothing
// of it (2.56 MB per FixedPoint 16 x 10000 report: no store traffic, no waits on the stores, and the
// staging memory goes to more reports per launch).
template <bool WIDE, bool INPLACE>
__global__ __launch_bounds__(64 * K1_WAVES) void xof_leader_kernel(Cfg c, Bufs b) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6);
  const uint64_t nblk = (b.n + 63) / 64;
  if (blk >= nblk) return;
  const uint64_t r0 = blk * 64 + lane;
  const uint64_t r = r0 < b.n ? r0 : b.n - 1;
  const uint8_t* ls = b.lis + b.lis_rs * r;
  const uint32_t MB = c.meas_len * 16;
  const uint32_t ML = 42 + MB;
  const uint32_t NM = (MB + 167) / 168;
  const uint32_t b_last = ML / 168;

  uint32_t buf[42];  // block m of the explicit measurement share (words past the share read as 0)
  auto load_block = [&](uint32_t m) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 21; q++) {
      const uint32_t off = 168 * m + 8 * q;
      uint2 v = make_uint2(0, 0);
      if (off < MB) v = *reinterpret_cast<const uint2*>(ls + off);
      buf[2 * q] = v.x;
      buf[2 * q + 1] = v.y;
    }
  };
  // a block wholly inside the share: no per-word guard, so nothing consumes the loaded words before
  // the next iteration and the loads stay in flight under the permutation (a guard's select would
  // make the compiler wait for them before it)
  auto load_block_full = [&](uint32_t m) __attribute__((always_inline)) {
    const uint2* src = reinterpret_cast<const uint2*>(ls + 168 * m);
#pragma unroll
    for (int q = 0; q < 21; q++) {
      const uint2 v = src[q];
      buf[2 * q] = v.x;
      buf[2 * q + 1] = v.y;
    }
  };
  const uint32_t NF = MB / 168;  // blocks 0 .. NF-1 lie wholly inside the share
  uint32_t carry0 = 0, carry1 = 0, unused_screen = 0;
  bool bad = false;
  TruncW tr;
  truncw_zero(tr);
  tr.j = 0;
  tr.i = 0;
  f128 trunc_lo = make128(0, 0);
  uint4* const mp = b.meas + il_idx(blk, c.meas_len, 0, lane);
  uint4* const op = b.outs + il_idx(blk, c.out_len, 0, lane);
  auto emit = [&](uint32_t e, uint4 v) __attribute__((always_inline)) {
    if (e < c.meas_len) bad |= ge_exact(v);
    emit_meas<WIDE, !INPLACE>(c, mp, op, e, v, unused_screen, tr, trunc_lo);
  };
  auto emit_block = [&](uint32_t m) __attribute__((always_inline)) {
    const uint32_t e0 = 21 * (m >> 1);
    if ((m & 1) == 0) {
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit(e0 + ci, make_uint4(buf[4 * ci], buf[4 * ci + 1], buf[4 * ci + 2], buf[4 * ci + 3]));
      carry0 = buf[40];
      carry1 = buf[41];
    } else {
      emit(e0 + 10, make_uint4(carry0, carry1, buf[0], buf[1]));
#pragma unroll
      for (int ci = 0; ci < 10; ci++)
        emit(e0 + 11 + ci, make_uint4(buf[2 + 4 * ci], buf[3 + 4 * ci], buf[4 + 4 * ci], buf[5 + 4 * ci]));
    }
  };
  uint32_t hdr[11];
  {
    uint32_t nonce[4], kblind[4];
    load16(b.nonces + 16 * r, nonce);
    load16(ls + MB + 16 * c.proof_len, kblind);
    Block h;
    blk_zero(h);
    int pos = blk_xof_prefix(h, c.dst_id, 7, kblind);
    blk_put_byte(h, pos, 0);  // agg_id
#pragma unroll
    for (int i = 0; i < 4; i++) blk_put_word(h, pos + 1 + 4 * i, nonce[i]);
#pragma unroll
    for (int w = 0; w < 11; w++) hdr[w] = h.w[w];
  }
  uint32_t J[50], prev[11];
  // J's message words of block m from prev (block m-1) and buf (block m, if present); block 0 starts
  // with the header
  auto message = [&](uint32_t m, bool have, uint32_t* jw) __attribute__((always_inline)) {
    const uint32_t s0 = have ? buf[0] : 0u;
    if (m == 0) {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = hdr[w];
      jw[10] = (hdr[10] & 0xffffu) | (s0 << 16);
    } else {
#pragma unroll
      for (int w = 0; w < 10; w++) jw[w] = alignbit(prev[w + 1], prev[w], 16);
      jw[10] = alignbit(s0, prev[10], 16);
    }
#pragma unroll
    for (int w = 11; w < 42; w++) jw[w] = have ? alignbit(buf[w - 10], buf[w - 11], 16) : 0u;
  };
  load_block(0);
  emit_block(0);
  if (b_last == 0) {
    uint32_t jw[42];
    message(0, true, jw);
    const uint32_t nb = ML;
#pragma unroll
    for (int w = 0; w < 42; w++) {
      const uint32_t lo_b = 4 * w;
      if (lo_b >= nb)
        jw[w] = 0;
      else if (lo_b + 4 > nb)
        jw[w] &= (1u << (8 * (nb - lo_b))) - 1u;
      if ((uint32_t)w == (nb >> 2)) jw[w] ^= 1u << (8 * (nb & 3));
    }
    jw[41] ^= 0x80000000u;
#pragma unroll
    for (int w = 0; w < 42; w++) J[w] = jw[w];
#pragma unroll
    for (int w = 42; w < 50; w++) J[w] = 0;
    keccak_p12(J);
  } else {
    {
      uint32_t jw[42];
      message(0, true, jw);
#pragma unroll
      for (int w = 0; w < 42; w++) J[w] = jw[w];
#pragma unroll
      for (int w = 42; w < 50; w++) J[w] = 0;
#pragma unroll
      for (int w = 0; w < 11; w++) prev[w] = buf[31 + w];
    }
    if (1 < NF)
      load_block_full(1);
    else if (1 < NM)
      load_block(1);
    keccak_p12(J);
    auto step = [&](uint32_t m) __attribute__((always_inline)) {  // block m < b_last <= NM holds measurement bytes
      emit_block(m);
      uint32_t jw[42];
      message(m, true, jw);
#pragma unroll
      for (int w = 0; w < 42; w++) J[w] ^= jw[w];
#pragma unroll
      for (int w = 0; w < 11; w++) prev[w] = buf[31 + w];
    };
    uint32_t m = 1;
#pragma unroll 1
    for (; m < b_last && m + 1 < NF; m++) {  // the next block is wholly inside the share
      step(m);
      load_block_full(m + 1);
      keccak_p12(J);  // (unrolled: slower, see keccak_p12_unrolled)
    }
#pragma unroll 1
    for (; m < b_last; m++) {
      step(m);
      if (m + 1 < NM) load_block(m + 1);
      keccak_p12(J);
    }
    const bool have = b_last < NM;
    if (have) emit_block(b_last);
    uint32_t jw[42];
    message(b_last, have, jw);
    const uint32_t nb = ML - 168 * b_last;
#pragma unroll
    for (int w = 0; w < 42; w++) {
      const uint32_t lo_b = 4 * w;
      if (lo_b >= nb)
        jw[w] = 0;
      else if (lo_b + 4 > nb)
        jw[w] &= (1u << (8 * (nb - lo_b))) - 1u;
      if ((uint32_t)w == (nb >> 2)) jw[w] ^= 1u << (8 * (nb & 3));
    }
    jw[41] ^= 0x80000000u;
#pragma unroll
    for (int w = 0; w < 42; w++) J[w] ^= jw[w];
    keccak_p12(J);
  }
  uint32_t own_part[4] = {J[0], J[1], J[2], J[3]};
  // proof share: explicit, decoded (>= p fails)
  uint4* const pp = b.proof + il_idx(blk, c.proof_len, 0, lane);
  const uint4* src = reinterpret_cast<const uint4*>(ls + MB);
#pragma unroll 1
  for (uint32_t e = 0; e < c.proof_len; e++) {
    const uint4 v = src[e];
    bad |= ge_exact(v);
    pp[(uint64_t)e * IL] = v;
  }
  uint32_t nonce[4], part_h[4];
  load16(b.nonces + 16 * r, nonce);
  // corrected seed = XOF(0, DST(6), own part || helper's part from the public share): the leader's
  // prepare state (written to msgs), and own part goes out in the prep share
  load16(b.ps + (uint64_t)c.ps_bytes * r + 16, part_h);
  uint32_t flags = xof_tail(c, b, blk, lane, r, r0 < b.n, nonce, own_part, own_part, part_h, 0u, false);
  if (flags & FLAG_SLOW)  // a rejected joint/query randomness sample (~2^-120): redo exactly
    flags = xof_tail(c, b, blk, lane, r, r0 < b.n, nonce, own_part, own_part, part_h, flags & ~FLAG_SLOW, true);
  if (bad) flags |= FLAG_INPUT_FAIL;
  if (r0 < b.n) {
    *reinterpret_cast<uint4*>(b.lps_out + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16) =
        make_uint4(own_part[0], own_part[1], own_part[2], own_part[3]);
    b.flags[r0] = flags;
  }
}

// ---------------------------------------------------------------------------- K1': slow XOF path
// General byte-stream implementation with rejection sampling at any position. Runs only
// for reports flagged FLAG_SLOW (a sampled chunk was >= p; ~1e-14 per SumVec report).

struct ByteAbs {
  uint32_t s[50];
  uint32_t pos;
};
__device__ void ba_byte(ByteAbs& a, uint32_t v) {
  a.s[a.pos >> 2] ^= (v & 0xffu) << (8 * (a.pos & 3));
  a.pos++;
  if (a.pos == 168) {
    keccak_p12(a.s);
    a.pos = 0;
  }
}
__device__ void ba_word(ByteAbs& a, uint32_t v) {
  for (int k = 0; k < 4; k++) ba_byte(a, v >> (8 * k));
}

__global__ __launch_bounds__(64) void xof_slow_kernel(Cfg c, Bufs b) {
  const uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r0 >= b.n) return;
  if (!(b.flags[r0] & FLAG_SLOW)) return;
  const uint64_t r = r0, blk = r0 / 64;
  const uint32_t lane = r0 % 64;
  uint32_t nonce[4], kmeas[4], kproof[4], kblind[4];
  load16(b.nonces + 16 * r, nonce);
  const uint8_t* hs = b.his + (uint64_t)c.his_bytes * r;
  load16(hs, kmeas);
  load16(hs + 16, kproof);
  load16(hs + 32, kblind);
  uint32_t flags = 0;
  ByteXof X;
  ByteAbs A;
  {
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 1, kmeas);
    blk_put_byte(m, pos, 1);
    blk_pad(m, pos + 1);
    sponge_oneblock(X.s, m);
    X.pos = 0;
  }
  for (int w = 0; w < 50; w++) A.s[w] = 0;
  A.pos = 0;
  {
    Block h;
    blk_zero(h);
    int pos = blk_xof_prefix(h, c.dst_id, 7, kblind);
    blk_put_byte(h, pos, 1);
    for (int i = 0; i < 4; i++) blk_put_word(h, pos + 1 + 4 * i, nonce[i]);
    for (int i = 0; i < 42; i++) ba_byte(A, h.w[i >> 2] >> (8 * (i & 3)));
  }
  Trunc tr;
  acc_zero(tr.a);
  tr.j = 0;
  tr.i = 0;
  for (uint32_t e = 0; e < c.meas_len; e++) {
    f128 x = bx_sample128(X);
    st_il(b.meas, blk, c.meas_len, e, lane, x);
    ba_word(A, lo32(x.lo));
    ba_word(A, hi32(x.lo));
    ba_word(A, lo32(x.hi));
    ba_word(A, hi32(x.hi));
    if (!c.out_is_meas && e < c.trunc_len) {
      trunc_add(tr.a, x, tr.j);
      if (++tr.j == c.bits) {
        st_il(b.outs, blk, c.out_len, tr.i, lane, acc_reduce(tr.a));
        acc_zero(tr.a);
        tr.j = 0;
        tr.i++;
      }
    }
  }
  A.s[A.pos >> 2] ^= 1u << (8 * (A.pos & 3));
  A.s[41] ^= 0x80000000u;
  keccak_p12(A.s);
  uint32_t part_h[4] = {A.s[0], A.s[1], A.s[2], A.s[3]};
  {
    Block m;
    blk_zero(m);
    int pos = blk_xof_prefix(m, c.dst_id, 2, kproof);
    blk_put_byte(m, pos, 1);
    blk_put_byte(m, pos + 1, 1);
    blk_pad(m, pos + 2);
    sponge_oneblock(X.s, m);
    X.pos = 0;
  }
  for (uint32_t e = 0; e < c.proof_len; e++) st_il(b.proof, blk, c.proof_len, e, lane, bx_sample128(X));
  uint32_t part_l[4], lead_part[4];
  load16(b.ps + (uint64_t)c.ps_bytes * r, part_l);
  load16(b.lps + (uint64_t)c.lps_bytes * r + c.lps_bytes - 16, lead_part);
  flags = xof_tail(c, b, blk, lane, r, true, nonce, part_l, lead_part, part_h, flags, true);
  b.flags[r0] = flags & ~FLAG_SLOW;
}

// ---------------------------------------------------------------------------- launchers

hipError_t launch_count(const Cfg& c, const Bufs& b, hipStream_t s) {
  uint32_t nb = nblk_of(b.n);
  if (b.leader)
    hipLaunchKernelGGL(count_kernel<true>, dim3((nb * 64 + 255) / 256), dim3(256), 0, s, c, b);
  else
    hipLaunchKernelGGL(count_kernel<false>, dim3((nb * 64 + 255) / 256), dim3(256), 0, s, c, b);
  return hipGetLastError();
}
// k1: from k1_plan, which never names the word or pair kernels (bits <= 32) for a wide instance
hipError_t launch_xof(const Cfg& c, const Bufs& b, K1Launch k1, hipStream_t s) {
  uint32_t nb = nblk_of(b.n);
  const dim3 grid((nb + K1_WAVES - 1) / K1_WAVES), block(64 * K1_WAVES);
  const bool wide = c.bits > 32 && (c.algo == ALGO_SUM || c.algo == ALGO_SUMVEC);
  if (b.leader && wide && b.meas_rs)
    hipLaunchKernelGGL((xof_leader_kernel<true, true>), grid, block, 0, s, c, b);
  else if (b.leader && wide)
    hipLaunchKernelGGL((xof_leader_kernel<true, false>), grid, block, 0, s, c, b);
  else if (b.leader && b.meas_rs)
    hipLaunchKernelGGL((xof_leader_kernel<false, true>), grid, block, 0, s, c, b);
  else if (b.leader)
    hipLaunchKernelGGL((xof_leader_kernel<false, false>), grid, block, 0, s, c, b);
  else if (k1.kernel == K1_WORDS) {  // a word per lane: one report per wave, then the truncation
    hipLaunchKernelGGL(xof_words_kernel, dim3((uint32_t)((b.n + KW_WAVES - 1) / KW_WAVES)), dim3(64 * KW_WAVES), 0, s, c, b);
    const uint32_t nout = c.out_is_meas ? 0u : (c.trunc_len < c.meas_len ? c.trunc_len : c.meas_len) / c.bits;
    if (nout) {
      const uint64_t threads = (uint64_t)nblk_of(b.n) * 64 * nout;
      hipLaunchKernelGGL(trunc_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, c, b, nout);
    }
  } else if (k1.kernel == K1_PAIRS_UNROLLED)  // lane pairs, unrolled rounds (<= one pair-wave per SIMD)
    hipLaunchKernelGGL(xof_pairs_kernel<true>, dim3((4 * nb + K1_WAVES - 1) / K1_WAVES), block, k1.lds, s, c, b);
  else if (k1.kernel == K1_PAIRS)  // lane pairs: 16 reports per wave
    hipLaunchKernelGGL(xof_pairs_kernel<false>, dim3((4 * nb + K1_WAVES - 1) / K1_WAVES), block, k1.lds, s, c, b);
  else if (k1.kernel == K1_LANES) {  // lane-split: 32 reports per wave
    const dim3 g2((2 * nb + K1_WAVES - 1) / K1_WAVES);
    if (wide)
      hipLaunchKernelGGL((xof_lanes_kernel<true>), g2, block, k1.lds, s, c, b);
    else
      hipLaunchKernelGGL((xof_lanes_kernel<false>), g2, block, k1.lds, s, c, b);
  } else if (wide)
    hipLaunchKernelGGL((xof_kernel<true>), grid, block, 0, s, c, b);
  else
    hipLaunchKernelGGL((xof_kernel<false>), grid, block, 0, s, c, b);
  return hipGetLastError();
}
Bufs bufs_tail(const Cfg& c, const Bufs& b, uint64_t S) {
  Bufs t = b;
  const uint64_t blk = S / 64;
  t.n = b.n - S;
  t.nonces += S * 16;
  t.ps += S * c.ps_bytes;
  t.his += S * c.his_bytes;
  t.lps += S * c.lps_bytes;
  t.meas += blk * c.meas_len * IL;
  t.proof += blk * c.proof_len * IL;
  t.outs += blk * c.out_len * IL;
  t.coef += blk * c.ncoef * IL;
  t.flags += S;
  t.verdicts += S;
  t.msgs += S * 16;
  // per-report rows that a coalesced launch carries: the verify keys (16 B, or the 64-B HMAC pads of the
  // multiproof instance) and, for a leader launch, its explicit input shares and outbound prep shares
  if (t.vkeys) t.vkeys += S * (c.algo == ALGO_SUMVEC_F64_MULTIPROOF ? 64u : 16u);
  if (t.lis) t.lis += S * b.lis_rs;
  if (t.meas_src) t.meas_src += S * b.meas_rs;
  if (t.lps_out) t.lps_out += S * c.lps_bytes;
  return t;
}

// Reports that occupy every K1 wave slot of the device exactly once: CUs x resident
// workgroups per CU (from the kernel's register/LDS footprint) x 64 reports per wave. K1 waves
// all run the same length, so a launch runs in ceil(reports / this) equal "rounds"; the
// engine sizes its launches in whole rounds so only the last launch has a partial one.
uint64_t k1_round_reports(const Cfg& c, int device) {
  if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF) return mp_k1_round_reports(device);
  int cus = 0, wgs = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return 0;
  const uint32_t threads = c.algo == ALGO_COUNT ? 256u : 64u * K1_WAVES;
  hipError_t st;
  uint32_t per_wg = threads;  // reports per workgroup
  if (c.algo == ALGO_COUNT) {
    st = hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, count_kernel<false>, threads, 0);
  } else {
    st = hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, xof_kernel<false>, threads, 0);
  }
  if (st != hipSuccess || wgs <= 0) return 0;
  return (uint64_t)cus * (uint64_t)wgs * per_wg;
}
hipError_t launch_xof_slow(const Cfg& c, const Bufs& b, hipStream_t s) {
  hipLaunchKernelGGL(xof_slow_kernel, dim3((uint32_t)((b.n + 63) / 64)), dim3(64), 0, s, c, b);
  return hipGetLastError();
}

}  // namespace jx
