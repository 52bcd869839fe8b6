// jx_ntt.h — number-theoretic transforms in Field128 for the Prio3 prover (FlpGeneric.prove, jx_shard.hip).
//
// A gadget wire is given by its P values at the P-th roots of unity alpha^k; the gadget polynomial
// G = sum_i wire_2i * wire_2i+1 has degree 2(P - 1) and is wanted as coefficients. With beta a primitive
// 2P-th root (beta^2 = alpha), a wire polynomial's values at the even points beta^(2k) are the wire values
// themselves, so per wire only the P odd-point values w(beta^(2k+1)) are computed (ntt_odd_points): an inverse
// size-P transform, a twist of coefficient j by beta^j / P, a forward size-P transform. G's coefficients come
// back from its 2P values through the first split of the inverse size-2P transform (ntt_gpoly_finish): with
// E, O the inverse size-P transforms of the even- and odd-point values, g_j = (E_j + beta^-j O_j) / 2 and
// g_(j+P) = (E_j - beta^-j O_j) / 2.
//
// The inverse transforms are decimation-in-frequency (natural order in, bit-reversed order out), the forward
// one decimation-in-time (bit-reversed in, natural out), so no transform permutes: the tables that meet
// bit-reversed data (the twists) are stored bit-reversed. Data stays canonical; table entries are in
// Montgomery form (jx_field.h), so mont128(x, tR) = x t is canonical after one reduction.
//
// Every routine runs over `nl` cooperating lanes (lane = 0, nl = 1 on the host; a wave's 64 lanes over its LDS
// region on the device) and calls sync() where one lane reads what another wrote.
#pragma once
#include <stdint.h>

#include "jx_field.h"

namespace jx {

#if defined(__HIPCC__) || defined(__HIP__)
// the device's sync(): what one lane of the wave wrote to LDS is visible to the others; no workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

// Table of one transform size P (f128 entries, Montgomery form):
//   [0, P/2)    alpha^k                      forward twiddles
//   [P/2, P)    alpha^-k                     inverse twiddles
//   [P, 2P)     beta^rev(i) / P              odd-point twist at bit-reversed position i
//   [2P, 3P)    beta^-rev(i)                 untwist of O at bit-reversed position i
//   [3P]        R / (2P)                     final scale: pointwise Montgomery products carry 1/R
JX_HD uint32_t ntt_table_len(uint32_t P) { return 3 * P + 1; }

JX_HD uint32_t ntt_rev(uint32_t i, uint32_t logP) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < logP; b++) r |= ((i >> b) & 1u) << (logP - 1 - b);
  return r;
}

// decimation in frequency: a[i] <- X[rev(i)], X_m = sum_j a_j w^(jm); w[k] = w^k R for k < P/2
template <class Sync>
JX_HD void ntt_dif(f128* a, uint32_t P, const f128* w, uint32_t lane, uint32_t nl, Sync sync) {
  for (uint32_t half = P >> 1, step = 1; half >= 1; half >>= 1, step <<= 1) {
    for (uint32_t b = lane; b < (P >> 1); b += nl) {
      const uint32_t k = b & (half - 1), i = ((b - k) << 1) + k;
      const f128 u = a[i], v = a[i + half];
      a[i] = add128(u, v);
      a[i + half] = mont128(sub128(u, v), w[k * step]);
    }
    sync();
  }
}

// decimation in time: a[i] holds x[rev(i)]; a[m] <- sum_j x_j w^(jm)
template <class Sync>
JX_HD void ntt_dit(f128* a, uint32_t P, const f128* w, uint32_t lane, uint32_t nl, Sync sync) {
  for (uint32_t half = 1, step = P >> 1; half < P; half <<= 1, step >>= 1) {
    for (uint32_t b = lane; b < (P >> 1); b += nl) {
      const uint32_t k = b & (half - 1), i = ((b - k) << 1) + k;
      const f128 u = a[i], v = mont128(a[i + half], w[k * step]);
      a[i] = add128(u, v);
      a[i + half] = sub128(u, v);
    }
    sync();
  }
}

// a[k] = w(alpha^k) (the wire values) -> a[k] = w(beta^(2k+1))
template <class Sync>
JX_HD void ntt_odd_points(f128* a, uint32_t P, const f128* tab, uint32_t lane, uint32_t nl, Sync sync) {
  ntt_dif(a, P, tab + (P >> 1), lane, nl, sync);
  for (uint32_t i = lane; i < P; i += nl) a[i] = mont128(a[i], tab[P + i]);
  sync();
  ntt_dit(a, P, tab, lane, nl, sync);
}

// E[k] = G(beta^(2k)) / R, O[k] = G(beta^(2k+1)) / R (sums of Montgomery products of canonical wire values):
// emit(j, g_j) for every j < 2P. E and O are overwritten.
template <class Sync, class Emit>
JX_HD void ntt_gpoly_finish(f128* E, f128* O, uint32_t P, uint32_t logP, const f128* tab, uint32_t lane, uint32_t nl,
                            Sync sync, Emit emit) {
  ntt_dif(E, P, tab + (P >> 1), lane, nl, sync);
  ntt_dif(O, P, tab + (P >> 1), lane, nl, sync);
  const f128 sc = tab[3 * P];
  for (uint32_t i = lane; i < P; i += nl) {
    const uint32_t j = ntt_rev(i, logP);
    const f128 t = mont128(O[i], tab[2 * P + i]);
    emit(j, mont128(add128(E[i], t), sc));
    emit(j + P, mont128(sub128(E[i], t), sc));
  }
}

// ---------------------------------------------------------------------------- host: the tables
inline f128 ntt_mpow(f128 aR, uint64_t ehi, uint64_t elo) {
  f128 r = make128(R1_128_LO, R1_128_HI);
  for (int i = 127; i >= 0; i--) {
    r = mont128(r, r);
    if (i >= 64 ? (ehi >> (i - 64)) & 1 : (elo >> i) & 1) r = mont128(r, aR);
  }
  return r;
}
inline f128 ntt_minv(f128 aR) { return ntt_mpow(aR, 0xFFFFFFFFFFFFFFE3ull, 0xFFFFFFFFFFFFFFFFull); }  // a^(p-2)

// out[ntt_table_len(P)] for P = 2^logP, 1 <= logP <= 65. alpha is the root the verifier interpolates the wires
// at: GEN^(2^(66 - logP)) with GEN = 7^((p-1) / 2^66) (VDAF-08 §6.1.2).
inline void ntt_build_table(uint32_t logP, f128* out) {
  const uint32_t P = 1u << logP;
  const f128 R1 = make128(R1_128_LO, R1_128_HI);
  f128 beta = ntt_mpow(to_mont128(make128(7, 0)), 0, 4611686018427387897ull);  // GEN, order 2^66
  for (uint32_t i = 0; i + logP + 1 < 66; i++) beta = mont128(beta, beta);       // order 2P
  const f128 alpha = mont128(beta, beta), ibeta = ntt_minv(beta), ialpha = mont128(ibeta, ibeta);
  f128 f = R1, g = R1;
  for (uint32_t k = 0; k < P / 2; k++) {
    out[k] = f;
    out[P / 2 + k] = g;
    f = mont128(f, alpha);
    g = mont128(g, ialpha);
  }
  const f128 invP = ntt_minv(to_mont128(make128(P, 0)));
  f = invP;  // beta^j / P
  g = R1;    // beta^-j
  for (uint32_t j = 0; j < P; j++) {
    const uint32_t i = ntt_rev(j, logP);
    out[P + i] = f;
    out[2 * P + i] = g;
    f = mont128(f, beta);
    g = mont128(g, ibeta);
  }
  out[3 * P] = to_mont128(ntt_minv(to_mont128(make128(2ull * P, 0))));  // (1 / 2P) R^2
}

}  // namespace jx
