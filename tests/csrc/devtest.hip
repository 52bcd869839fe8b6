// gfx950 harness for the device arithmetic headers (janus_amd/csrc/jx_*.h), for tests/test_gpu_device_math.py: the
// headers are included unchanged and one lane runs one case, so the __forceinline__ bodies and the device-only
// instruction choices (mac_c's v_mad_u64_u32 carry mask, __builtin_addc / __builtin_subc, v_bitop3, alignbit) are
// what runs. What each operation computes is in jx_testops.h, shared with the g++ host libraries. Test-only: it
// includes no .hip product file and needs neither torch nor the engine library.
//
// Every operation has a fixed-size input record and output record per case (little-endian fields, 8-byte aligned);
// an operation of variable length carries an offset and a length into one shared `aux` buffer and checks both
// against its size. dt_run takes HOST pointers: it allocates exactly n records and the aux bytes, copies in,
// launches whole waves with a guarded tail, synchronises, copies back, frees, and returns the HIP error code.
//
// A second launch shape, for the code that runs across a wave (jx_ntt.h with nl = 64): one wave per case over 64 KiB
// of dynamic LDS, the exchanges behind the prove kernel's wave_sync (the DT_WOP operations).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../janus_amd/csrc/jx_field.h"
#include "../../janus_amd/csrc/jx_keccak.h"
#include "../../janus_amd/csrc/jx_sha256.h"
#include "../../janus_amd/csrc/jx_sha512.h"
#include "../../janus_amd/csrc/jx_sample.h"
#include "../../janus_amd/csrc/jx_ntt.h"
#include "../../janus_amd/csrc/jx_hpke.h"
#include "../../janus_amd/csrc/jx_sha_aes.h"
#include "../../janus_amd/csrc/jx_chapoly.h"
#include "../../janus_amd/csrc/jx_p256.h"
#include "../../janus_amd/csrc/jx_hpke_suites.h"
#include "../../janus_amd/csrc/jx_ghash_lanes.h"
#include "../../janus_amd/csrc/jx_chapoly_lanes.h"
#include "../../janus_amd/csrc/jx_kernels.h"  // trunc_add (its device section)
#define JX_TESTOPS_BASE
#define JX_TESTOPS_SAMPLE
#define JX_TESTOPS_P256
#define JX_TESTOPS_CHAPOLY
#include "jx_testops.h"

#ifndef DT_SRC_HASH
#define DT_SRC_HASH "unset"
#endif

using namespace jx;
using namespace jxt;

namespace {

constexpr uint32_t DT_BLOCK = 64;  // one wave per block

__device__ inline uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}
__device__ inline uint64_t rd64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
__device__ inline void wr32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
__device__ inline void wr64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }
// [off, off + len) lies inside the aux buffer
__device__ inline bool in_aux(uint64_t off, uint64_t len, uint32_t aux_len) { return off + len <= aux_len; }

struct Ctx {
  const uint8_t* aux;
  uint32_t aux_len;
  const uint32_t* t0;  // LDS: aes_t0_entry(AES_SBOX[x]), filled for operations with T0 = true
};

#define DT_OP(name, in_bytes, out_bytes, needs_t0)                             \
  struct op_##name {                                                           \
    static constexpr uint32_t IN = in_bytes, OUT = out_bytes;                  \
    static constexpr bool T0 = needs_t0, WAVE = false;                         \
    static __device__ void run(const uint8_t* in, uint8_t* out, const Ctx& c); \
  };                                                                           \
  __device__ void op_##name::run(const uint8_t* in, uint8_t* out, const Ctx& c)

// u32 op, pad, a[16], b[16] -> r[16]
DT_OP(f128, 40, 16, false) { t_f128((int)rd32(in), in + 8, in + 24, out); }
// u32 form (0 reduce192, 1 reduce192_small), pad, w[3] -> r[16]
DT_OP(red192, 32, 16, false) {
  uint64_t w[3] = {rd64(in + 8), rd64(in + 16), rd64(in + 24)};
  if (rd32(in))
    t_reduce192_small(w, out);
  else
    t_reduce192(w, out);
}
// a[16], b[16] -> lo, hi, top
DT_OP(mont_lazy, 32, 24, false) {
  uint64_t o[3];
  t_mont_lazy(in, in + 16, o);
  for (int i = 0; i < 3; i++) wr64(out + 8 * i, o[i]);
}
// u32 form (0 ge_p128, 1 ge_exact), pad, a[16] -> u32
DT_OP(ge128, 24, 4, false) { wr32(out, (uint32_t)(rd32(in) ? t_ge_exact(in + 8) : t_ge_p128(in + 8))); }
// u32 element offset, u32 n: the running max of ge_screen over aux elements [off, off + n) -> u32
DT_OP(ge_screen, 8, 4, false) {
  const uint32_t off = rd32(in), n = rd32(in + 4);
  wr32(out, in_aux(16ull * off, 16ull * n, c.aux_len) ? t_ge_screen_max(c.aux + 16ull * off, (int)n) : 0xDEADu);
}
// u32 bits (< 64), u32 element offset: sum_j aux[off + j] << j over j < bits by trunc_add, then acc_reduce -> r[16]
DT_OP(trunc, 8, 16, false) {
  const uint32_t bits = rd32(in), off = rd32(in + 4);
  acc192 a;
  acc_zero(a);
  if (bits < 64 && in_aux(16ull * off, 16ull * bits, c.aux_len))
    for (uint32_t j = 0; j < bits; j++) trunc_add(a, ld(c.aux + 16ull * (off + j)), j);
  st(out, acc_reduce(a));
}
// u32 bits (1..64), u32 element offset: K1's word-column truncation of aux[off, off + bits) in emit_meas's order:
// truncw_mac with sh = 2^(j mod 32) per element; for bits > 32 (the WIDE path) the columns of bits 0..31 are folded
// into lo at j = 32 and restart, and the finish is lo + shl32_mod(high) -> r[16]
DT_OP(truncw, 8, 16, false) {
  const uint32_t bits = rd32(in), off = rd32(in + 4);
  const bool wide = bits > 32;
  TruncW tr;
  truncw_zero(tr);
  f128 lo = make128(0, 0), val = make128(0xDEAD, 0xDEAD);
  if (bits >= 1 && bits <= 64 && in_aux(16ull * off, 16ull * bits, c.aux_len)) {
    for (uint32_t j = 0; j < bits; j++) {
      uint4 v;
      memcpy(&v, c.aux + 16ull * (off + j), 16);
      truncw_mac(tr, v, opaque_u32(1u << (wide ? (j & 31u) : j)));
      if (wide && j + 1 == 32) {
        lo = truncw_value(tr);
        truncw_zero(tr);
      }
    }
    val = truncw_value(tr);
    if (wide) val = add128(lo, shl32_mod(val));
  }
  st(out, val);
}
// form (0 wacc_reduce -> r[16] in the first 16 bytes, 1 wacc_normalize -> 9 columns), pad, col[9] -> 72 bytes
DT_OP(wacc_cols, 80, 72, false) {
  uint64_t col[9], o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < 9; s++) col[s] = rd64(in + 8 + 8 * s);
  if (rd32(in)) {
    t_wacc_normalize(col, o);
  } else {
    uint8_t r[16];
    t_wacc_reduce(col, r);
    o[0] = rd64(r);
    o[1] = rd64(r + 8);
  }
  for (int s = 0; s < 9; s++) wr64(out + 8 * s, o[s]);
}
// u32 x offset, c offset (elements), n, norm_every -> r[16]
DT_OP(wide_dot, 16, 16, false) {
  const uint32_t xo = rd32(in), co = rd32(in + 4), n = rd32(in + 8), norm = rd32(in + 12);
  if (in_aux(16ull * xo, 16ull * n, c.aux_len) && in_aux(16ull * co, 16ull * n, c.aux_len))
    t_wide_dot(c.aux + 16ull * xo, c.aux + 16ull * co, (int)n, (int)norm, out);
  else
    st(out, make128(0xDEAD, 0xDEAD));
}
// c[16], d[16] -> to_limbs26(c)[5], to_limbs26(d)[5], pack_cd26 words[10], unpack_cd26 of them: c[5], d[5]
DT_OP(cd26, 32, 120, false) {
  uint32_t o[30];
  t_cl_to_limbs(in, o);
  t_cl_to_limbs(in + 16, o + 5);
  t_cl_pack(in, in + 16, o + 10);
  t_cl_unpack(o + 10, o + 20, o + 25);
  for (int i = 0; i < 30; i++) wr32(out + 4 * i, o[i]);
}
// u32 x, c, d offsets (elements), n, packed, pad -> even columns[9], odd columns[9]
DT_OP(cl_mac, 24, 144, false) {
  const uint32_t xo = rd32(in), co = rd32(in + 4), dof = rd32(in + 8), n = rd32(in + 12), packed = rd32(in + 16);
  uint64_t e[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (in_aux(16ull * xo, 16ull * n, c.aux_len) && in_aux(16ull * co, 16ull * n, c.aux_len) &&
      in_aux(16ull * dof, 16ull * n, c.aux_len))
    t_cl_mac(c.aux + 16ull * xo, c.aux + 16ull * co, c.aux + 16ull * dof, (int)n, (int)packed, e, o);
  for (int s = 0; s < 9; s++) {
    wr64(out + 8 * s, e[s]);
    wr64(out + 72 + 8 * s, o[s]);
  }
}
// u32 op, pad, a, b -> u64
DT_OP(f64, 24, 8, false) { wr64(out, t_f64((int)rd32(in), rd64(in + 8), rd64(in + 16))); }
// u32 x offset, c offset (u64 elements), n, pad -> u64
DT_OP(wacc64_dot, 16, 8, false) {
  const uint32_t xo = rd32(in), co = rd32(in + 4), n = rd32(in + 8);
  uint64_t r = 0xDEAD;
  if (in_aux(8ull * xo, 8ull * n, c.aux_len) && in_aux(8ull * co, 8ull * n, c.aux_len))  // aux is 8-byte aligned
    r = t_wacc64_dot((const uint64_t*)(c.aux + 8ull * xo), (const uint64_t*)(c.aux + 8ull * co), (int)n);
  wr64(out, r);
}
DT_OP(red192_p64, 24, 8, false) {
  const uint64_t w[3] = {rd64(in), rd64(in + 8), rd64(in + 16)};
  wr64(out, t_reduce192_p64(w));
}
DT_OP(ge64, 8, 4, false) { wr32(out, (uint32_t)t_ge_p64(rd32(in), rd32(in + 4))); }
// u32 n (1 | 5), pad, state[25] -> state[25], samples[5]
DT_OP(sample64, 208, 240, false) {
  uint64_t s[25], o[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 25; i++) s[i] = rd64(in + 8 + 8 * i);
  t_sample64((int)rd32(in), s, o);
  for (int i = 0; i < 25; i++) wr64(out + 8 * i, s[i]);
  for (int i = 0; i < 5; i++) wr64(out + 200 + 8 * i, o[i]);
}
// u32 cnt, slow, flags, pad, state[25] -> state[25], two samples[32], u32 flags, pad
DT_OP(sample2, 216, 240, false) {
  uint64_t s[25];
  for (int i = 0; i < 25; i++) s[i] = rd64(in + 16 + 8 * i);
  uint32_t flags = rd32(in + 8);
  t_sample2_f128(s, rd32(in), (int)rd32(in + 4), out + 200, &flags);
  for (int i = 0; i < 25; i++) wr64(out + 8 * i, s[i]);
  wr32(out + 232, flags);
  wr32(out + 236, 0);
}
// u32 pos (<= 168), n (<= 12), state[25] -> state[25], u32 final pos, pad, 12 elements
DT_OP(bx_sample, 208, 400, false) {
  uint64_t s[25];
  for (int i = 0; i < 25; i++) s[i] = rd64(in + 8 + 8 * i);
  const uint32_t pos = rd32(in), n = rd32(in + 4);
  for (int i = 0; i < 192; i++) out[208 + i] = 0;
  uint32_t end = 0xDEADu;
  if (pos <= 168 && n <= 12) end = t_bx_sample128(s, pos, (int)n, out + 208);
  for (int i = 0; i < 25; i++) wr64(out + 8 * i, s[i]);
  wr32(out + 200, end);
  wr32(out + 204, 0);
}
// u32 n (<= 48), pad, state[25] -> u32 emit calls (| 2^31: out of order), pad, 48 elements (0xA5 past n)
DT_OP(xof_stream, 208, 776, false) {
  uint64_t s[25];
  for (int i = 0; i < 25; i++) s[i] = rd64(in + 8 + 8 * i);
  const uint32_t n = rd32(in);
  wr32(out, n <= 48 ? t_xof_stream128(s, n, out + 8) : 0xDEADu);
  wr32(out + 4, 0);
}
// a, b, c, pad -> xor3, maj3
DT_OP(bitop, 16, 8, false) {
  wr32(out, xor3(rd32(in), rd32(in + 4), rd32(in + 8)));
  wr32(out + 4, maj3(rd32(in), rd32(in + 4), rd32(in + 8)));
}
DT_OP(keccak, 200, 200, false) {
  uint64_t s[25];
  for (int i = 0; i < 25; i++) s[i] = rd64(in + 8 * i);
  t_keccak_p12(s);
  for (int i = 0; i < 25; i++) wr64(out + 8 * i, s[i]);
}
// u32 kind, byte offset, len, pad -> digest[64] (zero filled). kind 0: SHA-256(msg); 1: SHA-512(msg); 2: HMAC-SHA256
// by hmac_pads / sha256_finish64 / hmac_outer, key = aux[off, off + 32), msg = the len (<= 119) bytes after it;
// 3: sha256_16 of aux[off, off + 16); 4: HMAC-SHA512 by hmac_pads_t / hmac_finish_t, the same layout as 2
DT_OP(hash, 16, 64, false) {
  const uint32_t kind = rd32(in), off = rd32(in + 4), len = rd32(in + 8);
  for (int i = 0; i < 64; i++) out[i] = 0;
  const uint8_t* p = c.aux + off;
  if (kind == 0 && in_aux(off, len, c.aux_len)) hash_bytes<HashSha256>(out, p, len);
  if (kind == 1 && in_aux(off, len, c.aux_len)) hash_bytes<HashSha512>(out, p, len);
  if (kind == 2 && len <= 119 && in_aux(off, 32ull + len, c.aux_len)) t_hmac32(p, p + 32, (int)len, out);
  if (kind == 3 && in_aux(off, 16, c.aux_len)) t_sha256_16(p, out);
  if (kind == 4 && in_aux(off, 32ull + len, c.aux_len)) {
    uint64_t ist[8], ost[8];
    hmac_pads_t<HashSha512>(p, 32, ist, ost);
    hmac_finish_t<HashSha512>(out, ist, ost, p + 32, len);
  }
}
DT_OP(shift16, 8, 4, false) { wr32(out, be_word_shift16(rd32(in), rd32(in + 4))); }
// u32 op, pad, a[32], b[32] -> r[32]
DT_OP(fe, 72, 32, false) { t_fe((int)rd32(in), in + 8, in + 40, out); }
// u32 op, pad, a[10], b[10] limbs -> r[10] limbs
DT_OP(fe_limbs, 88, 40, false) {
  uint32_t a[10], b[10], r[10];
  for (int i = 0; i < 10; i++) {
    a[i] = rd32(in + 8 + 4 * i);
    b[i] = rd32(in + 48 + 4 * i);
  }
  t_fe_limbs((int)rd32(in), a, b, r);
  for (int i = 0; i < 10; i++) wr32(out + 4 * i, r[i]);
}
DT_OP(x25519, 64, 32, false) { t_x25519(in, in + 32, out); }
// u32 op, pad, a[32], b[32] (big-endian) -> u32 ok, pad, r[32]
DT_OP(p256_fe, 72, 40, false) {
  for (int i = 0; i < 32; i++) out[8 + i] = 0;
  wr32(out, (uint32_t)t_p256_fe_op((int)rd32(in), in + 8, in + 40, out + 8));
  wr32(out + 4, 0);
}
// pt[65], pad to 72 -> u32 valid
DT_OP(p256_valid, 72, 4, false) { wr32(out, (uint32_t)t_p256_point_valid(in)); }
// sk[32], pt[65], pad to 104 -> u32 ok (both ladders succeeded and agree on x), pad, x || y
DT_OP(p256_mul, 104, 72, false) {
  for (int i = 0; i < 64; i++) out[8 + i] = 0;
  wr32(out, (uint32_t)t_p256_scalar_mul(in, in + 32, out + 8));
  wr32(out + 4, 0);
}
// h[5], m[5] limbs -> h m limbs[5]
DT_OP(pl_mul, 40, 20, false) {
  uint32_t h[5], m[5], r[5];
  for (int i = 0; i < 5; i++) {
    h[i] = rd32(in + 4 * i);
    m[i] = rd32(in + 20 + 4 * i);
  }
  t_pl_mul(h, m, r);
  for (int i = 0; i < 5; i++) wr32(out + 4 * i, r[i]);
}
// key[32], u32 byte offset, len: the serial poly1305_mac of jx_chapoly.h over aux[off, off + len) -> tag[16]
DT_OP(poly1305, 40, 16, false) {
  uint32_t key[8], tag[4] = {0, 0, 0, 0};
  for (int i = 0; i < 8; i++) key[i] = rd32(in + 4 * i);
  const uint32_t off = rd32(in + 32), len = rd32(in + 36);
  const uint8_t* p = c.aux + off;
  if (in_aux(off, len, c.aux_len)) poly1305_mac(key, len, [&](uint64_t i) { return p[i]; }, tag);
  for (int i = 0; i < 4; i++) wr32(out + 4 * i, tag[i]);
}
// u32 form (0 ghash_mul, 1 the 4-bit-table product with h's table), pad, x[16], h[16] -> x h [16]
DT_OP(ghash, 40, 16, false) {
  if (rd32(in) == 0) {
    t_ghash_mul(in + 8, in + 24, out);
    return;
  }
  uint32_t x[4], h[4], tab[16][4];
  for (int i = 0; i < 4; i++) {
    x[i] = bswap32(rd32(in + 8 + 4 * i));
    h[i] = bswap32(rd32(in + 24 + 4 * i));
  }
  for (uint32_t n = 0; n < 16; n++) gl_tab4_entry(n, h, tab[n]);
  ghash_mul_tab4(x, [&](uint32_t n, uint32_t e[4]) {
    for (int k = 0; k < 4; k++) e[k] = tab[n][k];
  });
  for (int i = 0; i < 4; i++) wr32(out + 4 * i, bswap32(x[i]));
}
// u32 otf, pad, key[16], block[16] -> AES-128 of the block by the T-table code, the table in LDS
DT_OP(aes_t, 40, 16, true) { t_aes128_t((int)rd32(in), c.t0, in + 8, in + 24, out); }

// ---- wave-per-case operations: a workgroup of one wave runs one case over DT_WAVE_LDS bytes of dynamic LDS, as a
// wave of shard_prove_kernel runs jx_ntt.h: lane = threadIdx.x, nl = 64, sync = wave_sync. Every branch on the
// record is uniform over the wave. A refused record leaves its output as the harness filled it.
constexpr uint32_t DT_WAVE_LDS = 65536, DT_WAVE_ELEMS = DT_WAVE_LDS / 16;

#define DT_WOP(name, in_bytes, out_bytes)                                                                 \
  struct op_##name {                                                                                      \
    static constexpr uint32_t IN = in_bytes, OUT = out_bytes;                                             \
    static constexpr bool T0 = false, WAVE = true;                                                        \
    static __device__ void run(const uint8_t* in, uint8_t* out, const Ctx& c, f128* lds, uint32_t lane);  \
  };                                                                                                      \
  __device__ void op_##name::run(const uint8_t* in, uint8_t* out, const Ctx& c, f128* lds, uint32_t lane)

// logP (1..10), npairs, table offset, data offset (elements of aux): the table is ntt_build_table's (dt_ntt_table)
struct NttCase {
  uint32_t logP, npairs, P;
  const f128* tab;
  const uint8_t* data;
  bool ok;
};
__device__ inline NttCase ntt_case(const uint8_t* in, const Ctx& c, uint32_t wires, uint32_t lds_per_P) {
  NttCase n = {rd32(in), rd32(in + 4), 0, nullptr, nullptr, false};
  const uint32_t tab_off = rd32(in + 8), data_off = rd32(in + 12);
  if (n.logP < 1 || n.logP > 10 || n.npairs < 1 || n.npairs > 16) return n;
  n.P = 1u << n.logP;
  n.ok = lds_per_P * n.P <= DT_WAVE_ELEMS && in_aux(16ull * tab_off, 16ull * ntt_table_len(n.P), c.aux_len) &&
         in_aux(16ull * data_off, 16ull * wires * n.npairs * n.P, c.aux_len);
  n.tab = reinterpret_cast<const f128*>(c.aux + 16ull * tab_off);  // aux is 16-byte aligned
  n.data = c.aux + 16ull * data_off;
  return n;
}
// ntt_odd_points on one wire of P values -> its P odd-point values (npairs must be 1)
DT_WOP(ntt_odd, 16, 16 * 1024) {
  const NttCase n = ntt_case(in, c, 1, 1);
  if (!n.ok || n.npairs != 1) return;
  const auto sync = [] { wave_sync(); };
  f128* const A = lds;
  for (uint32_t k = lane; k < n.P; k += 64) A[k] = ld(n.data + 16ull * k);
  sync();
  ntt_odd_points(A, n.P, n.tab, lane, 64u, sync);
  for (uint32_t k = lane; k < n.P; k += 64) st(out + 16ull * k, A[k]);
}
// The prove kernel's accumulation over npairs wire pairs (pair i: P values of wire 2i, then P of wire 2i + 1) and
// ntt_gpoly_finish, the wave's LDS laid out A, B, E, O as there -> the 2P coefficients of the gadget polynomial
DT_WOP(ntt_gpoly, 16, 16 * 2048) {
  const NttCase n = ntt_case(in, c, 2, 4);
  if (!n.ok) return;
  const uint32_t P = n.P;
  const auto sync = [] { wave_sync(); };
  f128 *const A = lds, *const B = A + P, *const E = B + P, *const O = E + P;
  for (uint32_t k = lane; k < P; k += 64) E[k] = O[k] = make128(0, 0);
  for (uint32_t i = 0; i < n.npairs; i++) {
    for (uint32_t k = lane; k < P; k += 64) {
      const f128 va = ld(n.data + 16ull * (2ull * i * P + k)), vb = ld(n.data + 16ull * ((2ull * i + 1) * P + k));
      A[k] = va;
      B[k] = vb;
      E[k] = add128(E[k], mont128(va, vb));
    }
    sync();
    ntt_odd_points(A, P, n.tab, lane, 64u, sync);
    ntt_odd_points(B, P, n.tab, lane, 64u, sync);
    for (uint32_t k = lane; k < P; k += 64) O[k] = add128(O[k], mont128(A[k], B[k]));
    sync();
  }
  ntt_gpoly_finish(E, O, P, n.logP, n.tab, lane, 64u, sync, [&](uint32_t j, f128 g) { st(out + 16ull * j, g); });
}

template <class Op>
__global__ void __launch_bounds__(DT_BLOCK) dt_wave_kernel(uint32_t n, const uint8_t* in, uint8_t* out,
                                                           const uint8_t* aux, uint32_t aux_len) {
  extern __shared__ uint4 dt_lds[];
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const Ctx c = {aux, aux_len, nullptr};
  if constexpr (Op::WAVE)
    Op::run(in + (uint64_t)i * Op::IN, out + (uint64_t)i * Op::OUT, c, reinterpret_cast<f128*>(dt_lds), threadIdx.x);
}

template <class Op>
__global__ void __launch_bounds__(DT_BLOCK) dt_kernel(uint32_t n, const uint8_t* in, uint8_t* out, const uint8_t* aux,
                                                      uint32_t aux_len) {
  __shared__ uint32_t t0[256];
  if (Op::T0) {
    for (uint32_t i = threadIdx.x; i < 256; i += DT_BLOCK) t0[i] = aes_t0_entry(AES_SBOX[i]);
    __syncthreads();
  }
  const uint32_t i = blockIdx.x * DT_BLOCK + threadIdx.x;
  if (i >= n) return;  // the last wave runs partly masked
  const Ctx c = {aux, aux_len, t0};
  if constexpr (!Op::WAVE) Op::run(in + (uint64_t)i * Op::IN, out + (uint64_t)i * Op::OUT, c);
}

template <class Op>
int dt_launch(uint32_t n, const void* in, uint32_t in_stride, void* out, uint32_t out_stride, const void* aux,
              uint32_t aux_len) {
  if (in_stride != Op::IN || out_stride != Op::OUT) return -2;
  if (n == 0 || n > (1u << 20)) return -3;
  uint8_t *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
  const size_t in_bytes = (size_t)n * Op::IN, out_bytes = (size_t)n * Op::OUT;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess && aux_len) e = hipMalloc(&d_aux, aux_len);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0xA5, out_bytes);
  if (e == hipSuccess && aux_len) e = hipMemcpy(d_aux, aux, aux_len, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if constexpr (Op::WAVE)
      dt_wave_kernel<Op><<<n, DT_BLOCK, DT_WAVE_LDS>>>(n, d_in, d_out, d_aux, aux_len);
    else
      dt_kernel<Op><<<(n + DT_BLOCK - 1) / DT_BLOCK, DT_BLOCK>>>(n, d_in, d_out, d_aux, aux_len);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_aux) (void)hipFree(d_aux);
  return (int)e;
}

}  // namespace

#define DT_OPS(X)                                                                                                    \
  X(f128) X(red192) X(mont_lazy) X(ge128) X(ge_screen) X(trunc) X(truncw) X(wacc_cols) X(wide_dot) X(cd26) X(cl_mac) X(f64)    \
  X(wacc64_dot) X(red192_p64) X(ge64) X(sample64) X(sample2) X(bx_sample) X(xof_stream) X(bitop) X(keccak) X(hash) X(shift16)     \
  X(fe) X(fe_limbs) X(x25519) X(p256_fe) X(p256_valid) X(p256_mul) X(pl_mul) X(poly1305) X(ghash) X(aes_t)   \
  X(ntt_odd) X(ntt_gpoly)

extern "C" {
// the hash of this file and every header it includes that the build passed in (tests recompute it: stale = rebuild)
// (the "DT_SRC_HASH=" prefix lets the build find the value in the file without loading it)
const char* dt_source_hash(void) { return &("DT_SRC_HASH=" DT_SRC_HASH)[12]; }

// Runs operation `name` on n cases. 0, a HIP error code, -1 for an unknown name, -2 when the strides are not the
// operation's record sizes, -3 for n == 0 or n > 2^20.
int dt_run(const char* name, uint32_t n, const void* in, uint32_t in_stride, void* out, uint32_t out_stride,
           const void* aux, uint32_t aux_len) {
#define DT_DISPATCH(op) \
  if (strcmp(name, #op) == 0) return dt_launch<op_##op>(n, in, in_stride, out, out_stride, aux, aux_len);
  DT_OPS(DT_DISPATCH)
#undef DT_DISPATCH
  return -1;
}
// ntt_build_table(logP), 1 <= logP <= 10, as the kernels read it (Montgomery form): out[16 (3 2^logP + 1)], host
// code, no launch. The wave-per-case transforms take it through aux.
int dt_ntt_table(uint32_t logP, uint8_t* out) {
  if (logP < 1 || logP > 10) return -3;
  f128 tab[3 * 1024 + 1];
  ntt_build_table(logP, tab);
  for (uint32_t i = 0; i < ntt_table_len(1u << logP); i++) {
    memcpy(out + 16 * i, &tab[i].lo, 8);
    memcpy(out + 16 * i + 8, &tab[i].hi, 8);
  }
  return 0;
}
// the record sizes of an operation; 0 for a known name
int dt_sizes(const char* name, uint32_t* in_bytes, uint32_t* out_bytes) {
#define DT_SIZES(op)            \
  if (strcmp(name, #op) == 0) { \
    *in_bytes = op_##op::IN;    \
    *out_bytes = op_##op::OUT;  \
    return 0;                   \
  }
  DT_OPS(DT_SIZES)
#undef DT_SIZES
  return -1;
}
}
