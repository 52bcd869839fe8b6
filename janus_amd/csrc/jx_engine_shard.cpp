// jx_engine_shard.cpp — the client: Prio3.shard (kernels: jx_shard.hip).
#include <cstring>
#include <string>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_field.h"
#include "jx_ntt.h"
#include "jx_shard.h"

using namespace jx;
using namespace jxi;

static_assert(JX_SHARD_MAX_P == jx::SHARD_MAX_P, "the header's cap is the prove kernel's");

namespace {
// Scratch of one launch at most (and at least 64 reports). The two XOF kernels run one report per lane and a
// launch's waves all run the same length, so a launch is as fast with one wave per SIMD as with one per device:
// the budget is what keeps the headline instance's 16,384-report call (133 KB of scratch per report) in one launch.
constexpr uint64_t SHARD_SCRATCH_BUDGET = 4ull << 30;

// the instance as the shard kernels take it; refuses what they do not cover
int32_t shard_args(jx_engine* e, ShardArgs& a) {
  const Cfg& c = e->cfg;
  if (c.algo == ALGO_SUMVEC_F64_MULTIPROOF || c.algo == ALGO_FIXEDPOINT_L2)
    return fail(e, JX_E_UNSUPPORTED,
                "shard: Prio3SumVecField64MultiproofHmacSha256Aes128 (algo id 4) and Prio3FixedPointBoundedL2VecSum "
                "(algo id 5) are not sharded on the device (they need a second XOF and the PolyEval gadget)");
  if (c.P > JX_SHARD_MAX_P)
    return fail(e, JX_E_UNSUPPORTED,
                "shard: the gadget's transform size P = " + std::to_string(c.P) + " exceeds JX_SHARD_MAX_P = " +
                    std::to_string(JX_SHARD_MAX_P));
  memset(&a, 0, sizeof a);
  a.algo = c.algo;
  a.bits = c.bits;
  a.length = c.length;
  a.chunk = c.chunk;
  a.meas_len = c.meas_len;
  a.calls = c.calls;
  a.P = c.P;
  a.logP = c.logP;
  a.gpoly_len = c.gpoly_len;
  a.proof_len = c.proof_len;
  a.arity = c.proof_len - c.gpoly_len;
  a.dst_id = c.dst_id;
  a.ps_bytes = c.ps_bytes;
  a.his_bytes = c.his_bytes;
  a.lis_bytes = c.lis_bytes;
  a.jr = c.jr_len > 0;
  a.rand_bytes = c.seed * (3 + (a.jr ? 2 : 0));
  a.mstride = c.algo == ALGO_SUMVEC ? c.length : 1;
  a.waves = shard_waves(c.algo, c.P, c.chunk);
  return JX_OK;
}

// the transform table of the engine's P, made on the host once per engine
int32_t shard_table(jx_engine* e) {
  const Cfg& c = e->cfg;
  if (e->d_shard_tab || c.algo == ALGO_COUNT) return JX_OK;
  std::vector<f128> t(ntt_table_len(c.P));
  ntt_build_table(c.logP, t.data());
  static_assert(sizeof(f128) == sizeof(uint4), "table entries are 16 bytes");
  uint4* d = nullptr;
  HIPCHK(e, hipMalloc((void**)&d, t.size() * sizeof(f128)));
  // the vector is pageable: the copy has left it when this returns
  const hipError_t st = hipMemcpy(d, t.data(), t.size() * sizeof(f128), hipMemcpyHostToDevice);
  if (st != hipSuccess) {
    (void)hipFree(d);
    HIPCHK(e, st);
  }
  e->d_shard_tab = d;
  return JX_OK;
}

uint64_t shard_chunk(const jx_engine* e, const ShardArgs& a, uint64_t n, uint64_t extra_per_report) {
  uint64_t chunk = SHARD_SCRATCH_BUDGET / (shard_scratch_bytes(a) + extra_per_report);
  if (chunk < 64) chunk = 64;
  if (e->shard_chunk) chunk = e->shard_chunk;  // debug option 10
  return chunk < n ? chunk : n;
}
// the scratch of a launch of m reports: the next regions of `cv` (sized only when cv has no base)
void shard_scratch(ShardArgs& a, Carver& cv, uint64_t m) {
  cv.take(a.status, m);
  cv.take(a.hmeas, 16 * m * a.meas_len);
  cv.take(a.prand, 16 * m * a.arity);
  cv.take(a.cpow, 16 * m * a.P);
  cv.take(a.rjr, 16 * m);
}

// the launches of n reports, `chunk` at a time, over the one scratch region `a` names (shard_scratch)
int32_t shard_launches(jx_engine* e, ShardArgs a, uint64_t n, uint64_t chunk, uint8_t* d_out_status) {
  a.tab = e->d_shard_tab;
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = n - off < chunk ? n - off : chunk;
    a.n = m;
    HIPCHK(e, launch_shard(a, e->stream));
    if (d_out_status) HIPCHK(e, hipMemcpyAsync(d_out_status + off, a.status, m, hipMemcpyDeviceToDevice, e->stream));
    a.meas += m * a.mstride;
    a.nonces += m * 16;
    a.rands += m * a.rand_bytes;
    if (a.ps) a.ps += m * a.ps_bytes;
    a.lis += m * a.lis_stride;
    a.his += m * a.his_bytes;
  }
  return JX_OK;
}
}  // namespace

extern "C" {

int32_t jx_client_rand_bytes(const jx_engine* e, uint32_t* bytes) {
  if (!e) return JX_E_INVALID;
  if (bytes) *bytes = e->cfg.seed * (3 + (e->cfg.jr_len ? 2 : 0));
  return JX_OK;
}

int32_t jx_client_shard_device(jx_engine* e, uint64_t n, const void* d_measurements, const void* d_nonces,
                               const void* d_rands, void* d_out_public_shares, void* d_out_leader_input_shares,
                               uint64_t lis_stride, void* d_out_helper_input_shares, void* d_out_status) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  ShardArgs a;
  if (const int32_t rc = shard_args(e, a)) return rc;
  if (n == 0) return JX_OK;
  if (!d_measurements || !d_nonces || !d_rands || !d_out_leader_input_shares || !d_out_helper_input_shares ||
      (a.ps_bytes && !d_out_public_shares))
    return JX_E_INVALID;
  if (const int32_t rc = lis_stride_ok(e, &lis_stride, "shard")) return rc;
  if ((reinterpret_cast<uintptr_t>(d_out_leader_input_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_measurements) & 7u) ||
      ((reinterpret_cast<uintptr_t>(d_nonces) | reinterpret_cast<uintptr_t>(d_rands) |
        reinterpret_cast<uintptr_t>(d_out_public_shares) | reinterpret_cast<uintptr_t>(d_out_helper_input_shares)) & 3u))
    return fail(e, JX_E_INVALID,
                "shard: the leader input share rows must be 16-byte aligned, the measurements 8-byte, the rest 4-byte");
  HIPCHK(e, hipSetDevice(e->device));
  if (const int32_t rc = shard_table(e)) return rc;
  a.lis_stride = lis_stride;
  a.meas = (const uint64_t*)d_measurements;
  a.nonces = (const uint8_t*)d_nonces;
  a.rands = (const uint8_t*)d_rands;
  a.ps = (uint8_t*)d_out_public_shares;
  a.lis = (uint8_t*)d_out_leader_input_shares;
  a.his = (uint8_t*)d_out_helper_input_shares;
  const uint64_t chunk = shard_chunk(e, a, n, 0);
  auto lay = [&](void* base) {
    Carver cv(base);
    shard_scratch(a, cv, chunk);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  return shard_launches(e, a, n, chunk, (uint8_t*)d_out_status);
}

int32_t jx_client_shard_batch(jx_engine* e, uint64_t n, const uint64_t* measurements, const uint8_t* nonces,
                              const uint8_t* rands, uint8_t* out_public_shares, uint8_t* out_leader_input_shares,
                              uint8_t* out_helper_input_shares, uint8_t* out_status) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  ShardArgs a;
  if (const int32_t rc = shard_args(e, a)) return rc;
  if (n == 0) return JX_OK;
  if (!measurements || !nonces || !rands || !out_leader_input_shares || !out_helper_input_shares ||
      (a.ps_bytes && !out_public_shares))
    return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  if (const int32_t rc = shard_table(e)) return rc;
  a.lis_stride = a.lis_bytes;  // a multiple of 16 for every Field128 instance; Prio3Count's 48 too
  const uint64_t mrow = 8ull * a.mstride;
  const uint64_t io = mrow + 16 + a.rand_bytes + a.ps_bytes + a.lis_stride + a.his_bytes + 6 * 256;
  const uint64_t chunk = shard_chunk(e, a, n, io);
  // the I/O regions of one launch, then its scratch; the launches read and write them in place (a's pointers)
  uint64_t* d_meas = nullptr;
  uint8_t *d_non = nullptr, *d_rand = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_meas, chunk * mrow);
    cv.take(d_non, chunk * 16);
    cv.take(d_rand, chunk * a.rand_bytes);
    cv.take(a.ps, chunk * a.ps_bytes + 1);
    cv.take(a.lis, chunk * a.lis_stride);
    cv.take(a.his, chunk * a.his_bytes);
    shard_scratch(a, cv, chunk);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  a.meas = d_meas;
  a.nonces = d_non;
  a.rands = d_rand;
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = n - off < chunk ? n - off : chunk;
    HIPCHK(e, hipMemcpyAsync(d_meas, measurements + off * a.mstride, m * mrow, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_non, nonces + off * 16, m * 16, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_rand, rands + off * a.rand_bytes, m * a.rand_bytes, hipMemcpyHostToDevice, e->stream));
    if (const int32_t rc = shard_launches(e, a, m, chunk, nullptr)) return rc;
    if (a.ps_bytes)
      HIPCHK(e, hipMemcpyAsync(out_public_shares + off * a.ps_bytes, a.ps, m * a.ps_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_leader_input_shares + off * a.lis_bytes, a.lis, m * a.lis_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_helper_input_shares + off * a.his_bytes, a.his, m * a.his_bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_status) HIPCHK(e, hipMemcpyAsync(out_status + off, a.status, m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  return JX_OK;
}

}  // extern "C"
