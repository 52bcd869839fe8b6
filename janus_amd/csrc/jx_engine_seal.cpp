// jx_engine_seal.cpp — the client's second half: seal both shares of the reports jx_client_shard_* wrote (kernels:
// jx_hpke_seal.hip).
#include <cstring>
#include <string>

#include "jx_engine_internal.h"
#include "jx_hpke_seal.h"

using namespace jx;
using namespace jxi;

namespace {
// Reports per launch: a launch's scratch is 136 bytes per report, so this only bounds the grid.
constexpr uint64_t SEAL_CHUNK = 1ull << 20;

uint64_t seal_chunk(const jx_engine* e, uint64_t n) {
  const uint64_t chunk = e->seal_chunk ? e->seal_chunk : SEAL_CHUNK;  // debug option 11
  return chunk < n ? chunk : n;
}

// what both calls check before anything is queued; the launch arguments that do not move between launches
int32_t seal_args(jx_engine* e, const uint8_t task_id[32], jx_hpke* leader, jx_hpke* helper, uint64_t lis_stride,
                  ClientSealArgs& a) {
  const Cfg& c = e->cfg;
  for (jx_hpke* h : {leader, helper}) {
    if (!h || hpke_device(h) != e->device)
      return fail(e, JX_E_INVALID, "client seal: both recipients must be HPKE contexts on the engine's device");
    if (hpke_enc_len(h) != 32)
      return fail(e, JX_E_UNSUPPORTED, "client seal: sealing under KEM 0x0010 (P-256) is out of scope");
  }
  if (lis_stride < c.lis_bytes) return fail(e, JX_E_INVALID, "client seal: the row stride must be 0, or >= the leader input share");
  memset(&a, 0, sizeof a);
  uint32_t cap = 0;
  hpke_registry(e->device, &a.keys, &cap);
  a.slot_leader = hpke_slot(leader);
  a.slot_helper = hpke_slot(helper);
  a.ps_bytes = c.ps_bytes;
  a.his_bytes = c.his_bytes;
  a.lis_bytes = c.lis_bytes;
  a.lis_stride = lis_stride;
  memcpy(a.task_id, task_id, 32);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, a.zero_ist, a.zero_ost);
  return JX_OK;
}

// the launches of n reports, `chunk` at a time, over the one scratch region (context rows and times) of a launch:
// a launch's times are copied in after the launch before it, in stream order
int32_t seal_launches(jx_engine* e, ClientSealArgs a, uint64_t n, uint64_t chunk, const uint64_t* times,
                      uint64_t* d_times) {
  const uint64_t lct = sealed_lis_bytes(e->cfg), hct = sealed_his_bytes(e->cfg);
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = n - off < chunk ? n - off : chunk;
    a.n = m;
    a.times = d_times;
    HIPCHK(e, hipMemcpyAsync(d_times, times + off, m * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, launch_client_seal(a, e->stream));
    a.ids += m * 16;
    if (a.ps) a.ps += m * a.ps_bytes;
    a.lis += m * a.lis_stride;
    a.his += m * a.his_bytes;
    a.sks += m * 64;
    if (a.shard_status) a.shard_status += m;
    a.leader_encs += m * 32;
    a.leader_cts += m * lct;
    a.helper_encs += m * 32;
    a.helper_cts += m * hct;
    a.status += m;
  }
  return JX_OK;
}
}  // namespace

extern "C" {

int32_t jx_client_seal_sizes(const jx_engine* e, uint32_t* leader_ct_len, uint32_t* helper_ct_len) {
  if (!e) return JX_E_INVALID;
  if (leader_ct_len) *leader_ct_len = (uint32_t)sealed_lis_bytes(e->cfg);
  if (helper_ct_len) *helper_ct_len = (uint32_t)sealed_his_bytes(e->cfg);
  return JX_OK;
}

int32_t jx_client_seal_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                              const void* d_public_shares, const void* d_leader_input_shares, uint64_t lis_stride,
                              const void* d_helper_input_shares, const uint8_t task_id[32], jx_hpke* leader,
                              jx_hpke* helper, const void* d_ephemeral_sks, const void* d_shard_status,
                              void* d_out_leader_encs, void* d_out_leader_cts, void* d_out_helper_encs,
                              void* d_out_helper_cts, void* d_out_status) {
  if (!e || !task_id) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (lis_stride == 0) lis_stride = c.lis_bytes;
  ClientSealArgs a;
  if (const int32_t rc = seal_args(e, task_id, leader, helper, lis_stride, a)) return rc;
  if (n == 0) return JX_OK;
  if (!d_report_ids || !times || !d_leader_input_shares || !d_helper_input_shares || !d_ephemeral_sks ||
      !d_out_leader_encs || !d_out_leader_cts || !d_out_helper_encs || !d_out_helper_cts || !d_out_status ||
      (c.ps_bytes && !d_public_shares))
    return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  a.ids = (const uint8_t*)d_report_ids;
  a.ps = (const uint8_t*)d_public_shares;
  a.lis = (const uint8_t*)d_leader_input_shares;
  a.his = (const uint8_t*)d_helper_input_shares;
  a.sks = (const uint8_t*)d_ephemeral_sks;
  a.shard_status = (const uint8_t*)d_shard_status;
  a.leader_encs = (uint8_t*)d_out_leader_encs;
  a.leader_cts = (uint8_t*)d_out_leader_cts;
  a.helper_encs = (uint8_t*)d_out_helper_encs;
  a.helper_cts = (uint8_t*)d_out_helper_cts;
  a.status = (uint8_t*)d_out_status;
  const uint64_t chunk = seal_chunk(e, n);
  uint64_t* d_times = nullptr;
  uint8_t* d_ctx = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_ctx, chunk * CLIENT_SEAL_CTX_BYTES);
    cv.take(d_times, chunk * 8);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  a.ctx = d_ctx;
  if (const int32_t rc = seal_launches(e, a, n, chunk, times, d_times)) return rc;
  // the times leave pageable host memory before the call returns; the launches themselves stay queued
  HIPCHK(e, wait_uploads(e));
  return JX_OK;
}

int32_t jx_client_seal_batch(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                             const uint8_t* public_shares, const uint8_t* leader_input_shares, uint64_t lis_stride,
                             const uint8_t* helper_input_shares, const uint8_t task_id[32], jx_hpke* leader,
                             jx_hpke* helper, const uint8_t* ephemeral_sks, const uint8_t* shard_status,
                             uint8_t* out_leader_encs, uint8_t* out_leader_cts, uint8_t* out_helper_encs,
                             uint8_t* out_helper_cts, uint8_t* out_status) {
  if (!e || !task_id) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (lis_stride == 0) lis_stride = c.lis_bytes;
  ClientSealArgs a;
  if (const int32_t rc = seal_args(e, task_id, leader, helper, lis_stride, a)) return rc;
  if (n == 0) return JX_OK;
  if (!report_ids || !times || !leader_input_shares || !helper_input_shares || !ephemeral_sks || !out_leader_encs ||
      !out_leader_cts || !out_helper_encs || !out_helper_cts || !out_status || (c.ps_bytes && !public_shares))
    return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t dev_stride = (c.lis_bytes + 15u) & ~15ull;  // the device rows; the caller's are lis_stride apart
  a.lis_stride = dev_stride;
  const uint64_t lct = sealed_lis_bytes(c), hct = sealed_his_bytes(c);
  const uint64_t chunk = seal_chunk(e, n);
  uint64_t* d_times = nullptr;
  uint8_t *d_ctx = nullptr, *d_ids = nullptr, *d_ps = nullptr, *d_lis = nullptr, *d_his = nullptr, *d_sks = nullptr,
          *d_ss = nullptr, *d_lenc = nullptr, *d_lct = nullptr, *d_henc = nullptr, *d_hct = nullptr, *d_st = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_ctx, chunk * CLIENT_SEAL_CTX_BYTES);
    cv.take(d_times, chunk * 8);
    cv.take(d_ids, chunk * 16);
    cv.take(d_ps, chunk * c.ps_bytes);
    cv.take(d_lis, chunk * dev_stride);
    cv.take(d_his, chunk * c.his_bytes);
    cv.take(d_sks, chunk * 64);
    cv.take(d_ss, chunk);
    cv.take(d_lenc, chunk * 32);
    cv.take(d_lct, chunk * lct);
    cv.take(d_henc, chunk * 32);
    cv.take(d_hct, chunk * hct);
    cv.take(d_st, chunk);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  a.ctx = d_ctx;
  a.ids = d_ids;
  a.ps = c.ps_bytes ? d_ps : nullptr;
  a.lis = d_lis;
  a.his = d_his;
  a.sks = d_sks;
  a.shard_status = shard_status ? d_ss : nullptr;
  a.leader_encs = d_lenc;
  a.leader_cts = d_lct;
  a.helper_encs = d_henc;
  a.helper_cts = d_hct;
  a.status = d_st;
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = n - off < chunk ? n - off : chunk;
    HIPCHK(e, hipMemcpyAsync(d_ids, report_ids + off * 16, m * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes)
      HIPCHK(e, hipMemcpyAsync(d_ps, public_shares + off * c.ps_bytes, m * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpy2DAsync(d_lis, dev_stride, leader_input_shares + off * lis_stride, lis_stride, c.lis_bytes, m,
                               hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_his, helper_input_shares + off * c.his_bytes, m * c.his_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_sks, ephemeral_sks + off * 64, m * 64, hipMemcpyHostToDevice, e->stream));
    if (shard_status) HIPCHK(e, hipMemcpyAsync(d_ss, shard_status + off, m, hipMemcpyHostToDevice, e->stream));
    if (const int32_t rc = seal_launches(e, a, m, chunk, times + off, d_times)) return rc;
    HIPCHK(e, hipMemcpyAsync(out_leader_encs + off * 32, d_lenc, m * 32, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_leader_cts + off * lct, d_lct, m * lct, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_helper_encs + off * 32, d_henc, m * 32, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_helper_cts + off * hct, d_hct, m * hct, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_status + off, d_st, m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  return JX_OK;
}

}  // extern "C"
