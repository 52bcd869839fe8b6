// jx_engine_wire_upload.cpp — the upload message in and out: jx_report_encode* writes the client's Report bodies from
// the rows the seal left on the device, jx_upload_decode* cuts the leader's uploads into the arrays the upload open and
// the request encode read (the rule: jx_wire.h; the kernels: jx_wire_upload.hip). Each call is two phases with one
// host round trip between them, because the packed sizes are the first phase's results: the decode reads m and the
// four totals, the encode the bodies' length, which it must compare with the capacity before a byte is written.
#include <cstring>
#include <new>
#include <string>

#include "jx_engine_internal.h"
#include "jx_wire.h"

using namespace jx;
using namespace jxi;

static_assert(JX_UPLOAD_OK == UPLOAD_OK && JX_UPLOAD_MALFORMED == UPLOAD_MALFORMED && JX_UPLOAD_TOO_EARLY == UPLOAD_TOO_EARLY &&
                  JX_UPLOAD_TASK_EXPIRED == UPLOAD_TASK_EXPIRED && JX_UPLOAD_EXPIRED == UPLOAD_EXPIRED &&
                  JX_UPLOAD_ODD_PUBLIC_SHARE == UPLOAD_ODD_PUBLIC_SHARE && JX_UPLOAD_NO_ROW == UPLOAD_NO_ROW,
              "the header's code points are the rule's");

struct jx_upload_req {
  jx_engine* e = nullptr;
  jx_upload_req_info_t info{};
  jx_upload_req_arrays_t arr{};
  Mirror arrays;  // the arrays with a pinned copy, then the dense ids and public-share rows
  Slab packed;    // the four packed fields
};

namespace {

void upload_req_free(jx_upload_req* r) {
  if (!r) return;
  jx_engine* e = r->e;
  r->arrays.put(e);
  if (r->packed.p) arena_put(e->arena, r->packed, e->stream);
  r->arrays.free(e);
  delete r;
}
using UploadReqGuard = HandleGuard<jx_upload_req, upload_req_free>;

// Waves per report for m reports of `bytes` together: one, unless so few reports with such long fields that one wave
// each would leave most of the device without work; then slices of at least 4 KiB, up to about 8192 waves in all.
uint32_t copy_parts(const jx_engine* e, uint64_t m, uint64_t bytes) {
  uint64_t parts = e->upload_parts;
  if (parts == 0) {
    parts = 1;
    if (m && m < 8192) {
      const uint64_t by_count = 8192 / m, by_size = bytes / m / 4096;
      parts = by_count < by_size ? by_count : by_size;
      if (parts < 1) parts = 1;
      if (parts > 64) parts = 64;
    }
  }
  if (m * parts >= 0x7FFFFFFFull) parts = 1;  // the grid: four waves per workgroup
  return (uint32_t)parts;
}

bool decode_args_ok(jx_engine* e, const void* bodies, uint64_t len, uint64_t n, const uint64_t* body_offsets,
                    const jx_upload_checks* checks, const uint8_t* k0, const uint8_t* k1, jx_upload_req** out) {
  return e && out && (bodies || len == 0) && (body_offsets || n == 0) && checks && k0 && k1;
}

// what is refused from the host array alone, with nothing queued
int32_t offsets_check(jx_engine* e, uint64_t len, uint64_t n, const uint64_t* body_offsets) {
  if (const int32_t rc = call_count_ok(e, n, "upload decode", "uploads")) return rc;
  for (uint64_t i = 0; i < n; i++)
    if (body_offsets[i + 1] < body_offsets[i]) return fail(e, JX_E_INVALID, "upload decode: body_offsets must not decrease");
  if (n && body_offsets[n] > len) return fail(e, JX_E_INVALID, "upload decode: a body offset lies past the bodies' length");
  return JX_OK;
}

// the bodies are on the device, readable by work queued on the engine stream; the engine mutex is held
int32_t decode_core(jx_engine* e, const uint8_t* d_bodies, uint64_t n, const uint64_t* body_offsets,
                    const jx_upload_checks* checks, const uint8_t* key_first, const uint8_t* key_second,
                    jx_upload_req** out) {
  const Cfg& c = e->cfg;
  UploadReqGuard g{new (std::nothrow) jx_upload_req};
  if (!g.r) return fail(e, JX_E_NOMEM, "upload decode: out of host memory");
  jx_upload_req* r = g.r;
  r->e = e;
  r->info.n = n;
  if (n == 0) {
    *out = g.give();
    return JX_OK;
  }
  WireUploadArgs a{};
  // the handle's arrays: sized by n, of which the dense ones use m
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(a.times_all, n * 8);
    cv.take(a.times, n * 8);
    for (int f = 0; f < 4; f++) cv.take(a.offs[f], (n + 1) * 8);
    cv.take(a.index, n * 4);
    cv.take(a.row_of, n * 4);
    cv.take(a.ids_all, n * 16);
    cv.take(a.key_index, n * 2);
    cv.take(a.config_ids, n);
    cv.take(a.status, n);
    r->arrays.host_bytes = cv.mark();  // up to here: one copy to the pinned buffer
    cv.take(a.ids, n * 16);
    cv.take(a.ps, n * c.ps_bytes);
    return cv.bytes();
  };
  if (const int32_t rc = slab_carve(e, r->arrays.slab, lay, "upload arrays")) return rc;
  // the call's own scratch
  uint64_t* d_boff = nullptr;
  uint8_t* d_keys = nullptr;
  auto lays = [&](void* base) {
    Carver cv(base);
    cv.take(d_boff, (n + 1) * 8);
    cv.take(d_keys, 512);
    cv.take(a.recs, n * sizeof(WireReportRec));
    cv.take(a.rank, (n + 1) * 8);
    for (int f = 0; f < 4; f++) cv.take(a.scan[f], (n + 1) * 8);
    cv.take(a.totals, sizeof(WireUploadTotals));
    return cv.bytes();
  };
  Scratch mem;
  if (const int32_t rc = scratch_carve(e, mem, lays)) return rc;
  uint8_t keys[512];
  memcpy(keys, key_first, 256);
  memcpy(keys + 256, key_second, 256);
  HIPCHK(e, hipMemcpyAsync(d_boff, body_offsets, (n + 1) * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(d_keys, keys, 512, hipMemcpyHostToDevice, e->stream));
  a.n = n;
  a.body = d_bodies;
  a.body_offsets = d_boff;
  a.ps_bytes = c.ps_bytes;
  a.checks.now = checks->now;
  a.checks.skew = checks->tolerable_clock_skew;
  a.checks.has_task_expiration = checks->has_task_expiration != 0;
  a.checks.task_expiration = checks->task_expiration;
  a.checks.has_report_expiry_age = checks->has_report_expiry_age != 0;
  a.checks.report_expiry_age = checks->report_expiry_age;
  a.key_first = d_keys;
  a.key_second = d_keys + 256;
  // ---- phase 1: parse, scan, compaction; the one round trip
  HIPCHK(e, launch_wire_upload_sizes(a, e->stream));
  WireUploadTotals t{};
  HIPCHK(e, hipMemcpyAsync(&t, a.totals, sizeof t, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the two host arrays have been read too
  // ---- phase 2: the copy into the dense rows and the packed arrays, and the pinned copy of the small ones
  auto layp = [&](void* base) {
    Carver cv(base);
    cv.take(a.packed[0], t.lenc_bytes);
    cv.take(a.packed[1], t.lpay_bytes);
    cv.take(a.packed[2], t.henc_bytes);
    cv.take(a.packed[3], t.hpay_bytes);
    return cv.bytes();
  };
  if (const int32_t rc = slab_carve(e, r->packed, layp, "upload ciphertexts")) return rc;
  const uint64_t m = t.m;
  const uint64_t field_bytes = t.lenc_bytes + t.lpay_bytes + t.henc_bytes + t.hpay_bytes;
  HIPCHK(e, launch_wire_upload_gather(a, m, copy_parts(e, m, field_bytes), e->stream));
  if (const int32_t rc = r->arrays.download(e)) return rc;
  const Mirror& M = r->arrays;
  jx_upload_req_arrays_t& A = r->arr;
  A.d_index = a.index;
  A.d_report_ids = a.ids;
  A.d_times = a.times;
  A.d_public_shares = c.ps_bytes ? a.ps : nullptr;
  A.d_key_index = a.key_index;
  A.d_leader_encs = a.packed[0];
  A.d_leader_enc_offsets = a.offs[0];
  A.d_leader_payloads = a.packed[1];
  A.d_leader_payload_offsets = a.offs[1];
  A.d_helper_config_ids = a.config_ids;
  A.d_helper_encs = a.packed[2];
  A.d_helper_enc_offsets = a.offs[2];
  A.d_helper_payloads = a.packed[3];
  A.d_helper_payload_offsets = a.offs[3];
  A.d_all_report_ids = a.ids_all;
  A.d_all_times = a.times_all;
  A.d_upload_status = a.status;
  A.d_row_of = a.row_of;
  A.index = M.host_of(a.index);
  A.times = M.host_of(a.times);
  A.key_index = M.host_of(a.key_index);
  A.leader_enc_offsets = M.host_of(a.offs[0]);
  A.leader_payload_offsets = M.host_of(a.offs[1]);
  A.helper_enc_offsets = M.host_of(a.offs[2]);
  A.helper_payload_offsets = M.host_of(a.offs[3]);
  A.helper_config_ids = M.host_of(a.config_ids);
  A.all_report_ids = M.host_of(a.ids_all);
  A.all_times = M.host_of(a.times_all);
  A.upload_status = M.host_of(a.status);
  A.row_of = M.host_of(a.row_of);
  jx_upload_req_info_t& info = r->info;
  info.m = m;
  info.leader_enc_bytes = t.lenc_bytes;
  info.leader_payload_bytes = t.lpay_bytes;
  info.helper_enc_bytes = t.henc_bytes;
  info.helper_payload_bytes = t.hpay_bytes;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t st = A.upload_status[i];
    if (st < 6) info.status_count[st]++;
  }
  *out = g.give();
  return JX_OK;
}

// ---- the client's encode
struct ReportIn {
  uint64_t n;
  const uint8_t *ids, *ps, *lencs, *lcts, *hencs, *hcts, *status;  // device pointers by the time the core runs
  const uint64_t* times;                                           // host
  uint32_t lenc_len, henc_len;
  uint8_t leader_config_id, helper_config_id;
};

int32_t report_check(jx_engine* e, const ReportIn& in, uint64_t* bound) {
  const Cfg& c = e->cfg;
  if (in.lenc_len >= (1u << 16) || in.henc_len >= (1u << 16))
    return fail(e, JX_E_INVALID, "report encode: an encapsulated key of 2^16 bytes or more");
  if (const int32_t rc = call_count_ok(e, in.n, "report encode", "reports")) return rc;
  if (in.n && (!in.ids || !in.times || !in.lcts || !in.hcts || (c.ps_bytes && !in.ps) || (in.lenc_len && !in.lencs) ||
               (in.henc_len && !in.hencs)))
    return JX_E_INVALID;
  *bound = in.n * wire_report_len(c.ps_bytes, in.lenc_len, sealed_lis_bytes(c), in.henc_len, sealed_his_bytes(c));
  return JX_OK;
}

// the engine mutex is held; d_out holds `capacity` bytes; d_offsets_out (nullable, device) and offsets_out (nullable,
// host) take the n + 1 offsets
int32_t report_encode_core(jx_engine* e, const ReportIn& in, uint8_t* d_out, uint64_t capacity, uint64_t* d_offsets_out,
                           uint64_t* offsets_out, uint64_t* out_len, bool may_wait) {
  const Cfg& c = e->cfg;
  const uint64_t n = in.n;
  WireReportArgs a{};
  uint64_t* d_times = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_times, n * 8);
    cv.take(a.offsets, (n + 1) * 8);
    cv.take(a.rank, (n + 1) * 8);
    cv.take(a.index, n * 4);
    cv.take(a.totals, sizeof(WireReportTotals));
    return cv.bytes();
  };
  Scratch mem;
  if (const int32_t rc = scratch_carve(e, mem, lay, may_wait)) return rc;
  if (n) HIPCHK(e, hipMemcpyAsync(d_times, in.times, n * 8, hipMemcpyHostToDevice, e->stream));
  a.n = n;
  a.ids = in.ids;
  a.ps = in.ps;
  a.lencs = in.lencs;
  a.lcts = in.lcts;
  a.hencs = in.hencs;
  a.hcts = in.hcts;
  a.times = d_times;
  a.status = in.status;
  a.ps_bytes = c.ps_bytes;
  a.lenc_len = in.lenc_len;
  a.lct_len = (uint32_t)sealed_lis_bytes(c);
  a.henc_len = in.henc_len;
  a.hct_len = (uint32_t)sealed_his_bytes(c);
  a.leader_config_id = in.leader_config_id;
  a.helper_config_id = in.helper_config_id;
  a.out = d_out;
  HIPCHK(e, launch_wire_report_sizes(a, e->stream));
  WireReportTotals t{};
  HIPCHK(e, hipMemcpyAsync(&t, a.totals, sizeof t, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (capacity < t.bytes) return fail(e, JX_E_INVALID, "report encode: the output buffer is shorter than the report bodies");
  HIPCHK(e, launch_wire_report_pack(a, t.m, copy_parts(e, t.m, t.bytes), e->stream));
  if (d_offsets_out)
    HIPCHK(e, hipMemcpyAsync(d_offsets_out, a.offsets, (n + 1) * 8, hipMemcpyDeviceToDevice, e->stream));
  if (offsets_out) HIPCHK(e, hipMemcpyAsync(offsets_out, a.offsets, (n + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *out_len = t.bytes;
  return JX_OK;
}

}  // namespace

extern "C" {

int32_t jx_upload_decode_device(jx_engine* e, const void* d_bodies, uint64_t len, uint64_t n, const uint64_t* body_offsets,
                                const jx_upload_checks* checks, const uint8_t key_first[256],
                                const uint8_t key_second[256], jx_upload_req** out) {
  if (!decode_args_ok(e, d_bodies, len, n, body_offsets, checks, key_first, key_second, out)) return JX_E_INVALID;
  *out = nullptr;
  LOCK(e);
  if (const int32_t rc = offsets_check(e, len, n, body_offsets)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  return decode_core(e, (const uint8_t*)d_bodies, n, body_offsets, checks, key_first, key_second, out);
}

int32_t jx_upload_decode(jx_engine* e, const uint8_t* bodies, uint64_t len, uint64_t n, const uint64_t* body_offsets,
                         const jx_upload_checks* checks, const uint8_t key_first[256], const uint8_t key_second[256],
                         jx_upload_req** out) {
  if (!decode_args_ok(e, bodies, len, n, body_offsets, checks, key_first, key_second, out)) return JX_E_INVALID;
  *out = nullptr;
  LOCK(e);
  if (const int32_t rc = offsets_check(e, len, n, body_offsets)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  Scratch mem;  // the bodies' one copy to the device; the call holds nothing else yet: it may wait for the arena
  if (const int32_t rc = scratch_get(e, len ? len : 1, mem, true)) return rc;
  if (len) HIPCHK(e, hipMemcpyAsync(mem.p(), bodies, len, hipMemcpyHostToDevice, e->stream));
  return decode_core(e, mem.p(), n, body_offsets, checks, key_first, key_second, out);
}

int32_t jx_upload_req_info(const jx_upload_req* r, jx_upload_req_info_t* out) {
  if (!r || !out) return JX_E_INVALID;
  *out = r->info;
  return JX_OK;
}

int32_t jx_upload_req_arrays(const jx_upload_req* r, jx_upload_req_arrays_t* out) {
  if (!r || !out) return JX_E_INVALID;
  *out = r->arr;  // all null for a call of no uploads
  return JX_OK;
}

void jx_upload_req_release(jx_upload_req* r) { handle_release(r, upload_req_free); }

int32_t jx_report_encode_bound(const jx_engine* e, uint64_t n, uint32_t leader_enc_len, uint32_t helper_enc_len,
                               uint64_t* out_bound) {
  if (!e || !out_bound || leader_enc_len >= (1u << 16) || helper_enc_len >= (1u << 16) || !call_count_fits(n))
    return JX_E_INVALID;
  *out_bound = n * wire_report_len(e->cfg.ps_bytes, leader_enc_len, sealed_lis_bytes(e->cfg), helper_enc_len,
                                   sealed_his_bytes(e->cfg));
  return JX_OK;
}

int32_t jx_report_encode_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                const void* d_public_shares, const void* d_leader_encs, uint32_t leader_enc_len,
                                const void* d_leader_cts, const void* d_helper_encs, uint32_t helper_enc_len,
                                const void* d_helper_cts, uint8_t leader_config_id, uint8_t helper_config_id,
                                const void* d_seal_status, void* d_out, uint64_t capacity, void* d_out_offsets,
                                uint64_t* out_offsets, uint64_t* out_len) {
  if (!e || !out_len || (!d_out && capacity)) return JX_E_INVALID;
  LOCK(e);
  const ReportIn in{n, (const uint8_t*)d_report_ids, (const uint8_t*)d_public_shares, (const uint8_t*)d_leader_encs,
                    (const uint8_t*)d_leader_cts, (const uint8_t*)d_helper_encs, (const uint8_t*)d_helper_cts,
                    (const uint8_t*)d_seal_status, times, leader_enc_len, helper_enc_len, leader_config_id, helper_config_id};
  uint64_t bound = 0;
  if (const int32_t rc = report_check(e, in, &bound)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  return report_encode_core(e, in, (uint8_t*)d_out, capacity, (uint64_t*)d_out_offsets, out_offsets, out_len, true);
}

int32_t jx_report_encode(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                         const uint8_t* public_shares, const uint8_t* leader_encs, uint32_t leader_enc_len,
                         const uint8_t* leader_cts, const uint8_t* helper_encs, uint32_t helper_enc_len,
                         const uint8_t* helper_cts, uint8_t leader_config_id, uint8_t helper_config_id,
                         const uint8_t* seal_status, uint8_t* out, uint64_t capacity, uint64_t* out_offsets,
                         uint64_t* out_len) {
  if (!e || !out_len || (!out && capacity)) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  ReportIn in{n, report_ids, public_shares, leader_encs, leader_cts, helper_encs, helper_cts, seal_status, times,
              leader_enc_len, helper_enc_len, leader_config_id, helper_config_id};
  uint64_t bound = 0;
  if (const int32_t rc = report_check(e, in, &bound)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t lct = sealed_lis_bytes(c), hct = sealed_his_bytes(c);
  uint8_t *d_ids = nullptr, *d_ps = nullptr, *d_le = nullptr, *d_lc = nullptr, *d_he = nullptr, *d_hc = nullptr,
          *d_st = nullptr, *d_body = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_ids, n * 16);
    cv.take(d_ps, n * c.ps_bytes);
    cv.take(d_le, n * leader_enc_len);
    cv.take(d_lc, n * lct);
    cv.take(d_he, n * helper_enc_len);
    cv.take(d_hc, n * hct);
    cv.take(d_st, n);
    cv.take(d_body, bound);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else yet: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  if (n) {
    HIPCHK(e, hipMemcpyAsync(d_ids, report_ids, n * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    if (leader_enc_len) HIPCHK(e, hipMemcpyAsync(d_le, leader_encs, n * leader_enc_len, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_lc, leader_cts, n * lct, hipMemcpyHostToDevice, e->stream));
    if (helper_enc_len) HIPCHK(e, hipMemcpyAsync(d_he, helper_encs, n * helper_enc_len, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_hc, helper_cts, n * hct, hipMemcpyHostToDevice, e->stream));
    if (seal_status) HIPCHK(e, hipMemcpyAsync(d_st, seal_status, n, hipMemcpyHostToDevice, e->stream));
  }
  in.ids = d_ids;
  in.ps = d_ps;
  in.lencs = d_le;
  in.lcts = d_lc;
  in.hencs = d_he;
  in.hcts = d_hc;
  in.status = seal_status ? d_st : nullptr;
  // the scratch holds `bound` bytes, the most the bodies can take; the core refuses what the caller's buffer cannot
  uint64_t len = 0;
  if (const int32_t rc = report_encode_core(e, in, d_body, capacity < bound ? capacity : bound, nullptr, out_offsets, &len, false))
    return rc;
  if (len) HIPCHK(e, hipMemcpyAsync(out, d_body, len, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *out_len = len;
  return JX_OK;
}

}  // extern "C"
