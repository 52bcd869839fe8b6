// jx_engine_upload.cpp — the leader's upload path: open and validate uploaded report shares (kernels: jx_hpke_long.hip).
#include <cstring>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_upload.h"

using namespace jx;
using namespace jxi;

namespace {
// What both upload calls check before anything is queued, and the reports' rows: keypair indices become slots of
// the device's key registry, as fill_enc_rows does for the helper's rows; ciphertext and encapsulated-key offsets
// are the caller's own.
int32_t upload_rows(jx_engine* e, uint64_t n, const uint64_t* times, jx_hpke* const* keypairs, uint32_t nkeypairs,
                    const uint8_t* key_index, const uint64_t* enc_offsets, const uint64_t* payload_offsets,
                    uint64_t* lis_stride, std::vector<UpRow>& rows, bool* any_p256) {
  if (nkeypairs > JX_ENC_MAX_KEYPAIRS || (nkeypairs && !keypairs))
    return fail(e, JX_E_INVALID, "upload open: at most JX_ENC_MAX_KEYPAIRS keypairs");
  uint32_t klen[JX_ENC_MAX_KEYPAIRS];
  uint16_t slot[JX_ENC_MAX_KEYPAIRS];
  *any_p256 = false;
  for (uint32_t k = 0; k < nkeypairs; k++) {
    if (!keypairs[k] || hpke_device(keypairs[k]) != e->device)
      return fail(e, JX_E_INVALID, "upload open: every keypair must be an HPKE context on the engine's device");
    if (hpke_is_sender(keypairs[k]))
      return fail(e, JX_E_INVALID, "upload open: a sender context (jx_hpke_create_sender) holds no private key");
    klen[k] = hpke_enc_len(keypairs[k]);
    slot[k] = hpke_slot(keypairs[k]);
    *any_p256 = *any_p256 || klen[k] == 65;
  }
  if (const int32_t rc = lis_stride_ok(e, lis_stride, "upload open")) return rc;
  rows.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t k0 = key_index[2 * i], k1 = key_index[2 * i + 1];
    if ((k0 >= nkeypairs && k0 != JX_KEY_NONE && k0 != JX_KEY_MALFORMED) || (k1 >= nkeypairs && k1 != JX_KEY_NONE) ||
        payload_offsets[i + 1] < payload_offsets[i] || payload_offsets[i + 1] - payload_offsets[i] > 0xFFFFFFFFull ||
        (enc_offsets && enc_offsets[i + 1] < enc_offsets[i]))
      return fail(e, JX_E_INVALID, "upload open: key_index out of range, offsets decreasing or a payload of 2^32 bytes or more");
    UpRow& w = rows[i];
    memset(&w, 0, sizeof w);
    w.ct_off = payload_offsets[i];
    w.ct_len = (uint32_t)(payload_offsets[i + 1] - payload_offsets[i]);
    w.enc_off = enc_offsets ? enc_offsets[i] : 32 * i;
    const uint64_t len = enc_offsets ? enc_offsets[i + 1] - enc_offsets[i] : 32;
    w.enc_len = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    // a trial can only succeed when the encapsulated key has the length of the keypair's KEM; a key that fits
    // neither keypair fails the report without an open
    const bool fits = (k0 < nkeypairs && klen[k0] == len) || (k1 < nkeypairs && klen[k1] == len);
    if (k0 == JX_KEY_MALFORMED || (k0 < nkeypairs && !fits)) w.flags |= UP_ROW_MALFORMED;
    w.key0 = k0 < nkeypairs ? slot[k0] : (k0 == JX_KEY_MALFORMED ? (uint16_t)0 : KEY_SLOT_NONE);
    w.key1 = k1 < nkeypairs ? slot[k1] : KEY_SLOT_NONE;
    for (int b = 0; b < 8; b++) w.time_be[b] = (uint8_t)(times[i] >> (56 - 8 * b));
  }
  return JX_OK;
}

// The launch, with everything on the device but the rows: d_rows / d_ctx / d_pts are scratch of n x sizeof(UpRow),
// n x UPLOAD_CTX_BYTES and the payloads' span. cts, pts and ext are indexed by the rows' absolute ct_off.
int32_t upload_launch(jx_engine* e, uint64_t n, const std::vector<UpRow>& rows, bool any_p256, const uint8_t task_id[32],
                      const uint8_t* d_ids, const uint8_t* d_ps, const uint8_t* d_encs, const uint8_t* cts, uint8_t* pts,
                      UpRow* d_rows, void* d_ctx, uint8_t* d_out_rows, uint64_t lis_stride, uint8_t* ext,
                      uint32_t* d_ext_len, uint8_t* d_status) {
  const Cfg& c = e->cfg;
  HIPCHK(e, hipMemcpyAsync(d_rows, rows.data(), n * sizeof(UpRow), hipMemcpyHostToDevice, e->stream));
  UploadArgs a{};
  a.n = n;
  a.rows = d_rows;
  uint32_t cap = 0;
  hpke_registry(e->device, &a.keys, &cap);
  a.nkeys = a.keys ? cap : 0;
  a.ps_bytes = c.ps_bytes;
  a.ids = d_ids;
  a.ps = d_ps;
  memcpy(a.task_id, task_id, 32);
  a.encs = d_encs;
  a.cts = cts;
  a.pts = pts;
  a.ctx = d_ctx;
  a.out_rows = d_out_rows;
  a.lis_stride = lis_stride;
  a.lis_bytes = c.lis_bytes;
  a.elem_bytes = c.lis_bytes - (c.jr_len ? c.seed : 0);
  a.fb = c.fb;
  a.out_ext = ext;
  a.out_ext_len = d_ext_len;
  a.out_status = d_status;
  HIPCHK(e, launch_upload_open(a, any_p256, e->stream));
  return JX_OK;
}
}  // namespace

extern "C" {

int32_t jx_leader_upload_open_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                     const void* d_public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                     uint32_t nkeypairs, const uint8_t* key_index, const void* d_encs,
                                     const uint64_t* enc_offsets, const void* d_payloads, const uint64_t* payload_offsets,
                                     void* d_out_rows, uint64_t lis_stride, void* d_out_extensions, void* d_out_ext_len,
                                     void* d_out_status) {
  if (!e || (n && (!d_report_ids || !times || !task_id || !key_index || !d_encs || !payload_offsets || !d_out_rows ||
                   !d_out_extensions || !d_out_ext_len || !d_out_status)))
    return JX_E_INVALID;
  if (n == 0) return JX_OK;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !d_public_shares) return JX_E_INVALID;
  if (reinterpret_cast<uintptr_t>(d_out_rows) & 15u)
    return fail(e, JX_E_INVALID, "upload open: d_out_rows must be 16-byte aligned");
  std::vector<UpRow> rows;
  bool any_p256 = false;
  if (const int32_t rc = upload_rows(e, n, times, keypairs, nkeypairs, key_index, enc_offsets, payload_offsets,
                                     &lis_stride, rows, &any_p256))
    return rc;
  const uint64_t c0 = payload_offsets[0], span = payload_offsets[n] - c0;
  if (span && !d_payloads) return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  UpRow* d_rows = nullptr;
  uint8_t *d_ctx = nullptr, *d_pt = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_rows, n * sizeof(UpRow));
    cv.take(d_ctx, n * UPLOAD_CTX_BYTES);
    cv.take(d_pt, span);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  int32_t rc = scratch_carve(e, mem, lay, true);
  if (rc) return rc;
  rc = upload_launch(e, n, rows, any_p256, task_id, (const uint8_t*)d_report_ids, (const uint8_t*)d_public_shares,
                     (const uint8_t*)d_encs, (const uint8_t*)d_payloads, d_pt - c0, d_rows, d_ctx, (uint8_t*)d_out_rows,
                     lis_stride, (uint8_t*)d_out_extensions, (uint32_t*)d_out_ext_len, (uint8_t*)d_out_status);
  if (rc) return rc;
  // the rows leave pageable host memory before the call returns; the launch itself stays queued
  HIPCHK(e, wait_uploads(e));
  return JX_OK;
}

int32_t jx_leader_upload_open_batch(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                                    const uint8_t* public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                    uint32_t nkeypairs, const uint8_t* key_index, const uint8_t* encs,
                                    const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                                    uint8_t* out_leader_input_shares, uint8_t* out_extensions, uint32_t* out_ext_len,
                                    uint8_t* out_status) {
  if (!e || (n && (!report_ids || !times || !task_id || !key_index || !encs || !payload_offsets ||
                   !out_leader_input_shares || !out_extensions || !out_ext_len || !out_status)))
    return JX_E_INVALID;
  if (n == 0) return JX_OK;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (c.ps_bytes && !public_shares) return JX_E_INVALID;
  std::vector<UpRow> rows;
  bool any_p256 = false;
  uint64_t lis_stride = (c.lis_bytes + 15u) & ~15ull;  // the device rows; the caller's are LIS apart
  if (const int32_t rc = upload_rows(e, n, times, keypairs, nkeypairs, key_index, enc_offsets, payload_offsets,
                                     &lis_stride, rows, &any_p256))
    return rc;
  const uint64_t c0 = payload_offsets[0], span = payload_offsets[n] - c0;
  if (span && !payloads) return JX_E_INVALID;
  const uint64_t e0 = enc_offsets ? enc_offsets[0] : 0, enc_bytes = (enc_offsets ? enc_offsets[n] : 32 * n) - e0;
  HIPCHK(e, hipSetDevice(e->device));
  UpRow* d_rows = nullptr;
  uint32_t* d_len = nullptr;
  uint8_t *d_ctx = nullptr, *d_pt = nullptr, *d_ct = nullptr, *d_ext = nullptr, *d_enc = nullptr, *d_ids = nullptr,
          *d_ps = nullptr, *d_out = nullptr, *d_st = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_rows, n * sizeof(UpRow));
    cv.take(d_ctx, n * UPLOAD_CTX_BYTES);
    cv.take(d_pt, span);
    cv.take(d_ct, span);
    cv.take(d_ext, span);
    cv.take(d_enc, enc_bytes);
    cv.take(d_ids, n * 16);
    cv.take(d_ps, n * c.ps_bytes);
    cv.take(d_out, n * lis_stride);
    cv.take(d_len, n * 4);
    cv.take(d_st, n);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  int32_t rc = scratch_carve(e, mem, lay, true);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(d_ids, report_ids, n * 16, hipMemcpyHostToDevice, e->stream));
  if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
  if (enc_bytes) HIPCHK(e, hipMemcpyAsync(d_enc, encs + e0, enc_bytes, hipMemcpyHostToDevice, e->stream));
  if (span) HIPCHK(e, hipMemcpyAsync(d_ct, payloads + c0, span, hipMemcpyHostToDevice, e->stream));
  rc = upload_launch(e, n, rows, any_p256, task_id, d_ids, d_ps, d_enc - e0, d_ct - c0, d_pt - c0, d_rows, d_ctx, d_out,
                     lis_stride, d_ext - c0, d_len, d_st);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy2DAsync(out_leader_input_shares, c.lis_bytes, d_out, lis_stride, c.lis_bytes, n, hipMemcpyDeviceToHost,
                             e->stream));
  HIPCHK(e, hipMemcpyAsync(out_ext_len, d_len, n * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  // the extension bytes: each report's own, where its payload was (most batches have none)
  bool any = false;
  for (uint64_t i = 0; i < n; i++) {
    if (!out_ext_len[i]) continue;
    any = true;
    HIPCHK(e, hipMemcpyAsync(out_extensions + payload_offsets[i], d_ext + (payload_offsets[i] - c0), out_ext_len[i],
                             hipMemcpyDeviceToHost, e->stream));
  }
  if (any) HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

}  // extern "C"
