// jx_engine_collect.cpp — collection: jx_collect_seal[_device] (the helper's aggregate-share handler and the leader's
// collection step: merge, check, seal) and jx_collect_open[_device] (the collector: open both shares, unshard).
// Kernels: jx_collect.hip; the seal and the opens are the long forms of jx_hpke_seal.hip and jx_hpke_long.hip, queued
// here on the engine's stream.
#include <cstring>
#include <string>
#include <vector>

#include "jx_collect.h"
#include "jx_engine_internal.h"
#include "jx_hpke_long.h"
#include "jx_hpke_seal.h"

using namespace jx;
using namespace jxi;

namespace {

bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// offsets[n + 1], non-decreasing, rebased to start at 0
bool rebase(const uint64_t* off, uint64_t n, std::vector<uint64_t>& out) {
  out.resize(n + 1);
  for (uint64_t i = 0; i <= n; i++) {
    if (i && off[i] < off[i - 1]) return false;
    out[i] = off[i] - off[0];
  }
  return true;
}

// the linear grids of the element kernels: (jobs or collections) x tiles workgroups
bool grid_fits(uint64_t n, uint64_t pt_bytes) {
  const uint64_t tiles = (pt_bytes / 8 + 2 + COLLECT_TILE - 1) / COLLECT_TILE;
  return n < (1ull << 31) / tiles;
}

int32_t collect_seal(jx_engine* e, bool host, uint64_t njobs, const uint8_t* records, uint64_t nrecords,
                     const uint64_t* record_offsets, const uint32_t* record_index, const uint64_t* expect_counts,
                     const uint8_t* expect_checksums, uint64_t min_batch_size, uint64_t max_batch_size,
                     const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* ephemeral_sks, jx_hpke* sender,
                     uint8_t* out_status, uint64_t* out_counts, uint8_t* out_checksums, uint8_t* out_encs,
                     uint8_t* out_cts, uint8_t* out_shares) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (!sender || hpke_device(sender) != e->device)
    return fail(e, JX_E_INVALID, "collect seal: the collector's key must be an HPKE context on the engine's device");
  if (hpke_enc_len(sender) != 32)
    return fail(e, JX_E_UNSUPPORTED, "collect seal: sealing under KEM 0x0010 (P-256) is out of scope");
  if (!hpke_is_sender(sender))
    return fail(e, JX_E_INVALID, "collect seal: the collector's key must be a sender context (jx_hpke_create_sender)");
  if (njobs == 0) return JX_OK;
  if (!record_offsets || !aad_offsets || !ephemeral_sks || !out_status || !out_counts || !out_checksums || !out_encs ||
      !out_cts || (expect_counts == nullptr) != (expect_checksums == nullptr))
    return JX_E_INVALID;
  const uint64_t pt_bytes = (uint64_t)c.out_len * c.fb, stride = pt_bytes + 40, ct_bytes = pt_bytes + 16;
  if (!grid_fits(njobs, pt_bytes)) return fail(e, JX_E_INVALID, "collect seal: too many jobs for one call");
  std::vector<uint64_t> roff, aoff;
  if (!rebase(record_offsets, njobs, roff) || !rebase(aad_offsets, njobs, aoff))
    return fail(e, JX_E_INVALID, "collect seal: offsets must be non-decreasing");
  const uint64_t nidx = roff[njobs], aad_bytes = aoff[njobs];
  if ((nidx && (!record_index || !records)) || (aad_bytes && !aads)) return JX_E_INVALID;
  const uint32_t* idx = record_index + record_offsets[0];
  {
    std::vector<uint64_t> seen(nrecords, 0);  // the last job (+ 1) that named the record
    for (uint64_t j = 0; j < njobs; j++)
      for (uint64_t q = roff[j]; q < roff[j + 1]; q++) {
        if (idx[q] >= nrecords) return fail(e, JX_E_INVALID, "collect seal: a record index is past the records");
        if (seen[idx[q]] == j + 1) return fail(e, JX_E_INVALID, "collect seal: a job names one record twice");
        seen[idx[q]] = j + 1;
      }
  }
  if (!host && (!aligned8(records) || !aligned8(out_counts) || !aligned8(out_checksums) || !aligned8(out_encs) ||
                !aligned8(out_cts) || !aligned8(out_shares)))
    return fail(e, JX_E_INVALID, "collect seal: device buffers must be 8-byte aligned");
  HIPCHK(e, hipSetDevice(e->device));

  std::vector<uint64_t> poff(njobs + 1);
  for (uint64_t j = 0; j <= njobs; j++) poff[j] = j * pt_bytes;
  uint64_t *d_roff = nullptr, *d_aoff = nullptr, *d_poff = nullptr, *d_ecount = nullptr, *d_counts = nullptr;
  uint32_t *d_idx = nullptr, *d_bad = nullptr;
  uint8_t *d_ecs = nullptr, *d_aads = nullptr, *d_st0 = nullptr, *d_ok = nullptr, *d_ctx = nullptr, *d_pts = nullptr,
          *d_rec = nullptr, *d_sks = nullptr, *d_st = nullptr, *d_cs = nullptr, *d_encs = nullptr, *d_cts = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_roff, (njobs + 1) * 8);
    cv.take(d_aoff, (njobs + 1) * 8);
    cv.take(d_poff, (njobs + 1) * 8);
    cv.take(d_idx, nidx * 4);
    cv.take(d_ecount, njobs * 8);
    cv.take(d_ecs, njobs * 32);
    cv.take(d_aads, aad_bytes);
    cv.take(d_bad, njobs * 4);
    cv.take(d_st0, njobs);
    cv.take(d_ok, njobs);
    cv.take(d_ctx, njobs * SEAL_CTX_BYTES);
    if (host || !out_shares) cv.take(d_pts, njobs * pt_bytes);
    if (host) {
      cv.take(d_rec, nrecords * stride);
      cv.take(d_sks, njobs * 32);
      cv.take(d_st, njobs);
      cv.take(d_counts, njobs * 8);
      cv.take(d_cs, njobs * 32);
      cv.take(d_encs, njobs * 32);
      cv.take(d_cts, njobs * ct_bytes);
    }
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  hipStream_t s = e->stream;
  if (!host) {
    d_rec = const_cast<uint8_t*>(records);
    d_sks = const_cast<uint8_t*>(ephemeral_sks);
    d_st = out_status;
    d_counts = out_counts;
    d_cs = out_checksums;
    d_encs = out_encs;
    d_cts = out_cts;
    if (out_shares) d_pts = out_shares;
  } else {
    if (nrecords) HIPCHK(e, hipMemcpyAsync(d_rec, records, nrecords * stride, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(d_sks, ephemeral_sks, njobs * 32, hipMemcpyHostToDevice, s));
  }
  HIPCHK(e, hipMemcpyAsync(d_roff, roff.data(), (njobs + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(d_aoff, aoff.data(), (njobs + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(d_poff, poff.data(), (njobs + 1) * 8, hipMemcpyHostToDevice, s));
  if (nidx) HIPCHK(e, hipMemcpyAsync(d_idx, idx, nidx * 4, hipMemcpyHostToDevice, s));
  if (aad_bytes) HIPCHK(e, hipMemcpyAsync(d_aads, aads + aad_offsets[0], aad_bytes, hipMemcpyHostToDevice, s));
  if (expect_counts) {
    HIPCHK(e, hipMemcpyAsync(d_ecount, expect_counts, njobs * 8, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(d_ecs, expect_checksums, njobs * 32, hipMemcpyHostToDevice, s));
  }
  HIPCHK(e, hipMemsetAsync(d_bad, 0, njobs * 4, s));
  Uploads up;  // behind the host arrays, before the kernels
  if (!host) HIPCHK(e, up.queued(s));

  CollectMergeArgs m{};
  m.njobs = (uint32_t)njobs;
  m.out_len = c.out_len;
  m.fb = c.fb;
  m.records = d_rec;
  m.rec_off = d_roff;
  m.rec_idx = d_idx;
  m.exp_counts = expect_counts ? d_ecount : nullptr;
  m.exp_checksums = expect_counts ? d_ecs : nullptr;
  m.min_batch_size = min_batch_size;
  m.max_batch_size = max_batch_size;
  m.bad = d_bad;
  m.pts = d_pts;
  m.status0 = d_st0;
  m.counts = d_counts;
  m.checksums = d_cs;
  HIPCHK(e, launch_collect_merge(m, s));

  SealArgs a{};
  a.n = njobs;
  uint32_t cap = 0;
  hpke_registry(e->device, &a.keys, &cap);
  a.slot = hpke_slot(sender);
  a.sks = d_sks;
  a.pts = d_pts;
  a.pt_off = d_poff;
  a.aads = d_aads;
  a.aad_off = d_aoff;
  a.encs = d_encs;
  a.cts = d_cts;
  a.ok = d_ok;
  a.ctx = d_ctx;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, a.zero_ist, a.zero_ost);
  HIPCHK(e, launch_hpke_seal(a, true, s));

  CollectFinishArgs f{};
  f.njobs = (uint32_t)njobs;
  f.pt_bytes = pt_bytes;
  f.status0 = d_st0;
  f.sealed = d_ok;
  f.status = d_st;
  f.encs = d_encs;
  f.cts = d_cts;
  f.pts = d_pts;
  HIPCHK(e, launch_collect_finish(f, s));

  if (host) {
    HIPCHK(e, hipMemcpyAsync(out_status, d_st, njobs, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out_counts, d_counts, njobs * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out_checksums, d_cs, njobs * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out_encs, d_encs, njobs * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out_cts, d_cts, njobs * ct_bytes, hipMemcpyDeviceToHost, s));
    if (out_shares) HIPCHK(e, hipMemcpyAsync(out_shares, d_pts, njobs * pt_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  } else {
    HIPCHK(e, up.consumed());
  }
  return JX_OK;
}

// one role's half of jx_collect_open: the opener and the caller's arrays
struct OpenSide {
  jx_hpke* h;
  const uint8_t* encs;
  const uint8_t* cts;
  const uint64_t* ct_off;
  uint32_t enc_len = 0;
  uint8_t *d_encs = nullptr, *d_cts = nullptr, *d_pts = nullptr, *d_ok = nullptr, *d_ctx = nullptr;
};

int32_t collect_open(jx_engine* e, bool host, jx_hpke* leader, jx_hpke* helper, uint64_t n, const uint8_t* leader_encs,
                     const uint8_t* leader_cts, const uint64_t* leader_ct_offsets, const uint8_t* helper_encs,
                     const uint8_t* helper_cts, const uint64_t* helper_ct_offsets, const uint8_t* aads,
                     const uint64_t* aad_offsets, uint8_t* out_aggregates, uint8_t* out_status) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  OpenSide side[2] = {{leader, leader_encs, leader_cts, leader_ct_offsets}, {helper, helper_encs, helper_cts, helper_ct_offsets}};
  for (OpenSide& sd : side) {
    if (!sd.h || hpke_device(sd.h) != e->device)
      return fail(e, JX_E_INVALID, "collect open: both openers must be HPKE contexts on the engine's device");
    if (hpke_is_sender(sd.h))
      return fail(e, JX_E_INVALID, "collect open: a sender context (jx_hpke_create_sender) holds no private key");
    sd.enc_len = hpke_enc_len(sd.h);
  }
  if (n == 0) return JX_OK;
  if (!leader_encs || !leader_cts || !leader_ct_offsets || !helper_encs || !helper_cts || !helper_ct_offsets ||
      !aad_offsets || !out_aggregates || !out_status)
    return JX_E_INVALID;
  const uint64_t pt_bytes = (uint64_t)c.out_len * c.fb, ct_bytes = pt_bytes + 16;
  if (!grid_fits(n, pt_bytes)) return fail(e, JX_E_INVALID, "collect open: too many collections for one call");
  for (uint64_t i = 0; i < n; i++)
    if (leader_ct_offsets[i + 1] < leader_ct_offsets[i] || helper_ct_offsets[i + 1] < helper_ct_offsets[i] ||
        aad_offsets[i + 1] < aad_offsets[i])
      return fail(e, JX_E_INVALID, "collect open: offsets must be non-decreasing");
  if (aad_offsets[n] > aad_offsets[0] && !aads) return JX_E_INVALID;
  if (!host && !aligned8(out_aggregates)) return fail(e, JX_E_INVALID, "collect open: device buffers must be 8-byte aligned");
  HIPCHK(e, hipSetDevice(e->device));

  // the lengths are in the offsets: a share of another length than OUT x FB + 16 is AggregateShareDecode without an
  // open; the others are gathered into dense rows
  std::vector<uint8_t> st0(n, 0);
  std::vector<uint32_t> row;
  std::vector<uint64_t> aoff(1, 0);
  std::vector<uint8_t> aad;
  for (uint64_t i = 0; i < n; i++) {
    if (leader_ct_offsets[i + 1] - leader_ct_offsets[i] != ct_bytes) {
      st0[i] = (uint8_t)COLLECT_DECODE_LEADER;
    } else if (helper_ct_offsets[i + 1] - helper_ct_offsets[i] != ct_bytes) {
      st0[i] = (uint8_t)COLLECT_DECODE_HELPER;
    } else {
      row.push_back((uint32_t)i);
      if (aad_offsets[i + 1] > aad_offsets[i]) aad.insert(aad.end(), aads + aad_offsets[i], aads + aad_offsets[i + 1]);
      aoff.push_back(aad.size());
    }
  }
  const uint64_t m = row.size();
  std::vector<uint64_t> coff(m + 1);
  for (uint64_t j = 0; j <= m; j++) coff[j] = j * ct_bytes;

  uint64_t *d_coff = nullptr, *d_aoff = nullptr;
  uint32_t *d_row = nullptr, *d_bad = nullptr;
  uint8_t *d_aad = nullptr, *d_out = nullptr, *d_st = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_coff, (m + 1) * 8);
    cv.take(d_aoff, (m + 1) * 8);
    cv.take(d_row, m * 4);
    cv.take(d_bad, m * 8);
    cv.take(d_aad, aad.size());
    for (OpenSide& sd : side) {
      cv.take(sd.d_encs, m * sd.enc_len);
      cv.take(sd.d_cts, m * ct_bytes);
      cv.take(sd.d_pts, m * pt_bytes);
      cv.take(sd.d_ok, m);
      cv.take(sd.d_ctx, m * sizeof(LongCtxRow));
    }
    if (host) {
      cv.take(d_out, n * pt_bytes);
      cv.take(d_st, n);
    }
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  hipStream_t s = e->stream;
  if (!host) {
    d_out = out_aggregates;
    d_st = out_status;
  }
  HIPCHK(e, hipMemsetAsync(d_out, 0, n * pt_bytes, s));
  HIPCHK(e, hipMemcpyAsync(d_st, st0.data(), n, hipMemcpyHostToDevice, s));
  Uploads up;
  if (!host && !m) HIPCHK(e, up.queued(s));
  if (m) {
    HIPCHK(e, hipMemcpyAsync(d_coff, coff.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(d_aoff, aoff.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(d_row, row.data(), m * 4, hipMemcpyHostToDevice, s));
    if (!aad.empty()) HIPCHK(e, hipMemcpyAsync(d_aad, aad.data(), aad.size(), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemsetAsync(d_bad, 0, m * 8, s));
    if (!host) HIPCHK(e, up.queued(s));
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (OpenSide& sd : side) {
      // one copy per run of collections that follow each other in the caller's arrays
      for (uint64_t j = 0; j < m;) {
        uint64_t k = j + 1;
        while (k < m && row[k] == row[k - 1] + 1) k++;
        HIPCHK(e, hipMemcpyAsync(sd.d_encs + j * sd.enc_len, sd.encs + (uint64_t)row[j] * sd.enc_len,
                                 (k - j) * sd.enc_len, kind, s));
        HIPCHK(e, hipMemcpyAsync(sd.d_cts + j * ct_bytes, sd.cts + sd.ct_off[row[j]], (k - j) * ct_bytes, kind, s));
        j = k;
      }
      LongCtxArgs ca{};
      ca.n = m;
      uint32_t cap = 0;
      hpke_registry(e->device, &ca.keys, &cap);
      ca.slot = hpke_slot(sd.h);
      ca.encs = sd.d_encs;
      ca.out = (LongCtxRow*)sd.d_ctx;
      hmac_pads(zero, ca.zero_ist, ca.zero_ost);
      const HpkeBufs b{m, sd.d_encs, sd.d_cts, d_coff, d_aad, d_aoff, sd.d_pts, sd.d_ok};
      HIPCHK(e, launch_hpke_long_open(ca, sd.enc_len == 65, b, s));
    }
    CollectUnshardArgs u{};
    u.n = (uint32_t)m;
    u.out_len = c.out_len;
    u.fb = c.fb;
    u.leader_pts = side[0].d_pts;
    u.helper_pts = side[1].d_pts;
    u.leader_ok = side[0].d_ok;
    u.helper_ok = side[1].d_ok;
    u.row = d_row;
    u.bad = d_bad;
    u.out = d_out;
    u.status = d_st;
    HIPCHK(e, launch_collect_unshard(u, s));
  }
  if (host) {
    HIPCHK(e, hipMemcpyAsync(out_aggregates, d_out, n * pt_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  } else {
    HIPCHK(e, up.consumed());
  }
  return JX_OK;
}

}  // namespace

extern "C" {

int32_t jx_collect_seal(jx_engine* e, uint64_t njobs, const uint8_t* records, uint64_t nrecords,
                        const uint64_t* record_offsets, const uint32_t* record_index, const uint64_t* expect_counts,
                        const uint8_t* expect_checksums, uint64_t min_batch_size, uint64_t max_batch_size,
                        const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* ephemeral_sks, jx_hpke* sender,
                        uint8_t* out_status, uint64_t* out_counts, uint8_t* out_checksums, uint8_t* out_encs,
                        uint8_t* out_cts, uint8_t* out_shares) {
  return collect_seal(e, true, njobs, records, nrecords, record_offsets, record_index, expect_counts, expect_checksums,
                      min_batch_size, max_batch_size, aads, aad_offsets, ephemeral_sks, sender, out_status, out_counts,
                      out_checksums, out_encs, out_cts, out_shares);
}

int32_t jx_collect_seal_device(jx_engine* e, uint64_t njobs, const void* d_records, uint64_t nrecords,
                               const uint64_t* record_offsets, const uint32_t* record_index,
                               const uint64_t* expect_counts, const uint8_t* expect_checksums, uint64_t min_batch_size,
                               uint64_t max_batch_size, const uint8_t* aads, const uint64_t* aad_offsets,
                               const void* d_ephemeral_sks, jx_hpke* sender, void* d_out_status, void* d_out_counts,
                               void* d_out_checksums, void* d_out_encs, void* d_out_cts, void* d_out_shares) {
  return collect_seal(e, false, njobs, (const uint8_t*)d_records, nrecords, record_offsets, record_index, expect_counts,
                      expect_checksums, min_batch_size, max_batch_size, aads, aad_offsets,
                      (const uint8_t*)d_ephemeral_sks, sender, (uint8_t*)d_out_status, (uint64_t*)d_out_counts,
                      (uint8_t*)d_out_checksums, (uint8_t*)d_out_encs, (uint8_t*)d_out_cts, (uint8_t*)d_out_shares);
}

int32_t jx_collect_open(jx_engine* e, jx_hpke* leader_opener, jx_hpke* helper_opener, uint64_t n,
                        const uint8_t* leader_encs, const uint8_t* leader_cts, const uint64_t* leader_ct_offsets,
                        const uint8_t* helper_encs, const uint8_t* helper_cts, const uint64_t* helper_ct_offsets,
                        const uint8_t* aads, const uint64_t* aad_offsets, uint8_t* out_aggregates, uint8_t* out_status) {
  return collect_open(e, true, leader_opener, helper_opener, n, leader_encs, leader_cts, leader_ct_offsets, helper_encs,
                      helper_cts, helper_ct_offsets, aads, aad_offsets, out_aggregates, out_status);
}

int32_t jx_collect_open_device(jx_engine* e, jx_hpke* leader_opener, jx_hpke* helper_opener, uint64_t n,
                               const void* d_leader_encs, const void* d_leader_cts, const uint64_t* leader_ct_offsets,
                               const void* d_helper_encs, const void* d_helper_cts, const uint64_t* helper_ct_offsets,
                               const uint8_t* aads, const uint64_t* aad_offsets, void* d_out_aggregates,
                               void* d_out_status) {
  return collect_open(e, false, leader_opener, helper_opener, n, (const uint8_t*)d_leader_encs,
                      (const uint8_t*)d_leader_cts, leader_ct_offsets, (const uint8_t*)d_helper_encs,
                      (const uint8_t*)d_helper_cts, helper_ct_offsets, aads, aad_offsets, (uint8_t*)d_out_aggregates,
                      (uint8_t*)d_out_status);
}

}  // extern "C"
