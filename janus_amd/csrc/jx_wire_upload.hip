// jx_wire_upload.hip — the upload message on the device (the rule: jx_wire.h; the host side: jx_engine_wire_upload.cpp).
//
// Decode, the leader's side: n Report bodies back to back with their boundaries known. upload_parse_kernel, one
// thread per upload, parses it (wire_upload_parse: the framing, the three time checks, the public share's length, the
// key slots) and stores its record, id, time and status. upload_scan_kernel, one workgroup, scans the accept flags and
// the four packed lengths, and every thread turns the ranks it stored itself into the compaction list, row_of and the
// dense offset arrays. upload_gather_kernel, `parts` waves per accepted report, copies its fixed fields by lanes and
// its five variable fields with wave_copy into the arrays the open and the request encode read; every output byte has
// one writer.
//
// Encode, the client's side: report_sizes_kernel, one workgroup, scans which reports take room (every one that does
// has the same length: the seal writes fixed rows); report_pack_kernel, `parts` waves per report that takes room,
// writes its 42 fixed bytes one per lane and its five fields with wave_copy.
//
// No launch reads what another workgroup of the same launch stored.
#include <hip/hip_runtime.h>

#include "jx_wire.h"
#include "jx_wire_dev.h"

namespace jx {
namespace {

__global__ __launch_bounds__(256) void upload_parse_kernel(WireUploadArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t lo = a.body_offsets[i], hi = a.body_offsets[i + 1];  // the host checked lo <= hi <= len
  WireReportRec r;
  uint64_t t;
  const uint8_t st = wire_upload_parse(a.body, lo, hi, a.ps_bytes, a.checks, a.key_first, a.key_second, r,
                                       a.ids_all + 16 * i, &t);
  a.recs[i] = r;
  a.status[i] = st;
  a.times_all[i] = t;
}

__global__ __launch_bounds__(1024) void upload_scan_kernel(WireUploadArgs a) {
  const uint64_t n = a.n;
  uint64_t *const s0 = a.scan[0], *const s1 = a.scan[1], *const s2 = a.scan[2], *const s3 = a.scan[3];
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)(a.status[i] == UPLOAD_OK); }, a.rank);
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)a.recs[i].lenc_len; }, s0);
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)a.recs[i].lpay_len; }, s1);
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)a.recs[i].henc_len; }, s2);
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)a.recs[i].hpay_len; }, s3);
  // thread t reads back the ranks and sums of i = t, t + 1024, .., which it stored itself
  for (uint64_t i = threadIdx.x; i < n; i += 1024) {
    if (a.status[i] != UPLOAD_OK) {
      a.row_of[i] = UPLOAD_NO_ROW;
      continue;
    }
    const uint64_t k = a.rank[i];
    a.row_of[i] = (uint32_t)k;
    a.index[k] = (uint32_t)i;
    a.offs[0][k] = s0[i];
    a.offs[1][k] = s1[i];
    a.offs[2][k] = s2[i];
    a.offs[3][k] = s3[i];
  }
  if (threadIdx.x == 0) {  // the totals are thread 0's own stores
    const uint64_t m = a.rank[n];
    a.offs[0][m] = s0[n];
    a.offs[1][m] = s1[n];
    a.offs[2][m] = s2[n];
    a.offs[3][m] = s3[n];
    a.totals->m = m;
    a.totals->lenc_bytes = s0[n];
    a.totals->lpay_bytes = s1[n];
    a.totals->henc_bytes = s2[n];
    a.totals->hpay_bytes = s3[n];
  }
}

// Slice `part` of `parts` of a field (wire_part_span); each slice goes through wave_copy with its own head and tail.
__device__ inline void wave_copy_part(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t lane, uint32_t part,
                                      uint32_t parts) {
  uint64_t lo, cnt;
  wire_part_span(len, part, parts, &lo, &cnt);
  wave_copy(dst + lo, src + lo, cnt, lane);
}

__global__ __launch_bounds__(256) void upload_gather_kernel(WireUploadArgs a, uint64_t m, uint32_t parts) {
  const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t k = w / parts;
  const uint32_t part = (uint32_t)(w % parts);
  if (k >= m) return;
  const uint64_t i = a.index[k];
  const WireReportRec r = a.recs[i];
  if (part == 0) {
    if (lane < 16) a.ids[16 * k + lane] = a.body[r.off + lane];
    if (lane == 16) a.times[k] = a.times_all[i];
    if (lane == 17) a.key_index[2 * k] = r.key0;
    if (lane == 18) a.key_index[2 * k + 1] = r.key1;
    if (lane == 19) a.config_ids[k] = r.helper_config_id;
    if (a.ps_bytes) wave_copy(a.ps + k * a.ps_bytes, a.body + r.ps_off, a.ps_bytes, lane);
  }
  wave_copy_part(a.packed[0] + a.offs[0][k], a.body + r.lenc_off, r.lenc_len, lane, part, parts);
  wave_copy_part(a.packed[1] + a.offs[1][k], a.body + r.lpay_off, r.lpay_len, lane, part, parts);
  wave_copy_part(a.packed[2] + a.offs[2][k], a.body + r.henc_off, r.henc_len, lane, part, parts);
  wave_copy_part(a.packed[3] + a.offs[3][k], a.body + r.hpay_off, r.hpay_len, lane, part, parts);
}

// ---- the client's encode
__global__ __launch_bounds__(1024) void report_sizes_kernel(WireReportArgs a) {
  const uint64_t L = wire_report_len(a.ps_bytes, a.lenc_len, a.lct_len, a.henc_len, a.hct_len);
  auto room = [&](uint64_t i) { return !(a.status && a.status[i]); };
  block_exclusive_scan(a.n, [&](uint64_t i) { return room(i) ? L : 0; }, a.offsets);
  block_exclusive_scan(a.n, [&](uint64_t i) { return (uint64_t)room(i); }, a.rank);
  for (uint64_t i = threadIdx.x; i < a.n; i += 1024)  // ranks this thread stored itself
    if (room(i)) a.index[a.rank[i]] = (uint32_t)i;
  if (threadIdx.x == 0) {
    a.totals->bytes = a.offsets[a.n];
    a.totals->m = a.rank[a.n];
  }
}

__global__ __launch_bounds__(256) void report_pack_kernel(WireReportArgs a, uint64_t m, uint32_t parts) {
  const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t k = w / parts;
  const uint32_t part = (uint32_t)(w % parts);
  if (k >= m) return;
  const uint64_t i = a.index[k];
  const WireReportLayout l = wire_report_layout(a.ps_bytes, a.lenc_len, a.lct_len, a.henc_len, a.hct_len);
  uint8_t* p = a.out + a.offsets[i];
  if (part == 0) {
    if (lane < WIRE_REPORT_FIXED) {
      uint64_t at;
      const uint8_t v = wire_report_fixed_byte(lane, a.ids + 16 * i, a.times[i], a.ps_bytes, a.leader_config_id, a.lenc_len,
                                               a.lct_len, a.helper_config_id, a.henc_len, a.hct_len, &at);
      p[at] = v;
    }
    if (a.ps_bytes) wave_copy(p + l.ps_off, a.ps + i * a.ps_bytes, a.ps_bytes, lane);
  }
  wave_copy_part(p + l.lenc_off, a.lencs + i * a.lenc_len, a.lenc_len, lane, part, parts);
  wave_copy_part(p + l.lpay_off, a.lcts + i * a.lct_len, a.lct_len, lane, part, parts);
  wave_copy_part(p + l.henc_off, a.hencs + i * a.henc_len, a.henc_len, lane, part, parts);
  wave_copy_part(p + l.hpay_off, a.hcts + i * a.hct_len, a.hct_len, lane, part, parts);
}

inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

hipError_t launch_wire_upload_sizes(const WireUploadArgs& a, hipStream_t s) {
  if (a.n) {
    hipLaunchKernelGGL(upload_parse_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(upload_scan_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_upload_gather(const WireUploadArgs& a, uint64_t m, uint32_t parts, hipStream_t s) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(upload_gather_kernel, dim3(blocks(m * parts, 4)), dim3(256), 0, s, a, m, parts);
  return hipGetLastError();
}

hipError_t launch_wire_report_sizes(const WireReportArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(report_sizes_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_report_pack(const WireReportArgs& a, uint64_t m, uint32_t parts, hipStream_t s) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(report_pack_kernel, dim3(blocks(m * parts, 4)), dim3(256), 0, s, a, m, parts);
  return hipGetLastError();
}

}  // namespace jx
