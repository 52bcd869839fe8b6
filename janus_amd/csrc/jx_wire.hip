// jx_wire.hip — the aggregate-init request decoded and its response encoded on the device (the rule: jx_wire.h).
//
// Decode: wire_header_kernel reads the header and the first PrepareInit's length l0. wire_fast_kernel tests the
// candidate boundary start + i * l0 in lane i of many workgroups and takes the lowest failing i with one agent-scope
// atomicMin; nothing else crosses workgroups, and the minimum is read by the next kernel, behind the kernel boundary.
// Every candidate below it has length l0 and starts where its predecessor ends, so by induction it is a true
// boundary. wire_gallop_kernel (one wave) continues from there for a body that is not uniform to the end, a pair of
// alternating lengths at a time. Then one thread per report writes its record and scalars, the duplicate check claims
// hash slots, one workgroup scans the encapsulated-key and payload lengths, and one wave per report copies its fields
// into the rows the prepare calls read.
//
// Encode: one thread per report decides its outcome (wire_outcome) and length, one workgroup scans the lengths, one
// thread per report writes its PrepareResp.
//
// The leader's end: the request body is written by wire_req_select_kernel (which reports are sent, how long each is),
// wire_req_scan_kernel (one workgroup: both exclusive scans and the compaction list) and wire_req_pack_kernel (one wave
// per sent report); the response body is walked on the host (jx_engine_wire.cpp) and wire_resp_scatter_kernel writes
// every row's prep message and peer verdict from what the walk found.
#include <hip/hip_runtime.h>

#include "../../include/jx_prio3.h"
#include "jx_wire.h"
#include "jx_wire_dev.h"  // block_exclusive_scan, wave_copy

namespace jx {
namespace {

__global__ void wire_header_kernel(const uint8_t* body, uint64_t len, uint32_t query_type, WireState* st) {
  if (blockIdx.x | threadIdx.x) return;
  WireHeader h;
  wire_parse_header(body, len, query_type, h);
  st->hdr = h;
  st->first_bad = ~0ull;
  st->status = h.status;
  st->err_off = h.err_off;
  st->dup = WIRE_NO_DUPLICATE;
}

__global__ __launch_bounds__(256) void wire_fast_kernel(const uint8_t* body, WireState* st, uint64_t cands) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const WireHeader& h = st->hdr;
  uint64_t at;
  const bool bad = i < cands && !wire_gallop_lane(body, h.end, h.start, h.l0, h.l0, i, &at);
  // one atomic per wave: its lowest failing lane's index
  const unsigned long long m = __ballot(bad);
  if (bad && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)m) - 1u)
    __hip_atomic_fetch_min(&st->first_bad, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave. offs (nullable): the start of message nfast + j for j < cap. Every lane holds the same off / n / iters.
__global__ __launch_bounds__(64) void wire_gallop_kernel(const uint8_t* body, WireState* st, uint64_t cands, uint64_t* offs,
                                                         uint64_t cap) {
  const uint32_t lane = threadIdx.x;
  const WireHeader h = st->hdr;
  uint64_t nfast = 0, off = h.start;
  if (h.l0) {
    const uint64_t fb = st->first_bad;  // the fast pass's, complete behind the kernel boundary
    nfast = fb < cands ? fb : cands;
    off = h.start + nfast * h.l0;
  }
  uint64_t n = nfast, err = 0, prev = nfast ? h.l0 : 0;  // prev: the length of the message before off (0: none)
  uint32_t iters = 0, status = WIRE_OK;
  while (off < h.end) {
    WireRec r;
    if (!wire_parse_prepare_init(body, h.end, off, r, &err)) {
      status = WIRE_MALFORMED;
      break;
    }
    const uint64_t la = r.len, lb = prev ? prev : r.len;
    uint64_t at;
    const bool ok = wire_gallop_lane(body, h.end, off, la, lb, lane, &at);
    const unsigned long long bad = ~__ballot(ok);
    const uint32_t m = bad ? (uint32_t)__ffsll((long long)bad) - 1u : WIRE_LANES;  // lane 0 is always accepted: m >= 1
    if (offs && lane < m && n - nfast + lane < cap) offs[n - nfast + lane] = at;
    n += m;
    off += (uint64_t)(m / 2) * (la + lb) + ((m & 1u) ? la : 0);
    prev = (m & 1u) ? la : lb;  // the last accepted message is candidate m - 1
    iters++;
  }
  if (lane == 0) {
    st->n = n;
    st->nfast = nfast;
    st->iters = iters;
    st->status = status;
    st->err_off = err;
  }
}

__global__ __launch_bounds__(256) void wire_records_kernel(WireDecodeArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t off = i < a.nfast ? a.start + i * a.l0 : a.offs[i - a.nfast];
  WireRec r;
  uint64_t eo;
  (void)wire_parse_prepare_init(a.body, a.end, off, r, &eo);  // a true boundary: it parsed when it was accepted
  a.recs[i] = r;
  const uint64_t t = wire_be64(a.body + off + 16);
  a.times[i] = t;
  uint8_t ws = WIRE_REPORT_OK;
  if (r.ps_len != a.ps_bytes) ws = WIRE_REPORT_ODD_PUBLIC_SHARE;
  else if (r.pp_type != 0) ws = WIRE_REPORT_NOT_INITIALIZE;
  else if (r.sh_len != a.lps_bytes) ws = WIRE_REPORT_ODD_PREP_SHARE;
  a.wire_status[i] = ws;
  const bool odd = ws == WIRE_REPORT_ODD_PUBLIC_SHARE;
  a.key_index[2 * i] = odd ? (uint8_t)JX_KEY_NONE : a.key_first[r.config_id];
  a.key_index[2 * i + 1] = odd ? (uint8_t)JX_KEY_NONE : a.key_second[r.config_id];
  a.route[i] = (ws != WIRE_REPORT_OK || (a.has_deadline && t > a.deadline)) ? 0xFFFFFFFFu : 0u;
  if (odd) atomicAdd(&a.st->odd_ps, 1u);
}

// ---- duplicate report ids. tab: 2n slots, zeroed; a slot holds index + 1. A report walks its probe chain from its
// keyed hash: an empty slot is claimed with a compare-exchange; an occupied one names its holder in the value the
// atomic returned, and the two ids are compared in the body, the kernel's input, never in anything this launch
// writes. Equal ids: the slot keeps the lower index (atomicMin), and what the atomicMin returns is an index with the
// same id, so max(i, that) has an equal id at a lower index. The atomics of one slot are totally ordered, so whichever
// of the two lowest members of a set of equal ids comes second reports the higher of them: the minimum over the
// reports is the lowest index with an earlier equal id.
__device__ bool wire_id_equal(const uint8_t* a, const uint8_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < 16; k++) d |= (uint32_t)(a[k] ^ b[k]);
  return d == 0;
}

__global__ __launch_bounds__(256) void wire_dup_kernel(const uint8_t* body, const WireRec* recs, uint64_t n, uint32_t* tab,
                                                       uint64_t slots, uint64_t k0, uint64_t k1, uint32_t* result) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* id = body + recs[i].off;
  uint64_t s = wire_id_hash(id, k0, k1) % slots;
  for (uint64_t probes = 0; probes < slots; probes++) {
    uint32_t seen = 0;
    if (__hip_atomic_compare_exchange_strong(&tab[s], &seen, (uint32_t)i + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;  // claimed
    if (wire_id_equal(id, body + recs[seen - 1u].off)) {
      const uint32_t before = __hip_atomic_fetch_min(&tab[s], (uint32_t)i + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t j = before - 1u;
      if (j != (uint32_t)i)
        __hip_atomic_fetch_min(result, j > (uint32_t)i ? j : (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = s + 1 == slots ? 0 : s + 1;
  }
}

// the second kernel: the result, complete behind the kernel boundary, into the state the host reads
__global__ void wire_dup_read_kernel(const uint32_t* result, WireState* st) {
  if (blockIdx.x | threadIdx.x) return;
  st->dup = *result;
}

__global__ __launch_bounds__(1024) void wire_scan_kernel(const WireRec* recs, uint64_t n, uint64_t* enc_offsets,
                                                         uint64_t* payload_offsets, WireState* st) {
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)recs[i].enc_len; }, enc_offsets);
  block_exclusive_scan(n, [&](uint64_t i) { return (uint64_t)recs[i].pay_len; }, payload_offsets);
  if (threadIdx.x == 0) {
    st->enc_total = enc_offsets[n];
    st->pay_total = payload_offsets[n];
  }
}

__global__ __launch_bounds__(256) void wire_gather_kernel(WireDecodeArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (i >= a.n) return;
  const WireRec r = a.recs[i];
  if (lane < 16) a.ids[16 * i + lane] = a.body[r.off + lane];
  if (a.ps_bytes) {
    uint8_t* row = a.ps + i * a.ps_bytes;
    if (r.ps_len == a.ps_bytes) wave_copy(row, a.body + r.ps_off, a.ps_bytes, lane);
    else for (uint32_t b = lane; b < a.ps_bytes; b += 64) row[b] = 0;
  }
  {
    uint8_t* row = a.lps + i * a.lps_bytes;
    if (r.pp_type == 0 && r.sh_len == a.lps_bytes) wave_copy(row, a.body + r.sh_off, a.lps_bytes, lane);
    else for (uint32_t b = lane; b < a.lps_bytes; b += 64) row[b] = 0;
  }
  wave_copy(a.encs + a.enc_offsets[i], a.body + r.enc_off, r.enc_len, lane);
  wave_copy(a.payloads + a.payload_offsets[i], a.body + r.pay_off, r.pay_len, lane);
}

__global__ __launch_bounds__(256) void wire_exclude_kernel(uint32_t* route, const uint8_t* mask, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && mask[i]) route[i] = 0xFFFFFFFFu;
}

// ---- the route: every report to its batch bucket (the rule: wire_bucket_start .. wire_route_of in jx_wire.h).
// Three launches. The claims find the distinct buckets in the hash table and give each a place in a list of at most
// WIRE_ROUTE_MAX_BUCKETS. One workgroup ranks the list's starts in LDS and writes the table's entries, empty. The last
// pass looks every report's bucket up again, writes its three per-report values and counts it in its entry. The
// reports of a request mostly arrive in time order, so the lanes of a wave mostly share a bucket: the wave's lanes are
// taken a group of equal starts at a time, and one lane of a group claims, looks up and issues the atomics for it.

// f(lead, in) for every group of active lanes with equal keys: lead is the group's lowest lane, `in` says whether
// this lane belongs to it. All 64 lanes run f, so f may use cross-lane operations.
template <class F>
__device__ void wave_groups(bool active, uint64_t key, F f) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const bool in = active && key == __shfl((unsigned long long)key, lead);
    f(lead, in);
    todo &= ~__ballot(in);  // the lead is in its group: the loop ends
  }
}

__global__ __launch_bounds__(256) void wire_route_claim_kernel(WireRouteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < a.n;
  const uint64_t b = active ? wire_bucket_start(a.times[i], a.precision) : 0;
  bool leads = false;
  wave_groups(active, b, [&](int lead, bool) { leads |= lane == lead; });
  if (!leads) return;
  auto cas = [](uint32_t* slot, uint32_t v) {
    uint32_t seen = 0;
    __hip_atomic_compare_exchange_strong(slot, &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return seen;
  };
  if (!wire_route_claim(i, a.times, a.precision, a.tab, a.slots, a.k0, a.k1, cas)) return;
  const uint32_t at = __hip_atomic_fetch_add(&a.st->claims, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (at < WIRE_ROUTE_MAX_BUCKETS) a.list[at] = (uint32_t)i;
}

// One workgroup, behind the kernel boundary of the claims. The starts are distinct, so a start's rank is the number
// of smaller ones: every thread counts them over the LDS copy, which all lanes read at the same address.
__global__ __launch_bounds__(1024) void wire_route_sort_kernel(WireRouteArgs a) {
  __shared__ uint64_t keys[WIRE_ROUTE_MAX_BUCKETS];
  const uint32_t m = a.st->claims, t = threadIdx.x;
  if (m > WIRE_ROUTE_MAX_BUCKETS) return;  // too many buckets: the whole workgroup leaves
  const uint32_t c = t < m ? a.list[t] : 0;
  if (t < m) keys[t] = wire_bucket_start(a.times[c], a.precision);
  __syncthreads();
  if (t >= m) return;
  const uint32_t r = wire_rank(keys, m, t);
  a.rank[c] = r;
  a.buckets[r] = WireBucket{keys[t], ~0ull, 0, 0, 0, wire_bucket_collected(a.collected, a.ncollected, keys[t]), 0};
}

__global__ __launch_bounds__(256) void wire_route_assign_kernel(WireRouteArgs a) {
  if (a.st->claims > WIRE_ROUTE_MAX_BUCKETS) return;  // too many buckets: route stays as it is
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < a.n;
  const uint64_t t = active ? a.times[i] : 0;
  const uint64_t b = active ? wire_bucket_start(t, a.precision) : 0;
  int my_lead = lane;
  wave_groups(active, b, [&](int lead, bool in) { my_lead = in ? lead : my_lead; });
  uint32_t k = WIRE_ROUTE_OUT;
  if (active && my_lead == lane) {
    const uint32_t c = wire_route_holder(b, a.times, a.precision, a.tab, a.slots, a.k0, a.k1);
    if (c != WIRE_ROUTE_OUT) k = a.rank[c];
  }
  k = __shfl(k, my_lead);
  const bool found = active && k < WIRE_ROUTE_MAX_BUCKETS;  // every bucket was claimed: a guard for the index below
  const bool collected = found && a.buckets[k].collected != 0;
  uint32_t to = WIRE_ROUTE_OUT;
  if (found) {
    to = wire_route_of(a.route[i], collected, k);
    a.route[i] = to;
    a.bucket_index[i] = k;
    a.bucket_collected[i] = collected;
  }
  wave_groups(found, b, [&](int lead, bool in) {
    const uint32_t reports = (uint32_t)__popcll(__ballot(in));
    const uint32_t routed = (uint32_t)__popcll(__ballot(in && to != WIRE_ROUTE_OUT));
    unsigned long long lo = in ? t : ~0ull, hi = in ? t : 0;
    if (reports > 1)  // the same for all lanes
      for (int d = 32; d; d >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
    if (lane != lead) return;
    WireBucket* e = &a.buckets[k];
    __hip_atomic_fetch_min((unsigned long long*)&e->min_time, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max((unsigned long long*)&e->max_time, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&e->reports, reports, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (routed) __hip_atomic_fetch_add(&e->routed, routed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
}

// ---- the response
__global__ __launch_bounds__(256) void wire_resp_outcome_kernel(WireEncodeArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint8_t err = wire_outcome_routed(a.host_err ? a.host_err[i] : (uint8_t)WIRE_ERR_NONE, a.open_status[i],
                                          a.has_deadline && a.times[i] > a.deadline, a.wire_status[i], a.verdicts[i],
                                          a.replayed && a.replayed[i], a.bucket_collected && a.bucket_collected[i]);
  a.err[i] = err;
  a.finished[i] = err == WIRE_ERR_NONE;
}

__global__ __launch_bounds__(1024) void wire_resp_scan_kernel(WireEncodeArgs a) {
  block_exclusive_scan(a.n, [&](uint64_t i) { return (uint64_t)wire_resp_len(a.err[i] == WIRE_ERR_NONE, a.prep_msg_bytes); },
                       a.offsets);
}

__global__ __launch_bounds__(256) void wire_resp_pack_kernel(WireEncodeArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) wire_put32(a.out, (uint32_t)a.offsets[a.n]);  // the host refuses a body of 2^32 bytes or more
  if (i >= a.n) return;
  uint8_t* p = a.out + 4 + a.offsets[i];
  const uint8_t* id = a.ids + 16 * i;
  for (int k = 0; k < 16; k++) p[k] = id[k];
  const uint8_t err = a.err[i];
  if (err != WIRE_ERR_NONE) {
    p[16] = 2;
    p[17] = err;
    return;
  }
  const uint32_t S = a.prep_msg_bytes;
  p[16] = 0;
  wire_put32(p + 17, 5 + S);
  p[21] = 2;
  wire_put32(p + 22, S);
  const uint8_t* m = a.prep_msgs + i * a.prep_msg_stride;
  for (uint32_t k = 0; k < S; k++) p[26 + k] = m[k];
}

// ---- the leader's request: which reports are sent and how long each is, the scans, one wave per sent report
__global__ __launch_bounds__(256) void wire_req_select_kernel(WireReqArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const bool send = a.verdicts[i] == JX_FINISHED && !(a.exclude && a.exclude[i]);
  const uint64_t el = a.enc_offsets ? a.enc_offsets[i + 1] - a.enc_offsets[i] : 32;
  const uint64_t pl = a.payload_offsets[i + 1] - a.payload_offsets[i];
  a.send[i] = send;
  a.msg_len[i] = send ? wire_init_len(a.ps_bytes, el, pl, a.lps_bytes) : 0;
}

__global__ __launch_bounds__(1024) void wire_req_scan_kernel(WireReqArgs a) {
  block_exclusive_scan(a.n, [&](uint64_t i) { return a.msg_len[i]; }, a.offsets);
  block_exclusive_scan(a.n, [&](uint64_t i) { return (uint64_t)a.send[i]; }, a.rank);
  // the compaction list: thread t reads back the ranks of i = t, t + 1024, .., which it stored itself
  for (uint64_t i = threadIdx.x; i < a.n; i += 1024)
    if (a.send[i]) a.sent_index[a.rank[i]] = (uint32_t)i;
  if (threadIdx.x == 0) {
    a.totals->vec_bytes = a.offsets[a.n];
    a.totals->n_sent = a.rank[a.n];
  }
}

// Wave k writes sent report k = report sent_index[k] at header_len + offsets[i]: the 44 fixed bytes one per lane, the
// four fields with wave_copy. Every destination offset is arbitrary mod 16. Thread 0 of the grid writes the header.
__global__ __launch_bounds__(256) void wire_req_pack_kernel(WireReqArgs a, uint64_t n_sent, uint32_t vec_bytes) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    (void)wire_put_req_header(a.out, a.agg_param, a.agg_param_len, a.query_type, a.batch_id, vec_bytes);
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (k >= n_sent) return;
  const uint64_t i = a.sent_index[k];
  const uint64_t eo = a.enc_offsets ? a.enc_offsets[i] : 32 * i;
  const uint32_t el = a.enc_offsets ? (uint32_t)(a.enc_offsets[i + 1] - eo) : 32u;
  const uint64_t po = a.payload_offsets[i];
  const uint32_t pl = (uint32_t)(a.payload_offsets[i + 1] - po);  // the host refused a field its prefix cannot hold
  const WireInitLayout l = wire_init_layout(a.ps_bytes, el, pl, a.lps_bytes);
  uint8_t* p = a.out + a.header_len + a.offsets[i];
  const uint8_t* id = a.ids + 16 * i;
  if (lane < WIRE_INIT_FIXED) {
    uint64_t at;
    const uint8_t v = wire_init_fixed_byte(lane, id, a.times[i], a.ps_bytes, a.config_ids[i], el, pl, a.lps_bytes, &at);
    p[at] = v;
  }
  if (lane < 16) a.sent_ids[16 * k + lane] = id[lane];
  if (a.ps_bytes) wave_copy(p + l.ps_off, a.ps + i * a.ps_bytes, a.ps_bytes, lane);
  wave_copy(p + l.enc_off, a.encs + eo, el, lane);
  wave_copy(p + l.pay_off, a.payloads + po, pl, lane);
  wave_copy(p + l.sh_off, a.lps + i * a.lps_stride, a.lps_bytes, lane);
}

// ---- the leader's response: one thread per row of the leader batch. A row without a continued response (never
// sent, rejected, Finished, a message of another kind or length) gets a non-zero peer verdict and a zero prep message,
// so the finish can never mark it finished; each row is written by one thread, so no write meets another.
__global__ __launch_bounds__(256) void wire_resp_scatter_kernel(WireRespArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t off = a.pm_off[i];
  const bool continued = off != WIRE_RESP_NO_MESSAGE;
  a.peer_verdicts[i] = continued ? 0 : 1;
  uint8_t* row = a.prep_msgs + i * a.pm_stride;
  for (uint32_t b = 0; b < a.pm_bytes; b++) row[b] = continued ? a.body[off + b] : (uint8_t)0;
}

inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

hipError_t launch_wire_req_sizes(const WireReqArgs& a, hipStream_t s) {
  if (a.n) {
    hipLaunchKernelGGL(wire_req_select_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(wire_req_scan_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_req_pack(const WireReqArgs& a, uint64_t n_sent, uint32_t vec_bytes, hipStream_t s) {
  hipLaunchKernelGGL(wire_req_pack_kernel, dim3(blocks(n_sent ? n_sent : 1, 4)), dim3(256), 0, s, a, n_sent, vec_bytes);
  return hipGetLastError();
}

hipError_t launch_wire_resp_scatter(const WireRespArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(wire_resp_scatter_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_header(const uint8_t* body, uint64_t len, uint32_t query_type, WireState* st, hipStream_t s) {
  hipLaunchKernelGGL(wire_header_kernel, dim3(1), dim3(1), 0, s, body, len, query_type, st);
  return hipGetLastError();
}

hipError_t launch_wire_index(const uint8_t* body, WireState* st, uint64_t cands, bool fast, uint64_t* offs, uint64_t cap,
                             hipStream_t s) {
  if (fast && cands) {
    hipLaunchKernelGGL(wire_fast_kernel, dim3(blocks(cands, 256)), dim3(256), 0, s, body, st, cands);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(wire_gallop_kernel, dim3(1), dim3(64), 0, s, body, st, cands, offs, cap);
  return hipGetLastError();
}

hipError_t launch_wire_records(const WireDecodeArgs& a, uint32_t* dup_tab, uint64_t slots, uint32_t* dup_result, uint64_t k0,
                               uint64_t k1, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(wire_records_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wire_dup_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a.body, (const WireRec*)a.recs, a.n, dup_tab,
                     slots, k0, k1, dup_result);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(wire_dup_read_kernel, dim3(1), dim3(1), 0, s, (const uint32_t*)dup_result, a.st);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(wire_scan_kernel, dim3(1), dim3(1024), 0, s, (const WireRec*)a.recs, a.n, a.enc_offsets,
                     a.payload_offsets, a.st);
  return hipGetLastError();
}

hipError_t launch_wire_gather(const WireDecodeArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(wire_gather_kernel, dim3(blocks(a.n, 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_exclude(uint32_t* route, const uint8_t* mask, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(wire_exclude_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, route, mask, n);
  return hipGetLastError();
}

hipError_t launch_wire_route(const WireRouteArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(wire_route_claim_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wire_route_sort_kernel, dim3(1), dim3(1024), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(wire_route_assign_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_encode_sizes(const WireEncodeArgs& a, hipStream_t s) {
  if (a.n) {
    hipLaunchKernelGGL(wire_resp_outcome_kernel, dim3(blocks(a.n, 256)), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(wire_resp_scan_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wire_encode_pack(const WireEncodeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(wire_resp_pack_kernel, dim3(blocks(a.n ? a.n : 1, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace jx
