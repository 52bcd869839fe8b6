// jx_engine_wire.cpp — wire in, wire out: an AggregationJobInitializeReq body decoded into the arrays the sealed fused
// call reads, and the AggregationJobResp body encoded from that call's outputs (the rule: jx_wire.h; the kernels:
// jx_wire.hip). A decode is three phases with the host reading the small WireState between them, because each
// phase's sizes are the one before's results: the header (is there a request, how long is its first message), the
// index (how many messages), the records with the duplicate check and the scans (how many packed bytes).
// The leader's end of the same exchange: jx_init_req_encode* writes the request body from the arrays the leader holds
// (one round trip: the body's length is a result), and jx_init_resp_decode walks the response on the host, matches it
// against the ids the request sent, and queues one upload and one kernel that fill the rows the leader's finish reads.
#include <algorithm>
#include <cstring>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "jx_engine_internal.h"
#include "jx_wire.h"

using namespace jx;
using namespace jxi;

static_assert(sizeof(jx_wire_record) == sizeof(WireRec), "jx_wire_record is WireRec");
static_assert(JX_WIRE_MALFORMED == WIRE_MALFORMED && JX_WIRE_WRONG_QUERY_TYPE == WIRE_WRONG_QUERY_TYPE &&
                  JX_WIRE_DUPLICATE_ID == WIRE_DUPLICATE_ID && JX_WIRE_NO_ERROR == WIRE_ERR_NONE,
              "the header's code points are the rule's");
static_assert(sizeof(jx_route_bucket) == sizeof(WireBucket) && JX_ROUTE_MAX_BUCKETS == WIRE_ROUTE_MAX_BUCKETS,
              "jx_route_bucket is WireBucket");
static_assert(JX_RESP_CONTINUED == RESP_CONTINUED && JX_RESP_REJECTED == RESP_REJECTED && JX_RESP_FINISHED == RESP_FINISHED &&
                  JX_RESP_MESSAGE_MISMATCH == RESP_MESSAGE_MISMATCH && JX_QUERY_FIXED_SIZE == WIRE_QUERY_FIXED_SIZE,
              "the response's results are the rule's");

struct jx_init_req {
  jx_engine* e = nullptr;
  jx_init_req_info_t info{};
  jx_init_req_arrays_t arr{};
  Mirror arrays;  // times .. wire_status with their pinned copy, then route and the two rows arrays
  Slab packed;    // the encapsulated keys and the payloads, packed
  Slab buckets;   // a routed request's bucket_index and bucket_collected
  bool routed = false;
  bool has_deadline = false;
  uint64_t deadline = 0;
  uint64_t n = 0;
  // the device arrays
  uint64_t *times = nullptr, *eoff = nullptr, *poff = nullptr;
  WireRec* recs = nullptr;
  uint8_t *ids = nullptr, *key_index = nullptr, *wire_status = nullptr, *ps = nullptr, *lps = nullptr, *encs = nullptr,
          *payloads = nullptr;
  uint32_t *route = nullptr, *bucket_index = nullptr;
  uint8_t* bucket_collected = nullptr;
};

// The leader's encoded request: which reports it sent, in order, for the response to be matched against.
struct jx_leader_req {
  jx_engine* e = nullptr;
  uint64_t n = 0, n_sent = 0, body_len = 0;
  Mirror dev;  // sent_index u32[n] | sent_ids [n x 16], and the pinned copy of both
  uint32_t* d_sent_index = nullptr;
  uint8_t* d_sent_ids = nullptr;
  const uint32_t* sent_index = nullptr;
  const uint8_t* sent_ids = nullptr;
  PinnedBuf up;  // a response decode's one upload: the body, then where each row's prep message lies
};

namespace {

void req_free(jx_init_req* r) {
  if (!r) return;
  jx_engine* e = r->e;
  r->arrays.put(e);
  if (r->packed.p) arena_put(e->arena, r->packed, e->stream);
  if (r->buckets.p) arena_put(e->arena, r->buckets, e->stream);
  r->arrays.free(e);
  delete r;
}
using ReqGuard = HandleGuard<jx_init_req, req_free>;

int32_t read_state(jx_engine* e, const WireState* d_st, WireState& st) {
  HIPCHK(e, hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

// the body is on the device, readable by work queued on the engine stream; the engine mutex is held
int32_t decode_core(jx_engine* e, const uint8_t* d_body, uint64_t len, uint32_t query_type, const uint8_t* key_first,
                    const uint8_t* key_second, const uint64_t* deadline, jx_init_req** out) {
  const Cfg& c = e->cfg;
  if (!e->wire_key_set) {  // the slot hash's key: the ids are the clients' and the peer's to choose, the key is not
    std::random_device rd;
    for (uint64_t& k : e->wire_key) k = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    e->wire_key_set = true;
  }
  ReqGuard g{new (std::nothrow) jx_init_req};
  if (!g.r) return fail(e, JX_E_NOMEM, "init req: out of host memory");
  jx_init_req* r = g.r;
  r->e = e;
  r->has_deadline = deadline != nullptr;
  r->deadline = deadline ? *deadline : 0;

  WireState* d_st = nullptr;
  uint8_t* d_keys = nullptr;
  uint32_t* d_dup = nullptr;
  auto lay0 = [&](void* base) {
    Carver cv(base);
    cv.take(d_st, sizeof(WireState));
    cv.take(d_keys, 512);
    cv.take(d_dup, 16);
    return cv.bytes();
  };
  Scratch small;
  if (const int32_t rc = scratch_carve(e, small, lay0)) return rc;
  HIPCHK(e, hipMemsetAsync(d_st, 0, sizeof(WireState), e->stream));
  uint8_t keys[512];
  memcpy(keys, key_first, 256);
  memcpy(keys + 256, key_second, 256);
  HIPCHK(e, hipMemcpyAsync(d_keys, keys, 512, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(d_dup, 0xFF, 16, e->stream));

  // ---- phase 1: the header
  HIPCHK(e, launch_wire_header(d_body, len, query_type, d_st, e->stream));
  WireState st;
  if (const int32_t rc = read_state(e, d_st, st)) return rc;
  jx_init_req_info_t& info = r->info;
  const WireHeader& h = st.hdr;
  auto refuse = [&](uint32_t status, uint64_t at) {
    info.status = status;
    info.error_offset = at;
    *out = g.give();
    return JX_OK;
  };
  if (h.status != WIRE_OK) return refuse(h.status, h.err_off);
  info.has_batch_id = h.has_batch_id;
  memcpy(info.batch_id, h.batch_id, 32);
  info.agg_param_off = h.param_off;
  info.agg_param_len = h.param_len;
  if (h.start == h.end) {  // no PrepareInit: an empty, valid request
    *out = g.give();
    return JX_OK;
  }

  // ---- phase 2: the index. The fallback loop writes where its messages start as it counts them when a table for
  // the most messages the vector can hold is affordable; else it runs again once they are counted.
  const uint64_t cands = h.l0 ? (h.end - h.start) / h.l0 : 0;
  const uint64_t most = (h.end - h.start) / WIRE_MIN_PREPARE_INIT + 1;
  const bool one_pass = most * 8 <= (64ull << 20);
  Scratch offs_mem;
  uint64_t* d_offs = nullptr;
  if (one_pass) {
    if (const int32_t rc = scratch_get(e, most * 8, offs_mem)) return rc;
    d_offs = (uint64_t*)offs_mem.p();
  }
  HIPCHK(e, launch_wire_index(d_body, d_st, cands, true, d_offs, one_pass ? most : 0, e->stream));
  if (const int32_t rc = read_state(e, d_st, st)) return rc;
  info.fallback_iterations = st.iters;
  if (st.status != WIRE_OK) return refuse(st.status, st.err_off);
  const uint64_t n = st.n, nfast = st.nfast;
  if (const int32_t rc = call_count_ok(e, n, "init req", "PrepareInits")) return rc;
  if (nfast < n && !one_pass) {
    if (const int32_t rc = scratch_get(e, (n - nfast) * 8, offs_mem)) return rc;
    d_offs = (uint64_t*)offs_mem.p();
    HIPCHK(e, launch_wire_index(d_body, d_st, cands, false, d_offs, n - nfast, e->stream));
  }

  // ---- phase 3: records, per-report scalars, the duplicate check, the scans
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(r->times, n * 8);
    cv.take(r->eoff, (n + 1) * 8);
    cv.take(r->poff, (n + 1) * 8);
    cv.take(r->recs, n * sizeof(WireRec));
    cv.take(r->ids, n * 16);
    cv.take(r->key_index, n * 2);
    cv.take(r->wire_status, n);
    r->arrays.host_bytes = cv.mark();  // up to here: one copy to the pinned buffer
    cv.take(r->route, n * 4);
    cv.take(r->ps, n * c.ps_bytes);
    cv.take(r->lps, n * c.lps_bytes);
    return cv.bytes();
  };
  if (const int32_t rc = slab_carve(e, r->arrays.slab, lay, "init req arrays")) return rc;
  const uint64_t slots = 2 * n;
  Scratch tab;
  if (const int32_t rc = scratch_get(e, slots * 4, tab)) return rc;
  HIPCHK(e, hipMemsetAsync(tab.p(), 0, slots * 4, e->stream));
  WireDecodeArgs a{};
  a.body = d_body;
  a.n = n;
  a.nfast = nfast;
  a.start = h.start;
  a.end = h.end;
  a.l0 = h.l0;
  a.offs = d_offs;
  a.ps_bytes = c.ps_bytes;
  a.lps_bytes = c.lps_bytes;
  a.has_deadline = r->has_deadline;
  a.deadline = r->deadline;
  a.key_first = d_keys;
  a.key_second = d_keys + 256;
  a.st = d_st;
  a.recs = r->recs;
  a.times = r->times;
  a.wire_status = r->wire_status;
  a.key_index = r->key_index;
  a.route = r->route;
  a.enc_offsets = r->eoff;
  a.payload_offsets = r->poff;
  a.ids = r->ids;
  a.ps = r->ps;
  a.lps = r->lps;
  HIPCHK(e, launch_wire_records(a, (uint32_t*)tab.p(), slots, d_dup, e->wire_key[0], e->wire_key[1], e->stream));
  if (const int32_t rc = read_state(e, d_st, st)) return rc;
  info.n = n;
  if (st.dup != WIRE_NO_DUPLICATE) {
    info.status = WIRE_DUPLICATE_ID;
    info.duplicate_index = st.dup;
    r->arrays.put(e);
    *out = g.give();
    return JX_OK;
  }
  info.odd_public_shares = st.odd_ps;
  info.enc_bytes = st.enc_total;
  info.payload_bytes = st.pay_total;

  // ---- the copy into the rows and the packed arrays, and the pinned copy of the small ones
  auto layp = [&](void* base) {
    Carver cv(base);
    cv.take(r->encs, st.enc_total);
    cv.take(r->payloads, st.pay_total);
    return cv.bytes();
  };
  if (const int32_t rc = slab_carve(e, r->packed, layp, "init req ciphertexts")) return rc;
  a.encs = r->encs;
  a.payloads = r->payloads;
  HIPCHK(e, launch_wire_gather(a, e->stream));
  if (const int32_t rc = r->arrays.download(e)) return rc;
  const Mirror& M = r->arrays;
  r->n = n;
  jx_init_req_arrays_t& A = r->arr;
  A.d_report_ids = r->ids;
  A.d_times = r->times;
  A.d_public_shares = c.ps_bytes ? r->ps : nullptr;
  A.d_leader_prep_shares = r->lps;
  A.d_encs = r->encs;
  A.d_enc_offsets = r->eoff;
  A.d_payloads = r->payloads;
  A.d_payload_offsets = r->poff;
  A.d_key_index = r->key_index;
  A.d_wire_status = r->wire_status;
  A.d_route = r->route;
  A.d_records = r->recs;
  A.times = M.host_of(r->times);
  A.enc_offsets = M.host_of(r->eoff);
  A.payload_offsets = M.host_of(r->poff);
  A.records = (const jx_wire_record*)M.host_of(r->recs);
  A.report_ids = M.host_of(r->ids);
  A.key_index = M.host_of(r->key_index);
  A.wire_status = M.host_of(r->wire_status);
  *out = g.give();
  return JX_OK;
}

bool decode_args_ok(jx_engine* e, const void* body, uint64_t len, uint32_t q, const uint8_t* k0, const uint8_t* k1,
                    jx_init_req** out) {
  return e && out && (body || len == 0) && k0 && k1 && (q == JX_QUERY_TIME_INTERVAL || q == JX_QUERY_FIXED_SIZE);
}

int32_t encode_core(jx_engine* e, jx_init_req* r, const void* d_verdicts, const void* d_open_status,
                    const void* d_prep_msgs, uint64_t prep_msg_stride, const uint8_t* host_errors, const uint8_t* replayed,
                    void* out, bool out_on_device, uint64_t capacity, uint64_t* out_len, void* out_finished) {
  if (!e || !r || r->e != e || !out || !out_len) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (r->info.status != WIRE_OK) return fail(e, JX_E_STATE, "init resp: the request was refused; it has no response body");
  const uint64_t n = r->n;
  const uint32_t S = c.jr_len ? c.seed : 0;
  if (n && (!d_verdicts || !d_open_status || (S && !d_prep_msgs))) return JX_E_INVALID;
  if (prep_msg_stride == 0) prep_msg_stride = S;
  if (prep_msg_stride < S || prep_msg_stride > 0xFFFFFFFFull) return JX_E_INVALID;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t bound = 4 + n * (26ull + S);
  uint8_t *d_err = nullptr, *d_fin = nullptr, *d_herr = nullptr, *d_rep = nullptr, *d_body = nullptr;
  uint64_t* d_off = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_off, (n + 1) * 8);
    cv.take(d_err, n);
    cv.take(d_fin, n);
    cv.take(d_herr, n);
    cv.take(d_rep, n);
    if (!out_on_device) cv.take(d_body, bound);
    return cv.bytes();
  };
  Scratch mem;
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  if (n && host_errors) HIPCHK(e, hipMemcpyAsync(d_herr, host_errors, n, hipMemcpyHostToDevice, e->stream));
  if (n && replayed) HIPCHK(e, hipMemcpyAsync(d_rep, replayed, n, hipMemcpyHostToDevice, e->stream));
  WireEncodeArgs a{};
  a.n = n;
  a.ids = r->ids;
  a.times = r->times;
  a.wire_status = r->wire_status;
  a.verdicts = (const uint8_t*)d_verdicts;
  a.open_status = (const uint8_t*)d_open_status;
  a.prep_msgs = (const uint8_t*)d_prep_msgs;
  a.host_err = n && host_errors ? d_herr : nullptr;
  a.replayed = n && replayed ? d_rep : nullptr;
  a.bucket_collected = n && r->routed ? r->bucket_collected : nullptr;
  a.prep_msg_bytes = S;
  a.prep_msg_stride = (uint32_t)prep_msg_stride;
  a.has_deadline = r->has_deadline;
  a.deadline = r->deadline;
  a.err = d_err;
  a.finished = d_fin;
  a.offsets = d_off;
  a.out = out_on_device ? (uint8_t*)out : d_body;
  HIPCHK(e, launch_wire_encode_sizes(a, e->stream));
  uint64_t items = 0;
  HIPCHK(e, hipMemcpyAsync(&items, d_off + n, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (items > 0xFFFFFFFFull) return fail(e, JX_E_UNSUPPORTED, "init resp: the PrepareResps exceed a u32 byte length");
  if (capacity < 4 + items) return fail(e, JX_E_INVALID, "init resp: the output buffer is shorter than the response body");
  HIPCHK(e, launch_wire_encode_pack(a, e->stream));
  if (!out_on_device) HIPCHK(e, hipMemcpyAsync(out, d_body, 4 + items, hipMemcpyDeviceToHost, e->stream));
  if (n && out_finished)
    HIPCHK(e, hipMemcpyAsync(out_finished, d_fin, n, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *out_len = 4 + items;
  return JX_OK;
}

// ---- the leader's end

void leader_req_free(jx_leader_req* r) {
  if (!r) return;
  jx_engine* e = r->e;
  if (r->up.ev) (void)hipEventSynchronize(r->up.ev);  // the last decode's upload has read the pinned buffer
  r->up.destroy();
  r->dev.free(e);
  delete r;
}
using LeaderReqGuard = HandleGuard<jx_leader_req, leader_req_free>;

// what both forms of the request encode take; the bulk pointers are device pointers by the time req_encode_core runs
struct ReqIn {
  uint64_t n;
  const uint8_t *ids, *ps, *encs, *payloads, *lps, *verdicts;
  const uint64_t* times;
  const uint8_t* config_ids;
  const uint64_t *enc_offsets, *payload_offsets;
  uint64_t lps_stride;
  const uint8_t *exclude, *agg_param;
  uint64_t agg_param_len;
  uint32_t query_type;
  const uint8_t* batch_id;
};

// everything that can be refused from the host arrays alone; the bound assumes every report is sent
int32_t req_check(jx_engine* e, const ReqIn& in, uint64_t* bound) {
  const Cfg& c = e->cfg;
  if (in.query_type != JX_QUERY_TIME_INTERVAL && in.query_type != JX_QUERY_FIXED_SIZE) return JX_E_INVALID;
  if (in.query_type == JX_QUERY_FIXED_SIZE && !in.batch_id) return JX_E_INVALID;
  if (in.agg_param_len > 0xFFFFFFFFull || (in.agg_param_len && !in.agg_param)) return JX_E_INVALID;
  if (const int32_t rc = call_count_ok(e, in.n, "init req encode", "reports")) return rc;
  if (in.n && (!in.ids || !in.times || !in.config_ids || !in.payload_offsets || !in.encs || !in.lps || !in.verdicts ||
               (c.ps_bytes && !in.ps)))
    return JX_E_INVALID;
  uint64_t vec = 0;
  for (uint64_t i = 0; i < in.n; i++) {
    if ((in.enc_offsets && in.enc_offsets[i + 1] < in.enc_offsets[i]) || in.payload_offsets[i + 1] < in.payload_offsets[i])
      return fail(e, JX_E_INVALID, "init req encode: offsets must not decrease");
    const uint64_t el = in.enc_offsets ? in.enc_offsets[i + 1] - in.enc_offsets[i] : 32;
    const uint64_t pl = in.payload_offsets[i + 1] - in.payload_offsets[i];
    const uint32_t bad = wire_req_field_check(el, pl);
    if (bad == WIRE_REQ_LONG_KEY) return fail(e, JX_E_INVALID, "init req encode: an encapsulated key of 2^16 bytes or more");
    if (bad) return fail(e, JX_E_INVALID, "init req encode: a payload of 2^32 bytes or more");
    vec += wire_init_len(c.ps_bytes, el, pl, c.lps_bytes);
  }
  if (in.n && in.payload_offsets[in.n] - in.payload_offsets[0] && !in.payloads) return JX_E_INVALID;
  *bound = wire_req_header_len(in.agg_param_len, in.query_type) + vec;
  return JX_OK;
}

// the engine mutex is held; in's bulk pointers are on the device; d_out holds `capacity` bytes
int32_t req_encode_core(jx_engine* e, const ReqIn& in, uint8_t* d_out, uint64_t capacity, uint64_t* out_len,
                        jx_leader_req** out_req, bool may_wait) {
  const Cfg& c = e->cfg;
  const uint64_t n = in.n;
  LeaderReqGuard g{new (std::nothrow) jx_leader_req};
  if (!g.r) return fail(e, JX_E_NOMEM, "init req encode: out of host memory");
  jx_leader_req* r = g.r;
  r->e = e;
  r->n = n;
  WireReqArgs a{};
  uint64_t *d_times = nullptr, *d_eoff = nullptr, *d_poff = nullptr;
  uint8_t *d_cfg = nullptr, *d_excl = nullptr, *d_param = nullptr, *d_bid = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_times, n * 8);
    cv.take(d_eoff, (n + 1) * 8);
    cv.take(d_poff, (n + 1) * 8);
    cv.take(d_cfg, n);
    cv.take(d_excl, n);
    cv.take(d_param, in.agg_param_len);
    cv.take(d_bid, 32);
    cv.take(a.msg_len, n * 8);
    cv.take(a.send, n);
    cv.take(a.offsets, (n + 1) * 8);
    cv.take(a.rank, (n + 1) * 8);
    cv.take(a.totals, sizeof(WireReqTotals));
    return cv.bytes();
  };
  Scratch mem;
  if (const int32_t rc = scratch_carve(e, mem, lay, may_wait)) return rc;
  auto layh = [&](void* base) {
    Carver cv(base);
    cv.take(r->d_sent_index, n * 4);
    cv.take(r->d_sent_ids, n * 16);
    return r->dev.host_bytes = cv.mark();  // all of it has a pinned copy
  };
  if (const int32_t rc = slab_carve(e, r->dev.slab, layh, "init req encode")) return rc;
  if (n) {
    HIPCHK(e, hipMemcpyAsync(d_times, in.times, n * 8, hipMemcpyHostToDevice, e->stream));
    if (in.enc_offsets) HIPCHK(e, hipMemcpyAsync(d_eoff, in.enc_offsets, (n + 1) * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_poff, in.payload_offsets, (n + 1) * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_cfg, in.config_ids, n, hipMemcpyHostToDevice, e->stream));
    if (in.exclude) HIPCHK(e, hipMemcpyAsync(d_excl, in.exclude, n, hipMemcpyHostToDevice, e->stream));
  }
  if (in.agg_param_len)
    HIPCHK(e, hipMemcpyAsync(d_param, in.agg_param, in.agg_param_len, hipMemcpyHostToDevice, e->stream));
  if (in.query_type == JX_QUERY_FIXED_SIZE)
    HIPCHK(e, hipMemcpyAsync(d_bid, in.batch_id, 32, hipMemcpyHostToDevice, e->stream));
  a.n = n;
  a.ids = in.ids;
  a.ps = in.ps;
  a.encs = in.encs;
  a.payloads = in.payloads;
  a.lps = in.lps;
  a.verdicts = in.verdicts;
  a.times = d_times;
  a.config_ids = d_cfg;
  a.enc_offsets = in.enc_offsets ? d_eoff : nullptr;
  a.payload_offsets = d_poff;
  a.exclude = in.exclude ? d_excl : nullptr;
  a.ps_bytes = c.ps_bytes;
  a.lps_bytes = c.lps_bytes;
  a.lps_stride = in.lps_stride;
  a.agg_param = d_param;
  a.batch_id = d_bid;
  a.agg_param_len = (uint32_t)in.agg_param_len;
  a.query_type = in.query_type;
  a.header_len = wire_req_header_len(in.agg_param_len, in.query_type);
  a.sent_index = r->d_sent_index;
  a.sent_ids = r->d_sent_ids;
  a.out = d_out;
  HIPCHK(e, launch_wire_req_sizes(a, e->stream));
  WireReqTotals t{};
  HIPCHK(e, hipMemcpyAsync(&t, a.totals, sizeof t, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (t.vec_bytes > 0xFFFFFFFFull) return fail(e, JX_E_UNSUPPORTED, "init req encode: the PrepareInits exceed a u32 byte length");
  const uint64_t total = a.header_len + t.vec_bytes;
  if (capacity < total) return fail(e, JX_E_INVALID, "init req encode: the output buffer is shorter than the request body");
  HIPCHK(e, launch_wire_req_pack(a, t.n_sent, (uint32_t)t.vec_bytes, e->stream));
  if (const int32_t rc = r->dev.download(e)) return rc;
  r->sent_index = r->dev.host_of(r->d_sent_index);
  r->sent_ids = r->dev.host_of(r->d_sent_ids);
  r->n_sent = t.n_sent;
  r->body_len = total;
  *out_len = total;
  *out_req = g.give();
  return JX_OK;
}

}  // namespace

extern "C" {

int32_t jx_init_req_decode_device(jx_engine* e, const void* d_body, uint64_t len, uint32_t expected_query_type,
                                  const uint8_t key_first[256], const uint8_t key_second[256],
                                  const uint64_t* report_deadline, jx_init_req** out) {
  if (!decode_args_ok(e, d_body, len, expected_query_type, key_first, key_second, out)) return JX_E_INVALID;
  *out = nullptr;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  return decode_core(e, (const uint8_t*)d_body, len, expected_query_type, key_first, key_second, report_deadline, out);
}

int32_t jx_init_req_decode(jx_engine* e, const uint8_t* body, uint64_t len, uint32_t expected_query_type,
                           const uint8_t key_first[256], const uint8_t key_second[256], const uint64_t* report_deadline,
                           jx_init_req** out) {
  if (!decode_args_ok(e, body, len, expected_query_type, key_first, key_second, out)) return JX_E_INVALID;
  *out = nullptr;
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  Scratch mem;  // the body's one copy to the device; the call holds nothing else yet: it may wait for the arena
  if (const int32_t rc = scratch_get(e, len ? len : 1, mem, true)) return rc;
  if (len) HIPCHK(e, hipMemcpyAsync(mem.p(), body, len, hipMemcpyHostToDevice, e->stream));
  return decode_core(e, mem.p(), len, expected_query_type, key_first, key_second, report_deadline, out);
}

int32_t jx_init_req_info(const jx_init_req* r, jx_init_req_info_t* out) {
  if (!r || !out) return JX_E_INVALID;
  *out = r->info;
  return JX_OK;
}

int32_t jx_init_req_arrays(const jx_init_req* r, jx_init_req_arrays_t* out) {
  if (!r || !out) return JX_E_INVALID;
  if (r->info.status != WIRE_OK) return JX_E_STATE;
  *out = r->arr;
  return JX_OK;
}

int32_t jx_init_req_exclude(jx_init_req* r, const uint8_t* exclude) {
  if (!r || !exclude) return JX_E_INVALID;
  jx_engine* e = r->e;
  LOCK(e);
  if (r->info.status != WIRE_OK) return fail(e, JX_E_STATE, "init req: the request was refused; it routes nothing");
  if (r->n == 0) return JX_OK;
  HIPCHK(e, hipSetDevice(e->device));
  Scratch mem;
  if (const int32_t rc = scratch_get(e, r->n, mem, true)) return rc;
  HIPCHK(e, hipMemcpyAsync(mem.p(), exclude, r->n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, launch_wire_exclude(r->route, mem.p(), r->n, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the caller's mask has been read
  return JX_OK;
}

int32_t jx_init_req_route(jx_engine* e, jx_init_req* r, uint64_t time_precision, const uint64_t* collected_starts,
                          uint64_t ncollected, uint32_t* out_status, uint32_t* out_nbuckets, jx_route_bucket* out_buckets) {
  if (!e || !r || r->e != e || !out_status || !out_nbuckets || !out_buckets || (ncollected && !collected_starts))
    return JX_E_INVALID;
  LOCK(e);
  if (time_precision == 0) return fail(e, JX_E_INVALID, "init req route: the time precision must not be 0");
  if (r->info.status != WIRE_OK) return fail(e, JX_E_STATE, "init req route: the request was refused; it routes nothing");
  if (r->info.has_batch_id) return fail(e, JX_E_INVALID, "init req route: a FixedSize request has one batch, its batch id's");
  if (r->routed) return fail(e, JX_E_STATE, "init req route: the request is routed already");
  *out_status = JX_ROUTE_OK;
  *out_nbuckets = 0;
  const uint64_t n = r->n;
  if (n == 0) {
    r->routed = true;
    return JX_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<uint64_t> collected(collected_starts, collected_starts + ncollected);
  std::sort(collected.begin(), collected.end());
  collected.erase(std::unique(collected.begin(), collected.end()), collected.end());
  WireRouteArgs a{};
  a.n = n;
  a.times = r->times;
  a.precision = time_precision;
  a.ncollected = collected.size();
  a.slots = 2 * n;
  a.k0 = e->wire_key[0];
  a.k1 = e->wire_key[1];
  a.route = r->route;
  uint64_t* d_collected = nullptr;
  size_t zeroed = 0;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(a.st, sizeof(WireRouteState));
    cv.take(a.tab, a.slots * 4);
    zeroed = cv.bytes();  // up to here: one memset
    cv.take(a.buckets, sizeof(WireBucket) * WIRE_ROUTE_MAX_BUCKETS);
    cv.take(a.list, 4 * WIRE_ROUTE_MAX_BUCKETS);
    cv.take(a.rank, n * 4);
    cv.take(d_collected, a.ncollected * 8);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else yet: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  Slab out;
  auto layb = [&](void* base) {
    Carver cv(base);
    cv.take(a.bucket_index, n * 4);
    cv.take(a.bucket_collected, n);
    return cv.bytes();
  };
  if (const int32_t rc = slab_carve(e, out, layb, "init req buckets")) return rc;
  struct PutBack {  // the per-report arrays go back unless the handle takes them
    jx_engine* e;
    Slab* s;
    ~PutBack() {
      if (s) arena_put(e->arena, *s, e->stream);
    }
  } back{e, &out};
  a.collected = d_collected;
  HIPCHK(e, hipMemsetAsync(a.st, 0, zeroed, e->stream));
  if (a.ncollected)
    HIPCHK(e, hipMemcpyAsync(d_collected, collected.data(), a.ncollected * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, launch_wire_route(a, e->stream));
  WireRouteState st{};
  std::vector<WireBucket> table(WIRE_ROUTE_MAX_BUCKETS);
  HIPCHK(e, hipMemcpyAsync(&st, a.st, sizeof st, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(table.data(), a.buckets, sizeof(WireBucket) * WIRE_ROUTE_MAX_BUCKETS, hipMemcpyDeviceToHost,
                           e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (st.claims > WIRE_ROUTE_MAX_BUCKETS) {
    *out_status = JX_ROUTE_TOO_MANY_BUCKETS;
    return JX_OK;
  }
  memcpy(out_buckets, table.data(), sizeof(WireBucket) * st.claims);
  *out_nbuckets = st.claims;
  back.s = nullptr;
  r->buckets = out;
  r->bucket_index = a.bucket_index;
  r->bucket_collected = a.bucket_collected;
  r->routed = true;
  return JX_OK;
}

int32_t jx_init_req_route_arrays(const jx_init_req* r, const void** d_bucket_index, const void** d_bucket_collected) {
  if (!r) return JX_E_INVALID;
  if (!r->routed) return JX_E_STATE;
  if (d_bucket_index) *d_bucket_index = r->bucket_index;
  if (d_bucket_collected) *d_bucket_collected = r->bucket_collected;
  return JX_OK;
}

int32_t jx_init_resp_encode_device(jx_engine* e, jx_init_req* r, const void* d_verdicts, const void* d_open_status,
                                   const void* d_prep_msgs, uint64_t prep_msg_stride, const uint8_t* host_errors,
                                   const uint8_t* replayed, void* d_out, uint64_t capacity, uint64_t* out_len,
                                   void* d_out_finished) {
  return encode_core(e, r, d_verdicts, d_open_status, d_prep_msgs, prep_msg_stride, host_errors, replayed, d_out, true,
                     capacity, out_len, d_out_finished);
}

int32_t jx_init_resp_encode(jx_engine* e, jx_init_req* r, const void* d_verdicts, const void* d_open_status,
                            const void* d_prep_msgs, uint64_t prep_msg_stride, const uint8_t* host_errors,
                            const uint8_t* replayed, uint8_t* out, uint64_t capacity, uint64_t* out_len,
                            uint8_t* out_finished) {
  return encode_core(e, r, d_verdicts, d_open_status, d_prep_msgs, prep_msg_stride, host_errors, replayed, out, false,
                     capacity, out_len, out_finished);
}

void jx_init_req_release(jx_init_req* r) { handle_release(r, req_free); }

int32_t jx_init_req_encode_bound(const jx_engine* e, uint64_t n, const uint64_t* enc_offsets, const uint64_t* payload_offsets,
                                 uint64_t agg_param_len, uint32_t query_type, uint64_t* out_bound) {
  if (!e || !out_bound || (n && !payload_offsets)) return JX_E_INVALID;
  const uint32_t st = wire_req_total(n, e->cfg.ps_bytes, e->cfg.lps_bytes, enc_offsets, payload_offsets, nullptr,
                                     agg_param_len, query_type, out_bound);
  if (st == WIRE_REQ_LONG_VECTOR) return JX_E_UNSUPPORTED;
  return st == WIRE_REQ_OK ? JX_OK : JX_E_INVALID;
}

int32_t jx_init_req_encode_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                  const void* d_public_shares, const uint8_t* config_ids, const void* d_encs,
                                  const uint64_t* enc_offsets, const void* d_payloads, const uint64_t* payload_offsets,
                                  const void* d_prep_shares, uint64_t prep_share_stride, const void* d_verdicts,
                                  const uint8_t* exclude, const uint8_t* agg_param, uint64_t agg_param_len,
                                  uint32_t query_type, const uint8_t* batch_id, void* d_out, uint64_t capacity,
                                  uint64_t* out_len, jx_leader_req** out_req) {
  if (!e || !d_out || !out_len || !out_req) return JX_E_INVALID;
  *out_req = nullptr;
  LOCK(e);
  if (prep_share_stride == 0) prep_share_stride = e->cfg.lps_bytes;
  if (prep_share_stride < e->cfg.lps_bytes) return JX_E_INVALID;
  const ReqIn in{n, (const uint8_t*)d_report_ids, (const uint8_t*)d_public_shares, (const uint8_t*)d_encs,
                 (const uint8_t*)d_payloads, (const uint8_t*)d_prep_shares, (const uint8_t*)d_verdicts, times, config_ids,
                 enc_offsets, payload_offsets, prep_share_stride, exclude, agg_param, agg_param_len, query_type, batch_id};
  uint64_t bound = 0;
  if (const int32_t rc = req_check(e, in, &bound)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  return req_encode_core(e, in, (uint8_t*)d_out, capacity, out_len, out_req, true);
}

int32_t jx_init_req_encode(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                           const uint8_t* public_shares, const uint8_t* config_ids, const uint8_t* encs,
                           const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                           const uint8_t* prep_shares, uint64_t prep_share_stride, const uint8_t* verdicts,
                           const uint8_t* exclude, const uint8_t* agg_param, uint64_t agg_param_len, uint32_t query_type,
                           const uint8_t* batch_id, uint8_t* out, uint64_t capacity, uint64_t* out_len,
                           jx_leader_req** out_req) {
  if (!e || !out || !out_len || !out_req) return JX_E_INVALID;
  *out_req = nullptr;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (prep_share_stride == 0) prep_share_stride = c.lps_bytes;
  if (prep_share_stride < c.lps_bytes) return JX_E_INVALID;
  ReqIn in{n, report_ids, public_shares, encs, payloads, prep_shares, verdicts, times, config_ids,
           enc_offsets, payload_offsets, prep_share_stride, exclude, agg_param, agg_param_len, query_type, batch_id};
  uint64_t bound = 0;
  if (const int32_t rc = req_check(e, in, &bound)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t e0 = n && enc_offsets ? enc_offsets[0] : 0, e1 = n ? (enc_offsets ? enc_offsets[n] : 32 * n) : 0;
  const uint64_t p0 = n ? payload_offsets[0] : 0, p1 = n ? payload_offsets[n] : 0;
  uint8_t *d_ids = nullptr, *d_ps = nullptr, *d_encs = nullptr, *d_pay = nullptr, *d_lps = nullptr, *d_v = nullptr,
          *d_body = nullptr;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(d_ids, n * 16);
    cv.take(d_ps, n * c.ps_bytes);
    cv.take(d_encs, e1 - e0);
    cv.take(d_pay, p1 - p0);
    cv.take(d_lps, n * prep_share_stride);
    cv.take(d_v, n);
    cv.take(d_body, bound);
    return cv.bytes();
  };
  Scratch mem;  // the call holds nothing else yet: it may wait for the arena
  if (const int32_t rc = scratch_carve(e, mem, lay, true)) return rc;
  if (n) {
    HIPCHK(e, hipMemcpyAsync(d_ids, report_ids, n * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    if (e1 > e0) HIPCHK(e, hipMemcpyAsync(d_encs, encs + e0, e1 - e0, hipMemcpyHostToDevice, e->stream));
    if (p1 > p0) HIPCHK(e, hipMemcpyAsync(d_pay, payloads + p0, p1 - p0, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_lps, prep_shares, (n - 1) * prep_share_stride + c.lps_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(d_v, verdicts, n, hipMemcpyHostToDevice, e->stream));
  }
  in.ids = d_ids;
  in.ps = d_ps;
  in.encs = d_encs - e0;  // the kernels index from the offset arrays' zero
  in.payloads = d_pay - p0;
  in.lps = d_lps;
  in.verdicts = d_v;
  uint64_t len = 0;
  jx_leader_req* r = nullptr;
  if (const int32_t rc = req_encode_core(e, in, d_body, bound, &len, &r, false)) return rc;
  LeaderReqGuard g{r};
  if (capacity < len) return fail(e, JX_E_INVALID, "init req encode: the output buffer is shorter than the request body");
  HIPCHK(e, hipMemcpyAsync(out, d_body, len, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *out_len = len;
  *out_req = g.give();
  return JX_OK;
}

int32_t jx_leader_req_info(const jx_leader_req* r, jx_leader_req_info_t* out) {
  if (!r || !out) return JX_E_INVALID;
  out->n = r->n;
  out->n_sent = r->n_sent;
  out->body_len = r->body_len;
  return JX_OK;
}

int32_t jx_leader_req_sent(const jx_leader_req* r, const uint32_t** sent_index, const void** d_sent_index) {
  if (!r) return JX_E_INVALID;
  if (sent_index) *sent_index = r->sent_index;
  if (d_sent_index) *d_sent_index = r->d_sent_index;
  return JX_OK;
}

int32_t jx_init_resp_decode(jx_engine* e, jx_leader_req* r, const uint8_t* body, uint64_t len, void* d_out_prep_msgs,
                            uint64_t prep_msg_stride, void* d_out_peer_verdicts, uint8_t* out_result, uint8_t* out_error,
                            jx_init_resp_info_t* info) {
  if (!e || !r || r->e != e || !info || (!body && len)) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  const uint32_t PM = c.jr_len ? c.seed : 0;
  const uint64_t n = r->n, ns = r->n_sent;
  if (prep_msg_stride == 0) prep_msg_stride = PM;
  if (prep_msg_stride < PM) return JX_E_INVALID;
  if (n && (!d_out_peer_verdicts || (PM && !d_out_prep_msgs))) return JX_E_INVALID;
  if (ns && (!out_result || !out_error)) return JX_E_INVALID;
  *info = jx_init_resp_info_t{};
  std::vector<WireRespRec> recs(ns ? ns : 1);
  const WireWalk w = wire_resp_walk(body, len, recs.data(), ns);
  info->n = w.n;
  if (w.status != WIRE_OK) {
    info->status = JX_WIRE_MALFORMED;
    info->error_offset = w.err_off;
    info->n = 0;
    return JX_OK;
  }
  // "missing, duplicate, out-of-order, or unexpected prepare steps": the first position that differs
  const uint64_t both = w.n < ns ? w.n : ns;
  uint64_t bad = both;
  for (uint64_t k = 0; k < both; k++)
    if (memcmp(body + recs[k].off, r->sent_ids + 16 * k, 16) != 0) {
      bad = k;
      break;
    }
  if (bad < both || w.n != ns) {
    info->status = JX_WIRE_RESP_MISMATCH;
    info->mismatch_index = bad;
    return JX_OK;
  }
  if (n == 0) return JX_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const uint64_t rows_at = (len + 7) / 8 * 8;
  void* hp = nullptr;
  HIPCHK(e, r->up.reserve(rows_at + n * 8, &hp));
  if (len) memcpy(hp, body, len);
  uint64_t* pm_off = (uint64_t*)((uint8_t*)hp + rows_at);
  for (uint64_t i = 0; i < n; i++) pm_off[i] = WIRE_RESP_NO_MESSAGE;
  for (uint64_t k = 0; k < ns; k++) {
    const uint8_t res = wire_resp_classify(recs[k], PM);
    out_result[k] = res;
    out_error[k] = res == RESP_CONTINUED ? (uint8_t)WIRE_ERR_NONE : res == RESP_REJECTED ? recs[k].error : (uint8_t)WIRE_ERR_VDAF_PREP;
    if (res == RESP_CONTINUED) pm_off[r->sent_index[k]] = recs[k].pm_off;
  }
  Scratch mem;
  if (const int32_t rc = scratch_get(e, rows_at + n * 8, mem, true)) return rc;
  HIPCHK(e, hipMemcpyAsync(mem.p(), hp, rows_at + n * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, r->up.mark(e->stream));
  WireRespArgs a{};
  a.n = n;
  a.body = mem.p();
  a.pm_off = (const uint64_t*)(mem.p() + rows_at);
  a.pm_bytes = PM;
  a.pm_stride = prep_msg_stride;
  a.prep_msgs = (uint8_t*)d_out_prep_msgs;
  a.peer_verdicts = (uint8_t*)d_out_peer_verdicts;
  HIPCHK(e, launch_wire_resp_scatter(a, e->stream));
  return JX_OK;
}

void jx_leader_req_release(jx_leader_req* r) { handle_release(r, leader_req_free); }

}  // extern "C"
