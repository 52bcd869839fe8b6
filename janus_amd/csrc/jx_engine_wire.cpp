// jx_engine_wire.cpp — wire in, wire out: an AggregationJobInitializeReq body decoded into the arrays the sealed fused
// call reads, and the AggregationJobResp body encoded from that call's outputs (the rule: jx_wire.h; the kernels:
// jx_wire.hip). A decode is three phases with the host reading the small WireState between them, because each
// phase's sizes are the one before's results: the header (is there a request, how long is its first message), the
// index (how many messages), the records with the duplicate check and the scans (how many packed bytes).
#include <cstring>
#include <new>
#include <random>
#include <string>

#include "jx_engine_internal.h"
#include "jx_wire.h"

using namespace jx;
using namespace jxi;

static_assert(sizeof(jx_wire_record) == sizeof(WireRec), "jx_wire_record is WireRec");
static_assert(JX_WIRE_MALFORMED == WIRE_MALFORMED && JX_WIRE_WRONG_QUERY_TYPE == WIRE_WRONG_QUERY_TYPE &&
                  JX_WIRE_DUPLICATE_ID == WIRE_DUPLICATE_ID && JX_WIRE_NO_ERROR == WIRE_ERR_NONE,
              "the header's code points are the rule's");

struct jx_init_req {
  jx_engine* e = nullptr;
  jx_init_req_info_t info{};
  jx_init_req_arrays_t arr{};
  Slab arrays;  // the pinned copy's device side (times .. wire_status), then route and the two rows arrays
  Slab packed;  // the encapsulated keys and the payloads, packed
  void* host = nullptr;  // pinned
  bool has_deadline = false;
  uint64_t deadline = 0;
  uint64_t n = 0;
  // the device arrays
  uint64_t *times = nullptr, *eoff = nullptr, *poff = nullptr;
  WireRec* recs = nullptr;
  uint8_t *ids = nullptr, *key_index = nullptr, *wire_status = nullptr, *ps = nullptr, *lps = nullptr, *encs = nullptr,
          *payloads = nullptr;
  uint32_t* route = nullptr;
};

namespace {

void req_free(jx_init_req* r) {
  if (!r) return;
  jx_engine* e = r->e;
  if (r->arrays.p) arena_put(e->arena, r->arrays, e->stream);
  if (r->packed.p) arena_put(e->arena, r->packed, e->stream);
  if (r->host) (void)hipHostFree(r->host);
  delete r;
}

// frees the handle unless the decode hands it out
struct ReqGuard {
  jx_init_req* r;
  ~ReqGuard() { req_free(r); }
  jx_init_req* give() {
    jx_init_req* x = r;
    r = nullptr;
    return x;
  }
};

int32_t read_state(jx_engine* e, const WireState* d_st, WireState& st) {
  HIPCHK(e, hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

int32_t slab_get(jx_engine* e, size_t bytes, Slab& out, const char* what) {
  const hipError_t st = arena_get(e->arena, bytes, e->stream, false, false, out);
  if (st == hipErrorOutOfMemory) return fail(e, JX_E_NOMEM, std::string(what) + ": the device arena cannot hold it");
  HIPCHK(e, st);
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
  if (const int32_t rc = scratch_get(e, lay0(nullptr), small)) return rc;
  lay0(small.p());
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
  if (n >= 0x7FFFFFFFull) return fail(e, JX_E_UNSUPPORTED, "init req: more than 2^31 - 2 PrepareInits in one request");
  if (nfast < n && !one_pass) {
    if (const int32_t rc = scratch_get(e, (n - nfast) * 8, offs_mem)) return rc;
    d_offs = (uint64_t*)offs_mem.p();
    HIPCHK(e, launch_wire_index(d_body, d_st, cands, false, d_offs, n - nfast, e->stream));
  }

  // ---- phase 3: records, per-report scalars, the duplicate check, the scans
  size_t host_bytes = 0;
  auto lay = [&](void* base) {
    Carver cv(base);
    cv.take(r->times, n * 8);
    cv.take(r->eoff, (n + 1) * 8);
    cv.take(r->poff, (n + 1) * 8);
    cv.take(r->recs, n * sizeof(WireRec));
    cv.take(r->ids, n * 16);
    cv.take(r->key_index, n * 2);
    cv.take(r->wire_status, n);
    host_bytes = cv.bytes();  // up to here: one copy to the pinned buffer
    cv.take(r->route, n * 4);
    cv.take(r->ps, n * c.ps_bytes);
    cv.take(r->lps, n * c.lps_bytes);
    return cv.bytes();
  };
  if (const int32_t rc = slab_get(e, lay(nullptr), r->arrays, "init req arrays")) return rc;
  lay(r->arrays.p);
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
    arena_put(e->arena, r->arrays, e->stream);
    r->arrays = Slab{};
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
  if (const int32_t rc = slab_get(e, layp(nullptr), r->packed, "init req ciphertexts")) return rc;
  layp(r->packed.p);
  a.encs = r->encs;
  a.payloads = r->payloads;
  HIPCHK(e, launch_wire_gather(a, e->stream));
  HIPCHK(e, hipHostMalloc(&r->host, host_bytes, hipHostMallocDefault));
  HIPCHK(e, hipMemcpyAsync(r->host, r->arrays.p, host_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  r->n = n;
  const uint8_t *hb = (const uint8_t*)r->host, *db = (const uint8_t*)r->arrays.p;
  auto host_of = [&](const void* d) { return hb + ((const uint8_t*)d - db); };
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
  A.times = (const uint64_t*)host_of(r->times);
  A.enc_offsets = (const uint64_t*)host_of(r->eoff);
  A.payload_offsets = (const uint64_t*)host_of(r->poff);
  A.records = (const jx_wire_record*)host_of(r->recs);
  A.report_ids = host_of(r->ids);
  A.key_index = host_of(r->key_index);
  A.wire_status = host_of(r->wire_status);
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
  if (const int32_t rc = scratch_get(e, lay(nullptr), mem, true)) return rc;
  lay(mem.p());
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

void jx_init_req_release(jx_init_req* r) {
  if (!r) return;
  std::lock_guard<FairMutex> lk(r->e->mu);
  (void)hipSetDevice(r->e->device);
  req_free(r);
}

}  // extern "C"
