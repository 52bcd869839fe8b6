// jx_wire.h — the framing rule of the DAP aggregate-init exchange, once: how an AggregationJobInitializeReq body is
// cut into its header and its PrepareInits, and how long the PrepareResps of the answer are.
//
// The rule is wire_parse_prepare_init: one PrepareInit at a byte offset, every read checked against the end of the
// prepare_inits vector, all offsets and sums in 64 bits (a u32 length near 2^32 must not wrap). Three callers walk a
// body with it: the sequential host walk wire_walk (what a host decoder does, and what the kernels are tested
// against), the index kernels of jx_wire.hip (a candidate offset that is not a true boundary reads garbage lengths:
// the bounds checks are what makes that harmless), and wire_gallop_lane, a lane of one iteration of the fallback loop, which the
// kernel runs with one candidate per lane and tests/csrc/hosttest_wire.cpp replays on the CPU one candidate per loop
// iteration. __host__ __device__ and without HIP calls.
#pragma once
#include <stdint.h>

#include "jx_field.h"

namespace jx {

// request status (jx_init_req_info: JX_WIRE_*)
enum : uint32_t { WIRE_OK = 0, WIRE_MALFORMED = 1, WIRE_WRONG_QUERY_TYPE = 2, WIRE_DUPLICATE_ID = 3 };
// per-report status (wire_status[n])
enum : uint8_t { WIRE_REPORT_OK = 0, WIRE_REPORT_ODD_PUBLIC_SHARE = 1, WIRE_REPORT_NOT_INITIALIZE = 2, WIRE_REPORT_ODD_PREP_SHARE = 3 };
enum : uint8_t { WIRE_QUERY_TIME_INTERVAL = 1, WIRE_QUERY_FIXED_SIZE = 2 };
// PrepareError code points (messages/src/lib.rs:2338-2349) the response encoder writes
enum : uint8_t {
  WIRE_ERR_REPORT_REPLAYED = 1, WIRE_ERR_UNKNOWN_CONFIG = 3, WIRE_ERR_DECRYPT = 4, WIRE_ERR_VDAF_PREP = 5,
  WIRE_ERR_INVALID_MESSAGE = 8, WIRE_ERR_TOO_EARLY = 9, WIRE_ERR_NONE = 0xFF
};
constexpr uint64_t WIRE_MIN_PREPARE_INIT = 16 + 8 + 4 + 1 + 2 + 4 + 4 + 1 + 4;  // every field empty, a one-field message
constexpr uint32_t WIRE_LANES = 64;  // candidates one iteration of the fallback loop tests

// One PrepareInit of a body: absolute byte offsets and lengths of its fields. The report id is at off, the time at
// off + 16. A ping-pong field the message's type does not carry has length 0 and the offset where it would start.
struct WireRec {
  uint64_t off, len;          // the whole PrepareInit
  uint64_t ps_off, enc_off, pay_off, msg_off, pm_off, sh_off;
  uint32_t ps_len, enc_len, pay_len, msg_len, pm_len, sh_len;
  uint8_t config_id, pp_type, pad_[6];
};
static_assert(sizeof(WireRec) == 96, "WireRec is copied to the host as bytes");

struct WireHeader {
  uint32_t status;            // WIRE_OK, WIRE_MALFORMED or WIRE_WRONG_QUERY_TYPE
  uint32_t has_batch_id;
  uint64_t err_off;           // the read that failed
  uint64_t param_off, param_len;
  uint64_t start, end;        // the prepare_inits vector: [start, end), end == the body's length
  uint64_t l0;                // the first PrepareInit's length (0: none, or it does not parse)
  uint8_t batch_id[32];
};

JX_HD uint32_t wire_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
JX_HD uint64_t wire_be64(const uint8_t* p) { return ((uint64_t)wire_be32(p) << 32) | wire_be32(p + 4); }
JX_HD void wire_put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// A cursor over body[.., lim): pos <= lim always, so `lim - pos` never wraps and no sum of a position and a length is
// formed before it is known to fit. A failed read leaves pos at the read that failed.
struct WireCur {
  const uint8_t* b;
  uint64_t pos, lim;
  bool ok;
};
JX_HD bool wire_need(WireCur& c, uint64_t n) {
  if (c.ok && c.lim - c.pos < n) c.ok = false;
  return c.ok;
}
JX_HD uint32_t wire_u8(WireCur& c) {
  if (!wire_need(c, 1)) return 0;
  return c.b[c.pos++];
}
JX_HD uint32_t wire_u16(WireCur& c) {
  if (!wire_need(c, 2)) return 0;
  const uint32_t v = ((uint32_t)c.b[c.pos] << 8) | c.b[c.pos + 1];
  c.pos += 2;
  return v;
}
JX_HD uint32_t wire_u32(WireCur& c) {
  if (!wire_need(c, 4)) return 0;
  const uint32_t v = wire_be32(c.b + c.pos);
  c.pos += 4;
  return v;
}
// a length prefix of `width` bytes and its bytes: where they start and how many
JX_HD void wire_opaque(WireCur& c, int width, uint64_t& off, uint32_t& len) {
  const uint64_t at = c.pos;
  const uint32_t l = width == 2 ? wire_u16(c) : wire_u32(c);
  off = c.pos;
  len = l;
  if (!c.ok) return;
  if (!wire_need(c, l)) {
    c.pos = at;  // the read that failed is the opaque as a whole
    return;
  }
  c.pos += l;
}

// The PrepareInit at byte `off` of body, which ends at `lim` (off <= lim). False: it does not parse, *err_off is the
// read that failed (an unknown ping-pong type: the type byte; bytes left over inside the message: the first of them).
JX_HD bool wire_parse_prepare_init(const uint8_t* body, uint64_t lim, uint64_t off, WireRec& r, uint64_t* err_off) {
  WireCur c{body, off, lim, true};
  r = WireRec{};
  r.off = off;
  if (wire_need(c, 24)) c.pos += 24;  // report id, time
  wire_opaque(c, 4, r.ps_off, r.ps_len);
  r.config_id = (uint8_t)wire_u8(c);
  wire_opaque(c, 2, r.enc_off, r.enc_len);
  wire_opaque(c, 4, r.pay_off, r.pay_len);
  wire_opaque(c, 4, r.msg_off, r.msg_len);
  if (!c.ok) {
    *err_off = c.pos;
    return false;
  }
  r.len = c.pos - off;
  // the message's bytes are exactly one PingPongMessage
  WireCur m{body, r.msg_off, r.msg_off + r.msg_len, true};
  const uint64_t type_at = m.pos;
  r.pp_type = (uint8_t)wire_u8(m);
  if (m.ok && r.pp_type > 2) {
    *err_off = type_at;
    return false;
  }
  r.pm_off = r.sh_off = m.pos;
  if (r.pp_type >= 1) wire_opaque(m, 4, r.pm_off, r.pm_len);
  if (r.pp_type == 1) wire_opaque(m, 4, r.sh_off, r.sh_len);
  else r.sh_off = m.pos;
  if (r.pp_type == 0) {
    wire_opaque(m, 4, r.sh_off, r.sh_len);
    r.pm_off = r.sh_off;
  }
  if (!m.ok || m.pos != m.lim) {
    *err_off = m.pos;
    return false;
  }
  return true;
}

// The request header: u32 + aggregation parameter, the PartialBatchSelector of the task's query type, the u32 byte
// length of the prepare_inits vector, which must end where the body ends. l0: the first PrepareInit's length.
JX_HD void wire_parse_header(const uint8_t* body, uint64_t len, uint32_t query_type, WireHeader& h) {
  h = WireHeader{};
  WireCur c{body, 0, len, true};
  uint32_t pl = 0;
  wire_opaque(c, 4, h.param_off, pl);
  h.param_len = pl;
  const uint64_t q_at = c.pos;
  const uint32_t q = wire_u8(c);
  if (c.ok && q != query_type) {
    h.status = WIRE_WRONG_QUERY_TYPE;
    h.err_off = q_at;
    return;
  }
  if (query_type == WIRE_QUERY_FIXED_SIZE && wire_need(c, 32)) {
    for (int i = 0; i < 32; i++) h.batch_id[i] = body[c.pos + i];
    h.has_batch_id = 1;
    c.pos += 32;
  }
  uint32_t vl = 0;
  wire_opaque(c, 4, h.start, vl);
  if (!c.ok) {
    h.status = WIRE_MALFORMED;
    h.err_off = c.pos;
    return;
  }
  h.end = h.start + vl;
  if (h.end != len) {  // bytes after the vector
    h.status = WIRE_MALFORMED;
    h.err_off = h.end;
    return;
  }
  WireRec r;
  uint64_t eo;
  if (h.start < h.end && wire_parse_prepare_init(body, h.end, h.start, r, &eo)) h.l0 = r.len;
}

// One iteration of the fallback loop from the true boundary `off` < end. The stride is re-learnt as a pair: la, the
// length of the message at off, and lb, the length of the message before it (la again when there is none), so that a
// body whose lengths alternate (two KEMs' encapsulated keys, say) still moves a wave's worth per iteration. Lane k
// tests candidate k: it lies at off + (k / 2) (la + lb) + (k odd: la), must parse inside [.., end) and must have the
// length the pattern expects there (la for even k, lb for odd k). The candidates up to the first that fails are
// accepted: each one starts where the one before it ends, so by induction every accepted candidate is a true boundary,
// and so is the first that fails when it only has another length: the next iteration starts there. The fast pass is
// the same test with la == lb == l0 and as many lanes as candidates. The decision of lane k, as the kernel's lanes and
// the CPU replay take it; *at: where the candidate lies (when it lies inside the body).
JX_HD bool wire_gallop_lane(const uint8_t* body, uint64_t end, uint64_t off, uint64_t la, uint64_t lb, uint64_t k,
                            uint64_t* at) {
  *at = off;
  if (k == 0) return true;
  const uint64_t pair = la + lb, pairs = k / 2;
  if ((end - off) / pair < pairs) return false;  // off + pairs * pair would pass the end (and cannot wrap)
  uint64_t p = off + pairs * pair;
  if (k & 1) {
    if (end - p < la) return false;
    p += la;
  }
  if (p >= end) return false;
  *at = p;
  WireRec r;
  uint64_t eo;
  return wire_parse_prepare_init(body, end, p, r, &eo) && r.len == ((k & 1) ? lb : la);
}

// ---- the response: a PrepareResp is id || 00 || u32(5 + S) || 02 || u32(S) || prep_msg[S] when the report finished
// (S: the engine's prep-message length), id || 02 || error otherwise; the AggregationJobResp is u32 + the items.
JX_HD uint32_t wire_resp_len(bool finished, uint32_t S) { return finished ? 16 + 1 + 4 + 1 + 4 + S : 18; }

// The outcome of report i by the helper loop's precedence: the PrepareError to answer with, or WIRE_ERR_NONE when the
// report finished. host_err: a host-resolved error (WIRE_ERR_NONE: none); open: JX_OPEN_*; too_early: its time is after
// the deadline; wire: wire_status; verdict: the engine's; replayed: the datastore saw the id before.
JX_HD uint8_t wire_outcome(uint8_t host_err, uint8_t open, bool too_early, uint8_t wire, uint8_t verdict, bool replayed) {
  if (host_err != WIRE_ERR_NONE) return host_err;
  if (open == 1) return WIRE_ERR_DECRYPT;
  if (open == 7) return WIRE_ERR_UNKNOWN_CONFIG;
  if (open != 0) return WIRE_ERR_INVALID_MESSAGE;
  if (too_early) return WIRE_ERR_TOO_EARLY;
  if (wire == WIRE_REPORT_NOT_INITIALIZE || wire == WIRE_REPORT_ODD_PREP_SHARE) return WIRE_ERR_VDAF_PREP;
  if (verdict != 0) return WIRE_ERR_VDAF_PREP;
  if (replayed) return WIRE_ERR_REPORT_REPLAYED;
  return WIRE_ERR_NONE;
}

// ---- the duplicate check's slot hash: SipHash-2-4 of the 16-byte id under a per-engine 128-bit key
JX_HD uint64_t wire_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
JX_HD uint64_t wire_le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}
JX_HD uint64_t wire_id_hash(const uint8_t id[16], uint64_t k0, uint64_t k1) {
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull,
           v3 = k1 ^ 0x7465646279746573ull;
#define JX_SIPROUND                                  \
  do {                                               \
    v0 += v1; v1 = wire_rotl(v1, 13); v1 ^= v0; v0 = wire_rotl(v0, 32); \
    v2 += v3; v3 = wire_rotl(v3, 16); v3 ^= v2;      \
    v0 += v3; v3 = wire_rotl(v3, 21); v3 ^= v0;      \
    v2 += v1; v1 = wire_rotl(v1, 17); v1 ^= v2; v2 = wire_rotl(v2, 32); \
  } while (0)
  const uint64_t m[3] = {wire_le64(id), wire_le64(id + 8), 16ull << 56};
  for (int i = 0; i < 3; i++) {
    v3 ^= m[i];
    JX_SIPROUND;
    JX_SIPROUND;
    v0 ^= m[i];
  }
  v2 ^= 0xff;
  JX_SIPROUND;
  JX_SIPROUND;
  JX_SIPROUND;
  JX_SIPROUND;
#undef JX_SIPROUND
  return v0 ^ v1 ^ v2 ^ v3;
}

// ---- the batch buckets of a time-interval task (aggregation_job_writer.rs:557-605, :608-708): a report belongs to the
// batch whose identifier is its time rounded down to the task's time_precision (Time::to_batch_interval_start).
// precision > 0; exact for every u64: the remainder is never more than the time.
JX_HD uint64_t wire_bucket_start(uint64_t time, uint64_t precision) { return time - time % precision; }

// is `start` one of the m collected starts, which ascend?
JX_HD bool wire_bucket_collected(const uint64_t* collected, uint64_t m, uint64_t start) {
  uint64_t lo = 0, hi = m;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (collected[mid] < start) lo = mid + 1;
    else hi = mid;
  }
  return lo < m && collected[lo] == start;
}

// wire_outcome for a routed request. The writer fails what is left of a batch that no longer accepts aggregations:
// BatchCollected ranks below every other error, ReportReplayed included, since the reference marks replays before the
// writer runs and the writer skips report aggregations that have already failed.
constexpr uint8_t WIRE_ERR_BATCH_COLLECTED = 0;
JX_HD uint8_t wire_outcome_routed(uint8_t host_err, uint8_t open, bool too_early, uint8_t wire, uint8_t verdict,
                                  bool replayed, bool collected) {
  const uint8_t err = wire_outcome(host_err, open, too_early, wire, verdict, replayed);
  return err == WIRE_ERR_NONE && collected ? WIRE_ERR_BATCH_COLLECTED : err;
}

// One bucket of a request (jx_route_bucket). min_time / max_time / reports: over every report of the bucket, excluded
// and failed ones included (the writer widens the batch's client-timestamp interval with all of them).
struct WireBucket {
  uint64_t start, min_time, max_time;
  uint32_t reports, routed, collected, pad_;
};
static_assert(sizeof(WireBucket) == 40, "WireBucket is copied to the host as bytes");
constexpr uint32_t WIRE_ROUTE_MAX_BUCKETS = 1024;
constexpr uint32_t WIRE_ROUTE_OUT = 0xFFFFFFFFu;

// The distinct buckets are found as the duplicate ids are: tab holds `slots` zeroed words, a slot holds claimant
// index + 1, and a report walks its bucket's probe chain from the keyed hash of the start. An empty slot is claimed
// (cas(&slot, value): a compare-exchange with 0 that returns what the slot held); an occupied one names its holder,
// whose bucket is recomputed from times, the pass's input, never from anything the pass writes. True: report i
// claimed its bucket's slot, as exactly one report of every bucket does, whichever comes first.
JX_HD uint64_t wire_bucket_slot(uint64_t start, uint64_t k0, uint64_t k1, uint64_t slots) {
  uint8_t id[16] = {0};
  for (int k = 0; k < 8; k++) id[k] = (uint8_t)(start >> (8 * k));
  return wire_id_hash(id, k0, k1) % slots;
}
template <class Cas>
JX_HD bool wire_route_claim(uint64_t i, const uint64_t* times, uint64_t precision, uint32_t* tab, uint64_t slots,
                            uint64_t k0, uint64_t k1, Cas cas) {
  const uint64_t b = wire_bucket_start(times[i], precision);
  uint64_t s = wire_bucket_slot(b, k0, k1, slots);
  for (uint64_t probes = 0; probes < slots; probes++) {
    const uint32_t seen = cas(&tab[s], (uint32_t)i + 1u);
    if (seen == 0) return true;
    if (wire_bucket_start(times[seen - 1u], precision) == b) return false;
    s = s + 1 == slots ? 0 : s + 1;
  }
  return false;  // not reached: fewer claimants than slots
}
// the claimant of start's slot once every claim is made (WIRE_ROUTE_OUT: none, which no bucket of the request gives)
JX_HD uint32_t wire_route_holder(uint64_t start, const uint64_t* times, uint64_t precision, const uint32_t* tab,
                                 uint64_t slots, uint64_t k0, uint64_t k1) {
  uint64_t s = wire_bucket_slot(start, k0, k1, slots);
  for (uint64_t probes = 0; probes < slots; probes++) {
    const uint32_t seen = tab[s];
    if (seen == 0) break;
    if (wire_bucket_start(times[seen - 1u], precision) == start) return seen - 1u;
    s = s + 1 == slots ? 0 : s + 1;
  }
  return WIRE_ROUTE_OUT;
}
// the place of keys[k] among m distinct keys in ascending order
JX_HD uint32_t wire_rank(const uint64_t* keys, uint32_t m, uint32_t k) {
  const uint64_t mine = keys[k];
  uint32_t r = 0;
  for (uint32_t j = 0; j < m; j++) r += keys[j] < mine;
  return r;
}
// route[i] after the route: the bucket's index for a report that was routed in and whose bucket is open
JX_HD uint32_t wire_route_of(uint32_t before, bool collected, uint32_t bucket) {
  return before == 0 && !collected ? bucket : WIRE_ROUTE_OUT;
}

// The whole index as the kernels compute it, one loop iteration per lane: the fast pass over every candidate at
// start + i * l0 (the kernel takes the minimum of the failing i with one atomic), then the fallback loop. iters: the
// fallback's iterations (0 for a uniform body).
struct WireIndex {
  uint32_t status;
  uint32_t iters;
  uint64_t err_off;
  uint64_t n;
  uint64_t nfast;  // boundaries the fast pass accepted: message i < nfast starts at start + i * l0
};
JX_HD uint32_t wire_gallop_accept(const uint8_t* body, uint64_t end, uint64_t off, uint64_t la, uint64_t lb) {
  uint32_t m = 1;
  uint64_t at;
  while (m < WIRE_LANES && wire_gallop_lane(body, end, off, la, lb, m, &at)) m++;
  return m;
}
// offs (nullable): offs[j] takes the start of message nfast + j, for up to cap of them
inline WireIndex wire_index_replay(const uint8_t* body, const WireHeader& h, uint64_t* offs, uint64_t cap) {
  WireIndex x{h.status, 0, h.err_off, 0, 0};
  if (h.status != WIRE_OK || h.start == h.end) return x;
  uint64_t off = h.start, at;
  if (h.l0) {
    const uint64_t cands = (h.end - h.start) / h.l0;
    uint64_t bad = cands;
    for (uint64_t i = 0; i < cands; i++)
      if (!wire_gallop_lane(body, h.end, h.start, h.l0, h.l0, i, &at)) {
        bad = i;
        break;
      }
    x.nfast = x.n = bad;
    off = h.start + bad * h.l0;
  }
  uint64_t prev = x.nfast ? h.l0 : 0;  // the length of the message before off (0: there is none)
  while (off < h.end) {
    WireRec r;
    if (!wire_parse_prepare_init(body, h.end, off, r, &x.err_off)) {
      x.status = WIRE_MALFORMED;
      return x;
    }
    const uint64_t la = r.len, lb = prev ? prev : r.len;
    const uint32_t m = wire_gallop_accept(body, h.end, off, la, lb);
    for (uint32_t k = 0; k < m; k++) {
      (void)wire_gallop_lane(body, h.end, off, la, lb, k, &at);
      if (offs && x.n - x.nfast + k < cap) offs[x.n - x.nfast + k] = at;
    }
    x.n += m;
    off += (uint64_t)(m / 2) * (la + lb) + ((m & 1) ? la : 0);
    prev = (m & 1) ? la : lb;  // the last accepted message is candidate m - 1
    x.iters++;
  }
  return x;
}

// ---- the sequential walk: the host decoder's pass, and the reference the kernels are compared with
struct WireWalk {
  uint32_t status;
  uint64_t err_off;
  uint64_t n;
};
// recs (nullable) takes up to cap records
inline WireWalk wire_walk(const uint8_t* body, const WireHeader& h, WireRec* recs, uint64_t cap) {
  WireWalk w{h.status, h.err_off, 0};
  if (h.status != WIRE_OK) return w;
  uint64_t off = h.start;
  while (off < h.end) {
    WireRec r;
    if (!wire_parse_prepare_init(body, h.end, off, r, &w.err_off)) {
      w.status = WIRE_MALFORMED;
      return w;
    }
    if (recs && w.n < cap) recs[w.n] = r;
    w.n++;
    off += r.len;
  }
  return w;
}

// ---- the leader's end of the exchange: the request written, the response read.
//
// A PrepareInit the leader writes is id[16] || time u64 || u32 PS || public share || config id || u16 + encapsulated
// key || u32 + payload || u32 M || 00 || u32 LPS || prep share, with M = 5 + LPS: 44 fixed bytes around four fields.
constexpr uint32_t WIRE_INIT_FIXED = 44;
JX_HD uint64_t wire_init_len(uint64_t PS, uint64_t enc_len, uint64_t pay_len, uint64_t LPS) {
  return WIRE_INIT_FIXED + PS + enc_len + pay_len + LPS;
}
JX_HD uint64_t wire_req_header_len(uint64_t agg_param_len, uint32_t query_type) {
  return 4 + agg_param_len + (query_type == WIRE_QUERY_FIXED_SIZE ? 33 : 1) + 4;
}
// where the four fields of a PrepareInit start, from the message's first byte
struct WireInitLayout {
  uint64_t ps_off, enc_off, pay_off, sh_off, len;
};
JX_HD WireInitLayout wire_init_layout(uint64_t PS, uint64_t enc_len, uint64_t pay_len, uint64_t LPS) {
  WireInitLayout l;
  l.ps_off = 28;
  l.enc_off = l.ps_off + PS + 3;
  l.pay_off = l.enc_off + enc_len + 4;
  l.sh_off = l.pay_off + pay_len + 9;
  l.len = l.sh_off + LPS;
  return l;
}
// Fixed byte k < 44 of a PrepareInit: its value, and in *at where it lies from the message's first byte. The kernel
// gives one k to a lane, the host writer loops over them.
JX_HD uint8_t wire_init_fixed_byte(uint32_t k, const uint8_t* id, uint64_t time, uint32_t PS, uint8_t config_id,
                                   uint32_t enc_len, uint32_t pay_len, uint32_t LPS, uint64_t* at) {
  *at = (uint64_t)k + (k >= 28 ? PS : 0) + (k >= 31 ? enc_len : 0) + (k >= 35 ? (uint64_t)pay_len : 0);
  if (k < 16) return id[k];
  if (k < 24) return (uint8_t)(time >> (8 * (23 - k)));
  if (k < 28) return (uint8_t)(PS >> (8 * (27 - k)));
  if (k == 28) return config_id;
  if (k < 31) return (uint8_t)(enc_len >> (8 * (30 - k)));
  if (k < 35) return (uint8_t)(pay_len >> (8 * (34 - k)));
  if (k < 39) return (uint8_t)((5 + LPS) >> (8 * (38 - k)));
  if (k == 39) return 0;  // PingPongMessage::Initialize
  return (uint8_t)(LPS >> (8 * (43 - k)));
}
JX_HD void wire_put_prepare_init_head(uint8_t* p, const uint8_t* id, uint64_t time, uint32_t PS, uint8_t config_id,
                                      uint32_t enc_len, uint32_t pay_len, uint32_t LPS) {
  for (uint32_t k = 0; k < WIRE_INIT_FIXED; k++) {
    uint64_t at;
    const uint8_t v = wire_init_fixed_byte(k, id, time, PS, config_id, enc_len, pay_len, LPS, &at);
    p[at] = v;
  }
}
// The request header at out: u32 + aggregation parameter || query type [|| batch id] || u32 vec_len. Returns its length.
JX_HD uint64_t wire_put_req_header(uint8_t* out, const uint8_t* agg_param, uint32_t agg_param_len, uint32_t query_type,
                                   const uint8_t* batch_id, uint32_t vec_len) {
  wire_put32(out, agg_param_len);
  uint64_t p = 4;
  for (uint32_t i = 0; i < agg_param_len; i++) out[p++] = agg_param[i];
  out[p++] = (uint8_t)query_type;
  if (query_type == WIRE_QUERY_FIXED_SIZE)
    for (int i = 0; i < 32; i++) out[p++] = batch_id[i];
  wire_put32(out + p, vec_len);
  return p + 4;
}
// What a request refuses before a byte is written: a field whose length has no place in its prefix, a vector whose
// byte length does not fit a u32. All sums in 64 bits.
enum : uint32_t { WIRE_REQ_OK = 0, WIRE_REQ_LONG_KEY = 1, WIRE_REQ_LONG_PAYLOAD = 2, WIRE_REQ_LONG_VECTOR = 3 };
JX_HD uint32_t wire_req_field_check(uint64_t enc_len, uint64_t pay_len) {
  if (enc_len >= (1ull << 16)) return WIRE_REQ_LONG_KEY;
  if (pay_len >= (1ull << 32)) return WIRE_REQ_LONG_PAYLOAD;
  return WIRE_REQ_OK;
}
// The body's length for the reports with send[i] != 0 (send nullable: all), from the offset arrays alone (enc_offsets
// nullable: 32 bytes each). *total is valid when WIRE_REQ_OK is returned.
inline uint32_t wire_req_total(uint64_t n, uint64_t PS, uint64_t LPS, const uint64_t* enc_offsets,
                               const uint64_t* payload_offsets, const uint8_t* send, uint64_t agg_param_len,
                               uint32_t query_type, uint64_t* total) {
  uint64_t vec = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t el = enc_offsets ? enc_offsets[i + 1] - enc_offsets[i] : 32;
    const uint64_t pl = payload_offsets[i + 1] - payload_offsets[i];
    if (const uint32_t bad = wire_req_field_check(el, pl)) return bad;
    if (send && !send[i]) continue;
    vec += wire_init_len(PS, el, pl, LPS);  // < 2^33 each: no wrap below 2^31 reports
    if (vec > 0xFFFFFFFFull) return WIRE_REQ_LONG_VECTOR;
  }
  *total = wire_req_header_len(agg_param_len, query_type) + vec;
  return WIRE_REQ_OK;
}

// One PrepareResp of an AggregationJobResp body (messages/src/lib.rs:2270-2333, :2361-2368): id[16] || tag, then
// Continue (0): u32 M + exactly one PingPongMessage; Finished (1): nothing; Reject (2): a PrepareError code point <= 9.
struct WireRespRec {
  uint64_t off, len;   // the whole PrepareResp
  uint64_t pm_off;     // Continue: the prep message of a Continue / Finish ping-pong message (else where it would start)
  uint32_t pm_len, sh_len;
  uint8_t tag, pp_type, error, pad_[5];
};
static_assert(sizeof(WireRespRec) == 40, "WireRespRec is plain bytes");
constexpr uint32_t WIRE_MAX_PREPARE_ERROR = 9;

// False: it does not parse, *err_off is the read that failed (an unknown tag, error code or ping-pong type: that byte;
// bytes left over inside the message: the first of them).
JX_HD bool wire_parse_prepare_resp(const uint8_t* body, uint64_t lim, uint64_t off, WireRespRec& r, uint64_t* err_off) {
  WireCur c{body, off, lim, true};
  r = WireRespRec{};
  r.off = off;
  if (wire_need(c, 16)) c.pos += 16;
  const uint64_t tag_at = c.pos;
  r.tag = (uint8_t)wire_u8(c);
  if (!c.ok) {
    *err_off = c.pos;
    return false;
  }
  if (r.tag > 2) {
    *err_off = tag_at;
    return false;
  }
  if (r.tag == 1) {
    r.len = c.pos - off;
    return true;
  }
  if (r.tag == 2) {
    const uint64_t e_at = c.pos;
    r.error = (uint8_t)wire_u8(c);
    if (!c.ok || r.error > WIRE_MAX_PREPARE_ERROR) {
      *err_off = e_at;
      return false;
    }
    r.len = c.pos - off;
    return true;
  }
  uint64_t msg_off;
  uint32_t msg_len;
  wire_opaque(c, 4, msg_off, msg_len);
  if (!c.ok) {
    *err_off = c.pos;
    return false;
  }
  r.len = c.pos - off;
  WireCur m{body, msg_off, msg_off + msg_len, true};
  const uint64_t type_at = m.pos;
  r.pp_type = (uint8_t)wire_u8(m);
  if (m.ok && r.pp_type > 2) {
    *err_off = type_at;
    return false;
  }
  r.pm_off = m.pos;
  uint64_t sh_off;
  if (r.pp_type >= 1) wire_opaque(m, 4, r.pm_off, r.pm_len);
  if (r.pp_type <= 1) wire_opaque(m, 4, sh_off, r.sh_len);
  if (!m.ok || m.pos != m.lim) {
    *err_off = m.pos;
    return false;
  }
  return true;
}

// The sequential walk of a response body: the u32 byte length of the PrepareResps, which must end where the body
// ends, then the messages to the end. recs (nullable) takes up to cap records; n counts them all.
inline WireWalk wire_resp_walk(const uint8_t* body, uint64_t len, WireRespRec* recs, uint64_t cap) {
  WireWalk w{WIRE_OK, 0, 0};
  WireCur c{body, 0, len, true};
  uint64_t start;
  uint32_t vl;
  wire_opaque(c, 4, start, vl);
  if (!c.ok) {
    w.status = WIRE_MALFORMED;
    w.err_off = c.pos;
    return w;
  }
  const uint64_t end = start + vl;
  if (end != len) {  // bytes after the vector
    w.status = WIRE_MALFORMED;
    w.err_off = end;
    return w;
  }
  uint64_t off = start;
  while (off < end) {
    WireRespRec r;
    if (!wire_parse_prepare_resp(body, end, off, r, &w.err_off)) {
      w.status = WIRE_MALFORMED;
      return w;
    }
    if (recs && w.n < cap) recs[w.n] = r;
    w.n++;
    off += r.len;
  }
  return w;
}

// What a one-round leader makes of a PrepareResp (aggregation_job_driver.rs:584-663). PM: its prep-message length.
enum : uint8_t { RESP_CONTINUED = 0, RESP_REJECTED = 1, RESP_FINISHED = 2, RESP_MESSAGE_MISMATCH = 3 };
JX_HD uint8_t wire_resp_classify(const WireRespRec& r, uint32_t PM) {
  if (r.tag == 2) return RESP_REJECTED;  // the helper's PrepareError: r.error
  if (r.tag == 1) return RESP_FINISHED;  // finish_mismatch: a one-round leader still waits for a message
  return r.pp_type == 2 && r.pm_len == PM ? RESP_CONTINUED : RESP_MESSAGE_MISMATCH;
}
constexpr uint64_t WIRE_RESP_NO_MESSAGE = ~0ull;  // a row of the leader batch without a continued response

// ---- what the kernels of jx_wire.hip and the engine (jx_engine_wire.cpp) share
constexpr uint32_t WIRE_NO_DUPLICATE = 0xFFFFFFFFu;

// One decode's state on the device, zeroed before the header kernel; the host reads it back between the phases.
struct WireState {
  WireHeader hdr;
  unsigned long long first_bad;  // the fast pass: the lowest candidate index that failed (~0: none)
  uint64_t n, nfast, err_off;
  uint64_t enc_total, pay_total;
  uint32_t status, iters;
  uint32_t dup;     // the lowest index with an equal id at a lower index (WIRE_NO_DUPLICATE: none)
  uint32_t odd_ps;  // reports of wire_status 1
};

struct WireDecodeArgs {
  const uint8_t* body;
  uint64_t n, nfast, start, end, l0;
  const uint64_t* offs;  // the starts of messages nfast.. (null when nfast == n)
  uint32_t ps_bytes, lps_bytes;
  uint32_t has_deadline;
  uint64_t deadline;
  const uint8_t *key_first, *key_second;  // [256] each: config id -> keypair index
  WireState* st;
  WireRec* recs;
  uint64_t* times;
  uint8_t *wire_status, *key_index;
  uint32_t* route;
  uint64_t *enc_offsets, *payload_offsets;
  uint8_t *ids, *ps, *lps, *encs, *payloads;
};

struct WireEncodeArgs {
  uint64_t n;
  const uint8_t* ids;
  const uint64_t* times;
  const uint8_t *wire_status, *verdicts, *open_status, *prep_msgs;
  const uint8_t *host_err, *replayed;  // nullable
  const uint8_t* bucket_collected;     // a routed request's (null: the request is not routed)
  uint32_t prep_msg_bytes, prep_msg_stride;
  uint32_t has_deadline;
  uint64_t deadline;
  uint8_t *err, *finished;  // [n]
  uint64_t* offsets;        // [n + 1]: PrepareResp i at 4 + offsets[i] of out
  uint8_t* out;
};

// The route. st->claims counts the buckets claimed; past WIRE_ROUTE_MAX_BUCKETS the request has too many, and the
// kernels behind the claims write nothing.
struct WireRouteState {
  uint32_t claims, pad_;
};
struct WireRouteArgs {
  uint64_t n;
  const uint64_t* times;
  uint64_t precision;
  const uint64_t* collected;  // ascending, distinct
  uint64_t ncollected;
  uint32_t* tab;              // [slots], zeroed
  uint64_t slots, k0, k1;
  WireRouteState* st;         // zeroed
  uint32_t* list;             // [WIRE_ROUTE_MAX_BUCKETS]: the claimants, in the order they drew their places
  uint32_t* rank;             // [n]: rank[c] of a claimant c is its bucket's index
  WireBucket* buckets;        // [WIRE_ROUTE_MAX_BUCKETS]
  uint32_t *route, *bucket_index;
  uint8_t* bucket_collected;
};

// The leader's request encode. The host arrays of the call (times .. exclude) are device copies here.
struct WireReqTotals {
  uint64_t vec_bytes;  // the PrepareInits of the reports that are sent
  uint64_t n_sent;
};
struct WireReqArgs {
  uint64_t n;
  const uint8_t *ids, *ps, *encs, *payloads, *lps, *verdicts;
  const uint64_t* times;
  const uint8_t* config_ids;
  const uint64_t *enc_offsets, *payload_offsets;  // enc_offsets nullable: 32 bytes each
  const uint8_t* exclude;                         // nullable
  uint32_t ps_bytes, lps_bytes;
  uint64_t lps_stride;
  const uint8_t *agg_param, *batch_id;  // device copies: agg_param_len bytes, 32 bytes (FixedSize)
  uint32_t agg_param_len, query_type;
  uint64_t header_len;
  uint64_t* msg_len;           // [n]: the PrepareInit's length, 0 when the report is not sent
  uint8_t* send;               // [n]
  uint64_t *offsets, *rank;    // [n + 1]: exclusive scans of msg_len and of send
  uint32_t* sent_index;        // [n]: sent_index[rank[i]] = i for the reports sent
  uint8_t* sent_ids;           // [n x 16]: the id of sent report k
  WireReqTotals* totals;
  uint8_t* out;
};

// The leader's response decode: what the host walk found, per row of the leader batch.
struct WireRespArgs {
  uint64_t n;
  const uint8_t* body;
  const uint64_t* pm_off;  // [n]: where row i's prep message lies in body, WIRE_RESP_NO_MESSAGE when it has none
  uint32_t pm_bytes;
  uint64_t pm_stride;
  uint8_t *prep_msgs, *peer_verdicts;
};

#if defined(__HIPCC__) || defined(__HIP__)
// select + the two scans + the compaction list; the host reads a.totals, then packs n_sent reports
hipError_t launch_wire_req_sizes(const WireReqArgs& a, hipStream_t s);
hipError_t launch_wire_req_pack(const WireReqArgs& a, uint64_t n_sent, uint32_t vec_bytes, hipStream_t s);
hipError_t launch_wire_resp_scatter(const WireRespArgs& a, hipStream_t s);
hipError_t launch_wire_header(const uint8_t* body, uint64_t len, uint32_t query_type, WireState* st, hipStream_t s);
// the fast pass over `cands` candidates (fast: not yet run for this body) and the fallback loop; offs / cap: where the
// starts of the messages the fallback accepts go (null: only count them)
hipError_t launch_wire_index(const uint8_t* body, WireState* st, uint64_t cands, bool fast, uint64_t* offs, uint64_t cap,
                             hipStream_t s);
// records and per-report scalars, the duplicate check (dup_tab: `slots` zeroed words; dup_result: WIRE_NO_DUPLICATE)
// and the two scans
hipError_t launch_wire_records(const WireDecodeArgs& a, uint32_t* dup_tab, uint64_t slots, uint32_t* dup_result, uint64_t k0,
                               uint64_t k1, hipStream_t s);
hipError_t launch_wire_gather(const WireDecodeArgs& a, hipStream_t s);
hipError_t launch_wire_exclude(uint32_t* route, const uint8_t* mask, uint64_t n, hipStream_t s);
// the claims, the sort of the claimed buckets, and the pass that routes every report and counts its bucket (n > 0)
hipError_t launch_wire_route(const WireRouteArgs& a, hipStream_t s);
hipError_t launch_wire_encode_sizes(const WireEncodeArgs& a, hipStream_t s);
hipError_t launch_wire_encode_pack(const WireEncodeArgs& a, hipStream_t s);
#endif

// ---- the upload: the Report a client sends the leader (messages/src/lib.rs:1353-1432) is id[16] || time u64 ||
// u32 + public share || config id || u16 + encapsulated key || u32 + payload || config id || u16 + encapsulated key ||
// u32 + payload (the leader's ciphertext, then the helper's): 42 fixed bytes around five fields. Every upload is an
// HTTP body of its own, so where a Report starts and ends is known: there is no index to build.
constexpr uint32_t WIRE_REPORT_FIXED = 42;
// per-upload status (upload_status[n]), first failing check first
enum : uint8_t {
  UPLOAD_OK = 0, UPLOAD_MALFORMED = 1, UPLOAD_TOO_EARLY = 2, UPLOAD_TASK_EXPIRED = 3, UPLOAD_EXPIRED = 4,
  UPLOAD_ODD_PUBLIC_SHARE = 5
};
constexpr uint32_t UPLOAD_NO_ROW = 0xFFFFFFFFu;  // row_of[i] of a report that is not accepted

// One Report of the uploads: absolute byte offsets and lengths of its five fields. The report id is at off, the
// time at off + 16. key0 / key1: the keypair slots of the leader ciphertext's config id (the decode fills them).
struct WireReportRec {
  uint64_t off, len;  // the whole Report
  uint64_t ps_off, lenc_off, lpay_off, henc_off, hpay_off;
  uint32_t ps_len, lenc_len, lpay_len, henc_len, hpay_len;
  uint8_t leader_config_id, helper_config_id, key0, key1;
};
static_assert(sizeof(WireReportRec) == 80, "WireReportRec is plain bytes");

// The Report in body[off, lim) (off <= lim): every field inside, nothing left over, as Report::get_decoded. False: it
// does not parse, *err_off is the read that failed (bytes left over: the first of them).
JX_HD bool wire_parse_report(const uint8_t* body, uint64_t lim, uint64_t off, WireReportRec& r, uint64_t* err_off) {
  WireCur c{body, off, lim, true};
  r = WireReportRec{};
  r.off = off;
  if (wire_need(c, 24)) c.pos += 24;  // report id, time
  wire_opaque(c, 4, r.ps_off, r.ps_len);
  r.leader_config_id = (uint8_t)wire_u8(c);
  wire_opaque(c, 2, r.lenc_off, r.lenc_len);
  wire_opaque(c, 4, r.lpay_off, r.lpay_len);
  r.helper_config_id = (uint8_t)wire_u8(c);
  wire_opaque(c, 2, r.henc_off, r.henc_len);
  wire_opaque(c, 4, r.hpay_off, r.hpay_len);
  if (!c.ok || c.pos != lim) {
    *err_off = c.pos;
    return false;
  }
  r.len = c.pos - off;
  return true;
}

JX_HD uint64_t wire_report_len(uint64_t PS, uint64_t lenc_len, uint64_t lpay_len, uint64_t henc_len, uint64_t hpay_len) {
  return WIRE_REPORT_FIXED + PS + lenc_len + lpay_len + henc_len + hpay_len;
}
// where the five fields of a Report start, from its first byte
struct WireReportLayout {
  uint64_t ps_off, lenc_off, lpay_off, henc_off, hpay_off, len;
};
JX_HD WireReportLayout wire_report_layout(uint64_t PS, uint64_t lenc_len, uint64_t lpay_len, uint64_t henc_len,
                                          uint64_t hpay_len) {
  WireReportLayout l;
  l.ps_off = 28;
  l.lenc_off = l.ps_off + PS + 3;
  l.lpay_off = l.lenc_off + lenc_len + 4;
  l.henc_off = l.lpay_off + lpay_len + 3;
  l.hpay_off = l.henc_off + henc_len + 4;
  l.len = l.hpay_off + hpay_len;
  return l;
}
// Fixed byte k < 42 of a Report: its value, and in *at where it lies from the Report's first byte. The kernel gives
// one k to a lane, a host writer loops over them.
JX_HD uint8_t wire_report_fixed_byte(uint32_t k, const uint8_t* id, uint64_t time, uint32_t PS, uint8_t leader_config_id,
                                     uint32_t lenc_len, uint32_t lpay_len, uint8_t helper_config_id, uint32_t henc_len,
                                     uint32_t hpay_len, uint64_t* at) {
  *at = (uint64_t)k + (k >= 28 ? PS : 0) + (k >= 31 ? lenc_len : 0) + (k >= 35 ? (uint64_t)lpay_len : 0) +
        (k >= 38 ? henc_len : 0);
  if (k < 16) return id[k];
  if (k < 24) return (uint8_t)(time >> (8 * (23 - k)));
  if (k < 28) return (uint8_t)(PS >> (8 * (27 - k)));
  if (k == 28) return leader_config_id;
  if (k < 31) return (uint8_t)(lenc_len >> (8 * (30 - k)));
  if (k < 35) return (uint8_t)(lpay_len >> (8 * (34 - k)));
  if (k == 35) return helper_config_id;
  if (k < 38) return (uint8_t)(henc_len >> (8 * (37 - k)));
  return (uint8_t)(hpay_len >> (8 * (41 - k)));
}

// The upload handler's three time checks in its order (aggregator/src/aggregator.rs:1544-1573): TooEarly, time >
// now + skew; TaskExpired, time > *task_expiration; Expired, now > time + *report_expiry_age (either pointer null: the
// task has no such limit). Both sums saturate at 2^64 - 1, which decides as the unbounded sum does: no u64 exceeds a
// sum that overflowed.
JX_HD uint64_t wire_sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}
JX_HD uint8_t wire_upload_check_limits(uint64_t time, uint64_t now, uint64_t skew, bool has_task_expiration,
                                       uint64_t task_expiration, bool has_report_expiry_age, uint64_t report_expiry_age) {
  if (time > wire_sat_add(now, skew)) return UPLOAD_TOO_EARLY;
  if (has_task_expiration && time > task_expiration) return UPLOAD_TASK_EXPIRED;
  if (has_report_expiry_age && now > wire_sat_add(time, report_expiry_age)) return UPLOAD_EXPIRED;
  return UPLOAD_OK;
}
JX_HD uint8_t wire_upload_check(uint64_t time, uint64_t now, uint64_t skew, const uint64_t* task_expiration,
                                const uint64_t* report_expiry_age) {
  return wire_upload_check_limits(time, now, skew, task_expiration != nullptr, task_expiration ? *task_expiration : 0,
                                  report_expiry_age != nullptr, report_expiry_age ? *report_expiry_age : 0);
}

// What the parse kernel decides for upload i of body, which lies in [lo, hi): its record, id, time and status. A
// report that is not accepted keeps zero lengths in its record, so the scans count nothing for it. An upload of fewer
// than 24 bytes has a zero id and time. ps_bytes: the engine's public-share length; key_first / key_second: [256].
struct WireUploadChecks {
  uint64_t now, skew, task_expiration, report_expiry_age;
  uint32_t has_task_expiration, has_report_expiry_age;
};
JX_HD uint8_t wire_upload_parse(const uint8_t* body, uint64_t lo, uint64_t hi, uint32_t ps_bytes,
                                const WireUploadChecks& ck, const uint8_t* key_first, const uint8_t* key_second,
                                WireReportRec& r, uint8_t id[16], uint64_t* time) {
  uint64_t eo;
  const bool parsed = wire_parse_report(body, hi, lo, r, &eo);
  const bool head = hi - lo >= 24;
  for (int k = 0; k < 16; k++) id[k] = head ? body[lo + k] : (uint8_t)0;
  *time = head ? wire_be64(body + lo + 16) : 0;
  uint8_t st = UPLOAD_MALFORMED;
  if (parsed) {
    st = wire_upload_check_limits(*time, ck.now, ck.skew, ck.has_task_expiration != 0, ck.task_expiration,
                                  ck.has_report_expiry_age != 0, ck.report_expiry_age);
    if (st == UPLOAD_OK && r.ps_len != ps_bytes) st = UPLOAD_ODD_PUBLIC_SHARE;
  }
  if (st != UPLOAD_OK) {
    r.ps_len = r.lenc_len = r.lpay_len = r.henc_len = r.hpay_len = 0;
    r.key0 = r.key1 = 0xFF;
  } else {
    r.key0 = key_first[r.leader_config_id];
    r.key1 = key_second[r.leader_config_id];
  }
  return st;
}

// A long field copied by `parts` waves: wave `part` takes bytes [*lo, *lo + *cnt) of its len. The slices have one
// length, a multiple of 16, so they neither overlap nor leave a gap (the last may be short or empty).
JX_HD void wire_part_span(uint64_t len, uint32_t part, uint32_t parts, uint64_t* lo, uint64_t* cnt) {
  const uint64_t chunk = ((len + parts - 1) / parts + 15) & ~15ull;
  uint64_t at = (uint64_t)part * chunk;
  if (at > len) at = len;
  *lo = at;
  *cnt = len - at < chunk ? len - at : chunk;
}

// ---- what the kernels of jx_wire_upload.hip and the engine (jx_engine_wire_upload.cpp) share
struct WireUploadTotals {
  uint64_t m;                                    // accepted reports
  uint64_t lenc_bytes, lpay_bytes, henc_bytes, hpay_bytes;  // their four packed fields
};
struct WireUploadArgs {
  uint64_t n;
  const uint8_t* body;
  const uint64_t* body_offsets;  // [n + 1], a device copy
  uint32_t ps_bytes;
  WireUploadChecks checks;
  const uint8_t *key_first, *key_second;  // [256] each
  // for all n
  WireReportRec* recs;
  uint8_t *ids_all, *status;
  uint64_t* times_all;
  uint32_t* row_of;
  uint64_t *rank, *scan[4];  // [n + 1] each: exclusive scans of the accept flags and of the four lengths
  WireUploadTotals* totals;
  // for the m accepted, dense and in order
  uint32_t* index;
  uint8_t *ids, *ps, *key_index, *config_ids;
  uint64_t* times;
  uint64_t* offs[4];  // [m + 1] each: leader enc, leader payload, helper enc, helper payload
  uint8_t* packed[4];
};

// The client's encode: the rows jx_client_seal_* wrote, every report of the same length.
struct WireReportTotals {
  uint64_t bytes, m;  // the bodies together; the reports that take room
};
struct WireReportArgs {
  uint64_t n;
  const uint8_t *ids, *ps, *lencs, *lcts, *hencs, *hcts;
  const uint64_t* times;    // a device copy
  const uint8_t* status;    // nullable: a non-zero entry takes no room
  uint32_t ps_bytes, lenc_len, lct_len, henc_len, hct_len;
  uint8_t leader_config_id, helper_config_id;
  uint64_t *offsets, *rank;  // [n + 1]
  uint32_t* index;           // [n]: index[rank[i]] = i for the reports that take room
  WireReportTotals* totals;
  uint8_t* out;
};

#if defined(__HIPCC__) || defined(__HIP__)
// parse + the scans with the compaction; the host reads a.totals, then gathers m reports with `parts` waves each
hipError_t launch_wire_upload_sizes(const WireUploadArgs& a, hipStream_t s);
hipError_t launch_wire_upload_gather(const WireUploadArgs& a, uint64_t m, uint32_t parts, hipStream_t s);
hipError_t launch_wire_report_sizes(const WireReportArgs& a, hipStream_t s);
hipError_t launch_wire_report_pack(const WireReportArgs& a, uint64_t m, uint32_t parts, hipStream_t s);
#endif

}  // namespace jx
