// hosttest_wire_leader.cpp — the leader's half of janus_amd/csrc/jx_wire.h on the CPU (tests/test_wire_leader_host.py).
// Built with the address and undefined-behaviour sanitizers: every body and every output lives in an allocation of
// exactly its length, so a read or write one byte past it stops the program.
//
//   resp FILE       u32 count, then per body u32 PM, u64 length and the bytes (little-endian). Each body is walked with
//                   wire_resp_walk and every record classified; one output line per body.
//   req FILE OUT    u32 count, then per case the fields of a request (see read_case). The body is written by a replay
//                   of the kernels: select, the two exclusive scans, then one wave's work per loop iteration (the 44
//                   fixed bytes one per lane, the four fields) into an allocation of exactly the total. OUT takes, per
//                   case, u32 status, u64 length, the body, u32 n_sent and the compaction list.
//   total FILE      u32 count, then per case u64 n, PS, LPS, param_len, u32 query type, u32 has_enc, the n + 1 enc
//                   offsets (when has_enc) and the n + 1 payload offsets: wire_req_total from lengths alone.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../janus_amd/csrc/jx_wire.h"

using namespace jx;

namespace {

FILE* in = nullptr;
template <class T>
T get() {
  T v{};
  if (fread(&v, sizeof v, 1, in) != 1) exit(2);
  return v;
}
// exactly n bytes (at least an allocation of one), so the sanitizer sees the first byte past them
uint8_t* get_bytes(uint64_t n) {
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n && fread(p, 1, n, in) != n) exit(2);
  return p;
}

int run_resp() {
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    const uint32_t PM = get<uint32_t>();
    const uint64_t len = get<uint64_t>();
    uint8_t* body = get_bytes(len);
    const uint64_t cap = len / 17 + 1;
    std::vector<WireRespRec> recs(cap);
    const WireWalk w = wire_resp_walk(body, len, recs.data(), cap);
    printf("body %u %u %" PRIu64 " %" PRIu64, b, w.status, w.status ? w.err_off : 0, w.n);
    if (w.status == WIRE_OK)
      for (uint64_t i = 0; i < w.n; i++) {
        const WireRespRec& r = recs[i];
        printf(" | %" PRIu64 " %" PRIu64 " %u %u %u %" PRIu64 " %u %u %u", r.off, r.len, r.tag, r.pp_type, r.error, r.pm_off,
               r.pm_len, r.sh_len, wire_resp_classify(r, PM));
      }
    printf("\n");
    free(body);
  }
  return 0;
}

struct Case {
  uint32_t n, PS, LPS, query, param_len;
  uint8_t *param, *batch_id;
  std::vector<uint8_t*> id, ps, enc, pay, lps;
  std::vector<uint64_t> time;
  std::vector<uint8_t> cfg, verdict, exclude;
  std::vector<uint64_t> eoff, poff;
};

Case read_case() {
  Case c;
  c.n = get<uint32_t>();
  c.PS = get<uint32_t>();
  c.LPS = get<uint32_t>();
  c.query = get<uint32_t>();
  c.param_len = get<uint32_t>();
  c.param = get_bytes(c.param_len);
  c.batch_id = get_bytes(32);
  c.eoff.push_back(0);
  c.poff.push_back(0);
  for (uint32_t i = 0; i < c.n; i++) {
    c.id.push_back(get_bytes(16));
    c.time.push_back(get<uint64_t>());
    c.cfg.push_back(get<uint8_t>());
    c.verdict.push_back(get<uint8_t>());
    c.exclude.push_back(get<uint8_t>());
    const uint32_t el = get<uint32_t>(), pl = get<uint32_t>();
    c.ps.push_back(get_bytes(c.PS));
    c.enc.push_back(get_bytes(el));
    c.pay.push_back(get_bytes(pl));
    c.lps.push_back(get_bytes(c.LPS));
    c.eoff.push_back(c.eoff.back() + el);
    c.poff.push_back(c.poff.back() + pl);
  }
  return c;
}

void free_case(Case& c) {
  free(c.param);
  free(c.batch_id);
  for (auto* v : {&c.id, &c.ps, &c.enc, &c.pay, &c.lps})
    for (uint8_t* p : *v) free(p);
}

void put(FILE* f, const void* p, size_t n) {
  if (n && fwrite(p, 1, n, f) != n) exit(2);
}

int run_req(const char* out_path) {
  FILE* out = fopen(out_path, "wb");
  if (!out) return 2;
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    Case c = read_case();
    const uint64_t n = c.n;
    // select
    std::vector<uint8_t> send(n);
    std::vector<uint64_t> msg_len(n), offsets(n + 1), rank(n + 1);
    for (uint64_t i = 0; i < n; i++) {
      send[i] = c.verdict[i] == 0 && !c.exclude[i];
      msg_len[i] = send[i] ? wire_init_len(c.PS, c.eoff[i + 1] - c.eoff[i], c.poff[i + 1] - c.poff[i], c.LPS) : 0;
    }
    // the scans, the compaction list
    std::vector<uint32_t> sent_index(n);
    for (uint64_t i = 0; i < n; i++) {
      offsets[i + 1] = offsets[i] + msg_len[i];
      rank[i + 1] = rank[i] + send[i];
      if (send[i]) sent_index[rank[i]] = (uint32_t)i;
    }
    uint64_t total = 0;
    const uint32_t st = wire_req_total(n, c.PS, c.LPS, c.eoff.data(), c.poff.data(), send.data(), c.param_len, c.query, &total);
    if (st != WIRE_REQ_OK) {
      put(out, &st, 4);
      free_case(c);
      continue;
    }
    const uint64_t header_len = wire_req_header_len(c.param_len, c.query);
    if (total != header_len + offsets[n]) return 3;
    uint8_t* body = (uint8_t*)malloc(total);
    memset(body, 0xEE, total);
    // pack: thread 0 writes the header, wave k the sent report k
    if (wire_put_req_header(body, c.param, c.param_len, c.query, c.batch_id, (uint32_t)offsets[n]) != header_len) return 3;
    for (uint64_t k = 0; k < rank[n]; k++) {
      const uint64_t i = sent_index[k];
      const uint32_t el = (uint32_t)(c.eoff[i + 1] - c.eoff[i]), pl = (uint32_t)(c.poff[i + 1] - c.poff[i]);
      const WireInitLayout l = wire_init_layout(c.PS, el, pl, c.LPS);
      if (l.len != msg_len[i]) return 3;
      uint8_t* p = body + header_len + offsets[i];
      for (uint32_t lane = 0; lane < 64; lane++)
        if (lane < WIRE_INIT_FIXED) {
          uint64_t at;
          const uint8_t v = wire_init_fixed_byte(lane, c.id[i], c.time[i], c.PS, c.cfg[i], el, pl, c.LPS, &at);
          p[at] = v;
        }
      memcpy(p + l.ps_off, c.ps[i], c.PS);
      memcpy(p + l.enc_off, c.enc[i], el);
      memcpy(p + l.pay_off, c.pay[i], pl);
      memcpy(p + l.sh_off, c.lps[i], c.LPS);
      // the host writer of the head gives the same bytes
      std::vector<uint8_t> again(l.len, 0);
      wire_put_prepare_init_head(again.data(), c.id[i], c.time[i], c.PS, c.cfg[i], el, pl, c.LPS);
      for (uint32_t lane = 0; lane < WIRE_INIT_FIXED; lane++) {
        uint64_t at;
        (void)wire_init_fixed_byte(lane, c.id[i], c.time[i], c.PS, c.cfg[i], el, pl, c.LPS, &at);
        if (again[at] != p[at]) return 3;
      }
    }
    const uint32_t ns = (uint32_t)rank[n];
    put(out, &st, 4);
    put(out, &total, 8);
    put(out, body, total);
    put(out, &ns, 4);
    put(out, sent_index.data(), 4 * (size_t)ns);
    free(body);
    free_case(c);
  }
  fclose(out);
  return 0;
}

int run_total() {
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    const uint64_t n = get<uint64_t>(), PS = get<uint64_t>(), LPS = get<uint64_t>(), param_len = get<uint64_t>();
    const uint32_t query = get<uint32_t>(), has_enc = get<uint32_t>();
    std::vector<uint64_t> eoff, poff(n + 1);
    if (has_enc) {
      eoff.resize(n + 1);
      for (auto& x : eoff) x = get<uint64_t>();
    }
    for (auto& x : poff) x = get<uint64_t>();
    uint64_t total = 0;
    const uint32_t st = wire_req_total(n, PS, LPS, has_enc ? eoff.data() : nullptr, poff.data(), nullptr, param_len, query, &total);
    printf("total %u %u %" PRIu64 "\n", b, st, st ? 0 : total);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  in = fopen(argv[2], "rb");
  if (!in) return 2;
  if (!strcmp(argv[1], "resp")) return run_resp();
  if (!strcmp(argv[1], "req") && argc == 4) return run_req(argv[3]);
  if (!strcmp(argv[1], "total")) return run_total();
  return 2;
}
