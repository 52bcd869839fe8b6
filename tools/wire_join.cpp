// wire_join.cpp — the host work the device request encode replaces, measured: one thread packs an
// AggregationJobInitializeReq body from the arrays a leader holds (report ids, times, config ids, fixed-stride
// public-share and prep-share rows, packed encapsulated keys and payloads with their offset tables) with the framing
// rule (janus_amd/csrc/jx_wire.h). The counterpart of wire_split.cpp; every report is sent.
// Stand-alone: g++ -O2 -std=c++17 -o wire_join tools/wire_join.cpp
//
//   wire_join ARRAYS_FILE BODY_OUT [runs] [warmups]   ->  one JSON line, and the body in BODY_OUT
//
// ARRAYS_FILE (little-endian): u64 n, u32 PS, u32 LPS, u32 query type, u32 param_len, the parameter, batch id[32],
// ids[n x 16], times[n] u64, config ids[n], public shares[n x PS], enc_offsets[n + 1] u64, the encapsulated keys,
// payload_offsets[n + 1] u64, the payloads, prep shares[n x LPS].
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../janus_amd/csrc/jx_wire.h"

using namespace jx;

namespace {
FILE* in = nullptr;
template <class T>
std::vector<T> get(uint64_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, in) != count) exit(2);
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  in = fopen(argv[1], "rb");
  if (!in) return 2;
  const uint64_t n = get<uint64_t>(1)[0];
  const auto head = get<uint32_t>(4);
  const uint32_t PS = head[0], LPS = head[1], query = head[2], param_len = head[3];
  const auto param = get<uint8_t>(param_len), batch_id = get<uint8_t>(32), ids = get<uint8_t>(n * 16);
  const auto times = get<uint64_t>(n);
  const auto cfg = get<uint8_t>(n), ps = get<uint8_t>(n * PS);
  const auto eoff = get<uint64_t>(n + 1);
  const auto encs = get<uint8_t>(eoff[n]);
  const auto poff = get<uint64_t>(n + 1);
  const auto pays = get<uint8_t>(poff[n]);
  const auto lps = get<uint8_t>(n * (uint64_t)LPS);
  fclose(in);
  const int runs = argc > 3 ? atoi(argv[3]) : 5, warmups = argc > 4 ? atoi(argv[4]) : 2;
  std::vector<double> ms;
  std::vector<uint8_t> body;
  for (int it = 0; it < warmups + runs; it++) {
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t total = 0;
    if (wire_req_total(n, PS, LPS, eoff.data(), poff.data(), nullptr, param_len, query, &total) != WIRE_REQ_OK) return 3;
    std::vector<uint8_t> out(total);  // as an encoder would: a fresh buffer of the encoded length per request
    const uint64_t header_len = wire_req_header_len(param_len, query);
    (void)wire_put_req_header(out.data(), param.data(), param_len, query, batch_id.data(), (uint32_t)(total - header_len));
    uint8_t* p = out.data() + header_len;
    for (uint64_t i = 0; i < n; i++) {
      const uint32_t el = (uint32_t)(eoff[i + 1] - eoff[i]), pl = (uint32_t)(poff[i + 1] - poff[i]);
      const WireInitLayout l = wire_init_layout(PS, el, pl, LPS);
      wire_put_prepare_init_head(p, ids.data() + 16 * i, times[i], PS, cfg[i], el, pl, LPS);
      if (PS) memcpy(p + l.ps_off, ps.data() + i * PS, PS);
      if (el) memcpy(p + l.enc_off, encs.data() + eoff[i], el);
      if (pl) memcpy(p + l.pay_off, pays.data() + poff[i], pl);
      if (LPS) memcpy(p + l.sh_off, lps.data() + i * (uint64_t)LPS, LPS);
      p += l.len;
    }
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (it >= warmups) ms.push_back(dt);
    body.swap(out);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || (body.size() && fwrite(body.data(), 1, body.size(), o) != body.size())) return 2;
  fclose(o);
  std::sort(ms.begin(), ms.end());
  printf("{\"n\": %" PRIu64 ", \"body_bytes\": %zu, \"threads\": 1, \"runs\": %d, \"ms_median\": %.3f, \"ms_min\": %.3f}\n", n,
         body.size(), runs, ms[ms.size() / 2], ms.front());
  return 0;
}
