// wire_split.cpp — the host work the device codec replaces, measured: one thread walks an AggregationJobInitializeReq
// body message by message with the framing rule (janus_amd/csrc/jx_wire.h) and splits it into what the sealed fused
// call takes: report ids, times, fixed-stride public-share and leader prep-share rows, packed encapsulated keys and
// payloads with their offset tables. Stand-alone: g++ -O2 -std=c++17 -o wire_split tools/wire_split.cpp
//
//   wire_split BODY_FILE QUERY_TYPE PS LPS [runs] [warmups]   ->  one JSON line
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../janus_amd/csrc/jx_wire.h"

using namespace jx;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const uint64_t len = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> body(len);
  if (len && fread(body.data(), 1, len, f) != len) return 2;
  fclose(f);
  const uint32_t q = (uint32_t)atoi(argv[2]), PS = (uint32_t)atoi(argv[3]), LPS = (uint32_t)atoi(argv[4]);
  const int runs = argc > 5 ? atoi(argv[5]) : 5, warmups = argc > 6 ? atoi(argv[6]) : 2;
  std::vector<double> ms;
  uint64_t n = 0, sink = 0;
  for (int it = 0; it < warmups + runs; it++) {
    const auto t0 = std::chrono::steady_clock::now();
    WireHeader h;
    wire_parse_header(body.data(), len, q, h);
    if (h.status != WIRE_OK) return 3;
    // as a decoder that grows its vectors would: nothing is sized before the walk has seen it
    std::vector<uint8_t> ids, ps, lps, encs, pays, status;
    std::vector<uint64_t> times, eoff{0}, poff{0};
    uint64_t off = h.start;
    n = 0;
    while (off < h.end) {
      WireRec r;
      uint64_t eo;
      if (!wire_parse_prepare_init(body.data(), h.end, off, r, &eo)) return 3;
      const uint8_t* b = body.data();
      ids.insert(ids.end(), b + r.off, b + r.off + 16);
      times.push_back(wire_be64(b + r.off + 16));
      const uint8_t ws = r.ps_len != PS ? 1 : r.pp_type != 0 ? 2 : r.sh_len != LPS ? 3 : 0;
      status.push_back(ws);
      ps.resize(ps.size() + PS);
      if (ws != 1 && PS) memcpy(ps.data() + ps.size() - PS, b + r.ps_off, PS);
      lps.resize(lps.size() + LPS);
      if (r.pp_type == 0 && r.sh_len == LPS && LPS) memcpy(lps.data() + lps.size() - LPS, b + r.sh_off, LPS);
      encs.insert(encs.end(), b + r.enc_off, b + r.enc_off + r.enc_len);
      pays.insert(pays.end(), b + r.pay_off, b + r.pay_off + r.pay_len);
      eoff.push_back(encs.size());
      poff.push_back(pays.size());
      off += r.len;
      n++;
    }
    sink += ids.size() + ps.size() + lps.size() + encs.size() + pays.size() + times.size() + status.size() + eoff.back() + poff.back();
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (it >= warmups) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"n\": %" PRIu64 ", \"body_bytes\": %" PRIu64 ", \"threads\": 1, \"runs\": %d, \"ms_median\": %.3f, \"ms_min\": %.3f, \"sink\": %" PRIu64 "}\n",
         n, len, runs, ms[ms.size() / 2], ms.front(), sink);
  return 0;
}
