// upload_split.cpp — the host work the device upload decode replaces, measured: one thread parses n Report bodies
// lying back to back with the framing rule (janus_amd/csrc/jx_wire.h), makes the upload checks and splits the accepted
// ones into what the upload open and the request encode take: ids, times, fixed-stride public-share rows, key slots,
// the leader's and the helper's encapsulated keys and payloads packed with their offset tables.
// Stand-alone: g++ -O2 -std=c++17 -o upload_split tools/upload_split.cpp
//
//   upload_split BODIES_FILE OFFSETS_FILE PS NOW [runs] [warmups]   ->  one JSON line
// OFFSETS_FILE: n + 1 little-endian u64.
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../janus_amd/csrc/jx_wire.h"

using namespace jx;

static std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const uint64_t len = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> b(len);
  if (len && fread(b.data(), 1, len, f) != len) exit(2);
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::vector<uint8_t> body = slurp(argv[1]), offs_raw = slurp(argv[2]);
  if (offs_raw.size() < 8 || offs_raw.size() % 8) return 2;
  const uint64_t n = offs_raw.size() / 8 - 1;
  std::vector<uint64_t> boff(n + 1);
  memcpy(boff.data(), offs_raw.data(), offs_raw.size());
  const uint32_t PS = (uint32_t)atoi(argv[3]);
  WireUploadChecks ck{};
  ck.now = strtoull(argv[4], nullptr, 10);
  const int runs = argc > 5 ? atoi(argv[5]) : 5, warmups = argc > 6 ? atoi(argv[6]) : 2;
  uint8_t kf[256], ks[256];
  memset(kf, 0, 256);
  memset(ks, 0xFF, 256);
  std::vector<double> ms;
  uint64_t m = 0, sink = 0;
  for (int it = 0; it < warmups + runs; it++) {
    const auto t0 = std::chrono::steady_clock::now();
    // as a decoder that grows its vectors would: nothing is sized before the loop has seen it
    std::vector<uint8_t> ids, ps, kidx, cfg, status, packed[4];
    std::vector<uint64_t> times, offs[4] = {{0}, {0}, {0}, {0}};
    std::vector<uint32_t> index, row_of;
    const uint8_t* b = body.data();
    for (uint64_t i = 0; i < n; i++) {
      if (boff[i + 1] < boff[i] || boff[i + 1] > body.size()) return 3;
      WireReportRec r;
      uint8_t id[16];
      uint64_t t;
      const uint8_t st = wire_upload_parse(b, boff[i], boff[i + 1], PS, ck, kf, ks, r, id, &t);
      status.push_back(st);
      if (st != UPLOAD_OK) {
        row_of.push_back(UPLOAD_NO_ROW);
        continue;
      }
      row_of.push_back((uint32_t)index.size());
      index.push_back((uint32_t)i);
      ids.insert(ids.end(), id, id + 16);
      times.push_back(t);
      ps.insert(ps.end(), b + r.ps_off, b + r.ps_off + PS);
      kidx.push_back(r.key0);
      kidx.push_back(r.key1);
      cfg.push_back(r.helper_config_id);
      const uint64_t src[4] = {r.lenc_off, r.lpay_off, r.henc_off, r.hpay_off};
      const uint32_t lens[4] = {r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len};
      for (int f = 0; f < 4; f++) {
        packed[f].insert(packed[f].end(), b + src[f], b + src[f] + lens[f]);
        offs[f].push_back(packed[f].size());
      }
    }
    m = index.size();
    sink += ids.size() + ps.size() + kidx.size() + cfg.size() + times.size() + status.size() + row_of.size();
    for (int f = 0; f < 4; f++) sink += offs[f].back() + (packed[f].empty() ? 0 : packed[f][packed[f].size() / 2]);
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (it >= warmups) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"n\": %" PRIu64 ", \"accepted\": %" PRIu64 ", \"body_bytes\": %zu, \"threads\": 1, \"runs\": %d, \"ms_median\": %.3f, "
         "\"ms_min\": %.3f, \"sink\": %" PRIu64 "}\n",
         n, m, body.size(), runs, ms[ms.size() / 2], ms.front(), sink);
  return 0;
}
