// hosttest_wire_upload.cpp — the upload half of janus_amd/csrc/jx_wire.h on the CPU (tests/test_wire_upload_host.py).
// Built with the address and undefined-behaviour sanitizers: every body and every output lives in an allocation of
// exactly its length, so a read or write one byte past it stops the program.
//
//   parse FILE        u32 count, then per body u64 length and the bytes (little-endian). wire_parse_report over
//                     [0, length); one output line per body: ok, the error offset, the record.
//   write FILE OUT    u32 count, then per case the fields of a Report (see read_report). The body is written by
//                     wire_report_layout and wire_report_fixed_byte into an allocation of exactly wire_report_len;
//                     OUT takes u64 length and the body per case.
//   check FILE        u32 count, then per case u64 time, now, skew, u32 has_expiration, u64 expiration, u32 has_age,
//                     u64 age: wire_upload_check, one status per line.
//   decode FILE OUT   one batch of uploads (see run_decode): a replay of the kernels, parse per upload, the scans and
//                     the compaction, then one wave's work per loop iteration of the gather with `parts` waves per
//                     report; every output array in an allocation of exactly its size, every byte of the packed arrays
//                     written exactly once.
//   pack FILE OUT     one batch of sealed rows (see run_pack): the client's scan and one wave's work per loop
//                     iteration of the pack into an allocation of exactly the total.
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
void put(FILE* f, const void* p, size_t n) {
  if (n && fwrite(p, 1, n, f) != n) exit(2);
}

int run_parse() {
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    const uint64_t len = get<uint64_t>();
    uint8_t* body = get_bytes(len);
    WireReportRec r;
    uint64_t eo = 0;
    const bool ok = wire_parse_report(body, len, 0, r, &eo);
    printf("body %u %d %" PRIu64, b, ok ? 1 : 0, ok ? 0 : eo);
    if (ok)
      printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %u %" PRIu64 " %u %u %" PRIu64 " %u %" PRIu64 " %u", r.off,
             r.len, r.ps_off, r.ps_len, r.leader_config_id, r.lenc_off, r.lenc_len, r.lpay_off, r.lpay_len,
             r.helper_config_id, r.henc_off, r.henc_len, r.hpay_off, r.hpay_len);
    printf("\n");
    free(body);
  }
  return 0;
}

struct Rep {
  uint8_t* id;
  uint64_t time;
  uint8_t lcfg, hcfg;
  uint32_t ps_len, lenc_len, lpay_len, henc_len, hpay_len;
  uint8_t *ps, *lenc, *lpay, *henc, *hpay;
};
Rep read_report() {
  Rep r;
  r.id = get_bytes(16);
  r.time = get<uint64_t>();
  r.lcfg = get<uint8_t>();
  r.hcfg = get<uint8_t>();
  r.ps_len = get<uint32_t>();
  r.lenc_len = get<uint32_t>();
  r.lpay_len = get<uint32_t>();
  r.henc_len = get<uint32_t>();
  r.hpay_len = get<uint32_t>();
  r.ps = get_bytes(r.ps_len);
  r.lenc = get_bytes(r.lenc_len);
  r.lpay = get_bytes(r.lpay_len);
  r.henc = get_bytes(r.henc_len);
  r.hpay = get_bytes(r.hpay_len);
  return r;
}
void free_report(Rep& r) {
  for (uint8_t* p : {r.id, r.ps, r.lenc, r.lpay, r.henc, r.hpay}) free(p);
}

// one Report at p, as the pack kernel's wave writes it: lanes 0-41 the fixed bytes, then the five fields in slices
void write_report(uint8_t* p, const Rep& r, uint32_t parts) {
  const WireReportLayout l = wire_report_layout(r.ps_len, r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len);
  for (uint32_t part = 0; part < parts; part++) {
    if (part == 0) {
      for (uint32_t lane = 0; lane < 64; lane++)
        if (lane < WIRE_REPORT_FIXED) {
          uint64_t at;
          const uint8_t v = wire_report_fixed_byte(lane, r.id, r.time, r.ps_len, r.lcfg, r.lenc_len, r.lpay_len, r.hcfg,
                                                   r.henc_len, r.hpay_len, &at);
          p[at] = v;
        }
      memcpy(p + l.ps_off, r.ps, r.ps_len);
    }
    const uint64_t offs[4] = {l.lenc_off, l.lpay_off, l.henc_off, l.hpay_off};
    const uint8_t* src[4] = {r.lenc, r.lpay, r.henc, r.hpay};
    const uint32_t lens[4] = {r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len};
    for (int f = 0; f < 4; f++) {
      uint64_t lo, cnt;
      wire_part_span(lens[f], part, parts, &lo, &cnt);
      memcpy(p + offs[f] + lo, src[f] + lo, cnt);
    }
  }
}

int run_write(const char* out_path) {
  FILE* out = fopen(out_path, "wb");
  if (!out) return 2;
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    Rep r = read_report();
    const uint64_t len = wire_report_len(r.ps_len, r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len);
    if (wire_report_layout(r.ps_len, r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len).len != len) return 3;
    uint8_t* body = (uint8_t*)malloc(len);
    memset(body, 0xEE, len);
    write_report(body, r, 1 + b % 3);
    put(out, &len, 8);
    put(out, body, len);
    free(body);
    free_report(r);
  }
  fclose(out);
  return 0;
}

int run_check() {
  const uint32_t count = get<uint32_t>();
  for (uint32_t b = 0; b < count; b++) {
    const uint64_t time = get<uint64_t>(), now = get<uint64_t>(), skew = get<uint64_t>();
    const uint32_t has_exp = get<uint32_t>();
    const uint64_t exp = get<uint64_t>();
    const uint32_t has_age = get<uint32_t>();
    const uint64_t age = get<uint64_t>();
    printf("check %u %u\n", b, wire_upload_check(time, now, skew, has_exp ? &exp : nullptr, has_age ? &age : nullptr));
  }
  return 0;
}

// an output array of exactly its size that counts the writes of every byte
struct Out {
  std::vector<uint8_t> buf, writes;  // buf: a heap block of exactly n bytes
  explicit Out(uint64_t n) : buf(n, 0xEE), writes(n, 0) {}
  const uint8_t* p() const { return buf.data(); }
  void copy(uint64_t at, const uint8_t* src, uint64_t n) {
    if (n) memcpy(buf.data() + at, src, n);
    for (uint64_t k = 0; k < n; k++) writes[at + k]++;
  }
  bool once() const {
    for (uint8_t w : writes)
      if (w != 1) return false;
    return true;
  }
};

// u32 n, PS, parts; u64 now, skew, u32 has_exp, u64 exp, u32 has_age, u64 age; key_first[256], key_second[256];
// (n + 1) u64 offsets; u64 len; the bodies.
int run_decode(const char* out_path) {
  FILE* out = fopen(out_path, "wb");
  if (!out) return 2;
  const uint32_t n = get<uint32_t>(), PS = get<uint32_t>(), parts = get<uint32_t>();
  WireUploadChecks ck{};
  ck.now = get<uint64_t>();
  ck.skew = get<uint64_t>();
  ck.has_task_expiration = get<uint32_t>();
  ck.task_expiration = get<uint64_t>();
  ck.has_report_expiry_age = get<uint32_t>();
  ck.report_expiry_age = get<uint64_t>();
  uint8_t *kf = get_bytes(256), *ks = get_bytes(256);
  std::vector<uint64_t> boff(n + 1);
  for (auto& x : boff) x = get<uint64_t>();
  const uint64_t len = get<uint64_t>();
  uint8_t* body = get_bytes(len);
  // parse: one thread per upload
  std::vector<WireReportRec> recs(n);
  std::vector<uint8_t> status(n), ids_all(16 * (size_t)n);
  std::vector<uint64_t> times_all(n);
  for (uint32_t i = 0; i < n; i++)
    status[i] = wire_upload_parse(body, boff[i], boff[i + 1], PS, ck, kf, ks, recs[i], ids_all.data() + 16 * (size_t)i, &times_all[i]);
  // scan: the accept flags and the four lengths, then the compaction
  std::vector<uint64_t> rank(n + 1), scan[4];
  for (auto& s : scan) s.assign(n + 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    const WireReportRec& r = recs[i];
    if (status[i] != UPLOAD_OK && (r.ps_len | r.lenc_len | r.lpay_len | r.henc_len | r.hpay_len)) return 3;
    rank[i + 1] = rank[i] + (status[i] == UPLOAD_OK);
    scan[0][i + 1] = scan[0][i] + r.lenc_len;
    scan[1][i + 1] = scan[1][i] + r.lpay_len;
    scan[2][i + 1] = scan[2][i] + r.henc_len;
    scan[3][i + 1] = scan[3][i] + r.hpay_len;
  }
  const uint64_t m = rank[n];
  std::vector<uint32_t> index(m), row_of(n);
  std::vector<uint64_t> offs[4];
  for (auto& o : offs) o.assign(m + 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (status[i] != UPLOAD_OK) {
      row_of[i] = UPLOAD_NO_ROW;
      continue;
    }
    const uint64_t k = rank[i];
    row_of[i] = (uint32_t)k;
    index[k] = i;
    for (int f = 0; f < 4; f++) offs[f][k] = scan[f][i];
  }
  for (int f = 0; f < 4; f++) offs[f][m] = scan[f][n];
  // gather: `parts` waves per accepted report
  Out ids(16 * m), ps((uint64_t)PS * m), kidx(2 * m), cfg(m), times(8 * m);
  Out packed[4] = {Out(scan[0][n]), Out(scan[1][n]), Out(scan[2][n]), Out(scan[3][n])};
  for (uint64_t w = 0; w < m * parts; w++) {
    const uint64_t k = w / parts;
    const uint32_t part = (uint32_t)(w % parts);
    const uint32_t i = index[k];
    const WireReportRec& r = recs[i];
    if (part == 0) {
      ids.copy(16 * k, body + r.off, 16);
      times.copy(8 * k, (const uint8_t*)&times_all[i], 8);
      kidx.copy(2 * k, &r.key0, 1);
      kidx.copy(2 * k + 1, &r.key1, 1);
      cfg.copy(k, &r.helper_config_id, 1);
      ps.copy((uint64_t)PS * k, body + r.ps_off, PS);
    }
    const uint64_t src[4] = {r.lenc_off, r.lpay_off, r.henc_off, r.hpay_off};
    const uint32_t lens[4] = {r.lenc_len, r.lpay_len, r.henc_len, r.hpay_len};
    for (int f = 0; f < 4; f++) {
      uint64_t lo, cnt;
      wire_part_span(lens[f], part, parts, &lo, &cnt);
      packed[f].copy(offs[f][k] + lo, body + src[f] + lo, cnt);
    }
  }
  for (const Out* o : {&ids, &ps, &kidx, &cfg, &times, &packed[0], &packed[1], &packed[2], &packed[3]})
    if (!o->once()) return 4;
  put(out, status.data(), n);
  put(out, row_of.data(), 4 * (size_t)n);
  put(out, ids_all.data(), 16 * (size_t)n);
  put(out, times_all.data(), 8 * (size_t)n);
  put(out, &m, 8);
  put(out, index.data(), 4 * m);
  put(out, ids.p(), 16 * m);
  put(out, times.p(), 8 * m);
  put(out, ps.p(), (uint64_t)PS * m);
  put(out, kidx.p(), 2 * m);
  put(out, cfg.p(), m);
  for (int f = 0; f < 4; f++) {
    put(out, offs[f].data(), 8 * (m + 1));
    put(out, packed[f].p(), scan[f][n]);
  }
  fclose(out);
  free(kf);
  free(ks);
  free(body);
  return 0;
}

// u32 n, PS, lenc, lct, henc, hct, u8 lcfg, hcfg, u32 has_status, parts; then per report id[16], u64 time, u8 status
// and the five rows.
int run_pack(const char* out_path) {
  FILE* out = fopen(out_path, "wb");
  if (!out) return 2;
  const uint32_t n = get<uint32_t>(), PS = get<uint32_t>(), le = get<uint32_t>(), lc = get<uint32_t>(), he = get<uint32_t>(),
                 hc = get<uint32_t>();
  const uint8_t lcfg = get<uint8_t>(), hcfg = get<uint8_t>();
  const uint32_t has_status = get<uint32_t>(), parts = get<uint32_t>();
  std::vector<Rep> reps(n);
  std::vector<uint8_t> status(n);
  for (uint32_t i = 0; i < n; i++) {
    Rep& r = reps[i];
    r.id = get_bytes(16);
    r.time = get<uint64_t>();
    status[i] = get<uint8_t>();
    r.lcfg = lcfg;
    r.hcfg = hcfg;
    r.ps_len = PS, r.lenc_len = le, r.lpay_len = lc, r.henc_len = he, r.hpay_len = hc;
    r.ps = get_bytes(PS);
    r.lenc = get_bytes(le);
    r.lpay = get_bytes(lc);
    r.henc = get_bytes(he);
    r.hpay = get_bytes(hc);
  }
  const uint64_t L = wire_report_len(PS, le, lc, he, hc);
  std::vector<uint64_t> offsets(n + 1), rank(n + 1);
  std::vector<uint32_t> index(n);
  for (uint32_t i = 0; i < n; i++) {
    const bool room = !(has_status && status[i]);
    offsets[i + 1] = offsets[i] + (room ? L : 0);
    rank[i + 1] = rank[i] + room;
    if (room) index[rank[i]] = i;
  }
  uint8_t* body = (uint8_t*)malloc(offsets[n] ? offsets[n] : 1);
  memset(body, 0xEE, offsets[n] ? offsets[n] : 1);
  for (uint64_t k = 0; k < rank[n]; k++) write_report(body + offsets[index[k]], reps[index[k]], parts);
  put(out, offsets.data(), 8 * (size_t)(n + 1));
  put(out, body, offsets[n]);
  free(body);
  for (Rep& r : reps) free_report(r);
  fclose(out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  in = fopen(argv[2], "rb");
  if (!in) return 2;
  if (!strcmp(argv[1], "parse")) return run_parse();
  if (!strcmp(argv[1], "write") && argc == 4) return run_write(argv[3]);
  if (!strcmp(argv[1], "check")) return run_check();
  if (!strcmp(argv[1], "decode") && argc == 4) return run_decode(argv[3]);
  if (!strcmp(argv[1], "pack") && argc == 4) return run_pack(argv[3]);
  return 2;
}
