// hosttest_wire.cpp — janus_amd/csrc/jx_wire.h on the CPU (tests/test_wire_host.py): every body of the input file is
// walked sequentially with the framing rule and indexed with the replay of the kernels' fast pass and fallback loop;
// both results are printed, with the records of an accepted body. Built with the address and undefined-behaviour
// sanitizers: a read past a body's end stops the program.
//
// Input: u32 count, then per body u32 query type, u64 length (little-endian) and the bytes.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../janus_amd/csrc/jx_wire.h"

using namespace jx;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t b = 0; b < count; b++) {
    uint32_t q = 0;
    uint64_t len = 0;
    if (fread(&q, 4, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    // an allocation of exactly len bytes: the sanitizer sees any read at or after body + len
    uint8_t* body = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(body, 1, len, f) != len) return 2;
    WireHeader h;
    wire_parse_header(body, len, q, h);
    const uint64_t cap = len / WIRE_MIN_PREPARE_INIT + 1;
    std::vector<WireRec> recs(cap);
    std::vector<uint64_t> offs(cap);
    const WireWalk w = wire_walk(body, h, recs.data(), cap);
    const WireIndex x = wire_index_replay(body, h, offs.data(), cap);
    printf("body %u walk %u %" PRIu64 " %" PRIu64 " index %u %" PRIu64 " %" PRIu64 " iters %u nfast %" PRIu64, b, w.status,
           w.status ? w.err_off : 0, w.n, x.status, x.status ? x.err_off : 0, x.n, x.iters, x.nfast);
    bool same = w.status == x.status && w.n == x.n && (!w.status || w.err_off == x.err_off);
    for (uint64_t i = 0; same && w.status == WIRE_OK && i < w.n; i++)
      same = recs[i].off == (i < x.nfast ? h.start + i * h.l0 : offs[i - x.nfast]);
    printf(" same %d", (int)same);
    if (w.status == WIRE_OK) {
      printf(" hdr %" PRIu64 " %" PRIu64 " %u ", h.param_off, h.param_len, h.has_batch_id);
      for (int i = 0; i < 32; i++) printf("%02x", h.batch_id[i]);
      for (uint64_t i = 0; i < w.n; i++) {
        const WireRec& r = recs[i];
        printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %u %" PRIu64 " %u %" PRIu64 " %u %" PRIu64
               " %u %" PRIu64 " %u %u %u",
               r.off, r.len, r.ps_off, r.ps_len, r.enc_off, r.enc_len, r.pay_off, r.pay_len, r.msg_off, r.msg_len,
               r.pm_off, r.pm_len, r.sh_off, r.sh_len, r.config_id, r.pp_type);
      }
    }
    printf("\n");
    free(body);
  }
  fclose(f);
  return 0;
}
