// Host build of janus_amd/csrc/jx_collect.h for tests/test_collect_host.py: the per-element decode and add and the
// per-job status decisions of the collection kernels, one call at a time.
#include <cstdint>
#include <cstring>

#include "../../janus_amd/csrc/jx_collect.h"

using namespace jx;

extern "C" {

// the element's 8 little-endian bytes as one word: 1 when canonical, and the value
int ch_decode64(uint64_t w, uint64_t* out) {
  uint64_t v;
  const bool ok = collect_decode64(w, v);
  *out = v;
  return ok;
}
int ch_decode128(uint64_t lo, uint64_t hi, uint64_t out[2]) {
  f128 v;
  const bool ok = collect_decode128(lo, hi, v);
  out[0] = v.lo;
  out[1] = v.hi;
  return ok;
}
uint64_t ch_add64(uint64_t a, uint64_t b) { return collect_add64(a, b); }
void ch_add128(const uint64_t a[2], const uint64_t b[2], uint64_t out[2]) {
  const f128 s = collect_add128(make128(a[0], a[1]), make128(b[0], b[1]));
  out[0] = s.lo;
  out[1] = s.hi;
}
// expect_checksum null: no expectations
uint32_t ch_status(uint64_t nrecords, int bad_record, uint64_t count, const uint8_t* checksum, uint64_t expect_count,
                   const uint8_t* expect_checksum, uint64_t min_batch_size, uint64_t max_batch_size) {
  return collect_status(nrecords, bad_record != 0, count, checksum, expect_count, expect_checksum, min_batch_size,
                        max_batch_size);
}
uint32_t ch_seal_status(uint32_t status, int sealed) { return collect_seal_status(status, sealed != 0); }
uint32_t ch_open_status(int leader_opened, int helper_opened, int leader_bad, int helper_bad) {
  return collect_open_status(leader_opened != 0, helper_opened != 0, leader_bad != 0, helper_bad != 0);
}
}
