// Host checks of the one rule that lays a sealed report out as an EncRow (janus_amd/csrc/jx_enc_rows.h): a
// stand-alone program for a build with -fsanitize=address,undefined (tests/test_enc_rows_host.py). One line per
// check, then "all ok"; exit status 0.
//
// Seeded random jobs go through three paths. `loop_before` is fill_enc_rows as it stood before the rule was
// shared, written out here once more: the expectation. fill_enc_rows_with is what fill_enc_rows runs now (the host
// callers). `as_the_kernel` is enc_rows_kernel's lane body: enc_row_make per report with the absolute ciphertext
// offsets and one 65-byte slot per report. The first must equal the expectation byte for byte; the kernel's rows
// differ from it only where the device form differs by design (ct_off absolute instead of counted from the first
// report, the 65-byte key in the report's own slot), and must equal it byte for byte once those two are mapped back.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../janus_amd/csrc/jx_enc_rows.h"

using namespace jx;

static int g_failed = 0;
static void check(bool ok, const char* what) {
  printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) g_failed++;
}

struct Job {
  uint64_t n = 0;
  EncRowKeys K{};
  uint8_t task_id[32];
  std::vector<uint64_t> times, enc_off, pay_off;
  std::vector<uint8_t> key_index, encs;
  bool offsets = true;  // enc_offsets given (else n x 32 bytes)
};

// fill_enc_rows before the rule was shared (jx_coalesce.cpp), over the same plain arrays
static uint64_t loop_before(const Job& j, EncRow* rows, uint64_t ct_base, uint8_t* enc65) {
  const uint64_t n = j.n, c0 = j.pay_off[0], enc65_base = ct_base + (j.pay_off[n] - j.pay_off[0]);
  uint64_t n65 = 0;
  for (uint64_t i = 0; i < n; i++) {
    EncRow& w = rows[i];
    memset(&w, 0, sizeof w);
    memcpy(w.task_id, j.task_id, 32);
    const uint64_t t = j.times[i];
    for (int b = 0; b < 8; b++) w.time_be[b] = (uint8_t)(t >> (56 - 8 * b));
    w.ct_off = ct_base + (j.pay_off[i] - c0);
    w.ct_len = (uint32_t)(j.pay_off[i + 1] - j.pay_off[i]);
    const uint8_t k0 = j.key_index[2 * i], k1 = j.key_index[2 * i + 1];
    w.flags = ENC_ROW_ENCRYPTED | ((j.K.flags & JX_ENC_REQUIRE_TASKPROV) ? ENC_ROW_REQUIRE_TASKPROV : 0);
    const uint64_t len = j.offsets ? j.enc_off[i + 1] - j.enc_off[i] : 32;
    const uint8_t* enc = j.encs.data() + (j.offsets ? j.enc_off[i] : 32 * i);
    const bool fits = (k0 < j.K.nkeys && j.K.klen[k0] == len) || (k1 < j.K.nkeys && j.K.klen[k1] == len);
    if (k0 == JX_KEY_MALFORMED || (k0 < j.K.nkeys && !fits)) {
      w.flags |= ENC_ROW_MALFORMED;
    } else if (fits && len == 65) {
      w.flags |= ENC_ROW_ENC65;
      w.enc65_off = enc65_base + 65 * n65;
      memcpy(enc65 + 65 * n65, enc, 65);
      n65++;
    } else if (len == 32) {
      memcpy(w.enc, enc, 32);
    }
    w.key0 = k0 < j.K.nkeys ? j.K.slot[k0] : (k0 == JX_KEY_MALFORMED ? (uint16_t)0 : KEY_SLOT_NONE);
    w.key1 = k1 < j.K.nkeys ? j.K.slot[k1] : KEY_SLOT_NONE;
  }
  return n65;
}

// enc_rows_kernel's lane body for report r of a launch that starts at report `first` of the job
static void as_the_kernel(const Job& j, uint64_t first, uint64_t m, EncRow* rows, uint8_t* enc65, uint64_t enc65_base) {
  for (uint64_t r = 0; r < m; r++) {
    const uint64_t i = first + r;
    const uint64_t eo = j.offsets ? j.enc_off[i] : 32 * i, elen = j.offsets ? j.enc_off[i + 1] - eo : 32;
    const uint64_t p0 = j.pay_off[i], p1 = j.pay_off[i + 1];
    enc_row_make(rows[r], j.K, j.task_id, j.times[i], j.key_index[2 * i], j.key_index[2 * i + 1], j.encs.data() + eo,
                 elen, p0, (uint32_t)(p1 - p0), enc65_base + 65 * r, enc65 + 65 * r);
  }
}

static Job make_job(std::mt19937_64& g, uint64_t n, bool offsets, bool taskprov, uint64_t pay0) {
  Job j;
  j.n = n;
  j.offsets = offsets;
  j.K.nkeys = 1 + g() % JX_ENC_MAX_KEYPAIRS;
  j.K.flags = taskprov ? JX_ENC_REQUIRE_TASKPROV : 0;
  for (uint32_t k = 0; k < j.K.nkeys; k++) {
    j.K.klen[k] = (g() % 3 == 0) ? 65 : 32;  // both KEMs among the request's keypairs
    j.K.slot[k] = (uint16_t)(g() % 16384);
  }
  for (int b = 0; b < 32; b++) j.task_id[b] = (uint8_t)g();
  j.enc_off.push_back(offsets ? g() % 7 : 0);
  j.pay_off.push_back(pay0);
  const uint64_t lens[6] = {32, 65, 32, 65, 31, 0};  // 32- and 65-byte keys, and keys of other lengths
  for (uint64_t i = 0; i < n; i++) {
    j.times.push_back(g());
    const uint64_t len = offsets ? (g() % 11 == 0 ? 33 + g() % 40 : lens[g() % 6]) : 32;
    j.enc_off.push_back(j.enc_off.back() + len);
    j.pay_off.push_back(j.pay_off.back() + (g() % 5 == 0 ? g() % 16 : 70 + g() % 30));
    // first keypair: an index, JX_KEY_NONE or JX_KEY_MALFORMED; fallback: an index (often of the other KEM) or none
    const uint64_t a = g() % 10, b = g() % 3;
    j.key_index.push_back(a == 0 ? JX_KEY_NONE : a == 1 ? JX_KEY_MALFORMED : (uint8_t)(g() % j.K.nkeys));
    j.key_index.push_back(b == 0 ? JX_KEY_NONE : (uint8_t)(g() % j.K.nkeys));
  }
  j.encs.resize((offsets ? j.enc_off.back() : 32 * n) + 1);
  for (auto& x : j.encs) x = (uint8_t)g();
  return j;
}

int main() {
  std::mt19937_64 g(20261020);
  bool host_equal = true, kernel_equal = true, counts = true;
  uint64_t rows_seen = 0, seen65 = 0, seen_malformed = 0, seen_none = 0, seen_other_kem = 0;
  for (int t = 0; t < 400; t++) {
    const uint64_t n = 1 + g() % 200;
    const Job j = make_job(g, n, t % 4 != 0, t % 3 == 0, t % 2 ? 1000 + g() % 5000 : 0);
    const uint64_t ct_base = t % 5 ? g() % 100000 : 0;
    std::vector<EncRow> want(n), got(n);
    std::vector<uint8_t> want65(65 * n + 1, 0xAA), got65(65 * n + 1, 0xAA);
    const uint64_t w65 = loop_before(j, want.data(), ct_base, want65.data());
    const uint64_t g65 = fill_enc_rows_with(j.K, j.task_id, j.times.data(), j.key_index.data(), j.encs.data(),
                                            j.offsets ? j.enc_off.data() : nullptr, j.pay_off.data(), n, got.data(),
                                            ct_base, ct_base + (j.pay_off[n] - j.pay_off[0]), got65.data());
    counts = counts && w65 == g65;
    host_equal = host_equal && memcmp(want.data(), got.data(), n * sizeof(EncRow)) == 0 && want65 == got65;
    // the kernel's path, launch by launch (a launch size that is no divisor of n)
    const uint64_t chunk = 1 + g() % 64, base65 = 0x7000000000000000ull + g() % 4096;
    for (uint64_t first = 0; first < n; first += chunk) {
      const uint64_t m = n - first < chunk ? n - first : chunk;
      std::vector<EncRow> k(m);
      std::vector<uint8_t> k65(65 * m + 1, 0xAA);
      as_the_kernel(j, first, m, k.data(), k65.data(), base65);
      for (uint64_t r = 0; r < m; r++) {
        EncRow a = k[r];
        const EncRow& w = want[first + r];
        if (a.flags & ENC_ROW_ENC65) {  // the key: the same bytes, in the report's own slot
          kernel_equal = kernel_equal && a.enc65_off == base65 + 65 * r && (w.flags & ENC_ROW_ENC65) &&
                         memcmp(&k65[65 * r], &want65[w.enc65_off - (ct_base + (j.pay_off[n] - j.pay_off[0]))], 65) == 0;
          a.enc65_off = w.enc65_off;
        } else {
          for (int b = 0; b < 65; b++) kernel_equal = kernel_equal && k65[65 * r + b] == 0xAA;  // slot untouched
        }
        kernel_equal = kernel_equal && a.ct_off == j.pay_off[first + r];  // absolute, as the caller counts
        a.ct_off = w.ct_off;
        kernel_equal = kernel_equal && memcmp(&a, &w, sizeof a) == 0;
      }
    }
    for (uint64_t i = 0; i < n; i++) {
      rows_seen++;
      seen65 += (want[i].flags & ENC_ROW_ENC65) != 0;
      seen_malformed += (want[i].flags & ENC_ROW_MALFORMED) != 0;
      seen_none += want[i].key0 == KEY_SLOT_NONE;
      const uint8_t k0 = j.key_index[2 * i], k1 = j.key_index[2 * i + 1];
      seen_other_kem += k0 < j.K.nkeys && k1 < j.K.nkeys && j.K.klen[k0] != j.K.klen[k1];
    }
  }
  check(counts, "the host loop counts the 65-byte rows as before");
  check(host_equal, "fill_enc_rows_with equals the loop as it was, rows and packed 65-byte keys, byte for byte");
  check(kernel_equal, "the kernel's lane body equals it too, but for absolute ct_off and per-report key slots");
  check(rows_seen > 30000 && seen65 > 500 && seen_malformed > 2000 && seen_none > 2000 && seen_other_kem > 2000,
        "the jobs held 65-byte rows, malformed rows, unknown configs and fallbacks of the other KEM");
  check(sizeof(EncRowsArgs) <= 256, "the kernel's arguments stay small");
  printf(g_failed ? "%d FAILED\n" : "all ok\n", g_failed);
  return g_failed ? 1 : 0;
}
