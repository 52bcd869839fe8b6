// Host checks of the helper K1 choice (janus_amd/csrc/jx_k1_plan.h): a stand-alone program for a build with
// -fsanitize=address,undefined (tests/test_k1_plan_host.py). One line per check, then "all ok"; exit status 0.
// The expectations are those of the engine's prep_core before the choice had a header of its own, at the MI355X's
// round_reports of 131,072 (256 CUs x 2 workgroups x 256 reports): they pin the thresholds, which no parity test
// sees (a slip there only costs speed).
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../janus_amd/csrc/jx_k1_plan.h"

using namespace jx;

static int g_failed = 0;
static void check(bool ok, const char* what) {
  printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) g_failed++;
}

constexpr uint64_t RR = 131072;
constexpr uint32_t LDS_LANES = 55296, LDS_ONE_WG = 82944;  // lanes_lds_bytes(2), lanes_lds_bytes(1)

// the base case: helper, not wide, automatic, lanes_wg_cap 2
static K1Plan base(uint64_t n, bool busy = false, uint64_t rr = RR, uint32_t cap = 2) {
  return k1_plan(n, rr, K1_AUTO, false, false, false, cap, busy);
}
// forced, with another engine's big launch in flight so that no split arises
static K1Plan forced(K1Kernel k, uint64_t n, bool wide = false) { return k1_plan(n, RR, k, false, wide, false, 2, true); }

static bool single(const K1Plan& p, K1Kernel k, uint32_t lds) {
  return p.split == 0 && p.head.kernel == k && p.head.lds == lds;
}
static bool mixed(const K1Plan& p, uint64_t split, K1Kernel tail) {
  return p.split == split && p.head.kernel == K1_LANES && p.head.lds == LDS_LANES && p.tail.kernel == tail &&
         p.tail.lds == 0;
}

int main() {
  check(K1_AUTO == 0 && K1_LANES == 3 && K1_FUSED == 5 && K1_PAIRS == 6 && K1_WORDS == 7 && K1_PAIRS_UNROLLED == 8,
        "the enum keeps the numbers of debug option 3");
  check(k1_forceable(0) && k1_forceable(3) && k1_forceable(5) && k1_forceable(6) && k1_forceable(7) &&
            !k1_forceable(8) && !k1_forceable(1) && !k1_forceable(2) && !k1_forceable(4) && !k1_forceable(9) &&
            !k1_forceable(-1) && !k1_forceable((int64_t)1 << 32),
        "debug option 3 takes 0, 3, 5, 6 and 7");
  check(lanes_lds_bytes(0) == 0 && lanes_lds_bytes(1) == LDS_ONE_WG && lanes_lds_bytes(2) == LDS_LANES,
        "lanes_lds_bytes: 0, 82,944 and 55,296");

  // ---- automatic, idle device
  check(single(base(1), K1_WORDS, 0) && single(base(1024), K1_WORDS, 0), "1 and 1,024 reports: WORDS");
  check(single(base(1025), K1_PAIRS_UNROLLED, LDS_ONE_WG) && single(base(8192), K1_PAIRS_UNROLLED, LDS_ONE_WG),
        "1,025 and 8,192: PAIRS_UNROLLED with LDS 82,944");
  check(single(base(8193), K1_PAIRS_UNROLLED, 0) && single(base(16384), K1_PAIRS_UNROLLED, 0),
        "8,193 and 16,384: PAIRS_UNROLLED with LDS 0");
  check(single(base(16385), K1_PAIRS, 0) && single(base(32768), K1_PAIRS, 0), "16,385 and 32,768: PAIRS with LDS 0");
  check(mixed(base(32769), 32768, K1_PAIRS_UNROLLED), "32,769: LANES over 32,768 (LDS 55,296), PAIRS_UNROLLED over 1");
  check(mixed(base(49152), 32768, K1_PAIRS_UNROLLED), "49,152: tail PAIRS_UNROLLED over 16,384");
  check(mixed(base(49153), 32768, K1_PAIRS) && mixed(base(65536), 32768, K1_PAIRS),
        "49,153 and 65,536: tail PAIRS over 16,385 and 32,768");
  check(single(base(65537), K1_FUSED, 0), "65,537: FUSED");

  // ---- automatic, another engine's big launch in flight
  check(single(base(32769, true), K1_LANES, LDS_LANES) && single(base(65536, true), K1_LANES, LDS_LANES),
        "busy: 32,769 and 65,536 run LANES alone");
  check(single(base(1024, true), K1_WORDS, 0) && single(base(8192, true), K1_PAIRS_UNROLLED, LDS_ONE_WG) &&
            single(base(32768, true), K1_PAIRS, 0) && single(base(65537, true), K1_FUSED, 0),
        "busy: nothing else changes");

  // ---- forced kernels
  check(single(forced(K1_LANES, 40000), K1_LANES, LDS_LANES) &&
            single(k1_plan(40000, RR, K1_LANES, false, false, false, 2, false), K1_LANES, LDS_LANES),
        "forced LANES, 40,000: no split (mixing is automatic only)");
  check(single(forced(K1_PAIRS, 16384), K1_PAIRS_UNROLLED, 0), "forced PAIRS, 16,384: PAIRS_UNROLLED, LDS 0");
  check(single(forced(K1_PAIRS, 16385), K1_PAIRS, 0), "forced PAIRS, 16,385: PAIRS");
  check(single(forced(K1_PAIRS, 8192), K1_PAIRS_UNROLLED, 0),
        "forced PAIRS, 8,192: PAIRS_UNROLLED, LDS 0 (the reservation is automatic only)");
  check(single(forced(K1_WORDS, 40000), K1_WORDS, 0) && single(forced(K1_FUSED, 100), K1_FUSED, 0),
        "forced WORDS and FUSED at any size");
  check(single(forced(K1_WORDS, 100, true), K1_FUSED, 0) && single(forced(K1_PAIRS, 100, true), K1_FUSED, 0) &&
            single(forced(K1_PAIRS, 20000, true), K1_FUSED, 0),
        "wide: forced WORDS or PAIRS run FUSED");
  check(single(forced(K1_LANES, 100, true), K1_LANES, LDS_LANES), "wide: forced LANES runs LANES");
  check(single(k1_plan(100, RR, K1_AUTO, false, true, false, 2, false), K1_FUSED, 0) &&
            single(k1_plan(40000, RR, K1_AUTO, false, true, false, 2, false), K1_FUSED, 0),
        "wide: automatic is FUSED");

  // ---- leader, Count and multiproof
  {
    bool ok = true;
    for (uint64_t n : {1ull, 1024ull, 8192ull, 32769ull, 65536ull, 65537ull})
      for (K1Kernel k : {K1_AUTO, K1_LANES, K1_FUSED, K1_PAIRS, K1_WORDS})
        ok = ok && single(k1_plan(n, RR, k, true, false, false, 2, false), K1_FUSED, 0);
    check(ok, "leader: FUSED, no split");
  }
  {
    bool ok = true;
    for (uint64_t n : {32769ull, 49152ull, 65536ull})
      ok = ok && single(k1_plan(n, RR, K1_AUTO, false, false, true, 2, false), K1_LANES, LDS_LANES);
    check(ok, "Count and multiproof: never split");
  }

  // ---- round_reports and lanes_wg_cap
  {
    bool ok = true;
    for (uint64_t n : {1ull, 1024ull, 8192ull, 32769ull, 65536ull, 1000000ull}) ok = ok && single(base(n, false, 0), K1_FUSED, 0);
    check(ok, "round_reports 0: FUSED for any n");
  }
  {
    const K1Plan p = base(24577, false, 98304), q = base(24576, false, 98304);
    check(p.split == 24576 && p.head.kernel == K1_LANES && p.tail.kernel == K1_PAIRS_UNROLLED &&
              single(q, K1_PAIRS, 0) && k1_split_point(98304) == 24576 && k1_big(24577, 98304) && !k1_big(24576, 98304),
          "round_reports 98,304: split point 24,576");
  }
  check(!k1_big(1u << 30, 0) && k1_big(32769, RR) && !k1_big(32768, RR), "k1_big: past the split point, never without one");
  {
    const K1Plan p0 = base(40000, false, RR, 0), p1 = base(40000, false, RR, 1);
    check(p0.split == 32768 && p0.head.lds == 0 && p1.split == 32768 && p1.head.lds == LDS_ONE_WG &&
              single(base(40000, true, RR, 0), K1_LANES, 0) && single(base(40000, true, RR, 1), K1_LANES, LDS_ONE_WG),
          "lanes_wg_cap 0: lane-split LDS 0; 1: 82,944");
  }

  if (g_failed) {
    printf("%d FAILED\n", g_failed);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
