// Host checks of the fused call's launch plan (janus_amd/csrc/jx_fused_plan.h): a stand-alone program for a build
// with -fsanitize=address,undefined (tests/test_fused_plan_host.py). One line per check, then "all ok"; exit status 0.
// The expectations are those of the engine's launch_chunk and pipes_for before the plan had a header of its own;
// n == 0 is new (those two divided by zero there). They pin the launch shapes and the pipeline counts, which no
// parity test sees (a slip there only costs speed).
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../janus_amd/csrc/jx_fused_plan.h"

using namespace jx;

static int g_failed = 0;
static void check(bool ok, const char* what) {
  printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) g_failed++;
}

constexpr uint64_t RR = 131072;  // the MI355X's round_reports for the small VDAFs

// the device form of an algorithm that pipelines, one aggregation, automatic pipeline count
static FusedPlan dev(uint64_t n, uint64_t dc, uint64_t rr, uint32_t npipes = 0) {
  return fused_plan(n, dc, rr, npipes, true, false, false);
}
static FusedPlan host(uint64_t n, uint64_t dc, uint64_t rr, uint32_t npipes = 0) {
  return fused_plan(n, dc, rr, npipes, true, false, true);
}
static bool is(const FusedPlan& p, uint64_t chunk, uint64_t launches, uint32_t pipes) {
  return p.chunk == chunk && p.launches == launches && p.pipes == pipes;
}
// the reports of the last launch
static uint64_t last(uint64_t n, const FusedPlan& p) { return n - (p.launches - 1) * p.chunk; }

int main() {
  check(MAX_PIPES == 4, "debug option 4 takes 0 to 4");

  // ---- n == 0: nothing to launch, nothing divided
  {
    bool ok = true;
    for (uint64_t dc : {64ull, 1024ull, 262144ull})
      for (uint64_t rr : {(uint64_t)0, (uint64_t)64, RR})
        for (uint32_t np = 0; np <= MAX_PIPES; np++)
          for (int f = 0; f < 8; f++) ok = ok && is(fused_plan(0, dc, rr, np, f & 1, f & 2, f & 4), 0, 0, 1);
    check(ok, "0 reports: chunk 0, no launch, one pipeline, whatever the rest");
  }

  // ---- one launch
  check(is(dev(1000, 1024, 0), 1000, 1, 1) && is(host(1000, 1024, RR), 1000, 1, 1) && is(dev(1, 64, RR), 1, 1, 1),
        "n <= default_chunk: one launch of n, one pipeline");
  check(is(dev(1024, 1024, 0), 1024, 1, 1) && is(dev(1024, 1024, 256), 1024, 1, 1) &&
            is(host(262144, 262144, 65536, 4), 262144, 1, 1),
        "n == default_chunk: one launch, also with 4 pipelines asked for");

  // ---- default_chunk a whole number of K1 rounds: full chunks and a ragged last launch
  {
    const FusedPlan p = dev(1250000, 262144, 65536);
    check(is(p, 262144, 5, 2) && last(1250000, p) == 201424, "1,250,000 at 262,144 / 65,536: 4 x 262,144 + 201,424");
  }
  check(is(dev(1025, 1024, 256), 1024, 2, 2) && last(1025, dev(1025, 1024, 256)) == 1,
        "one over the chunk, whole rounds: 1,024 + 1");
  check(is(dev(2048, 1024, 1024), 1024, 2, 2) && is(dev(524288, 262144, RR), 262144, 2, 2),
        "twice the chunk, whole rounds: two full launches");

  // ---- otherwise an even split, rounded up to 64
  {
    const FusedPlan p = dev(4429, 1024, 0);
    check(is(p, 896, 5, 2) && last(4429, p) == 845 && is(dev(4429, 1024, RR), 896, 5, 2),
          "4,429 at 1,024, round_reports 0 or 131,072: 4 x 896 + 845");
  }
  {
    const FusedPlan p = dev(1250000, 196608, RR);
    check(is(p, 178624, 7, 2) && last(1250000, p) == 178256, "1,250,000 at 196,608 / 131,072: 6 x 178,624 + 178,256");
  }
  check(is(dev(1025, 1024, 0), 576, 2, 2) && last(1025, dev(1025, 1024, 0)) == 449 &&
            is(dev(1025, 1024, RR), 576, 2, 2),
        "one over the chunk, split evenly: 576 + 449");
  check(is(dev(2048, 1024, 0), 1024, 2, 2) && is(dev(3072, 1024, RR), 1024, 3, 2),
        "a multiple of the chunk splits into full chunks");
  {
    const FusedPlan p = dev(193, 64, RR), q = dev(130, 64, 0);
    check(is(p, 64, 4, 2) && last(193, p) == 1 && is(q, 64, 3, 2) && last(130, q) == 2,
          "193 and 130 at 64: 3 x 64 + 1 and 2 x 64 + 2");
  }
  check(is(dev(4 * 1024 + 333, 1024, RR), 896, 5, 2) && is(host(3 * 1024 + 77, 1024, RR), 832, 4, 3),
        "4,429 and 3,149 at 1,024: 5 launches of 896, 4 of 832");

  // ---- pipelines, automatic: 2 for the device form, 3 for the host form, at most one per launch
  check(dev(1250000, 262144, 65536).pipes == 2 && host(1250000, 262144, 65536).pipes == 3,
        "5 launches: device 2, host 3");
  check(dev(3072, 1024, 0).pipes == 2 && host(3072, 1024, 0).pipes == 3, "3 launches: device 2, host 3");
  check(dev(2048, 1024, 0).pipes == 2 && host(2048, 1024, 0).pipes == 2, "2 launches: device 2, host 2");
  check(dev(1024, 1024, 0).pipes == 1 && host(1024, 1024, 0).pipes == 1, "1 launch: 1");

  // ---- pipelines, debug option 4
  {
    bool ok = true;
    for (uint32_t np = 1; np <= MAX_PIPES; np++)
      ok = ok && is(dev(4429, 1024, 0, np), 896, 5, np) && is(host(4429, 1024, 0, np), 896, 5, np);
    check(ok, "5 launches, npipes 1 to 4: as asked, both forms");
  }
  check(dev(3072, 1024, 0, 4).pipes == 3 && host(2048, 1024, 0, 3).pipes == 2 && dev(1000, 1024, 0, 2).pipes == 1,
        "npipes above the launches: one pipeline per launch");

  // ---- one pipeline for several aggregations, Count and the multiproof instance
  {
    bool ok = true;
    for (uint32_t np = 0; np <= MAX_PIPES; np++)
      for (bool h : {false, true})
        ok = ok && is(fused_plan(4429, 1024, 0, np, true, true, h), 896, 5, 1) &&
             is(fused_plan(4429, 1024, 0, np, false, false, h), 896, 5, 1) &&
             is(fused_plan(1250000, 262144, 65536, np, false, true, h), 262144, 5, 1);
    check(ok, "many, or an algorithm that does not pipeline: 1, the launches unchanged");
  }

  if (g_failed) {
    printf("%d FAILED\n", g_failed);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
