// jx_fused_plan.h — how a fused prepare + aggregate call of n reports is cut into launches and how many pipelines
// run them (jx_engine_fused.cpp run_fused obeys; jx_engine_debug options 4 and 5 set npipes and default_chunk).
//
// Host only and without HIP, so tests/csrc/hosttest_fused_plan.cpp pins the values on the CPU: a slip here costs
// speed (or, at n == 0, a division by zero), never results, so no GPU parity test would see it.
#pragma once
#include <stdint.h>

namespace jx {

// Pipelines a fused call can run, and the upper bound of debug option 4.
constexpr uint32_t MAX_PIPES = 4;

struct FusedPlan {
  uint64_t chunk;     // reports per launch (the last one takes the rest); the staging is sized for it
  uint64_t launches;  // 0 when n == 0
  uint32_t pipes;     // 1: the engine stream alone
};

// default_chunk (> 0): the reports per launch that fit the staging budget. round_reports: the reports that fill
// every K1 wave slot once (0: unknown). npipes: debug option 4 (0: automatic). pipelines: the algorithm pipelines
// at all (not Count, not the multiproof instance). many: the call's reports go to several aggregations by a
// per-report index. host: the host-buffer form.
inline FusedPlan fused_plan(uint64_t n, uint64_t default_chunk, uint64_t round_reports, uint32_t npipes,
                            bool pipelines, bool many, bool host) {
  if (n == 0) return {0, 0, 1};
  // Reports per launch for an n-report fused call: the fewest launches that fit the staging
  // budget (default_chunk), split evenly (multiple of 64) so every launch has the same shape.
  // When the chunk is a whole number of K1 rounds (round_reports), launches are full chunks and
  // only the last one carries a partial round (1.25M SumVec reports: 4 x 262,144 + 201,424
  // instead of 4 x 312,500). Measured on MI355X: K1 time per report is unchanged (its waves do
  // not finish in lockstep rounds), the step went 188.4 -> 184.6 ms, within run-to-run noise.
  uint64_t chunk;
  if (n <= default_chunk) {
    chunk = n;
  } else if (round_reports && default_chunk % round_reports == 0) {
    chunk = default_chunk;
  } else {
    const uint64_t fewest = (n + default_chunk - 1) / default_chunk;
    const uint64_t per = (n + fewest - 1) / fewest;
    chunk = (per + 63) / 64 * 64;
  }
  const uint64_t launches = (n + chunk - 1) / chunk;
  // A helper launch of the fused path runs K1 (two sponges per lane, two waves per SIMD, VALU), then K3
  // (LDS-DMA ring: HBM + limb products) and K4 (HBM): one after the other, every launch's waves are in the
  // same phase at the same time (the K1 waves of a round reach their FLP-coefficient tails together, K3 runs
  // at a throttled clock beside an idle Keccak pipe). With P pipelines the launches of one call alternate
  // over P child engines, each with its own stream and per-call staging from the arena, so different
  // launches' phases overlap; only the K4s are ordered (they add into the same aggregation). Measured on
  // MI355X with P independent engines (tools/multi_engine_probe.py): SumVec 8x1000/88, 1.25M reports,
  // 7.28M (one) -> 7.67M (two) -> 7.79M reports/s (three). Used when a call spans >= 2 launches of one
  // segment; not for Count (one tiny kernel) or the multiproof path.
  // host: the host-buffer path, whose pageable copies also take turns (3 by default there: SumVec 1.25M
  // reports 5.02M -> 6.44M (two) -> 7.12M (three) reports/s including the copies, tools/bench_host_path.py).
  if (many || !pipelines) return {chunk, launches, 1};
  const uint64_t want = npipes ? npipes : (host ? 3 : 2);
  return {chunk, launches, (uint32_t)(launches < want ? launches : want)};
}

}  // namespace jx
