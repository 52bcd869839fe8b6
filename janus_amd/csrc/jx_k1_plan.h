// jx_k1_plan.h — which helper K1 kernel a prepare launch runs (jx_engine.cpp prep_core asks, jx_kernels.hip
// launch_xof obeys; jx_engine_debug option 3 and tools/kernel_probe.hip name the kernels by this enum).
//
// Host only and without HIP, so tests/csrc/hosttest_k1_plan.cpp pins the thresholds on the CPU: a slip here costs
// speed, never results, so no GPU parity test would see it.
#pragma once
#include <stdint.h>

namespace jx {

// The values are what jx_engine_debug option 3 takes (0, 3, 5, 6, 7; include/jx_prio3.h).
enum K1Kernel : uint32_t {
  K1_AUTO = 0,            // k1_plan chooses
  K1_LANES = 3,           // lane-split, 32 reports per wave (xof_lanes_kernel)
  K1_FUSED = 5,           // two sponges per lane, 64 reports per wave (xof_kernel)
  K1_PAIRS = 6,           // lane pairs, 16 reports per wave (xof_pairs_kernel<false>; bits <= 32)
  K1_WORDS = 7,           // a word per lane, one report per wave (xof_words_kernel + trunc_kernel; bits <= 32)
  K1_PAIRS_UNROLLED = 8,  // lane pairs with unrolled rounds (xof_pairs_kernel<true>); never forced
};
inline bool k1_forceable(int64_t v) {
  return v == K1_AUTO || v == K1_LANES || v == K1_FUSED || v == K1_PAIRS || v == K1_WORDS;
}

struct K1Launch {
  K1Kernel kernel;
  uint32_t lds;  // dynamic LDS bytes: not used by the kernel, it caps the workgroups per CU
};
struct K1Plan {
  K1Launch head;   // reports [0, split), or all of them when split == 0
  uint64_t split;  // 0: one launch
  K1Launch tail;   // reports [split, n), beside the head on a second stream
};

// Dynamic LDS that caps the lane-split kernel at `wgs_per_cu` workgroups per CU (0: no cap).
inline uint32_t lanes_lds_bytes(uint32_t wgs_per_cu) {
  if (wgs_per_cu == 0) return 0;
  constexpr uint32_t LDS_PER_CU = 160u << 10;
  return (LDS_PER_CU / (wgs_per_cu + 1) + 1024u) / 1024u * 1024u;
}

// A launch past this many reports is a "big" one: the lane-split kernel's one wave per SIMD (0: none is).
inline uint64_t k1_split_point(uint64_t round_reports) { return round_reports / 4 / 64 * 64; }
inline bool k1_big(uint64_t n, uint64_t round_reports) {
  const uint64_t s = k1_split_point(round_reports);
  return s && n > s;
}

// The K1 launch(es) of n reports. round_reports: the reports that fill every wave slot of the fused kernel once
// (k1_round_reports; 131,072 on MI355X; 0: unknown). forced: debug option 3. wide: Sum / SumVec with bits > 32.
// no_split: Count or the multiproof instance, whose K1s are kernels of their own. lanes_wg_cap: debug option 6.
// other_big_busy: another engine of the device has a big K1 launch in flight; it only ever turns a split plan into
// an unsplit one, so prep_core asks the arena (event queries) only when the plan with `false` splits.
inline K1Plan k1_plan(uint64_t n, uint64_t round_reports, K1Kernel forced, bool leader, bool wide, bool no_split,
                      uint32_t lanes_wg_cap, bool other_big_busy) {
  const K1Launch fused{K1_FUSED, 0};
  if (leader) return {fused, 0, fused};  // launch_xof runs the leader kernels whatever the plan says
  K1Kernel k = forced;
  // A helper launch that would give the fused two-sponge K1 less than one wave per SIMD is bound by
  // the per-report sponge latency, not by issue: the lane-split kernel runs it in twice the waves
  // (FixedPointBoundedL2VecSum 16 x 10000, 24,576 reports: 153 -> 92 ms on MI355X), below one
  // lane-split wave per SIMD the lane-pair kernel splits every sponge over two lanes, and up to one
  // report-wave per SIMD the word-per-lane kernel spreads it over 25 (round_reports: the fused kernel's
  // two waves per SIMD, 4 x that many lane-split or 8 x lane-pair lanes; profiles/r05_words_sweep.jsonl).
  if (forced == K1_AUTO && !wide && round_reports) {
    if (128 * n <= round_reports)  // a report per wave, <= one wave per SIMD (1,024 on MI355X): 2.6 vs 3.6 ms
      k = K1_WORDS;
    else if (4 * n <= round_reports)
      k = K1_PAIRS;
    else if (2 * n <= round_reports)
      k = K1_LANES;
  }
  // the lane pairs with unrolled rounds while each pair-wave has a SIMD to itself (<= 16,384 reports on MI355X)
  if (k == K1_PAIRS && 8 * n <= round_reports) k = K1_PAIRS_UNROLLED;
  // the word and pair kernels are 32-bit only
  if (k == K1_AUTO || (wide && k != K1_LANES)) k = K1_FUSED;
  uint32_t lds = 0;
  if (k == K1_LANES) lds = lanes_lds_bytes(lanes_wg_cap);
  // A lane-pair launch of at most half the CUs' workgroups (<= 8,192 reports on MI355X: the coalescer's launches
  // of Janus-sized jobs, two in flight) reserves LDS for one workgroup per CU, so a second such launch lands on
  // other CUs instead of doubling up SIMDs with the first (profiles/r06_jobs_*: K1 3.6 ms alone, 4.5 ms beside
  // another launch on shared CUs).
  if ((k == K1_PAIRS || k == K1_PAIRS_UNROLLED) && forced == K1_AUTO && 16 * n <= round_reports)
    lds = lanes_lds_bytes(1);
  const K1Launch head{k, lds};
  // A lane-split launch past one wave per SIMD puts two of its long chains on some SIMDs and the launch waits
  // for those. Instead the first round_reports / 4 reports (a lane-split wave per SIMD) run lane-split and the
  // rest as lane pairs beside them on the side stream: FixedPointBoundedL2VecSum 16 x 10000, 40,960 reports,
  // 148.4 -> 123.5 ms (tools/kernel_probe fpmix, profiles/r05_fp_mixed_k1.jsonl). Only while no other engine
  // on the device has a large K1 launch in flight: beside the leader's 640 K1 waves (configs[4] with two jobs in
  // flight) the 1,536 mixed waves pack worse than 1,280 lane-split ones (helper K1 154 -> 161 ms, every split
  // point tried; profiles/r05_fp_mixed_k1.jsonl).
  const uint64_t split_at = k1_split_point(round_reports);
  if (forced == K1_AUTO && k == K1_LANES && !wide && k1_big(n, round_reports) && !no_split && !other_big_busy)
    return {head, split_at, {8 * (n - split_at) <= round_reports ? K1_PAIRS_UNROLLED : K1_PAIRS, 0}};
  return {head, 0, fused};
}

}  // namespace jx
