// hosttest_route.cpp — the batch-bucket rule of janus_amd/csrc/jx_wire.h on the CPU (tests/test_wire_route_host.py),
// built with the address and undefined-behaviour sanitizers.
//
//   start FILE    u32 count, then (u64 time, u64 precision) pairs: prints wire_bucket_start of each
//   outcome       wire_outcome_routed and wire_outcome over the full product of their inputs, one line per point
//   route FILE    u32 count, then per case u64 n, precision, ncollected, seed, then times u64[n], route u32[n],
//                 collected u64[ncollected]. The three passes of jx_wire.hip are replayed with one loop iteration per
//                 thread, every thread claiming (the kernel lets one lane of a group of equal starts claim for it),
//                 each pass in an order shuffled by the seed, which also keys the slot hash. Prints the status, the
//                 table and route / bucket_index / bucket_collected of every report.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../../janus_amd/csrc/jx_wire.h"

using namespace jx;

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}

static std::vector<uint64_t> shuffled(uint64_t n, std::mt19937_64& rng) {
  std::vector<uint64_t> o(n);
  std::iota(o.begin(), o.end(), 0);
  std::shuffle(o.begin(), o.end(), rng);
  return o;
}

static int run_start(FILE* f) {
  uint32_t count = 0;
  if (!rd(f, &count, 1)) return 2;
  for (uint32_t k = 0; k < count; k++) {
    uint64_t tp[2];
    if (!rd(f, tp, 2)) return 2;
    printf("%" PRIu64 "\n", wire_bucket_start(tp[0], tp[1]));
  }
  return 0;
}

static int run_outcome() {
  const int host_errs[] = {WIRE_ERR_NONE, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
  for (int he : host_errs)
    for (int open = 0; open < 9; open++)
      for (int early = 0; early < 2; early++)
        for (int wire = 0; wire < 4; wire++)
          for (int verdict = 0; verdict < 7; verdict++)
            for (int rep = 0; rep < 2; rep++)
              for (int col = 0; col < 2; col++)
                printf("%d %d %d %d %d %d %d %d %d\n", he, open, early, wire, verdict, rep, col,
                       wire_outcome_routed((uint8_t)he, (uint8_t)open, early, (uint8_t)wire, (uint8_t)verdict, rep, col),
                       wire_outcome((uint8_t)he, (uint8_t)open, early, (uint8_t)wire, (uint8_t)verdict, rep));
  return 0;
}

static int run_route(FILE* f) {
  uint32_t count = 0;
  if (!rd(f, &count, 1)) return 2;
  for (uint32_t cs = 0; cs < count; cs++) {
    uint64_t hd[4];
    if (!rd(f, hd, 4)) return 2;
    const uint64_t n = hd[0], P = hd[1], nc = hd[2], seed = hd[3];
    // allocations of exactly the arrays' sizes: the sanitizer sees any index past them
    std::vector<uint64_t> times(n), collected(nc);
    std::vector<uint32_t> route(n);
    if (!rd(f, times.data(), n) || !rd(f, route.data(), n) || !rd(f, collected.data(), nc)) return 2;
    std::sort(collected.begin(), collected.end());
    collected.erase(std::unique(collected.begin(), collected.end()), collected.end());
    std::mt19937_64 rng(seed);
    const uint64_t k0 = rng(), k1 = rng(), slots = 2 * n;
    std::vector<uint32_t> tab(slots, 0), list(WIRE_ROUTE_MAX_BUCKETS), rank(n, WIRE_ROUTE_OUT), index(n, WIRE_ROUTE_OUT);
    std::vector<uint8_t> in_collected(n, 0);
    std::vector<WireBucket> buckets(WIRE_ROUTE_MAX_BUCKETS);
    uint32_t claims = 0;
    auto cas = [](uint32_t* slot, uint32_t v) {
      const uint32_t seen = *slot;
      if (seen == 0) *slot = v;
      return seen;
    };
    for (uint64_t i : shuffled(n, rng))  // pass 1: the claims
      if (wire_route_claim(i, times.data(), P, tab.data(), slots, k0, k1, cas)) {
        const uint32_t at = claims++;
        if (at < WIRE_ROUTE_MAX_BUCKETS) list[at] = (uint32_t)i;
      }
    if (claims > WIRE_ROUTE_MAX_BUCKETS) {
      printf("case %u status 1 buckets 0 |", cs);
    } else {
      std::vector<uint64_t> keys(claims);
      for (uint32_t t = 0; t < claims; t++) keys[t] = wire_bucket_start(times[list[t]], P);
      for (uint64_t t : shuffled(claims, rng)) {  // pass 2: the ranks and the empty entries
        const uint32_t r = wire_rank(keys.data(), claims, (uint32_t)t);
        rank[list[t]] = r;
        buckets[r] = WireBucket{keys[t], ~0ull, 0, 0, 0, wire_bucket_collected(collected.data(), collected.size(), keys[t]), 0};
      }
      for (uint64_t i : shuffled(n, rng)) {  // pass 3: every report to its bucket
        const uint64_t t = times[i];
        const uint32_t c = wire_route_holder(wire_bucket_start(t, P), times.data(), P, tab.data(), slots, k0, k1);
        if (c == WIRE_ROUTE_OUT) return 3;
        const uint32_t k = rank[c];
        WireBucket& e = buckets[k];
        route[i] = wire_route_of(route[i], e.collected != 0, k);
        index[i] = k;
        in_collected[i] = e.collected != 0;
        e.min_time = std::min(e.min_time, t);
        e.max_time = std::max(e.max_time, t);
        e.reports++;
        e.routed += route[i] != WIRE_ROUTE_OUT;
      }
      printf("case %u status 0 buckets %u |", cs, claims);
      for (uint32_t k = 0; k < claims; k++)
        printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u", buckets[k].start, buckets[k].min_time, buckets[k].max_time,
               buckets[k].reports, buckets[k].routed, buckets[k].collected);
    }
    printf(" |");
    for (uint64_t i = 0; i < n; i++) printf(" %u %u %u", route[i], index[i], (unsigned)in_collected[i]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "outcome")) return run_outcome();
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  const int rc = !strcmp(argv[1], "start") ? run_start(f) : !strcmp(argv[1], "route") ? run_route(f) : 2;
  fclose(f);
  return rc;
}
