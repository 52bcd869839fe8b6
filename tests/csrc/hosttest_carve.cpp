// Host checks of the slab carver (janus_amd/csrc/jx_carve.h): a stand-alone program for a build with
// -fsanitize=address,undefined (tests/test_carve_host.py). One line per check, then "all ok"; exit status 0.
// Slab sizes feed the arena's size-keyed reuse and batch_new's recycle match, so the rule is pinned here: a sizing
// pass and a carving pass of one layout agree, and the offsets are those the engine's hand-written chains gave.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../janus_amd/csrc/jx_carve.h"

using namespace jxi;

static int g_failed = 0;
static void check(bool ok, const char* what) {
  printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) g_failed++;
}

// One layout of differently typed regions, as the engine writes its own: a function of the base.
struct Regions {
  uint8_t* a = nullptr;
  uint32_t* b = nullptr;
  uint64_t* c = nullptr;
  uint8_t* empty = nullptr;
  uint16_t* d = nullptr;
};
static const size_t kSizes[5] = {1, 4 * 77, 8 * 1000, 0, 2 * 128};  // odd, below and above 256, empty, exactly 256
// prefix (optional): the layout marks the first three regions as a handle's host-visible prefix (Carver::mark)
static size_t lay(Regions& r, void* base, size_t* prefix = nullptr) {
  Carver cv(base);
  cv.take(r.a, kSizes[0]);
  cv.take(r.b, kSizes[1]);
  cv.take(r.c, kSizes[2]);
  if (prefix) *prefix = cv.mark() == cv.bytes() ? cv.marked() : 0;  // the running total where it is taken
  cv.take(r.empty, kSizes[3]);
  cv.take(r.d, kSizes[4]);
  return cv.bytes();
}

int main() {
  check(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256 rounds up");

  // ---- a null base only sizes: no pointer is touched, and the total is the carved pass's
  Regions sized;
  uint8_t mark = 0;
  sized.a = &mark;
  const size_t total = lay(sized, nullptr);
  check(sized.a == &mark && !sized.b && !sized.c && !sized.empty && !sized.d, "a null base sets no pointer");
  std::vector<uint8_t> slab(total + 256);
  uint8_t* const base = slab.data() + (256 - reinterpret_cast<uintptr_t>(slab.data()) % 256) % 256;
  Regions r;
  check(lay(r, base) == total, "the sizing pass and the carving pass give one total");
  check(total == 256 + 512 + 8192 + 256 + 256, "each region takes its bytes rounded up to 256");

  // ---- every region starts 256-aligned from the base, holds its bytes and overlaps no other
  {
    const uint8_t* p[5] = {r.a, (const uint8_t*)r.b, (const uint8_t*)r.c, r.empty, (const uint8_t*)r.d};
    bool aligned = true, apart = true, inside = true;
    for (int i = 0; i < 5; i++) {
      aligned = aligned && p[i] >= base && (p[i] - base) % 256 == 0;
      inside = inside && p[i] + (kSizes[i] ? kSizes[i] : 1) <= base + total;
      for (int j = 0; j < i; j++) {
        const uint8_t *lo = p[i] < p[j] ? p[i] : p[j], *hi = p[i] < p[j] ? p[j] : p[i];
        const size_t lo_bytes = p[i] < p[j] ? kSizes[i] : kSizes[j];
        apart = apart && lo != hi && lo + lo_bytes <= hi;
      }
    }
    check(aligned, "every region starts 256-aligned from the base");
    check(inside, "every region lies inside the sized total");
    check(apart, "no two regions overlap or share a pointer");
    check(r.a == base, "the first region is the base");
    // written end to end under the sanitizers: the regions are really there
    for (size_t i = 0; i < kSizes[0]; i++) r.a[i] = 1;
    for (size_t i = 0; i < kSizes[1] / 4; i++) r.b[i] = 2;
    for (size_t i = 0; i < kSizes[2] / 8; i++) r.c[i] = 3;
    for (size_t i = 0; i < kSizes[4] / 2; i++) r.d[i] = 4;
    check(r.a[0] == 1 && r.b[76] == 2 && r.c[999] == 3 && r.d[127] == 4, "the regions hold their elements");
  }

  // ---- an empty region still takes 256 bytes and gets a pointer of its own
  check(r.empty == (const uint8_t*)r.c + 8192 && (const uint8_t*)r.d == r.empty + 256,
        "a zero-byte region takes 256 bytes and has its own pointer");
  {
    uint8_t *x = nullptr, *y = nullptr;
    Carver cv(base);
    cv.take(x, 0);
    cv.take(y, 0);
    check(cv.bytes() == 512 && x == base && y == base + 256, "two empty regions are two pointers, 256 apart");
  }

  // ---- batch_new's regions for 64 reports, out_len 3, a 32-byte seed: output shares, verdicts, prep messages,
  // report ids. The offsets are those of its former chain o_ver = align256(cap * out_len * 16), o_msg = o_ver +
  // align256(cap), o_non = o_msg + align256(cap * seed), bytes = o_non + align256(cap * 16).
  {
    const uint64_t cap = 64, out_len = 3, seed = 32;
    uint8_t *outs = nullptr, *ver = nullptr, *msg = nullptr, *non = nullptr;
    auto batch = [&](void* b) {
      Carver cv(b);
      cv.take(outs, cap * out_len * 16);
      cv.take(ver, cap);
      cv.take(msg, cap * seed);
      cv.take(non, cap * 16);
      return cv.bytes();
    };
    const size_t sized_total = batch(nullptr);
    std::vector<uint8_t> mem(6400);
    const size_t carved_total = batch(mem.data());
    check(cap * out_len * 16 == 3072 && cap == 64 && cap * seed == 2048 && cap * 16 == 1024, "the sizes are 3072 / 64 / 2048 / 1024");
    check(outs - mem.data() == 0 && ver - mem.data() == 3072 && msg - mem.data() == 3328 && non - mem.data() == 5376,
          "a batch of 64 reports: offsets 0 / 3072 / 3328 / 5376");
    check(sized_total == 6400 && carved_total == 6400, "a batch of 64 reports: 6400 bytes, sized or carved");
  }

  // ---- a handle's layout: the regions up to the mark are the prefix its pinned host copy holds, and a pointer into
  // the device slab is the same offset of the copy (same_offset)
  {
    Regions h;
    size_t sized_prefix = 0, prefix = 0;
    const size_t sized_total = lay(h, nullptr, &sized_prefix), carved_total = lay(h, base, &prefix);
    check(sized_prefix == 256 + 512 + 8192 && prefix == sized_prefix,
          "the mark is the running total where it is taken, sized or carved");
    check(sized_total == total && carved_total == total, "a layout with a mark has the total of the layout without");
    const std::vector<uint8_t> copy(base, base + prefix);
    const uint8_t* first = same_offset(h.a, base, copy.data());
    const uint64_t* last = same_offset(h.c, base, copy.data());
    check(first == copy.data() && (const uint8_t*)last == copy.data() + 768 && first[0] == 1 && last[999] == 3 &&
              (const uint8_t*)(last + 1000) <= copy.data() + prefix,
          "the prefix's first and last region lie at the same offsets of its copy");
  }

  if (g_failed) {
    printf("%d FAILED\n", g_failed);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
