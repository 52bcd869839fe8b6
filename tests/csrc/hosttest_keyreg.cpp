// Host checks of the HPKE key registry's slot bookkeeping (janus_amd/csrc/jx_keyreg.h) and of the X25519 ladder
// whose swaps are masked selects (janus_amd/csrc/jx_hpke.h): a stand-alone program for a build with
// -fsanitize=address,undefined (tests/test_keyreg_host.py). One line per check, then "all ok"; exit status 0.
// The ladder's expectations: RFC 7748 §5.2, and 200 random (scalar, u) pairs recorded from oracle/hpke_oracle.py's
// x25519 (hosttest_keyreg_vectors.h).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../janus_amd/csrc/jx_hpke.h"
#include "../../janus_amd/csrc/jx_keyreg.h"
#include "hosttest_keyreg_vectors.h"

using namespace jx;

static int g_failed = 0;
static void check(bool ok, const char* what) {
  printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) g_failed++;
}

static void unhex(const char* s, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) {
    unsigned v = 0;
    sscanf(s + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}

// X25519 as the engine computes it: jx_hpke_create_key's clamp, then the ladder on little-endian words
static void x25519(const uint8_t k[32], const uint8_t u[32], uint8_t out[32]) {
  uint8_t c[32];
  memcpy(c, k, 32);
  c[0] &= 248;
  c[31] &= 127;
  c[31] |= 64;
  uint32_t kw[8], uw[8], ow[8];
  for (int i = 0; i < 8; i++) {
    memcpy(&kw[i], c + 4 * i, 4);
    memcpy(&uw[i], u + 4 * i, 4);
  }
  x25519_ladder(ow, kw, uw);
  memcpy(out, ow, 32);
}

static bool x25519_is(const char* k_hex, const char* u_hex, const char* want_hex) {
  uint8_t k[32], u[32], want[32], got[32];
  unhex(k_hex, k, 32);
  unhex(u_hex, u, 32);
  unhex(want_hex, want, 32);
  x25519(k, u, got);
  return memcmp(got, want, 32) == 0;
}

int main() {
  // ---- the registry's slots
  {
    KeySlots s;
    bool distinct = s.capacity() == 16384 && KEY_SLOTS == 16384;
    std::vector<uint8_t> seen(KEY_SLOTS, 0);
    for (uint32_t i = 0; i < KEY_SLOTS; i++) {
      const int32_t v = s.take();
      if (v < 0 || v >= (int32_t)KEY_SLOTS || seen[v]) distinct = false;
      if (v >= 0 && v < (int32_t)KEY_SLOTS) seen[v] = 1;
    }
    check(distinct && s.live() == KEY_SLOTS, "16,384 slots taken, all distinct and below the capacity");
    check(s.take() == -1 && s.take() == -1 && s.live() == KEY_SLOTS, "the 16,385th is refused");
    const uint32_t gone[5] = {0, 255, 256, 9000, 16383};
    for (uint32_t g : gone) s.free(g);
    check(s.live() == KEY_SLOTS - 5, "five slots freed");
    std::set<int32_t> back;
    for (int i = 0; i < 5; i++) back.insert(s.take());
    check(back == std::set<int32_t>({0, 255, 256, 9000, 16383}) && s.take() == -1, "freed slots are reused, and no others");
    // a context freed and created over and over keeps to one slot
    KeySlots t(4);
    const int32_t a = t.take(), b = t.take();
    bool same = a == 0 && b == 1;
    for (int i = 0; i < 100; i++) {
      t.free((uint32_t)b);
      same = same && t.take() == b;
    }
    check(same && t.live() == 2 && t.take() == 2 && t.take() == 3 && t.take() == -1, "a slot freed and taken again; small capacity");
  }
  // ---- slots in an EncRow
  {
    EncRow w;
    memset(&w, 0, sizeof w);
    w.key0 = 256;
    w.key1 = (uint16_t)(KEY_SLOTS - 1);
    bool ok = w.key0 == 256 && w.key1 == 16383 && w.flags == 0 && w.ct_len == 0 && w.enc65_off == 0;
    w.key0 = 0x1234;
    w.key1 = KEY_SLOT_NONE;
    ok = ok && w.key0 == 0x1234 && w.key1 == 0xFFFF && (uint32_t)w.key1 >= KEY_SLOTS;  // the kernels' break
    w.key0 = KEY_SLOT_NONE;
    w.flags = ENC_ROW_ENCRYPTED | ENC_ROW_ENC65;
    w.ct_len = 0xFFFFFFFFu;
    ok = ok && w.key0 == KEY_SLOT_NONE && w.key1 == KEY_SLOT_NONE && w.flags == 9 && w.enc65_off == 0;
    check(ok && sizeof(EncRow) % 8 == 0, "slots above 255 and the 0xFFFF sentinel survive EncRow::key0 / key1");
  }
  // ---- the ladder
  check(x25519_is("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
                  "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
                  "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
        "RFC 7748 5.2 vector 1");
  check(x25519_is("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
                  "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
                  "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
        "RFC 7748 5.2 vector 2 (u with bit 255 set)");
  {
    uint8_t k[32] = {9}, u[32] = {9}, r[32], w1[32], w1000[32];
    unhex("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079", w1, 32);
    unhex("684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51", w1000, 32);
    bool ok1 = false;
    for (int i = 0; i < 1000; i++) {
      x25519(k, u, r);
      memcpy(u, k, 32);
      memcpy(k, r, 32);
      if (i == 0) ok1 = memcmp(k, w1, 32) == 0;
    }
    check(ok1, "RFC 7748 5.2 iterated, 1 iteration");
    check(memcmp(k, w1000, 32) == 0, "RFC 7748 5.2 iterated, 1,000 iterations");
  }
  {
    // low-order points: u = 0 and u = 1 give the all-zero output (hpke_decap fails the open on it)
    uint8_t k[32], u[32] = {0}, r[32], zero[32] = {0};
    for (int i = 0; i < 32; i++) k[i] = (uint8_t)(37 * i + 5);
    x25519(k, u, r);
    bool ok = memcmp(r, zero, 32) == 0;
    u[0] = 1;
    x25519(k, u, r);
    check(ok && memcmp(r, zero, 32) == 0, "the all-zero output (u = 0, u = 1)");
  }
  {
    int bad = 0;
    for (int i = 0; i < X25519_NVEC; i++)
      if (!x25519_is(X25519_VEC[i][0], X25519_VEC[i][1], X25519_VEC[i][2])) bad++;
    check(X25519_NVEC == 200 && bad == 0, "200 random (scalar, u) pairs against oracle/hpke_oracle.py's x25519");
  }
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
