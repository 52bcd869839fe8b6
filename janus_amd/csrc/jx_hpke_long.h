// jx_hpke_long.h — what jx_hpke_long.hip (the wave-per-report open of long payloads) shares with the unit that
// holds the C ABI (jx_hpke.hip).
#pragma once
#include "jx_hpke_open.h"
#include "jx_keyreg.h"

namespace jx {

// What stage A leaves for stage B, one row per report: the AEAD's key and base nonce as little-endian words (Nk
// bytes of key, the rest zero), its id, and whether the KEM gave a usable secret (DH output non-zero / the
// encapsulated key a point of the curve).
struct LongCtxRow {
  uint32_t kw[8];
  uint32_t nw[3];
  uint32_t aead;
  uint32_t ok;
  uint32_t pad[3];
};
static_assert(sizeof(LongCtxRow) == 64, "LongCtxRow layout");

struct LongCtxArgs {
  uint64_t n;
  const HpkeKeyRow* keys;  // the device's key registry
  uint32_t slot;           // the recipient key's row
  const uint8_t* encs;     // n x 32 (X25519) or n x 65 (P-256)
  LongCtxRow* out;
  uint32_t zero_ist[8], zero_ost[8];  // HMAC-SHA256 pads of the empty salt
};

// Both stages on `s`: the context kernel of the key's KEM, then the open. b.n == ca.n.
hipError_t launch_hpke_long_open(const LongCtxArgs& ca, bool p256, const HpkeBufs& b, hipStream_t s);

}  // namespace jx
