// jx_flags.h — the per-report flag word that the XOF stage hands to the FLP stage. On its own (no HIP runtime
// needed) so that the sampling code of jx_sample.h, which raises FLAG_SLOW, also builds for the host tests.
#pragma once
#include <stdint.h>

namespace jx {

// per-report flag bits written by the XOF stage, consumed by the FLP stage
enum : uint32_t {
  FLAG_INIT_FAIL = 1u,  // query randomness t is a P-th root of unity -> prepare_init_failure
  FLAG_NEXT_FAIL = 2u,  // leader's joint-rand part disagrees with the public share -> prepare_next_failure
  FLAG_SLOW = 4u,       // a rejected XOF sample shifted a stream: the slow kernel redoes this report
  FLAG_DFAIL = 8u,      // a leader verifier element is >= p -> leader_prep_share_decode_failure
  FLAG_INPUT_FAIL = 16u,  // leader: an explicit input-share element is >= p -> prepare_init_failure
};

}  // namespace jx
