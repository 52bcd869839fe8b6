// jx_shard.h — arguments and launcher of the client-side kernels (Prio3.shard, jx_shard.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jx_kernels.h"

namespace jx {

// Largest transform size (gadget-call points P = next_pow2(1 + calls)) the prove kernel holds: one wave's wire
// pair and its two accumulators, 4 x P x 16 B, are 64 KiB of LDS at 1024. The same value as JX_SHARD_MAX_P
// (include/jx_prio3.h).
constexpr uint32_t SHARD_MAX_P = 1024;
constexpr uint32_t SHARD_WG_LDS = 65536;  // LDS of one prove workgroup at most: two fit a CU

struct ShardArgs {
  uint64_t n;
  uint32_t algo, bits, length, chunk, meas_len, calls, P, logP, arity, gpoly_len, proof_len, dst_id;
  uint32_t ps_bytes, his_bytes, lis_bytes, rand_bytes, jr;  // jr: the instance has joint randomness
  uint32_t mstride;                                        // uint64 words per measurement
  uint64_t lis_stride;
  const uint64_t* meas;
  const uint8_t* nonces;
  const uint8_t* rands;
  uint8_t* ps;
  uint8_t* lis;
  uint8_t* his;
  // per-launch scratch
  uint8_t* status;  // [n] 0 or JX_SHARD_INVALID_MEASUREMENT
  uint4* hmeas;     // [n][meas_len] the helper's measurement share
  uint4* prand;     // [n][arity] prove randomness
  uint4* cpow;      // [n][P]: r^(chunk k), canonical, k < calls
  uint4* rjr;       // [n] joint_rand[0] in Montgomery form
  const uint4* tab;  // ntt_build_table(logP)
  uint32_t waves;    // waves of one prove workgroup
};

uint64_t shard_scratch_bytes(const ShardArgs& a);  // per report
uint32_t shard_waves(uint32_t algo, uint32_t P, uint32_t chunk);
hipError_t launch_shard(const ShardArgs& a, hipStream_t s);

}  // namespace jx
