// jx_collect.h — collection (the protocol's last stage): what jx_collect.hip shares with the unit that holds the C ABI
// (jx_engine_collect.cpp), and the per-element and per-job pieces of the kernels. The pieces are __host__ __device__:
// tests/csrc/collect_hosttest.cpp runs the same code on the CPU.
//
// Seal (helper and leader): a collection job names some of the call's shard records (encoded aggregate share ||
// count u64 LE || checksum 32 B, jx_shard_record_bytes: the state of one batch_aggregations row). The job's share is
// the element-wise sum mod p of its records' shares, its count their sum, its checksum their XOR
// (compute_aggregate_share, aggregator/src/aggregator/aggregate_share.rs:55-110); the share is then sealed to the
// collector by the long seal (jx_hpke_seal.hip). Open (collector): both sealed shares are opened by the long open
// (jx_hpke_long.hip) and added mod p (Prio3.unshard, collector/src/lib.rs:573-629).
#pragma once
#include "jx_field.h"

namespace jx {

// JX_COLLECT_* of include/jx_prio3.h
constexpr uint32_t COLLECT_OK = 0, COLLECT_INVALID_BATCH_SIZE = 1, COLLECT_BATCH_MISMATCH = 2, COLLECT_BAD_RECORD = 3,
                   COLLECT_SEAL_FAILED = 4;
// JX_COLLECT_OPEN_*
constexpr uint32_t COLLECT_OPEN_OK = 0, COLLECT_OPEN_LEADER = 1, COLLECT_OPEN_HELPER = 2, COLLECT_DECODE_LEADER = 3,
                   COLLECT_DECODE_HELPER = 4;

constexpr uint32_t COLLECT_TILE = 256;  // elements per workgroup of the element kernels, one per lane

// ---- decode with the canonical check: the 8 (16) little-endian bytes of an element as one (two) 64-bit words.
// False when the encoding is >= p (the datastore's and the collector's decode fail, FieldError::ModulusOverflow).
JX_HD bool collect_decode64(uint64_t w, uint64_t& v) {
  v = w;
  return w < P64;
}
JX_HD bool collect_decode128(uint64_t lo, uint64_t hi, f128& v) {
  v = make128(lo, hi);
  return !ge_p128(v);
}

// ---- the add: canonical in, canonical out
JX_HD uint64_t collect_add64(uint64_t a, uint64_t b) { return add64(a, b); }
JX_HD f128 collect_add128(f128 a, f128 b) { return add128(a, b); }

// task.validate_batch_size (aggregator_core/src/task.rs:365-377): at least min, and at most max when there is one
// (max == 0: none)
JX_HD bool collect_batch_size_ok(uint64_t count, uint64_t min_batch_size, uint64_t max_batch_size) {
  return count >= min_batch_size && (max_batch_size == 0 || count <= max_batch_size);
}

// ---- the status of one collection job, in Janus's order: a record that does not decode fails the datastore read;
// then the batch size (aggregate_share.rs:98-110; a job without records has no aggregate share at all: the same
// error); then the other aggregator's count and checksum (aggregator.rs:2927-2939). expect_checksum null: the
// leader, which has nothing to compare against.
JX_HD uint32_t collect_status(uint64_t nrecords, bool bad_record, uint64_t count, const uint8_t checksum[32],
                              uint64_t expect_count, const uint8_t* expect_checksum, uint64_t min_batch_size,
                              uint64_t max_batch_size) {
  if (bad_record) return COLLECT_BAD_RECORD;
  if (nrecords == 0 || !collect_batch_size_ok(count, min_batch_size, max_batch_size)) return COLLECT_INVALID_BATCH_SIZE;
  if (expect_checksum) {
    uint32_t diff = count != expect_count;
    for (int k = 0; k < 32; k++) diff |= (uint32_t)(checksum[k] ^ expect_checksum[k]);
    if (diff) return COLLECT_BATCH_MISMATCH;
  }
  return COLLECT_OK;
}

// a job that passed every check and whose seal did not come about (X25519(skE, pkR) all zero: a low-order key)
JX_HD uint32_t collect_seal_status(uint32_t status, bool sealed) {
  return status != COLLECT_OK ? status : sealed ? COLLECT_OK : COLLECT_SEAL_FAILED;
}

// ---- the collector's status of one collection (collector/src/lib.rs:573-629: both opens, then both decodes)
JX_HD uint32_t collect_open_status(bool leader_opened, bool helper_opened, bool leader_bad, bool helper_bad) {
  if (!leader_opened) return COLLECT_OPEN_LEADER;
  if (!helper_opened) return COLLECT_OPEN_HELPER;
  if (leader_bad) return COLLECT_DECODE_LEADER;
  if (helper_bad) return COLLECT_DECODE_HELPER;
  return COLLECT_OPEN_OK;
}

// ---- kernel arguments and launchers (jx_collect.hip). Every pointer is device memory and 8-byte aligned; a row of
// OUT x FB bytes is a multiple of 8, and so is the record stride OUT x FB + 40 (not of 16: the loads are 8 bytes).
struct CollectMergeArgs {
  uint32_t njobs, out_len, fb;
  const uint8_t* records;       // nrecords x (out_len * fb + 40)
  const uint64_t* rec_off;      // njobs + 1
  const uint32_t* rec_idx;      // rec_off[njobs]: the jobs' records
  const uint64_t* exp_counts;   // njobs, or null together with exp_checksums
  const uint8_t* exp_checksums;  // njobs x 32
  uint64_t min_batch_size, max_batch_size;
  uint32_t* bad;       // njobs, zeroed: set by a tile that met an element >= p
  uint8_t* pts;        // njobs x out_len * fb: the merged shares
  uint8_t* status0;    // njobs: the status before the seal
  uint64_t* counts;    // njobs
  uint8_t* checksums;  // njobs x 32
};

struct CollectFinishArgs {
  uint32_t njobs;
  uint64_t pt_bytes;  // out_len * fb
  const uint8_t* status0;
  const uint8_t* sealed;  // njobs: the seal's ok
  uint8_t* status;        // njobs: out
  uint8_t* encs;          // njobs x 32
  uint8_t* cts;           // njobs x (pt_bytes + 16)
  uint8_t* pts;           // njobs x pt_bytes
};

struct CollectUnshardArgs {
  uint32_t n, out_len, fb;  // n: the collections that were opened
  const uint8_t* leader_pts;  // n x out_len * fb
  const uint8_t* helper_pts;
  const uint8_t* leader_ok;  // n: the opens' ok
  const uint8_t* helper_ok;
  const uint32_t* row;  // n: the collection's row of out / status
  uint32_t* bad;        // n x 2, zeroed: an element >= p in the leader's / the helper's share
  uint8_t* out;         // rows of out_len * fb
  uint8_t* status;
};

#ifdef __HIPCC__
// the merge (one launch for all jobs: a workgroup per (job, tile)), then the decision (a wave per job)
hipError_t launch_collect_merge(const CollectMergeArgs& a, hipStream_t s);
// the final status; zero enc, ciphertext and share of every job that is not COLLECT_OK
hipError_t launch_collect_finish(const CollectFinishArgs& a, hipStream_t s);
// check and add the two opened shares (a workgroup per (collection, tile)), then the status per collection and
// zeros in the row of one that failed
hipError_t launch_collect_unshard(const CollectUnshardArgs& a, hipStream_t s);
#endif

}  // namespace jx
