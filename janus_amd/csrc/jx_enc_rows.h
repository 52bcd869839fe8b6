// jx_enc_rows.h — how one sealed report share becomes the EncRow the rows kernels read (jx_keyreg.h, jx_hpke_open.h).
//
// The rule exists once, enc_row_make: which flags a row gets, which registry slots, and whether its encapsulated key
// goes into the row (32 bytes, X25519) or beside it (65 bytes, P-256). Two callers lay rows out with it: the host
// loop fill_enc_rows_with (jx_helper_prep_encrypted_batch2, alone and coalesced, and the host form of the sealed
// fused call, per launch) and enc_rows_kernel (jx_hpke.hip), which the device form of the sealed fused call runs so
// that neither the rows nor the encapsulated keys pass through host memory. __host__ __device__ and without HIP
// calls, so tests/csrc/hosttest_enc_rows.cpp runs both callers' paths on the CPU against the loop as it was written
// before it was shared.
#pragma once
#include <stdint.h>

#include "../../include/jx_prio3.h"
#include "jx_field.h"
#include "jx_keyreg.h"

namespace jx {

// A request's keypairs as the rule reads them, by the request's keypair index: the keypair's slot of the device's
// key registry and the length of its KEM's encapsulated keys (32 or 65). flags: the request's JX_ENC_*.
struct EncRowKeys {
  uint32_t nkeys;
  uint32_t flags;
  uint16_t slot[JX_ENC_MAX_KEYPAIRS];
  uint8_t klen[JX_ENC_MAX_KEYPAIRS];
};

// Report i's row: its time, ciphertext span, keypair indices (k0, k1: JX_KEY_NONE / JX_KEY_MALFORMED or an index
// below K.nkeys) and encapsulated key (enc_len bytes at enc). A trial can only succeed when the encapsulated key has
// the length of the keypair's KEM (32: X25519, 65: P-256); the others fail as the hpke crate's deserialisation does,
// on the device by the key row's KEM id. A key that fits neither keypair marks the row malformed. A 32-byte key goes
// into the row; a 65-byte key that a P-256 keypair of the row can try is copied to enc65_dst, the row says where the
// rows kernel finds it (enc65_off, from the launch's ciphertext base) and the function returns true.
JX_HD bool enc_row_make(EncRow& w, const EncRowKeys& K, const uint8_t* task_id, uint64_t time, uint8_t k0, uint8_t k1,
                        const uint8_t* enc, uint64_t enc_len, uint64_t ct_off, uint32_t ct_len, uint64_t enc65_off,
                        uint8_t* enc65_dst) {
  w = EncRow{};
  for (int b = 0; b < 32; b++) w.task_id[b] = task_id[b];
  for (int b = 0; b < 8; b++) w.time_be[b] = (uint8_t)(time >> (56 - 8 * b));
  w.ct_off = ct_off;
  w.ct_len = ct_len;
  w.flags = ENC_ROW_ENCRYPTED | ((K.flags & JX_ENC_REQUIRE_TASKPROV) ? ENC_ROW_REQUIRE_TASKPROV : 0);
  const bool fits = (k0 < K.nkeys && K.klen[k0] == enc_len) || (k1 < K.nkeys && K.klen[k1] == enc_len);
  bool took65 = false;
  if (k0 == JX_KEY_MALFORMED || (k0 < K.nkeys && !fits)) {
    w.flags |= ENC_ROW_MALFORMED;
  } else if (fits && enc_len == 65) {
    w.flags |= ENC_ROW_ENC65;
    w.enc65_off = enc65_off;
    for (int b = 0; b < 65; b++) enc65_dst[b] = enc[b];
    took65 = true;
  } else if (enc_len == 32) {
    for (int b = 0; b < 32; b++) w.enc[b] = enc[b];
  }
  w.key0 = k0 < K.nkeys ? K.slot[k0] : (k0 == JX_KEY_MALFORMED ? (uint16_t)0 : KEY_SLOT_NONE);
  w.key1 = k1 < K.nkeys ? K.slot[k1] : KEY_SLOT_NONE;
  return took65;
}

// enc_rows_kernel's arguments (jx_hpke.hip): the compact per-report arrays of one launch as the caller passed them
// (26 bytes per report, staged unchanged), the caller's encapsulated keys in place, and where the rows go.
struct EncRowsArgs {
  uint64_t n;                       // reports of the launch
  uint64_t first;                   // the first one's index in the call (enc_offsets null: report r's key is at
                                    // 32 * (first + r) of encs)
  const uint64_t* times;            // [n]
  const uint8_t* key_index;         // [n x 2]
  const uint64_t* enc_offsets;      // [n + 1] into encs, as the caller counts them; null: n x 32 bytes
  const uint64_t* payload_offsets;  // [n + 1] as the caller counts them: the rows' ct_off are these
  const uint8_t* encs;              // the caller's device array
  EncRow* rows;                     // out: [n]
  uint8_t* enc65;                   // out: row r's 65-byte key at 65 r (written for ENC_ROW_ENC65 rows only)
  uint64_t enc65_base;              // enc65 counted from the rows kernels' ciphertext base (modulo 2^64)
  uint8_t task_id[32];
  EncRowKeys keys;
};

// The rows of n reports on the host, ciphertexts at ct_base + their offset from the first one's; the 65-byte keys
// are packed into enc65, which the caller places at enc65_base of the launch's ciphertext bytes. enc_offsets null:
// n x 32 bytes. Returns the number of ENC_ROW_ENC65 rows.
inline uint64_t fill_enc_rows_with(const EncRowKeys& K, const uint8_t* task_id, const uint64_t* times,
                                   const uint8_t* key_index, const uint8_t* encs, const uint64_t* enc_offsets,
                                   const uint64_t* payload_offsets, uint64_t n, EncRow* rows, uint64_t ct_base,
                                   uint64_t enc65_base, uint8_t* enc65) {
  const uint64_t c0 = payload_offsets[0];
  uint64_t n65 = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t eo = enc_offsets ? enc_offsets[i] : 32 * i, len = enc_offsets ? enc_offsets[i + 1] - eo : 32;
    n65 += enc_row_make(rows[i], K, task_id, times[i], key_index[2 * i], key_index[2 * i + 1], encs + eo, len,
                        ct_base + (payload_offsets[i] - c0), (uint32_t)(payload_offsets[i + 1] - payload_offsets[i]),
                        enc65_base + 65 * n65, enc65 + 65 * n65);
  }
  return n65;
}

}  // namespace jx
