// jx_upload.h — the leader's upload path on the device (jx_leader_upload_open_*, include/jx_prio3.h): what
// jx_engine_upload.cpp hands to the kernels of jx_hpke_long.hip. Plain structs, no device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jx_keyreg.h"

namespace jx {

enum : uint8_t {
  UP_ROW_MALFORMED = 1,  // the encapsulated key has the length of neither keypair's KEM: DecryptFailure without an open
};
// One uploaded report's leader share: where its encapsulated key and ciphertext lie in the call's buffers, the
// keypairs to try (registry slots; key0 KEY_SLOT_NONE: the config id is unknown) and its time as the
// InputShareAad encodes it.
struct UpRow {
  uint64_t ct_off, enc_off;
  uint32_t ct_len, enc_len;
  uint16_t key0, key1;
  uint8_t flags, pad[3];
  uint8_t time_be[8];
};
static_assert(sizeof(UpRow) == 40, "UpRow layout");

constexpr size_t UPLOAD_CTX_BYTES = 2 * 64;  // scratch per report: one LongCtxRow per trial

struct UploadArgs {
  uint64_t n;
  const UpRow* rows;
  const HpkeKeyRow* keys;  // the device's key registry
  uint32_t nkeys;
  uint32_t ps_bytes;
  const uint8_t* ids;  // n x 16
  const uint8_t* ps;   // n x ps_bytes
  uint8_t task_id[32];
  const uint8_t* encs;
  const uint8_t* cts;
  uint8_t* pts;  // scratch as long as cts: report i's plaintext at its ct_off
  void* ctx;     // scratch, n x UPLOAD_CTX_BYTES
  uint8_t* out_rows;
  uint64_t lis_stride;
  uint32_t lis_bytes;   // the leader input share: elements || [blind]
  uint32_t elem_bytes;  // its measurement-share and proofs-share part, fb bytes per element
  uint32_t fb;          // 8: Field64, 16: Field128
  uint8_t* out_ext;     // as long as cts: report i's extensions at its ct_off
  uint32_t* out_ext_len;
  uint8_t* out_status;
  uint32_t zero_ist[8], zero_ost[8];  // filled by the launcher
};

// Stage A for both trials of every report (the P-256 kernel only when a keypair of that KEM is among the call's),
// then open + decode + validate + lay out, one wave per report. All on `s`.
hipError_t launch_upload_open(UploadArgs a, bool any_p256, hipStream_t s);

}  // namespace jx
