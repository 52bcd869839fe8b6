// jx_keyreg.h — slot bookkeeping of the device-resident HPKE key registry (jx_hpke.hip; include/jx_hpke.h).
//
// Every jx_hpke context owns one row of a fixed device array of HpkeKeyRow for as long as it lives; the EncRows of a
// prepare launch name their keypairs by that row's index (16 bits, KEY_SLOT_NONE: no key). This unit hands the
// indices out: take, free, reuse, exhaustion. Host only and without HIP, so tests/csrc/hosttest_keyreg.cpp runs it
// on the CPU. Not synchronised: the registry holds its mutex around every call. The two row types the slots tie
// together, HpkeKeyRow and EncRow, are defined here too (plain structs: host code, kernels and that test share them).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/jx_hpke.h"

namespace jx {

constexpr uint32_t KEY_SLOTS = JX_HPKE_MAX_CONTEXTS;  // rows of a device's registry: live contexts per device (16,384)
constexpr uint16_t KEY_SLOT_NONE = 0xFFFF;  // EncRow::key0 / key1: no keypair to try

// A recipient keypair as the rows kernels read it, one row of the registry: the private and public key and the RFC
// 9180 key_schedule_context of its application info (0x00 || psk_id_hash || info_hash: 1 + 2 Nh bytes, 65 for
// HKDF-SHA256, 97 for -SHA384, 129 for -SHA512) under the key's own suite, whose KDF, AEAD and KEM ids follow (kem:
// the low byte of the id, 0x20 or 0x10). KEM 0x0020: sk the clamped X25519 scalar, pk the public key, both as LE
// words. KEM 0x0010 (P-256): sk the LE words of the private integer (sk[0] least significant), pk the 32
// big-endian bytes of the public point's x and pky those of its y, in memory order. The default-suite kernels
// read the first 65 context bytes and no ids.
struct HpkeKeyRow {
  uint32_t sk[8];
  uint32_t pk[8];
  uint8_t ksc[132];
  uint8_t kdf, aead, kem;
  uint8_t pad;
  uint8_t pky[32];
};
static_assert(sizeof(HpkeKeyRow) == 232, "HpkeKeyRow layout");
enum : uint8_t {
  ENC_ROW_ENCRYPTED = 1,         // the report's helper input share is inside `enc` / the ciphertext (else: uploaded)
  ENC_ROW_REQUIRE_TASKPROV = 2,  // the task is provisioned by taskprov (aggregator.rs:1869-1879)
  ENC_ROW_MALFORMED = 4,         // the encapsulated key has the length of neither keypair's KEM: HpkeDecryptError
                                 // without an open
  ENC_ROW_ENC65 = 8,             // a 65-byte (P-256) encapsulated key, at enc65_off of the launch's ciphertext bytes:
                                 // hpke_rows_p256_kernel's row, skipped by the X25519 rows kernels
};
// One report's encrypted input share: the HpkeCiphertext's encapsulated key and ciphertext (at ct_off of the
// launch's ciphertext bytes), what its InputShareAad needs besides the id and public share rows, and the
// keypairs to try (registry slots; key0 KEY_SLOT_NONE: the config id is unknown).
struct EncRow {
  uint8_t enc[32];
  uint8_t task_id[32];
  uint8_t time_be[8];  // ReportMetadata.time, big-endian as encoded
  uint64_t ct_off;
  uint32_t ct_len;
  uint16_t key0, key1;
  uint64_t enc65_off;  // ENC_ROW_ENC65: where the encapsulated key lies (`enc` is zero)
  uint8_t flags, pad[7];
};
static_assert(sizeof(EncRow) == 104 && sizeof(EncRow) % 8 == 0, "EncRow layout");

class KeySlots {
 public:
  explicit KeySlots(uint32_t capacity = KEY_SLOTS) : cap_(capacity) {}
  // A free slot, or -1 when `capacity` slots are taken. Freed slots go out again first (latest freed first), then
  // the slots never used, in order: the live slots stay at the low end of the array.
  int32_t take() {
    if (!freed_.empty()) {
      const uint32_t s = freed_.back();
      freed_.pop_back();
      live_++;
      return (int32_t)s;
    }
    if (next_ >= cap_) return -1;
    live_++;
    return (int32_t)next_++;
  }
  // Hand back a slot that take() returned and that is not free already.
  void free(uint32_t slot) {
    freed_.push_back(slot);
    live_--;
  }
  uint32_t live() const { return live_; }
  uint32_t capacity() const { return cap_; }

 private:
  uint32_t cap_, next_ = 0, live_ = 0;
  std::vector<uint32_t> freed_;
};

}  // namespace jx
