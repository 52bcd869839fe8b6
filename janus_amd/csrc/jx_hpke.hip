// jx_hpke.hip — batched HPKE open of report shares on the GPU.
//
// Replaces the per-report `hpke::open(&helper_keypair, &HpkeApplicationInfo::new(
// &Label::InputShare, &Role::Client, &Role::Helper), encrypted_input_share, &input_share_aad)`
// of the helper's aggregate-init loop (aggregator/src/aggregator.rs:1772-1832; core/src/hpke.rs:
// 200-230): RFC 9180 base mode, DHKEM(X25519, HKDF-SHA256), HKDF-SHA256, AES-128-GCM. One
// report per lane: X25519 decapsulation, the HKDF key schedule, AES-128-GCM open.
// The other eight X25519 suites an HpkeConfig can name (HKDF-SHA256 / -SHA384 / -SHA512 with AES-128-GCM /
// AES-256-GCM / ChaCha20Poly1305; jx_hpke_suites.h) go through a second pair of kernels, hpke_open_suite_kernel
// and hpke_rows_suite_kernel, which read the suite from the key row and dispatch per lane. They are launched only
// for a context, or a launch with a job, that holds a key outside the default suite (then for every row of the
// launch), so the default suite's kernels and their register budget are what they were.
// The second KEM the reference opens under, DHKEM(P-256, HKDF-SHA256) (0x0010; jx_p256.h), has a third pair,
// hpke_open_p256_kernel and hpke_rows_p256_kernel: its encapsulated keys are 65 bytes, so the rows of a prepare
// launch partition by that length (a trial of a keypair of the other KEM fails without an open), the X25519 rows
// kernels skip the 65-byte rows, and the P-256 rows kernel, launched only when the launch holds one, takes them.
//
// Two kernels (each with its suite twin and its P-256 twin):
//  - hpke_open_kernel: the standalone batch open of include/jx_hpke.h (caller's ciphertexts and AADs);
//  - hpke_rows_kernel: the open INSIDE a helper prepare launch (jx_helper_prep_encrypted_batch, alone or
//    coalesced): per report it builds the InputShareAad from the report's task id, id, time and public share
//    rows, tries the task's and then the global keypair (aggregator.rs:1807-1820), decodes the
//    PlaintextInputShare and checks its extensions (:1834-1893) and writes the payload into the helper
//    input-share row K1 reads, with one status byte per report (include/jx_prio3.h, JX_OPEN_*).
// C ABI in include/jx_hpke.h; the rows kernel's launcher is internal (jx_engine_internal.h).
//
// This unit holds the C ABI, the key registry, open_mask_kernel, enc_rows_kernel (the rows of a launch of the sealed
// fused call's device form, laid out on the device by the rule of jx_enc_rows.h) and the two dispatchers, launch_open
// and jxi::launch_hpke_rows. Each kernel pair is a translation unit of its own, so that the three compile side by side:
// jx_hpke_default.hip, jx_hpke_suite.hip and jx_hpke_p256.hip; what they share is in jx_hpke_open.h. The seal calls
// (jx_hpke_create_sender, jx_hpke_seal_*) are here too; their kernels are in jx_hpke_seal.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/jx_hpke.h"
#include "jx_engine_internal.h"
#include "jx_hpke_long.h"
#include "jx_hpke_open.h"
#include "jx_hpke_seal.h"
#include "jx_hpke_suites.h"
#include "jx_keyreg.h"

using namespace jx;

namespace {

__global__ __launch_bounds__(256) void open_mask_kernel(const uint8_t* status, uint8_t* verdicts, uint64_t n) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n && status[r] != JX_OPEN_OK) verdicts[r] = JX_OPEN_FAILURE;
}

// The EncRows of one launch from the caller's compact arrays (jx_enc_rows.h), one report per lane. A lane reads its
// 26 bytes of the staged arrays (neighbouring lanes neighbouring addresses) and its encapsulated key where it lies in
// the caller's array (32 contiguous bytes per lane when every key is an X25519 one), makes its row with the rule the
// host loop uses, and the workgroup writes its ENC_ROWS_WG rows, which are contiguous in memory, through LDS in
// whole dwords: lane t stores dwords t, t + 256, ... of the workgroup's span, so every store instruction covers 1 KiB
// without a gap (a lane storing its own 104-byte row would touch 64 cache lines per instruction).
constexpr uint32_t ENC_ROWS_WG = 256, ENC_ROW_WORDS = sizeof(EncRow) / 4;
__global__ __launch_bounds__(ENC_ROWS_WG) void enc_rows_kernel(const EncRowsArgs a) {
  __shared__ uint32_t sm[ENC_ROWS_WG * ENC_ROW_WORDS];
  const uint64_t r0 = (uint64_t)blockIdx.x * ENC_ROWS_WG, r = r0 + threadIdx.x;
  if (r < a.n) {
    const uint64_t eo = a.enc_offsets ? a.enc_offsets[r] : 32 * (a.first + r);
    const uint64_t elen = a.enc_offsets ? a.enc_offsets[r + 1] - eo : 32;
    const uint64_t p0 = a.payload_offsets[r], p1 = a.payload_offsets[r + 1];
    EncRow w;
    enc_row_make(w, a.keys, a.task_id, a.times[r], a.key_index[2 * r], a.key_index[2 * r + 1], a.encs + eo, elen, p0,
                 (uint32_t)(p1 - p0), a.enc65_base + 65 * r, a.enc65 + 65 * r);
    uint32_t words[ENC_ROW_WORDS];
    __builtin_memcpy(words, &w, sizeof w);
#pragma unroll
    for (uint32_t k = 0; k < ENC_ROW_WORDS; k++) sm[threadIdx.x * ENC_ROW_WORDS + k] = words[k];
  }
  __syncthreads();
  const uint64_t left = a.n - r0;  // r0 < n: the grid is ceil(n / ENC_ROWS_WG) workgroups
  const uint32_t nw = (uint32_t)(left < ENC_ROWS_WG ? left : ENC_ROWS_WG) * ENC_ROW_WORDS;
  uint32_t* out = reinterpret_cast<uint32_t*>(a.rows + r0);
  for (uint32_t i = threadIdx.x; i < nw; i += ENC_ROWS_WG) out[i] = sm[i];
}

}  // namespace

struct jx_hpke {
  HpkeCfg cfg{};
  bool default_suite = true;  // X25519 with (HKDF-SHA256, AES-128-GCM): opened by hpke_open_kernel / hpke_rows_kernel
  uint32_t kem = HPKE_KEM_X25519_SHA256;
  bool sender = false;  // jx_hpke_create_sender: the recipient's public key alone (sk is zero); it seals, never opens
  int device = 0;
  uint32_t slot = 0;            // the context's row of the device's key registry, for as long as it lives
  hipStream_t stream = nullptr;  // created at the first standalone open or jx_hpke_stream (ensure_stream)
  jxi::Arena* arena = nullptr;  // the device's arena: the host-buffer open's device buffers
  std::mutex mu;                // one call at a time per handle (its stream and staging)
};

// errors: per calling thread (jx_hpke_last_error)
static thread_local std::string t_hpke_err;

static int32_t hfail(int32_t code, const std::string& m) {
  t_hpke_err = m;
  return code;
}
#define HCHK(call)                                                                                   \
  do {                                                                                               \
    hipError_t _st = (call);                                                                         \
    if (_st != hipSuccess) return hfail(JX_HPKE_E_HIP, std::string(#call) + ": " + hipGetErrorString(_st)); \
  } while (0)

// The device's key registry: KEY_SLOTS rows of device memory of its own (not the arena's: a launch in flight must
// never see the table move), allocated at the first context creation on the device and kept for the life of the
// process; one stream for the rows' uploads.
namespace {
struct KeyRegistry {
  std::mutex mu;
  HpkeKeyRow* d_rows = nullptr;
  hipStream_t stream = nullptr;
  KeySlots slots;
};
std::mutex g_reg_mu;
std::vector<KeyRegistry*> g_regs;  // by device

KeyRegistry* registry_for(int device) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if ((size_t)device >= g_regs.size()) g_regs.resize(device + 1, nullptr);
  if (!g_regs[device]) g_regs[device] = new KeyRegistry();
  return g_regs[device];
}

// Take a slot and write the row, synchronously: the row is on the device when this returns.
int32_t registry_add(int device, const HpkeKeyRow& row, uint32_t* slot) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  HCHK(hipSetDevice(device));
  if (!R->d_rows) {
    HpkeKeyRow* p = nullptr;
    const hipError_t st = hipMalloc((void**)&p, (size_t)KEY_SLOTS * sizeof(HpkeKeyRow));
    if (st == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (HPKE key registry)");
    HCHK(st);
    if (!R->stream) HCHK(hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking));
    R->d_rows = p;
  }
  const int32_t s = R->slots.take();
  if (s < 0)
    return hfail(JX_HPKE_E_NOMEM, "the device's HPKE key registry is full: " + std::to_string(KEY_SLOTS) +
                                      " live contexts (jx_hpke_destroy frees a slot)");
  hipError_t st = hipMemcpyAsync(R->d_rows + s, &row, sizeof row, hipMemcpyHostToDevice, R->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(R->stream);
  if (st != hipSuccess) {
    R->slots.free((uint32_t)s);
    return hfail(JX_HPKE_E_HIP, std::string("HPKE key registry upload: ") + hipGetErrorString(st));
  }
  *slot = (uint32_t)s;
  return JX_HPKE_OK;
}

// Wipe the row (it held a private key) and free the slot for the next context.
void registry_remove(int device, uint32_t slot) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  const HpkeKeyRow zero{};
  if (hipSetDevice(device) == hipSuccess &&
      hipMemcpyAsync(R->d_rows + slot, &zero, sizeof zero, hipMemcpyHostToDevice, R->stream) == hipSuccess)
    (void)hipStreamSynchronize(R->stream);
  R->slots.free(slot);
}

// with h->mu held
int32_t ensure_stream(jx_hpke* h) {
  if (h->stream) return JX_HPKE_OK;
  HCHK(hipSetDevice(h->device));
  HCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  return JX_HPKE_OK;
}
}  // namespace

// a context of jx_hpke_create_sender holds no private key: refused before anything is queued
static int32_t refuse_sender() {
  return hfail(JX_HPKE_E_INVALID, "a sender context (jx_hpke_create_sender) holds no private key: it cannot open");
}

// the default suite keeps its own kernel; any other goes through the suite kernel of its KEM
static void launch_open(const jx_hpke* h, const HpkeBufs& b) {
  if (h->kem == HPKE_KEM_P256_SHA256)
    launch_hpke_open_p256(h->cfg, b, h->stream);
  else if (h->default_suite)
    launch_hpke_open_default(h->cfg, b, h->stream);
  else
    launch_hpke_open_suite(h->cfg, b, h->stream);
}

namespace jxi {

int hpke_device(const jx_hpke* h) { return h->device; }
uint16_t hpke_slot(const jx_hpke* h) { return (uint16_t)h->slot; }
void hpke_registry(int device, const HpkeKeyRow** rows, uint32_t* capacity) {
  KeyRegistry* R = registry_for(device);
  std::lock_guard<std::mutex> lk(R->mu);
  *rows = R->d_rows;
  *capacity = KEY_SLOTS;
}
bool hpke_default_suite(const jx_hpke* h) { return h->default_suite; }
bool hpke_is_sender(const jx_hpke* h) { return h->sender; }
uint32_t hpke_enc_len(const jx_hpke* h) { return jx::hpke_enc_len(h->kem); }

hipError_t launch_hpke_rows(const HpkeRowsArgs& a, bool suites, bool p256_rows, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  RowsArgs ra;
  ra.a = a;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, ra.zero_ist, ra.zero_ost);
  // a key of another suite among the launch's jobs: every row of the launch goes through the suite kernel
  if (suites)
    launch_hpke_rows_suite(ra, s);
  else
    launch_hpke_rows_default(ra, s);
  // the rows with a 65-byte encapsulated key (the others' rows it skips; both write his / status of their own rows)
  if (p256_rows) launch_hpke_rows_p256(ra, s);
  return hipGetLastError();
}

hipError_t launch_enc_rows(const EncRowsArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(enc_rows_kernel, dim3((uint32_t)((a.n + ENC_ROWS_WG - 1) / ENC_ROWS_WG)), dim3(ENC_ROWS_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_open_mask(const uint8_t* status, uint8_t* verdicts, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(open_mask_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, status, verdicts, n);
  return hipGetLastError();
}

}  // namespace jxi

// The context of a key row whose sk / pk / pky are filled in: the device, the key_schedule_context under the key's
// own suite, the registry row.
static int32_t create_context(const HpkeKeyRow& key, uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id,
                              const uint8_t* info, uint32_t info_len, int32_t device, bool sender, jx_hpke** out) {
  const bool p256 = kem_id == HPKE_KEM_P256_SHA256;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return JX_HPKE_E_NODEVICE;
  if (device < 0 || device >= ndev) return JX_HPKE_E_INVALID;
  jx_hpke* h = new jx_hpke();
  h->device = device;
  h->cfg.key = key;
  h->kem = kem_id;
  h->sender = sender;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, h->cfg.zero_ist, h->cfg.zero_ost);
  // the key_schedule_context under the key's own suite and hash (jx_hpke_suites.h)
  static_assert(sizeof(h->cfg.key.ksc) >= HPKE_KSC_MAX, "HpkeKeyRow holds the longest key_schedule_context");
  hpke_key_schedule_context(kdf_id, aead_id, info, info_len, h->cfg.key.ksc, kem_id);
  h->cfg.key.kdf = (uint8_t)kdf_id;
  h->cfg.key.aead = (uint8_t)aead_id;
  h->cfg.key.kem = (uint8_t)kem_id;
  h->default_suite = !p256 && kdf_id == HPKE_KDF_SHA256 && aead_id == HPKE_AEAD_AES128GCM;
  // the context's row of the device's key registry (full: JX_HPKE_E_NOMEM)
  if (const int32_t rc = registry_add(device, h->cfg.key, &h->slot)) {
    delete h;
    return rc;
  }
  h->arena = jxi::arena_for(device);
  *out = h;
  return JX_HPKE_OK;
}

extern "C" {

int32_t jx_hpke_create(const uint8_t sk[32], const uint8_t pk[32], const uint8_t* info, uint32_t info_len,
                       int32_t device, jx_hpke** out) {
  return jx_hpke_create_suite(HPKE_KEM_X25519_SHA256, HPKE_KDF_SHA256, HPKE_AEAD_AES128GCM, sk, pk, info, info_len,
                              device, out);
}

int32_t jx_hpke_create_suite(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t sk[32],
                             const uint8_t pk[32], const uint8_t* info, uint32_t info_len, int32_t device,
                             jx_hpke** out) {
  if (!sk || !pk || !out || (info_len && !info)) return JX_HPKE_E_INVALID;
  *out = nullptr;
  if (!hpke_suite_supported(kem_id, kdf_id, aead_id))
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "unsupported HPKE suite (KEM " + std::to_string(kem_id) + ", KDF " + std::to_string(kdf_id) + ", AEAD " +
                     std::to_string(aead_id) + "): KEM 0x0020 (X25519) with 32-byte keys (KEM 0x0010, P-256, has 65-byte "
                     "public keys: jx_hpke_create_key), KDF 1..3 (HKDF-SHA256/384/512), AEAD 1..3 (AES-128-GCM, "
                     "AES-256-GCM, ChaCha20Poly1305)");
  return jx_hpke_create_key(kem_id, kdf_id, aead_id, sk, 32, pk, 32, info, info_len, device, out);
}

int32_t jx_hpke_create_key(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t* sk, uint32_t sk_len,
                           const uint8_t* pk, uint32_t pk_len, const uint8_t* info, uint32_t info_len, int32_t device,
                           jx_hpke** out) {
  if (!sk || !pk || !out || (info_len && !info)) return JX_HPKE_E_INVALID;
  *out = nullptr;
  if (!hpke_key_supported(kem_id, kdf_id, aead_id))
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "unsupported HPKE suite (KEM " + std::to_string(kem_id) + ", KDF " + std::to_string(kdf_id) + ", AEAD " +
                     std::to_string(aead_id) + "): KEM 0x0020 (X25519) or 0x0010 (P-256), KDF 1..3 (HKDF-SHA256/384/512), "
                     "AEAD 1..3 (AES-128-GCM, AES-256-GCM, ChaCha20Poly1305)");
  const bool p256 = kem_id == HPKE_KEM_P256_SHA256;
  if (sk_len != 32 || pk_len != hpke_enc_len(kem_id))
    return hfail(JX_HPKE_E_INVALID, p256 ? "P-256 keypair: the private key is 32 bytes, the public key 65"
                                         : "X25519 keypair: the private and the public key are 32 bytes each");
  HpkeKeyRow key{};
  if (p256) {  // the same code as the kernels', on the host (jx_p256.h)
    if (const char* why = hpke_p256_keypair(sk, pk, key.sk, (uint8_t*)key.pk, key.pky)) return hfail(JX_HPKE_E_INVALID, why);
  } else {
    uint8_t k[32];
    memcpy(k, sk, 32);
    k[0] &= 248;
    k[31] &= 127;
    k[31] |= 64;
    for (int i = 0; i < 8; i++) {
      memcpy(&key.sk[i], k + 4 * i, 4);
      memcpy(&key.pk[i], pk + 4 * i, 4);
    }
  }
  return create_context(key, kem_id, kdf_id, aead_id, info, info_len, device, false, out);
}

int32_t jx_hpke_create_sender(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t* pk, uint32_t pk_len,
                              const uint8_t* info, uint32_t info_len, int32_t device, jx_hpke** out) {
  if (!pk || !out || (info_len && !info)) return JX_HPKE_E_INVALID;
  *out = nullptr;
  if (kem_id == HPKE_KEM_P256_SHA256 && kdf_id >= 1 && kdf_id <= 3 && aead_id >= 1 && aead_id <= 3)
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "sealing under KEM 0x0010 (P-256) is out of scope: the engine seals under KEM 0x0020 (X25519) only");
  if (!hpke_suite_supported(kem_id, kdf_id, aead_id))
    return hfail(JX_HPKE_E_UNSUPPORTED,
                 "unsupported HPKE suite (KEM " + std::to_string(kem_id) + ", KDF " + std::to_string(kdf_id) + ", AEAD " +
                     std::to_string(aead_id) + "): a sender seals under KEM 0x0020 (X25519), KDF 1..3 (HKDF-SHA256/384/512), "
                     "AEAD 1..3 (AES-128-GCM, AES-256-GCM, ChaCha20Poly1305)");
  if (pk_len != 32) return hfail(JX_HPKE_E_INVALID, "X25519 sender: the recipient's public key is 32 bytes");
  HpkeKeyRow key{};  // the private-key words stay zero
  for (int i = 0; i < 8; i++) memcpy(&key.pk[i], pk + 4 * i, 4);
  return create_context(key, kem_id, kdf_id, aead_id, info, info_len, device, true, out);
}

int32_t jx_hpke_suite(const jx_hpke* h, uint32_t* kem_id, uint32_t* kdf_id, uint32_t* aead_id) {
  if (!h) return JX_HPKE_E_INVALID;
  if (kem_id) *kem_id = h->kem;
  if (kdf_id) *kdf_id = h->cfg.key.kdf;
  if (aead_id) *aead_id = h->cfg.key.aead;
  return JX_HPKE_OK;
}

int32_t jx_hpke_enc_len(const jx_hpke* h) { return h ? (int32_t)hpke_enc_len(h->kem) : 0; }

int32_t jx_hpke_stream(const jx_hpke* h, void** out_stream) {
  if (!h || !out_stream) return JX_HPKE_E_INVALID;
  jx_hpke* m = const_cast<jx_hpke*>(h);  // the stream is created at its first use
  std::lock_guard<std::mutex> lk(m->mu);
  if (const int32_t rc = ensure_stream(m)) return rc;
  *out_stream = (void*)h->stream;
  return JX_HPKE_OK;
}

void jx_hpke_destroy(jx_hpke* h) {
  if (!h) return;
  if (h->stream) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  registry_remove(h->device, h->slot);
  delete h;
}

int32_t jx_hpke_open_batch_device(jx_hpke* h, uint64_t n, const void* d_encs, const void* d_cts,
                                  const uint64_t* d_ct_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                  void* d_out_plaintexts, void* d_out_ok) {
  if (!h || (n && (!d_encs || !d_cts || !d_ct_offsets || !d_aad_offsets || !d_out_plaintexts || !d_out_ok))) {
    return JX_HPKE_E_INVALID;
  }
  if (h->sender) return refuse_sender();
  if (n == 0) return JX_HPKE_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  HpkeBufs b{n,
             (const uint8_t*)d_encs,
             (const uint8_t*)d_cts,
             d_ct_offsets,
             (const uint8_t*)d_aads,
             d_aad_offsets,
             (uint8_t*)d_out_plaintexts,
             (uint8_t*)d_out_ok};
  launch_open(h, b);
  HCHK(hipGetLastError());
  return JX_HPKE_OK;
}

// Host buffers: one staging slab from the device's arena (no per-call hipMalloc / hipFree, which would wait
// for the whole device), handed back stream-ordered; only this handle's stream is synchronized.
int32_t jx_hpke_open_batch(jx_hpke* h, uint64_t n, const uint8_t* encs, const uint8_t* cts,
                           const uint64_t* ct_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                           uint8_t* out_plaintexts, uint8_t* out_ok) {
  if (!h || (n && (!encs || !cts || !ct_offsets || !aad_offsets || !out_plaintexts || !out_ok)))
    return JX_HPKE_E_INVALID;
  if (h->sender) return refuse_sender();
  if (n == 0) return JX_HPKE_OK;
  for (uint64_t i = 0; i < n; i++)
    if (ct_offsets[i + 1] < ct_offsets[i] + 16 || aad_offsets[i + 1] < aad_offsets[i])
      return hfail(JX_HPKE_E_INVALID, "offsets must be non-decreasing and every ciphertext >= 16 bytes");
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  const uint64_t ct_bytes = ct_offsets[n], aad_bytes = aad_offsets[n], pt_bytes = ct_bytes - 16 * n;
  const uint64_t enc_bytes = n * hpke_enc_len(h->kem);
  const size_t o_enc = 0, o_ct = o_enc + jxi::align256(enc_bytes), o_aad = o_ct + jxi::align256(ct_bytes),
               o_pt = o_aad + jxi::align256(aad_bytes ? aad_bytes : 1), o_ok = o_pt + jxi::align256(pt_bytes ? pt_bytes : 1),
               o_co = o_ok + jxi::align256(n), o_ao = o_co + jxi::align256((n + 1) * 8), bytes = o_ao + jxi::align256((n + 1) * 8);
  jxi::Slab slab;
  const hipError_t ga = jxi::arena_get(h->arena, bytes, h->stream, true, true, slab);
  if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
  HCHK(ga);
  uint8_t* base = (uint8_t*)slab.p;
  int32_t rc = JX_HPKE_OK;
  do {
    if (hipMemcpyAsync(base + o_enc, encs, enc_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ct, cts, ct_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (aad_bytes && hipMemcpyAsync(base + o_aad, aads, aad_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        hipMemcpyAsync(base + o_co, ct_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ao, aad_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "host-to-device copy failed");
      break;
    }
    HpkeBufs b{n, base + o_enc, base + o_ct, (const uint64_t*)(base + o_co), base + o_aad, (const uint64_t*)(base + o_ao),
               base + o_pt, base + o_ok};
    launch_open(h, b);
    if (hipGetLastError() != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "kernel launch failed");
      break;
    }
    if ((pt_bytes && hipMemcpyAsync(out_plaintexts, base + o_pt, pt_bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
        hipMemcpyAsync(out_ok, base + o_ok, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "device-to-host copy failed");
      break;
    }
  } while (0);
  jxi::arena_put(h->arena, slab, h->stream);  // reused after this stream's work
  return rc;
}

// ---- the wave-per-report open of long payloads (jx_hpke_long.hip)

// with h->mu held and the device set: both stages on the context's stream, the context rows in a slab of the
// arena that goes back stream-ordered
static int32_t launch_open_long(jx_hpke* h, const HpkeBufs& b) {
  const HpkeKeyRow* rows = nullptr;
  uint32_t cap = 0;
  jxi::hpke_registry(h->device, &rows, &cap);
  jxi::Slab slab;
  const hipError_t ga = jxi::arena_get(h->arena, jxi::align256(b.n * sizeof(LongCtxRow)), h->stream, true, true, slab);
  if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
  HCHK(ga);
  LongCtxArgs ca{};
  ca.n = b.n;
  ca.keys = rows;
  ca.slot = h->slot;
  ca.encs = b.encs;
  ca.out = (LongCtxRow*)slab.p;
  memcpy(ca.zero_ist, h->cfg.zero_ist, 32);
  memcpy(ca.zero_ost, h->cfg.zero_ost, 32);
  const hipError_t st = launch_hpke_long_open(ca, h->kem == HPKE_KEM_P256_SHA256, b, h->stream);
  jxi::arena_put(h->arena, slab, h->stream);
  if (st != hipSuccess) return hfail(JX_HPKE_E_HIP, std::string("long open launch: ") + hipGetErrorString(st));
  return JX_HPKE_OK;
}

int32_t jx_hpke_open_long_batch_device(jx_hpke* h, uint64_t n, const void* d_encs, const void* d_cts,
                                       const uint64_t* d_ct_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                       void* d_out_plaintexts, void* d_out_ok) {
  if (!h || (n && (!d_encs || !d_cts || !d_ct_offsets || !d_aad_offsets || !d_out_plaintexts || !d_out_ok))) {
    return JX_HPKE_E_INVALID;
  }
  if (h->sender) return refuse_sender();
  if (n == 0) return JX_HPKE_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  HpkeBufs b{n,
             (const uint8_t*)d_encs,
             (const uint8_t*)d_cts,
             d_ct_offsets,
             (const uint8_t*)d_aads,
             d_aad_offsets,
             (uint8_t*)d_out_plaintexts,
             (uint8_t*)d_out_ok};
  return launch_open_long(h, b);
}

int32_t jx_hpke_open_long_batch(jx_hpke* h, uint64_t n, const uint8_t* encs, const uint8_t* cts,
                                const uint64_t* ct_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                                uint8_t* out_plaintexts, uint8_t* out_ok) {
  if (!h || (n && (!encs || !cts || !ct_offsets || !aad_offsets || !out_plaintexts || !out_ok)))
    return JX_HPKE_E_INVALID;
  if (h->sender) return refuse_sender();
  if (n == 0) return JX_HPKE_OK;
  for (uint64_t i = 0; i < n; i++) {
    if (ct_offsets[i + 1] < ct_offsets[i] + 16 || aad_offsets[i + 1] < aad_offsets[i])
      return hfail(JX_HPKE_E_INVALID, "offsets must be non-decreasing and every ciphertext >= 16 bytes");
    if (ct_offsets[i + 1] - ct_offsets[i] >= (1ull << 32))
      return hfail(JX_HPKE_E_INVALID, "a ciphertext of 2^32 bytes or more is no report share");
  }
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  const uint64_t ct_bytes = ct_offsets[n], aad_bytes = aad_offsets[n], pt_bytes = ct_bytes - 16 * n;
  const uint64_t enc_bytes = n * hpke_enc_len(h->kem);
  const size_t o_enc = 0, o_ct = o_enc + jxi::align256(enc_bytes), o_aad = o_ct + jxi::align256(ct_bytes),
               o_pt = o_aad + jxi::align256(aad_bytes ? aad_bytes : 1), o_ok = o_pt + jxi::align256(pt_bytes ? pt_bytes : 1),
               o_co = o_ok + jxi::align256(n), o_ao = o_co + jxi::align256((n + 1) * 8), bytes = o_ao + jxi::align256((n + 1) * 8);
  jxi::Slab slab;
  const hipError_t ga = jxi::arena_get(h->arena, bytes, h->stream, true, true, slab);
  if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
  HCHK(ga);
  uint8_t* base = (uint8_t*)slab.p;
  int32_t rc = JX_HPKE_OK;
  do {
    if (hipMemcpyAsync(base + o_enc, encs, enc_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ct, cts, ct_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (aad_bytes && hipMemcpyAsync(base + o_aad, aads, aad_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        hipMemcpyAsync(base + o_co, ct_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ao, aad_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "host-to-device copy failed");
      break;
    }
    HpkeBufs b{n, base + o_enc, base + o_ct, (const uint64_t*)(base + o_co), base + o_aad, (const uint64_t*)(base + o_ao),
               base + o_pt, base + o_ok};
    if ((rc = launch_open_long(h, b)) != JX_HPKE_OK) break;
    if ((pt_bytes && hipMemcpyAsync(out_plaintexts, base + o_pt, pt_bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
        hipMemcpyAsync(out_ok, base + o_ok, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "device-to-host copy failed");
      break;
    }
  } while (0);
  jxi::arena_put(h->arena, slab, h->stream);  // reused after this stream's work
  return rc;
}

// ---- seal (jx_hpke_seal.hip)

// with h->mu held and the device set: the launches on the context's stream; the long form's context rows in a slab of
// the arena that goes back stream-ordered
static int32_t launch_seal(jx_hpke* h, SealArgs& a, bool long_form) {
  uint32_t cap = 0;
  jxi::hpke_registry(h->device, &a.keys, &cap);
  a.slot = h->slot;
  memcpy(a.zero_ist, h->cfg.zero_ist, 32);
  memcpy(a.zero_ost, h->cfg.zero_ost, 32);
  jxi::Slab slab;
  if (long_form) {
    const hipError_t ga = jxi::arena_get(h->arena, jxi::align256(a.n * SEAL_CTX_BYTES), h->stream, true, true, slab);
    if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
    HCHK(ga);
    a.ctx = slab.p;
  }
  const hipError_t st = launch_hpke_seal(a, long_form, h->stream);
  if (long_form) jxi::arena_put(h->arena, slab, h->stream);
  if (st != hipSuccess) return hfail(JX_HPKE_E_HIP, std::string("seal launch: ") + hipGetErrorString(st));
  return JX_HPKE_OK;
}

static int32_t seal_device(jx_hpke* h, uint64_t n, const void* d_sks, const void* d_pts, const uint64_t* d_pt_offsets,
                           const void* d_aads, const uint64_t* d_aad_offsets, void* d_out_encs, void* d_out_cts,
                           void* d_out_ok, bool long_form) {
  if (!h || (n && (!d_sks || !d_pt_offsets || !d_aad_offsets || !d_out_encs || !d_out_cts || !d_out_ok)))
    return JX_HPKE_E_INVALID;
  if (h->kem != HPKE_KEM_X25519_SHA256)
    return hfail(JX_HPKE_E_UNSUPPORTED, "sealing under KEM 0x0010 (P-256) is out of scope");
  if (n == 0) return JX_HPKE_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  SealArgs a{};
  a.n = n;
  a.sks = (const uint8_t*)d_sks;
  a.pts = (const uint8_t*)d_pts;
  a.pt_off = d_pt_offsets;
  a.aads = (const uint8_t*)d_aads;
  a.aad_off = d_aad_offsets;
  a.encs = (uint8_t*)d_out_encs;
  a.cts = (uint8_t*)d_out_cts;
  a.ok = (uint8_t*)d_out_ok;
  return launch_seal(h, a, long_form);
}

// Host buffers: one staging slab from the device's arena, as the opens take theirs.
static int32_t seal_host(jx_hpke* h, uint64_t n, const uint8_t* sks, const uint8_t* pts, const uint64_t* pt_offsets,
                         const uint8_t* aads, const uint64_t* aad_offsets, uint8_t* out_encs, uint8_t* out_cts,
                         uint8_t* out_ok, bool long_form) {
  if (!h || (n && (!sks || !pt_offsets || !aad_offsets || !out_encs || !out_cts || !out_ok))) return JX_HPKE_E_INVALID;
  if (h->kem != HPKE_KEM_X25519_SHA256)
    return hfail(JX_HPKE_E_UNSUPPORTED, "sealing under KEM 0x0010 (P-256) is out of scope");
  if (n == 0) return JX_HPKE_OK;
  for (uint64_t i = 0; i < n; i++) {
    if (pt_offsets[i + 1] < pt_offsets[i] || aad_offsets[i + 1] < aad_offsets[i])
      return hfail(JX_HPKE_E_INVALID, "offsets must be non-decreasing");
    if (pt_offsets[i + 1] - pt_offsets[i] >= (1ull << 32) - 16)
      return hfail(JX_HPKE_E_INVALID, "a plaintext of 2^32 - 16 bytes or more is no report share");
  }
  const uint64_t p0 = pt_offsets[0], pt_bytes = pt_offsets[n] - p0, a0 = aad_offsets[0], aad_bytes = aad_offsets[n] - a0;
  if ((pt_bytes && !pts) || (aad_bytes && !aads)) return JX_HPKE_E_INVALID;
  std::lock_guard<std::mutex> lk(h->mu);
  HCHK(hipSetDevice(h->device));
  if (const int32_t rc = ensure_stream(h)) return rc;
  const uint64_t ct_bytes = pt_bytes + 16 * n;
  const size_t o_sk = 0, o_pt = o_sk + jxi::align256(32 * n), o_aad = o_pt + jxi::align256(pt_bytes ? pt_bytes : 1),
               o_enc = o_aad + jxi::align256(aad_bytes ? aad_bytes : 1), o_ct = o_enc + jxi::align256(32 * n),
               o_ok = o_ct + jxi::align256(ct_bytes), o_po = o_ok + jxi::align256(n), o_ao = o_po + jxi::align256((n + 1) * 8),
               bytes = o_ao + jxi::align256((n + 1) * 8);
  jxi::Slab slab;
  const hipError_t ga = jxi::arena_get(h->arena, bytes, h->stream, true, true, slab);
  if (ga == hipErrorOutOfMemory) return hfail(JX_HPKE_E_NOMEM, "device allocation failed (arena)");
  HCHK(ga);
  uint8_t* base = (uint8_t*)slab.p;
  int32_t rc = JX_HPKE_OK;
  do {
    if (hipMemcpyAsync(base + o_sk, sks, 32 * n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (pt_bytes && hipMemcpyAsync(base + o_pt, pts + p0, pt_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        (aad_bytes && hipMemcpyAsync(base + o_aad, aads + a0, aad_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        hipMemcpyAsync(base + o_po, pt_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(base + o_ao, aad_offsets, (n + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "host-to-device copy failed");
      break;
    }
    SealArgs a{};
    a.n = n;
    a.sks = base + o_sk;
    a.pts = base + o_pt - p0;  // the kernels index by the caller's offsets
    a.pt_off = (const uint64_t*)(base + o_po);
    a.aads = base + o_aad - a0;
    a.aad_off = (const uint64_t*)(base + o_ao);
    a.encs = base + o_enc;
    a.cts = base + o_ct - p0;
    a.ok = base + o_ok;
    if ((rc = launch_seal(h, a, long_form)) != JX_HPKE_OK) break;
    if (hipMemcpyAsync(out_encs, base + o_enc, 32 * n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(out_cts + p0, base + o_ct, ct_bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(out_ok, base + o_ok, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      rc = hfail(JX_HPKE_E_HIP, "device-to-host copy failed");
      break;
    }
  } while (0);
  jxi::arena_put(h->arena, slab, h->stream);  // reused after this stream's work
  return rc;
}

int32_t jx_hpke_seal_batch(jx_hpke* h, uint64_t n, const uint8_t* ephemeral_sks, const uint8_t* pts,
                           const uint64_t* pt_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                           uint8_t* out_encs, uint8_t* out_cts, uint8_t* out_ok) {
  return seal_host(h, n, ephemeral_sks, pts, pt_offsets, aads, aad_offsets, out_encs, out_cts, out_ok, false);
}
int32_t jx_hpke_seal_long_batch(jx_hpke* h, uint64_t n, const uint8_t* ephemeral_sks, const uint8_t* pts,
                                const uint64_t* pt_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                                uint8_t* out_encs, uint8_t* out_cts, uint8_t* out_ok) {
  return seal_host(h, n, ephemeral_sks, pts, pt_offsets, aads, aad_offsets, out_encs, out_cts, out_ok, true);
}
int32_t jx_hpke_seal_batch_device(jx_hpke* h, uint64_t n, const void* d_ephemeral_sks, const void* d_pts,
                                  const uint64_t* d_pt_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                  void* d_out_encs, void* d_out_cts, void* d_out_ok) {
  return seal_device(h, n, d_ephemeral_sks, d_pts, d_pt_offsets, d_aads, d_aad_offsets, d_out_encs, d_out_cts, d_out_ok,
                     false);
}
int32_t jx_hpke_seal_long_batch_device(jx_hpke* h, uint64_t n, const void* d_ephemeral_sks, const void* d_pts,
                                       const uint64_t* d_pt_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                       void* d_out_encs, void* d_out_cts, void* d_out_ok) {
  return seal_device(h, n, d_ephemeral_sks, d_pts, d_pt_offsets, d_aads, d_aad_offsets, d_out_encs, d_out_cts, d_out_ok,
                     true);
}

const char* jx_hpke_last_error(const jx_hpke* h) {
  (void)h;
  return t_hpke_err.c_str();
}

}  // extern "C"
