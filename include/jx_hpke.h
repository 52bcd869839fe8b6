/*
 * jx_hpke.h — C ABI of batched HPKE open, and seal, on the MI355X.
 *
 * Replaces the per-report HPKE open of the helper's aggregate-init loop,
 *   /root/reference/aggregator/src/aggregator.rs:1772-1832
 *     hpke::open(&hpke_keypair, &HpkeApplicationInfo::new(&Label::InputShare, &Role::Client,
 *                &Role::Helper), prepare_init.report_share().encrypted_input_share(), &aad)
 * (core/src/hpke.rs:200-230): RFC 9180 base mode, DHKEM(X25519, HKDF-SHA256) (0x0020) or DHKEM(P-256,
 * HKDF-SHA256) (0x0010) with any of HKDF-SHA256 / -SHA384 / -SHA512 and AES-128-GCM / AES-256-GCM /
 * ChaCha20Poly1305: the 18 suites the reference opens (jx_hpke_create_key; jx_hpke_create_suite for the X25519
 * ones; the default is X25519, HKDF-SHA256 (0x0001), AES-128-GCM (0x0001), docs/samples/tasks.yaml:54-58). Once prepare
 * runs on the GPU this is the next per-report CPU cost (X25519 + key schedule + AEAD per report).
 *
 * Conventions as in jx_prio3.h: int32 status (0 = OK), caller-owned buffers, one context per
 * (keypair, application info, GPU). Calls on one context from several threads are serialized (a mutex per
 * context); jx_hpke_last_error returns the calling thread's last failure. The host-buffer open takes its
 * device buffers from the device's arena (shared with the prepare engines) and synchronizes only the
 * context's stream. jx_helper_prep_encrypted_batch (jx_prio3.h) opens inside the prepare launch instead.
 *
 * The key registry. Every device has one registry of keypairs: a fixed array of JX_HPKE_MAX_CONTEXTS (16,384) rows
 * of device memory (3.8 MB, allocated at the first context creation on the device, outside the arena, and never
 * moved or reallocated). Creating a context takes a free row and writes the keypair into it, synchronously, before
 * the call returns; jx_hpke_destroy wipes the row and frees it for the next context. So a row's lifetime is its
 * context's lifetime, and the prepare launches of jx_helper_prep_encrypted_batch[2] read the keys from there: a
 * launch carries no key table, and jobs of any number of tasks, each with its own keypair, share one launch. A
 * context passed to a call is borrowed for the duration of that call, as everywhere in this ABI: destroy it only
 * when no call that was given it is still running. With JX_HPKE_MAX_CONTEXTS contexts alive on a device the next
 * creation returns JX_HPKE_E_NOMEM, with the reason in jx_hpke_last_error. A context costs its registry row and a
 * few hundred bytes of host memory; its stream is created at its first jx_hpke_open_batch[_device] or
 * jx_hpke_stream, so a context that is only ever passed to a prepare call never has one.
 *
 * No branch and no address of the X25519 ladder or of the P-256 scalar multiplication depends on the private key
 * (masked selects).
 *  - encs:        n x jx_hpke_enc_len(h) bytes (HpkeCiphertext.encapsulated_key: 32 under X25519, 65 under
 *                 P-256, the uncompressed SEC 1 point)
 *  - cts:         ciphertexts (payload || 16-byte tag) back to back; ct_offsets[n + 1], ciphertext i
 *                 is [ct_offsets[i], ct_offsets[i+1]) and at least 16 bytes
 *  - aads:        associated data back to back (the encoded InputShareAad), aad_offsets[n + 1]
 *  - plaintexts:  plaintext i (ct length - 16 bytes) at offset ct_offsets[i] - 16 * i
 *  - ok:          n bytes, 1 = opened, 0 = HpkeDecryptError (bad tag, bad length, all-zero DH, under P-256 an
 *                 encapsulated key that is no point of the curve)
 */
#ifndef JX_HPKE_H
#define JX_HPKE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JX_HPKE_OK 0
#define JX_HPKE_E_INVALID (-1)
#define JX_HPKE_E_UNSUPPORTED (-2) /* a KEM, KDF or AEAD id outside the suites below */
#define JX_HPKE_E_HIP (-3)
#define JX_HPKE_E_NOMEM (-4) /* device memory, or JX_HPKE_MAX_CONTEXTS contexts alive on the device */
#define JX_HPKE_E_NODEVICE (-6)

#define JX_HPKE_MAX_CONTEXTS 16384 /* live contexts per device: the rows of its key registry */

typedef struct jx_hpke jx_hpke;

/* sk/pk: the recipient's X25519 key pair (SerializePrivateKey / public key, 32 bytes each);
 * info: the HPKE application info (Janus: "dap-09 input share" || sender role || recipient role). */
int32_t jx_hpke_create(const uint8_t sk[32], const uint8_t pk[32], const uint8_t* info, uint32_t info_len,
                       int32_t device, jx_hpke** out);
/* The same for the suite of the keypair's HpkeConfig (messages/src/lib.rs:768-846: kem_id, kdf_id, aead_id):
 * KEM 0x0020 DHKEM(X25519, HKDF-SHA256); KDF 0x0001 HKDF-SHA256, 0x0002 HKDF-SHA384, 0x0003 HKDF-SHA512; AEAD
 * 0x0001 AES-128-GCM, 0x0002 AES-256-GCM, 0x0003 ChaCha20Poly1305: nine suites. Any other id returns
 * JX_HPKE_E_UNSUPPORTED, with the reason in jx_hpke_last_error; that includes the P-256 KEM 0x0010, whose public
 * key does not fit this call's 32 bytes (jx_hpke_create_key). jx_hpke_create is the (0x0020, 0x0001, 0x0001)
 * case. Contexts of any suites may be passed together to jx_helper_prep_encrypted_batch[2]. */
int32_t jx_hpke_create_suite(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t sk[32],
                             const uint8_t pk[32], const uint8_t* info, uint32_t info_len, int32_t device,
                             jx_hpke** out);
/* A keypair of either KEM, with the lengths of its keys. KEM 0x0020: sk_len = pk_len = 32, exactly
 * jx_hpke_create_suite. KEM 0x0010, DHKEM(P-256, HKDF-SHA256): sk is the private key as 32 big-endian bytes
 * (SerializePrivateKey), pk the public key as the 65-byte uncompressed SEC 1 point (SerializePublicKey);
 * JX_HPKE_E_INVALID, with the reason in jx_hpke_last_error, unless sk_len == 32, 1 <= sk <= n - 1, pk_len == 65, pk is
 * a point of the curve and pk == sk * G (computed on the host by the kernels' own code). Ids are checked first
 * (JX_HPKE_E_UNSUPPORTED), then the keypair, then the device. */
int32_t jx_hpke_create_key(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t* sk, uint32_t sk_len,
                           const uint8_t* pk, uint32_t pk_len, const uint8_t* info, uint32_t info_len, int32_t device,
                           jx_hpke** out);
/* A SENDER context: the recipient's public key alone, which is all a client has. It seals (below) and cannot open: its
 * private-key words in the key registry are zero, and every call that opens refuses it before anything is queued
 * (jx_hpke_open_*: JX_HPKE_E_INVALID; jx_helper_prep_encrypted_batch[2], jx_helper_prep_aggregate_encrypted[_device]
 * and jx_leader_upload_open_* of jx_prio3.h: JX_E_INVALID). It takes a key-registry row like any other context. KEM
 * 0x0020 (X25519, pk_len 32) with KDF 1..3 and AEAD 1..3; sealing under the P-256 KEM 0x0010 is out of scope and
 * returns JX_HPKE_E_UNSUPPORTED, with the reason in jx_hpke_last_error. */
int32_t jx_hpke_create_sender(uint32_t kem_id, uint32_t kdf_id, uint32_t aead_id, const uint8_t* pk, uint32_t pk_len,
                              const uint8_t* info, uint32_t info_len, int32_t device, jx_hpke** out);
/* The suite a context was created with (any of the three may be NULL). */
int32_t jx_hpke_suite(const jx_hpke* h, uint32_t* kem_id, uint32_t* kdf_id, uint32_t* aead_id);
/* The length of an encapsulated key under the context's KEM: 32 (X25519) or 65 (P-256); 0 for NULL. */
int32_t jx_hpke_enc_len(const jx_hpke* h);
void jx_hpke_destroy(jx_hpke* h);

/* Host buffers. */
int32_t jx_hpke_open_batch(jx_hpke* h, uint64_t n, const uint8_t* encs, const uint8_t* cts,
                           const uint64_t* ct_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                           uint8_t* out_plaintexts, uint8_t* out_ok);
/* Device buffers (asynchronous on the context's stream; e.g. chain into jx_helper_prep_*). */
int32_t jx_hpke_open_batch_device(jx_hpke* h, uint64_t n, const void* d_encs, const void* d_cts,
                                  const uint64_t* d_ct_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                  void* d_out_plaintexts, void* d_out_ok);
/* The same two calls for LONG payloads, such as a leader input share (the whole measurement and proof share: 135 KB
 * for Prio3SumVec 8x1000/88): the arguments and the contract of jx_hpke_open_batch[_device], and the same bytes in
 * out_plaintexts (for every report that opens) and out_ok. The calls above open one report per lane, which suits
 * the helper's 48-byte shares; these run the decapsulation and key schedule one report per lane, then the AEAD one
 * wave per report (AES-GCM: GHASH and CTR split over the 64 lanes; ChaCha20Poly1305: the same
 * serial code in one lane of the wave, so no faster than above). The recipient key is read from the device's key
 * registry; a launch uploads no key material. Scratch (64 bytes per report) comes from the device's arena. A
 * ciphertext of 2^32 bytes or more is refused with JX_HPKE_E_INVALID before any launch by the host-buffer call,
 * which sees the offsets; the device-buffer call cannot read them, and its kernel fails that report (ok = 0). */
int32_t jx_hpke_open_long_batch(jx_hpke* h, uint64_t n, const uint8_t* encs, const uint8_t* cts,
                                const uint64_t* ct_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                                uint8_t* out_plaintexts, uint8_t* out_ok);
int32_t jx_hpke_open_long_batch_device(jx_hpke* h, uint64_t n, const void* d_encs, const void* d_cts,
                                       const uint64_t* d_ct_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                       void* d_out_plaintexts, void* d_out_ok);
/* ---- Seal: RFC 9180 base-mode single-shot seal (sequence number 0, nonce = base_nonce; core/src/hpke.rs:167), the
 * mirror of the open calls above, under any X25519 context: a sender context, or a recipient context (its public key
 * is what the seal uses). A P-256 context returns JX_HPKE_E_UNSUPPORTED.
 *  - ephemeral_sks: n x 32, the ephemeral X25519 private keys, one per seal, clamped by the engine. The engine draws
 *                   no randomness: the caller owns the CSPRNG. They are secrets: on the device they pass through the
 *                   masked-swap ladder only.
 *  - pts:           plaintexts back to back, pt_offsets[n + 1]; aads / aad_offsets[n + 1] as for the opens
 *  - out_encs:      n x 32, enc = X25519(skE, 9)
 *  - out_cts:       ciphertext i (plaintext length + 16 bytes) at offset pt_offsets[i] + 16 i
 *  - out_ok:        n bytes, 1 = sealed, 0 = X25519(skE, pkR) was all zero (a low-order recipient key): that seal's
 *                   enc and ciphertext are zeros
 * jx_hpke_seal_batch is the short form, one seal per lane pair, for payloads such as the helper's 54-byte plaintext;
 * jx_hpke_seal_long_batch spreads the AEAD of each seal over a wave and gives the same bytes. The
 * host forms check the offsets (decreasing offsets, or a plaintext of 2^32 - 16 bytes or more: JX_HPKE_E_INVALID); the
 * device forms cannot read them, and their kernels fail such a seal (ok = 0, nothing written). n == 0 is
 * JX_HPKE_OK. The device forms are asynchronous on the context's stream. */
int32_t jx_hpke_seal_batch(jx_hpke* h, uint64_t n, const uint8_t* ephemeral_sks, const uint8_t* pts,
                           const uint64_t* pt_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                           uint8_t* out_encs, uint8_t* out_cts, uint8_t* out_ok);
int32_t jx_hpke_seal_batch_device(jx_hpke* h, uint64_t n, const void* d_ephemeral_sks, const void* d_pts,
                                  const uint64_t* d_pt_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                  void* d_out_encs, void* d_out_cts, void* d_out_ok);
int32_t jx_hpke_seal_long_batch(jx_hpke* h, uint64_t n, const uint8_t* ephemeral_sks, const uint8_t* pts,
                                const uint64_t* pt_offsets, const uint8_t* aads, const uint64_t* aad_offsets,
                                uint8_t* out_encs, uint8_t* out_cts, uint8_t* out_ok);
int32_t jx_hpke_seal_long_batch_device(jx_hpke* h, uint64_t n, const void* d_ephemeral_sks, const void* d_pts,
                                       const uint64_t* d_pt_offsets, const void* d_aads, const uint64_t* d_aad_offsets,
                                       void* d_out_encs, void* d_out_cts, void* d_out_ok);
/* The context's stream (a hipStream_t), on which jx_hpke_open_batch_device enqueues: for events around an open,
 * or to order other work after it. Created by the first call that needs it (this one included). */
int32_t jx_hpke_stream(const jx_hpke* h, void** out_stream);
const char* jx_hpke_last_error(const jx_hpke* h);

#ifdef __cplusplus
}
#endif
#endif /* JX_HPKE_H */
