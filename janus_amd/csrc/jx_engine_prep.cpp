// jx_engine_prep.cpp — the prepare calls that leave a resident batch: helper prepare (plaintext and sealed input
// shares), leader prepare_init and prepare_next (jx_leader_prep_finish_*).
#include <string>
#include <vector>

#include "jx_engine_internal.h"

using namespace jx;
using namespace jxi;

// measurement staging for a helper prepare whose outputs go to a batch (Histogram writes its
// measurement share, which is its output share, straight into the batch)
static uint32_t helper_meas_flag(const Cfg& c) { return outs_alias_meas(c) ? 0u : SG_MEAS; }

// The batch a prepare call has just made: released when the call leaves without keeping it. Declared before the
// call's Stage, so that on a failure the staging goes back to the arena before the batch does.
namespace {
struct NewBatch {
  jx_engine* e;
  uint64_t id = 0;
  Batch* B = nullptr;
  bool kept = false;
  explicit NewBatch(jx_engine* e) : e(e) {}
  NewBatch(const NewBatch&) = delete;
  NewBatch& operator=(const NewBatch&) = delete;
  ~NewBatch() {
    auto it = id && !kept ? e->batches.find(id) : e->batches.end();
    if (it != e->batches.end()) batch_free(e, it);
  }
  int32_t make(uint64_t n, bool leader) { return batch_new(e, n, leader, &id, &B); }
  uint64_t keep() {
    kept = true;
    return id;
  }
};
}  // namespace

static int32_t copy_out_shares(jx_engine* e, const uint4* outs, uint64_t n, uint8_t* dst) {
  const Cfg& c = e->cfg;
  Scratch tmp;
  int32_t rc = scratch_get(e, n * c.out_len * c.fb, tmp);
  if (rc) return rc;
  HIPCHK(e, launch_transpose_out(c, outs, n, tmp.p(), e->stream));
  HIPCHK(e, hipMemcpyAsync(dst, tmp.p(), n * c.out_len * c.fb, hipMemcpyDeviceToHost, e->stream));
  return JX_OK;
}

// jx_helper_prep_encrypted_batch2 and the two sealed fused calls
int32_t jxi::enc_job_check(jx_engine* e, uint64_t n, const uint64_t* times, const uint8_t* task_id,
                           jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index, const uint8_t* encs,
                           const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                           uint32_t flags, EncJob& job) {
  if (nkeypairs > JX_ENC_MAX_KEYPAIRS || (nkeypairs && !keypairs) || (flags & ~JX_ENC_REQUIRE_TASKPROV))
    return fail(e, JX_E_INVALID, "encrypted prepare: at most JX_ENC_MAX_KEYPAIRS keypairs, flags JX_ENC_*");
  for (uint32_t k = 0; k < nkeypairs; k++) {
    if (!keypairs[k] || hpke_device(keypairs[k]) != e->device)
      return fail(e, JX_E_INVALID, "encrypted prepare: every keypair must be an HPKE context on the engine's device");
    if (hpke_is_sender(keypairs[k]))
      return fail(e, JX_E_INVALID, "encrypted prepare: a sender context (jx_hpke_create_sender) holds no private key");
  }
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t k0 = key_index[2 * i], k1 = key_index[2 * i + 1];
    if ((k0 >= nkeypairs && k0 != JX_KEY_NONE && k0 != JX_KEY_MALFORMED) || (k1 >= nkeypairs && k1 != JX_KEY_NONE) ||
        payload_offsets[i + 1] < payload_offsets[i] || payload_offsets[i + 1] - payload_offsets[i] > 0xFFFFFFFFull)
      return fail(e, JX_E_INVALID, "encrypted prepare: key_index out of range or payload offsets decreasing");
  }
  if (n && payload_offsets[n] > payload_offsets[0] && !payloads) return JX_E_INVALID;
  for (uint64_t i = 0; enc_offsets && i < n; i++) {
    if (enc_offsets[i + 1] < enc_offsets[i])
      return fail(e, JX_E_INVALID, "encrypted prepare: encapsulated-key offsets decreasing");
    job.enc65 += enc_offsets[i + 1] - enc_offsets[i] == 65;
  }
  job.enc_offsets = enc_offsets;
  job.times = times;
  job.task_id = task_id;
  job.keypairs = keypairs;
  job.nkeys = nkeypairs;
  job.key_index = key_index;
  job.encs = encs;
  job.payloads = payloads;
  job.payload_offsets = payload_offsets;
  job.flags = flags;
  return JX_OK;
}

extern "C" {

static int32_t helper_prep_batch_locked(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* ps,
                                        const uint8_t* his, const uint8_t* lps, uint8_t* out_msgs, uint8_t* out_verdicts,
                                        uint8_t* out_shares, Batch* B) {
  const Cfg& c = e->cfg;
  Stage st;
  int32_t rc = stage_acquire(e, n, SG_IN | SG_HIN | helper_meas_flag(c) | SG_PREP, st);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
  if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(e->d_ps, ps, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_his, his, n * c.his_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_lps, lps, n * c.lps_bytes, hipMemcpyHostToDevice, e->stream));
  rc = prep_core(e, n, B->nonces, e->d_ps, e->d_his, e->d_lps, B->verdicts, B->msgs, B->outs);
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
  if (out_msgs && c.jr_len)
    HIPCHK(e, hipMemcpyAsync(out_msgs, B->msgs, n * c.seed, hipMemcpyDeviceToHost, e->stream));
  if (out_shares) {
    rc = copy_out_shares(e, B->outs, n, out_shares);
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return drain_timing(e);
}

// Coalesced prepares take jobs up to a quarter of a launch (larger ones fill the device by themselves) that fit
// one of the coalescer's lanes for their role (a leader's explicit input shares can be MBs per report); the
// rest take the direct path.
static bool coalescible(const jx_engine* e, uint64_t n, bool leader = false, bool encrypted = false,
                        uint64_t ct_bytes = 0) {
  return e->coalesce && n > 0 && n <= e->default_chunk / 4 && coalescer_accepts(e, leader, n, encrypted, ct_bytes);
}

int32_t jx_helper_prep_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                             const uint8_t* helper_input_shares, const uint8_t* leader_prep_shares,
                             uint8_t* out_prep_msgs, uint8_t* out_verdicts, uint8_t* out_output_shares,
                             uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !helper_input_shares || !leader_prep_shares || !out_verdicts))) return JX_E_INVALID;
  if (n && e->cfg.ps_bytes && !public_shares) return JX_E_INVALID;
  if (!out_output_shares && coalescible(e, n)) {
    thread_error().clear();
    return coalesced_helper_prep(e, n, nonces, public_shares, helper_input_shares, leader_prep_shares, out_prep_msgs,
                                 out_verdicts, out_batch_id);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  NewBatch nb(e);
  int32_t rc = nb.make(n, false);
  if (rc) return rc;
  if (n) {
    rc = helper_prep_batch_locked(e, n, nonces, public_shares, helper_input_shares, leader_prep_shares, out_prep_msgs,
                                  out_verdicts, out_output_shares, nb.B);
    if (rc) return rc;
  }
  const uint64_t id = nb.keep();
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
}

int32_t jx_helper_prep_encrypted_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                       const uint8_t* public_shares, const uint8_t task_id[32],
                                       jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                       const uint8_t* encs, const uint8_t* payloads, const uint64_t* payload_offsets,
                                       uint32_t flags, const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs,
                                       uint8_t* out_verdicts, uint8_t* out_open_status, uint64_t* out_batch_id) {
  // the case of the call below in which every encapsulated key is 32 bytes
  return jx_helper_prep_encrypted_batch2(e, n, nonces, times, public_shares, task_id, keypairs, nkeypairs, key_index, encs,
                                         nullptr, payloads, payload_offsets, flags, leader_prep_shares, out_prep_msgs,
                                         out_verdicts, out_open_status, out_batch_id);
}

int32_t jx_helper_prep_encrypted_batch2(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                        const uint8_t* public_shares, const uint8_t task_id[32],
                                        jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                        const uint8_t* encs, const uint64_t* enc_offsets, const uint8_t* payloads,
                                        const uint64_t* payload_offsets, uint32_t flags,
                                        const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs, uint8_t* out_verdicts,
                                        uint8_t* out_open_status, uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !times || !task_id || !key_index || !encs || !payload_offsets || !leader_prep_shares ||
                   !out_verdicts)))
    return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !public_shares) return JX_E_INVALID;
  EncJob job;
  if (const int32_t rc = enc_job_check(e, n, times, task_id, keypairs, nkeypairs, key_index, encs, enc_offsets, payloads,
                                       payload_offsets, flags, job))
    return rc;
  const uint64_t ct = n ? job.ct_bytes(n) : 0;
  if (coalescible(e, n, false, true, ct)) {
    thread_error().clear();
    return coalesced_helper_prep(e, n, nonces, public_shares, nullptr, leader_prep_shares, out_prep_msgs, out_verdicts,
                                 out_batch_id, &job, out_open_status);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  NewBatch nb(e);
  int32_t rc = nb.make(n, false);
  if (rc) return rc;
  if (n) {
    Batch* const B = nb.B;
    // the job's rows in pageable host memory, uploaded with its inputs; they name their keypairs by their slots
    // of the device's key registry, where the keys have been since the contexts were created
    std::vector<EncRow> rows(n);
    bool suites = false;
    for (uint32_t k = 0; k < nkeypairs; k++) suites = suites || !hpke_default_suite(keypairs[k]);
    const HpkeKeyRow* reg = nullptr;
    uint32_t reg_cap = 0;
    hpke_registry(e->device, &reg, &reg_cap);
    // the 65-byte encapsulated keys follow the ciphertexts in the launch's ciphertext region
    std::vector<uint8_t> enc65(job.enc65 ? 65 * job.enc65 : 1);
    const uint64_t pb = job.payload_bytes(n), n65 = fill_enc_rows(job, n, rows.data(), 0, enc65.data());
    Stage st;
    rc = stage_acquire(e, n, SG_IN | SG_HIN | SG_ENC | helper_meas_flag(c) | SG_PREP, st, true, ct);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes) HIPCHK(e, hipMemcpyAsync(e->d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_lps, leader_prep_shares, n * c.lps_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_encrows, rows.data(), n * sizeof(EncRow), hipMemcpyHostToDevice, e->stream));
    if (pb) HIPCHK(e, hipMemcpyAsync(e->d_ct, payloads + payload_offsets[0], pb, hipMemcpyHostToDevice, e->stream));
    if (n65) HIPCHK(e, hipMemcpyAsync(e->d_ct + pb, enc65.data(), 65 * n65, hipMemcpyHostToDevice, e->stream));
    HpkeRowsArgs ha{n, e->d_encrows, e->d_ct, e->d_pt, reg, reg ? reg_cap : 0, B->nonces, e->d_ps, c.ps_bytes,
                    e->d_his, c.his_bytes, e->d_status};
    HIPCHK(e, launch_hpke_rows(ha, suites, n65 != 0, e->stream));
    rc = prep_core(e, n, B->nonces, e->d_ps, e->d_his, e->d_lps, B->verdicts, B->msgs, B->outs);
    if (rc) return rc;
    HIPCHK(e, launch_open_mask(e->d_status, B->verdicts, n, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
    if (out_prep_msgs && c.jr_len)
      HIPCHK(e, hipMemcpyAsync(out_prep_msgs, B->msgs, n * c.seed, hipMemcpyDeviceToHost, e->stream));
    if (out_open_status) HIPCHK(e, hipMemcpyAsync(out_open_status, e->d_status, n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // the pageable rows and the caller's outputs
    rc = drain_timing(e);
    if (rc) return rc;
  }
  const uint64_t id = nb.keep();
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
}

int32_t jx_engine_leader_sizes(const jx_engine* e, uint32_t* leader_input_share) {
  if (!e) return JX_E_INVALID;
  if (leader_input_share) *leader_input_share = e->cfg.lis_bytes;
  return JX_OK;
}

int32_t jx_leader_prep_init_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                  const uint8_t* leader_input_shares, uint8_t* out_prep_shares,
                                  uint8_t* out_verdicts, uint64_t* out_batch_id) {
  if (out_batch_id) *out_batch_id = 0;
  if (!e || (n && (!nonces || !leader_input_shares || !out_prep_shares || !out_verdicts))) return JX_E_INVALID;
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !public_shares) return JX_E_INVALID;
  if (coalescible(e, n, true)) {
    thread_error().clear();
    return coalesced_leader_init(e, n, nonces, public_shares, leader_input_shares, out_prep_shares, out_verdicts,
                                 out_batch_id);
  }
  LOCK(e);
  HIPCHK(e, hipSetDevice(e->device));
  NewBatch nb(e);
  int32_t rc = nb.make(n, true);
  if (rc) return rc;
  if (n) {
    Batch* const B = nb.B;
    Stage st;
    rc = stage_acquire(e, n, SG_IN | SG_LEAD | SG_PREP | (leader_inplace(c) ? 0u : SG_MEAS), st);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(B->nonces, nonces, n * 16, hipMemcpyHostToDevice, e->stream));
    if (c.ps_bytes)
      HIPCHK(e, hipMemcpyAsync(e->d_ps, public_shares, n * c.ps_bytes, hipMemcpyHostToDevice, e->stream));
    if (e->lis_stride == c.lis_bytes)
      HIPCHK(e, hipMemcpyAsync(e->d_lis, leader_input_shares, n * c.lis_bytes, hipMemcpyHostToDevice, e->stream));
    else  // padded rows (aligned in-place reads of the measurement share)
      HIPCHK(e, hipMemcpy2DAsync(e->d_lis, e->lis_stride, leader_input_shares, c.lis_bytes, c.lis_bytes, n,
                                 hipMemcpyHostToDevice, e->stream));
    rc = prep_core(e, n, B->nonces, e->d_ps, nullptr, nullptr, B->verdicts, B->msgs, B->outs, e->d_lis, e->d_lps_out,
                   e->lis_stride);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_prep_shares, e->d_lps_out, n * c.lps_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    rc = drain_timing(e);
    if (rc) return rc;
  }
  const uint64_t id = nb.keep();
  if (out_batch_id) *out_batch_id = id;
  return JX_OK;
}

int32_t jx_leader_prep_init_device_ex(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                      const void* d_leader_input_shares, uint64_t lis_stride, void* d_out_prep_shares,
                                      void* d_out_verdicts, uint64_t* out_batch_id) {
  if (!out_batch_id) return JX_E_INVALID;
  *out_batch_id = 0;
  if (!e || (n && (!d_nonces || !d_leader_input_shares || !d_out_prep_shares))) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  if (n && c.ps_bytes && !d_public_shares) return JX_E_INVALID;
  if (lis_stride == 0) lis_stride = c.lis_bytes;
  if (lis_stride < c.lis_bytes || (lis_stride & 15u))
    return fail(e, JX_E_INVALID, "leader init: the row stride must be >= the leader input share and a multiple of 16");
  // the in-place FLP kernels read the measurement share in 16-byte vectors (header contract)
  if (n && leader_inplace(c) && (reinterpret_cast<uintptr_t>(d_leader_input_shares) & 15u))
    return fail(e, JX_E_INVALID, "leader init: d_leader_input_shares must be 16-byte aligned");
  HIPCHK(e, hipSetDevice(e->device));
  NewBatch nb(e);
  int32_t rc = nb.make(n, true);
  if (rc) return rc;
  if (n) {
    Batch* const B = nb.B;
    Stage st;
    rc = stage_acquire(e, n, SG_PREP | (leader_inplace(c) ? 0u : SG_MEAS), st);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(B->nonces, d_nonces, n * 16, hipMemcpyDeviceToDevice, e->stream));
    rc = prep_core(e, n, B->nonces, (const uint8_t*)d_public_shares, nullptr, nullptr, B->verdicts, B->msgs, B->outs,
                   (const uint8_t*)d_leader_input_shares, (uint8_t*)d_out_prep_shares, lis_stride);
    if (rc) return rc;
    if (d_out_verdicts) HIPCHK(e, hipMemcpyAsync(d_out_verdicts, B->verdicts, n, hipMemcpyDeviceToDevice, e->stream));
  }
  *out_batch_id = nb.keep();
  return JX_OK;
}

int32_t jx_leader_prep_init_device(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                   const void* d_leader_input_shares, void* d_out_prep_shares, void* d_out_verdicts,
                                   uint64_t* out_batch_id) {
  return jx_leader_prep_init_device_ex(e, n, d_nonces, d_public_shares, d_leader_input_shares, 0, d_out_prep_shares,
                                       d_out_verdicts, out_batch_id);
}

static int32_t leader_batch(jx_engine* e, uint64_t batch_id, uint64_t n, Batch** B) {
  int32_t rc = find_batch(e, batch_id, n, "leader finish", B);
  if (rc) return rc;
  if (!(*B)->leader) return fail(e, JX_E_STATE, "leader finish: the batch is a helper batch");
  if ((*B)->finished) return fail(e, JX_E_STATE, "leader finish: the batch was already finished");
  return JX_OK;
}

int32_t jx_leader_prep_finish_batch(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* prep_msgs,
                                    uint8_t* out_verdicts, uint8_t* out_output_shares) {
  if (!e || (n && !out_verdicts)) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  Batch* B = nullptr;
  int32_t rc = leader_batch(e, batch_id, n, &B);
  if (rc) return rc;
  if (n && c.jr_len && !prep_msgs) return JX_E_INVALID;
  if (n == 0) {
    B->finished = true;
    return JX_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  Stage st;
  if (c.jr_len) {
    rc = stage_acquire(e, n, SG_LMSG, st);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_in_msgs, prep_msgs, n * c.seed, hipMemcpyHostToDevice, e->stream));
    Bufs b{};
    b.n = n;
    b.verdicts = B->verdicts;
    b.msgs = B->msgs;
    HIPCHK(e, launch_leader_finish(c, b, e->d_in_msgs, nullptr, e->stream));
  }
  // finished once prepare_next is queued: a failure above leaves the batch finishable (or releasable)
  B->finished = true;
  HIPCHK(e, hipMemcpyAsync(out_verdicts, B->verdicts, n, hipMemcpyDeviceToHost, e->stream));
  if (out_output_shares) {
    rc = copy_out_shares(e, B->outs, n, out_output_shares);
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return JX_OK;
}

int32_t jx_leader_prep_finish_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_prep_msgs,
                                     const void* d_peer_verdicts, void* d_out_verdicts) {
  if (!e) return JX_E_INVALID;
  LOCK(e);
  const Cfg& c = e->cfg;
  Batch* B = nullptr;
  int32_t rc = leader_batch(e, batch_id, n, &B);
  if (rc) return rc;
  if (n && c.jr_len && !d_prep_msgs) return JX_E_INVALID;
  if (n == 0) {
    B->finished = true;
    return JX_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  Bufs b{};
  b.n = n;
  b.verdicts = B->verdicts;
  b.msgs = B->msgs;
  HIPCHK(e, launch_leader_finish(c, b, (const uint8_t*)d_prep_msgs, (const uint8_t*)d_peer_verdicts, e->stream));
  B->finished = true;
  if (d_out_verdicts) HIPCHK(e, hipMemcpyAsync(d_out_verdicts, B->verdicts, n, hipMemcpyDeviceToDevice, e->stream));
  return JX_OK;
}

}  // extern "C"
