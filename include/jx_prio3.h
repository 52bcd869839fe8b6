/*
 * jx_prio3.h — C ABI of the MI355X batched Prio3 helper prepare + aggregate engine.
 *
 * Drop-in boundary. In Janus the hot path is reached through the
 * `prio::vdaf::Aggregator<16, 16>` trait + `PingPongTopology`, called once per
 * report from the helper's aggregate-init loop:
 *   /root/reference/aggregator/src/aggregator.rs:1945-1967
 *     vdaf.helper_initialized(verify_key, agg_param, nonce = report_id,
 *                             public_share, input_share, leader_msg).evaluate(vdaf)
 * and the per-report accumulation
 *   /root/reference/aggregator/src/aggregator/aggregation_job_writer.rs:608-708
 *   /root/reference/aggregator_core/src/datastore/models.rs:1275-1330 (merged_with)
 * plus the shard merge of compute_aggregate_share
 *   /root/reference/aggregator/src/aggregator/aggregate_share.rs:55-96.
 * This ABI replaces that loop body with one call per batch. HPKE-open, plaintext
 * decode, replay / collected-batch checks and the datastore stay on the host.
 * Further entry points cover the rest of a report's path on the device: sealed input shares opened inside the
 * prepare calls, the leader's upload open, the client's shard and seal, the aggregate-init request and response as
 * wire bytes at both ends, and the upload message itself: jx_report_encode* writes the client's Report bodies,
 * jx_upload_decode* cuts the leader's uploads into the arrays the upload open and the request encode read.
 *
 * Conventions:
 *  - Every function returns int32 status: 0 = OK, < 0 = engine error (JX_E_*).
 *    Per-report preparation failures are NOT errors: they are verdict bytes.
 *  - The caller owns every host buffer; it is borrowed for the duration of the call.
 *  - An engine is one task's handle on one device (VdafOps per task, aggregator/src/aggregator.rs:
 *    1156-1183): its verify key, its resident batches, its running aggregations and one HIP stream.
 *    It holds no launch staging between calls: staging is checked out of the device's arena per call
 *    and handed back stream-ordered, and resident batches come from the same arena (jx_engine_memory),
 *    so any number of engines (tasks) share one GPU's HBM. Every entry point takes the engine's mutex
 *    for the duration of the call, so one engine can serve concurrent aggregation jobs from several
 *    host threads; the device work of the calls is serialized on the engine stream. What a job keeps
 *    between calls (its prepared reports) is a batch handle. (A helper launch past one lane-split K1
 *    wave per SIMD, while no other engine on the device runs a large K1 launch, puts part of its K1 on
 *    a second stream of the engine, forked from and joined back into the engine stream by events: the
 *    ordering below is unchanged.)
 *  - Coalesced prepares (jx_engine_coalesce): with coalescing on, jx_helper_prep_batch and
 *    jx_leader_prep_init_batch of jobs up to a quarter of a launch join the device's next shared launch
 *    with the concurrent jobs of every coalescing engine of the same Prio3 instance on the device (each
 *    report with its own engine's verify key), and wait for it without holding the engine mutex. Results,
 *    batches and errors are per job, exactly as without coalescing.
 *  - Host-buffer entry points are synchronous. Device-pointer entry points (*_device) are
 *    asynchronous on the engine stream, a NON-BLOCKING stream that orders itself after nothing:
 *    PRODUCER ORDERING is the caller's. Before a *_device call whose inputs were written by work
 *    queued on another stream, call jx_engine_wait_stream(e, producer) (or jx_engine_wait_event on an
 *    event recorded after the producer's writes); after it, jx_engine_join_stream(e, consumer) (or
 *    jx_engine_record_event + a wait) before the consumer reads the outputs or reuses the inputs.
 *    Neither blocks the host. Creating an engine synchronizes only the engine stream.
 *  - jx_last_error returns the message of the calling thread's last failed call.
 *  - Byte layouts are the DAP/VDAF encodings (fixed stride per report):
 *      nonces               n x 16   (report ids; VDAF nonce, aggregator.rs:1951)
 *      public_shares        n x PS   (Prio3PublicShare: joint-rand parts, 0 or 32 B)
 *      helper_input_shares  n x HIS  (k_meas || k_proofs || [k_blind])
 *      leader_prep_shares   n x LPS  (the prep_share inside PingPongMessage::Initialize)
 *      prep_msgs            n x PM   (prep_msg inside PingPongMessage::Finish; 0 or 16 B)
 *      output shares        n x OUT x FB, aggregate shares OUT x FB, field elements LE.
 */
#ifndef JX_PRIO3_H
#define JX_PRIO3_H

#include <stdint.h>

#include "jx_hpke.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes */
#define JX_OK 0
#define JX_E_INVALID (-1)     /* bad argument */
#define JX_E_UNSUPPORTED (-2) /* parameter set not supported by the engine */
#define JX_E_HIP (-3)         /* HIP runtime error (see jx_last_error) */
#define JX_E_NOMEM (-4)       /* device allocation failed */
#define JX_E_STATE (-5)       /* call out of order (e.g. accumulate without a prepared batch) */
#define JX_E_NODEVICE (-6)

/* Verdict bytes. Labels match handle_ping_pong_error, aggregator/src/aggregator/error.rs:379-424;
 * every non-zero verdict goes on the wire as PrepareError::VdafPrepError (messages/src/lib.rs:2344). */
#define JX_FINISHED 0
#define JX_PREPARE_INIT_FAILURE 1          /* PingPongError::VdafPrepareInit */
#define JX_PREP_SHARE_DECODE_FAILURE 2     /* PingPongError::CodecPrepShare (leader share malformed) */
#define JX_PREPARE_MESSAGE_FAILURE 3       /* PingPongError::VdafPrepareSharesToPrepareMessage */
#define JX_PREPARE_NEXT_FAILURE 4          /* PingPongError::VdafPrepareNext */
/* Leader only: the helper answered PrepareStepResult::Reject for this report (label
 * helper_step_failure, aggregation_job_driver.rs:646-660). */
#define JX_HELPER_STEP_FAILURE 5
/* Helper, encrypted inputs only: the report's input share did not open or decode; its out_open_status byte
 * names why (not a prepare failure: the report never reached helper_initialized). */
#define JX_OPEN_FAILURE 6

/* Open status of an encrypted report share (jx_helper_prep_encrypted_batch out_open_status): the checks of
 * the helper's loop before helper_initialized, in its order (aggregator/src/aggregator.rs:1781-1910), with the
 * PrepareError each goes on the wire as and its janus_step_failures label. */
#define JX_OPEN_OK 0
#define JX_OPEN_HPKE_DECRYPT_ERROR 1         /* HpkeDecryptError, "decrypt_failure" */
#define JX_OPEN_PLAINTEXT_DECODE_FAILURE 2   /* InvalidMessage, "plaintext_input_share_decode_failure" */
#define JX_OPEN_DUPLICATE_EXTENSION 3        /* InvalidMessage, "duplicate_extension" */
#define JX_OPEN_UNEXPECTED_TASKPROV 4        /* InvalidMessage, "unexpected_taskprov_extension" */
#define JX_OPEN_MISSING_TASKPROV 5           /* InvalidMessage, "missing_or_malformed_taskprov_extension" */
#define JX_OPEN_INPUT_SHARE_DECODE_FAILURE 6 /* InvalidMessage, "input_share_decode_failure" */
#define JX_OPEN_UNKNOWN_CONFIG 7             /* HpkeUnknownConfigId, "unknown_hpke_config_id" */
/* key_index values besides keypair indices */
#define JX_KEY_NONE 0xFF      /* no keypair (first: the config id is unknown; second: no fallback) */
/* first only: the caller found the encapsulated key malformed (HpkeDecryptError without an open). A length that
 * fits no keypair of the report is found by the engine itself (jx_helper_prep_encrypted_batch2). */
#define JX_KEY_MALFORMED 0xFE
#define JX_ENC_MAX_KEYPAIRS 8
/* flags */
#define JX_ENC_REQUIRE_TASKPROV 1u /* the task is provisioned by taskprov (aggregator.rs:1869-1879) */

/* Prio3 instance, mirroring janus_core::vdaf::VdafInstance (core/src/vdaf.rs:65-108).
 * algo_id: 0 Prio3Count, 1 Prio3Sum{bits}, 2 Prio3SumVec{bits,length,chunk_length},
 *          3 Prio3Histogram{length,chunk_length}  (== Prio3 algorithm ids, messages/src/taskprov.rs:358-363)
 *          4 Prio3SumVecField64MultiproofHmacSha256Aes128{proofs,bits,length,chunk_length}
 *            (core/src/vdaf.rs:173-199: Field64, XofHmacSha256Aes128, 32-byte seeds and verify key;
 *            DST algorithm id 0xFFFF1003; prep messages and joint-rand parts are 32 bytes)
 *          5 Prio3FixedPointBoundedL2VecSum{bitsize, length} (core/src/vdaf.rs:86-91; built at
 *            aggregator/src/aggregator.rs:916-932): bits = 16 (BitSize16, FixedI16<U15>) or 32
 *            (BitSize32, FixedI32<U31>), length = entries, chunk_length ignored (prio derives both
 *            gadgets' chunk lengths); Field128, TurboSHAKE, DST algorithm id 0xFFFF0000. The
 *            dp_strategy is applied at collection time and is not part of this ABI.
 * num_proofs: 1 for ids 0-3 and 5 (the TurboSHAKE variants, core/src/vdaf.rs:203-262); 2..8 for id 4. */
#define JX_ALGO_COUNT 0
#define JX_ALGO_SUM 1
#define JX_ALGO_SUMVEC 2
#define JX_ALGO_HISTOGRAM 3
#define JX_ALGO_SUMVEC_F64_MULTIPROOF_HMACSHA256_AES128 4
#define JX_ALGO_FIXEDPOINT_BOUNDED_L2_VEC_SUM 5
typedef struct {
  uint32_t algo_id;
  uint32_t bits;
  uint32_t length;
  uint32_t chunk_length;
  uint32_t num_proofs;
} jx_prio3_params;

typedef struct jx_engine jx_engine;

/* Create an engine for one Prio3 instance and one verify key (VERIFY_KEY_LENGTH = 16,
 * core/src/vdaf.rs:16) on HIP device `device`. */
int32_t jx_engine_create(const jx_prio3_params* params, const uint8_t verify_key[16], int32_t device,
                         jx_engine** out);
/* Same with an explicit verify key length: 16 (VERIFY_KEY_LENGTH) or, for algo_id 4, 32
 * (VERIFY_KEY_LENGTH_HMACSHA256_AES128, core/src/vdaf.rs:24). */
int32_t jx_engine_create_ex(const jx_prio3_params* params, const uint8_t* verify_key, uint32_t verify_key_len,
                            int32_t device, jx_engine** out);
void jx_engine_destroy(jx_engine* e);

/* Encoded sizes (bytes) for this instance. Any pointer may be NULL. */
int32_t jx_engine_sizes(const jx_engine* e, uint32_t* public_share, uint32_t* helper_input_share,
                        uint32_t* leader_prep_share, uint32_t* prep_msg, uint32_t* output_len,
                        uint32_t* field_bytes);

/* Reserve staging for `reports` reports (two-phase API needs n <= capacity; grows on demand). */
int32_t jx_engine_set_capacity(jx_engine* e, uint64_t reports);

/* ---- Resident prepared batches (one per aggregation job in flight).
 * Every prepare call (jx_helper_prep_batch, jx_leader_prep_init_*) creates a NEW resident batch and
 * returns its handle (batch id, never reused, never 0); it does not disturb other resident batches,
 * so any number of aggregation jobs can be prepared, finished and aggregated interleaved on one
 * engine (Janus steps max_concurrent_job_workers jobs at once, aggregator/src/binary_utils/
 * job_driver.rs:116-138; the leader holds each job's prepare state across the helper round trip,
 * aggregation_job_driver.rs:396-416 -> :540-701). A batch holds its output shares, verdicts, prep
 * messages (leader: the corrected joint-rand seeds) and report ids in HBM until it is released
 * (jx_batch_release) or accumulated into the running aggregations (jx_accumulate*, which releases it).
 * Calls naming a released or unknown batch return JX_E_STATE; a report count other than the
 * batch's returns JX_E_INVALID. */

/* Device memory of the engine and of its device's arena (shared by every engine on the device), and
 * the engine's coalescer (jx_engine_coalesce). */
typedef struct {
  uint64_t resident_batches;   /* this engine's resident batches */
  uint64_t batch_bytes;        /* device bytes they hold (arena slabs) */
  uint64_t arena_budget;       /* bytes the device arena may hold (JX_ARENA_GB, default 90% of HBM) */
  uint64_t arena_allocated;    /* bytes it holds: checked out + idle */
  uint64_t arena_in_use;       /* checked out now (staging of calls in progress + resident batches) */
  uint64_t arena_peak;         /* max arena_in_use */
  uint64_t arena_allocs;       /* device allocations it made */
  uint64_t arena_reuses;       /* check-outs served from idle slabs */
  uint64_t arena_waits;        /* check-outs that waited for another call's staging */
  uint64_t arena_engines;      /* live engines on the device */
  uint64_t last_pipelines;     /* pipelines the engine's last fused call ran */
  uint64_t coalesced_launches; /* launches of the device coalescer this engine uses (all its engines) */
  uint64_t coalesced_jobs;
  uint64_t coalesced_reports;
  uint64_t coalesce_window_us; /* its current gathering window */
  /* phase totals over the coalescer's launches (us): gathering (first job -> closed), the callers' input
   * copies after the close, queueing the launch, the device (queued -> done) */
  uint64_t coalesce_gather_us;
  uint64_t coalesce_copy_us;
  uint64_t coalesce_enqueue_us;
  uint64_t coalesce_device_us;
  uint64_t arena_cross_stream_waits; /* check-outs that had to wait for another stream's work */
  /* the coalescer's pinned host rows (all its lanes; released after 2 s without jobs) and its launches / jobs
   * by role (one gathering lane per role: leader and helper jobs never close each other's gathers) */
  uint64_t coalesce_pinned_bytes;
  uint64_t coalesced_helper_launches;
  uint64_t coalesced_helper_jobs;
  uint64_t coalesced_leader_launches;
  uint64_t coalesced_leader_jobs;
  uint64_t coalesced_encrypted_jobs;  /* helper jobs whose input shares were opened inside the launch */
  uint64_t arena_frees;               /* slabs the arena returned to the device (trims) */
} jx_memory_stats;
int32_t jx_engine_memory(const jx_engine* e, jx_memory_stats* out);

/* Coalesced prepares (Conventions). enable != 0 joins the device coalescer of this Prio3 instance;
 * window_us: the longest a launch gathers jobs after its first one arrives (0 = automatic: 1.5x the recent
 * launch latency, 0.1 .. 20 ms). A launch closes earlier when it is full, or once no job has joined for
 * 100 us while no other launch of the coalescer is running (or it already holds a quarter of a full
 * launch). Calls already waiting are unaffected by a later disable. The window is a setting of the device
 * coalescer, which every coalescing engine of the same Prio3 instance on the device shares: the last call
 * sets it for all of them. */
int32_t jx_engine_coalesce(jx_engine* e, int32_t enable, uint32_t window_us);

/* Batched helper_initialized + evaluate for n reports (host buffers).
 * out_verdicts[n] receives JX_FINISHED or a failure code; out_prep_msgs[n x PM] the outbound
 * Finish{prep_msg} payload (meaningful where verdict == JX_FINISHED); out_output_shares
 * (nullable) the output shares; *out_batch_id (nullable) the new batch's handle. */
int32_t jx_helper_prep_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                             const uint8_t* helper_input_shares, const uint8_t* leader_prep_shares,
                             uint8_t* out_prep_msgs, uint8_t* out_verdicts, uint8_t* out_output_shares,
                             uint64_t* out_batch_id);
/* The same prepare for report shares still under HPKE, the helper's whole per-report loop up to
 * helper_initialized (aggregator/src/aggregator.rs:1763-1967): on the device, report i's encrypted input share
 * is opened with keypairs[key_index[2i]] and, if that fails to decrypt, keypairs[key_index[2i + 1]] (the
 * task's keypair, then the global one for the same config id, :1807-1820), the PlaintextInputShare is decoded
 * and its extensions checked (:1834-1893), its payload decoded as the helper input share (:1895-1910), and the
 * report prepared in the same launch (coalesced with other jobs like jx_helper_prep_batch). A report that fails
 * before helper_initialized gets verdict JX_OPEN_FAILURE and out_open_status[i] (JX_OPEN_*); every other
 * report gets JX_OPEN_OK and its verdict as from jx_helper_prep_batch.
 *   times[n]            ReportMetadata.time (seconds); InputShareAad = task_id || id || time || public share
 *   task_id             32 bytes
 *   keypairs            nkeypairs (<= JX_ENC_MAX_KEYPAIRS) HPKE contexts on the engine's device, created with
 *                       the input-share application info (Label::InputShare, Client -> Helper). Borrowed for the
 *                       call. Their keys are in the device's key registry since they were created (jx_hpke.h):
 *                       the request carries no key material, and the limit is per request only. Coalesced jobs of
 *                       any number of tasks, each with keypairs of its own, share one launch (up to
 *                       JX_HPKE_MAX_CONTEXTS keypairs alive on the device)
 *   key_index[n x 2]    per report: first keypair, fallback keypair (JX_KEY_NONE / JX_KEY_MALFORMED above)
 *   encs[n x 32]        HpkeCiphertext.encapsulated_key (X25519; a P-256 keypair here is a failed trial: see
 *                       jx_helper_prep_encrypted_batch2)
 *   payloads            ciphertexts back to back; report i's is [payload_offsets[i], payload_offsets[i+1])
 *   flags               JX_ENC_REQUIRE_TASKPROV or 0
 * Public shares are fixed-length rows: a report whose public share has another length cannot go here (the
 * caller opens it alone and fails it with public_share_decode_failure, :1912-1925). out_open_status nullable. */
int32_t jx_helper_prep_encrypted_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                       const uint8_t* public_shares, const uint8_t task_id[32],
                                       jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                       const uint8_t* encs, const uint8_t* payloads, const uint64_t* payload_offsets,
                                       uint32_t flags, const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs,
                                       uint8_t* out_verdicts, uint8_t* out_open_status, uint64_t* out_batch_id);
/* The same call for encapsulated keys of any length, so that one request may mix KEMs: encs holds them back to
 * back, report i's is [enc_offsets[i], enc_offsets[i+1]) (enc_offsets[n + 1]; NULL: n x 32 bytes, the call above).
 * A trial of a keypair can only succeed when the report's encapsulated key has the length of the keypair's KEM
 * (jx_hpke_enc_len: 32 for X25519, 65 for P-256); any other trial fails without an open, as the hpke crate's
 * deserialisation of the encapsulated key does, and a report none of whose keypairs fits gets
 * JX_OPEN_HPKE_DECRYPT_ERROR (JX_OPEN_UNKNOWN_CONFIG still comes first when key_index[2i] is JX_KEY_NONE).
 * Reports with 65-byte keys are opened by a kernel of their own in the same launch; a request without any runs
 * exactly what the call above runs. */
int32_t jx_helper_prep_encrypted_batch2(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                        const uint8_t* public_shares, const uint8_t task_id[32],
                                        jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                        const uint8_t* encs, const uint64_t* enc_offsets, const uint8_t* payloads,
                                        const uint64_t* payload_offsets, uint32_t flags,
                                        const uint8_t* leader_prep_shares, uint8_t* out_prep_msgs, uint8_t* out_verdicts,
                                        uint8_t* out_open_status, uint64_t* out_batch_id);
/* The fused prepare + aggregate (jx_helper_prep_aggregate / _device below) from report shares still under HPKE: what
 * a helper serves, at the size the fused path is built for. The call is cut into the same launches over the same
 * pipelines as the plaintext call, and every launch opens its own reports first, with the rows kernels of
 * jx_helper_prep_encrypted_batch2: no resident batch, no limit of one launch's staging. Per report the semantics
 * are exactly that call's (keypairs tried in the same order, a trial only when the encapsulated key has the
 * length of the keypair's KEM, JX_KEY_NONE / JX_KEY_MALFORMED, JX_ENC_REQUIRE_TASKPROV); a report that fails
 * before helper_initialized gets verdict JX_OPEN_FAILURE and its JX_OPEN_* status. Exactly the reports with verdict
 * JX_FINISHED are accumulated: a report that did not open never reaches an aggregation. The arguments are checked
 * as there (key indices, decreasing offsets, a payload of 2^32 bytes or more, a keypair on another device, unknown
 * flags): JX_E_INVALID before anything is queued, the aggregations untouched. n == 0 is JX_OK.
 * Host form: host buffers, one `segment`; out_prep_msgs, out_verdicts and out_open_status nullable; returns with
 * the results in the caller's buffers.
 * Device form: device pointers for the bulk data (report ids, public shares, encapsulated keys, payloads, leader
 * prep shares, the three nullable outputs) and HOST arrays for times, key_index, enc_offsets (NULL: n x 32 bytes)
 * and payload_offsets, as jx_leader_upload_open_device takes them; d_segment / segment_ids / nsegments as
 * jx_helper_prep_aggregate_device. Asynchronous on the engine stream; the host arrays are consumed before it
 * returns. The ciphertexts and encapsulated keys are read in place from the caller's arrays (which must stay
 * unchanged until the call's work has run), and the per-report rows are laid out on the device, so nothing but
 * 26 bytes per report crosses the host. */
int32_t jx_helper_prep_aggregate_encrypted(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint64_t* times,
                                           const uint8_t* public_shares, const uint8_t task_id[32],
                                           jx_hpke* const* keypairs, uint32_t nkeypairs, const uint8_t* key_index,
                                           const uint8_t* encs, const uint64_t* enc_offsets, const uint8_t* payloads,
                                           const uint64_t* payload_offsets, uint32_t flags,
                                           const uint8_t* leader_prep_shares, uint32_t segment, uint8_t* out_prep_msgs,
                                           uint8_t* out_verdicts, uint8_t* out_open_status);
int32_t jx_helper_prep_aggregate_encrypted_device(jx_engine* e, uint64_t n, const void* d_nonces, const uint64_t* times,
                                                  const void* d_public_shares, const uint8_t task_id[32],
                                                  jx_hpke* const* keypairs, uint32_t nkeypairs,
                                                  const uint8_t* key_index, const void* d_encs,
                                                  const uint64_t* enc_offsets, const void* d_payloads,
                                                  const uint64_t* payload_offsets, uint32_t flags, const void* d_lps,
                                                  const void* d_segment, const uint32_t* segment_ids, uint32_t nsegments,
                                                  void* d_out_prep_msgs, void* d_out_verdicts, void* d_out_open_status);
/* Handle of the most recently prepared batch if it is still resident (0 otherwise). */
int32_t jx_engine_batch_id(const jx_engine* e, uint64_t* batch_id);
/* Resident batches and the device bytes they hold (either pointer nullable). */
int32_t jx_engine_batches(const jx_engine* e, uint64_t* resident, uint64_t* device_bytes);
/* Drop a resident batch (its device memory returns to the engine). */
int32_t jx_batch_release(jx_engine* e, uint64_t batch_id);

/* Per-job batch-aggregation deltas (the retry-safe accumulation contract).
 * Aggregates the finished reports of batch `batch_id` (helper; leader after finish) with
 * accept_mask[i] != 0 (nullable = all) into nsegments ZEROED aggregations, report i into aggregation
 * segment_index[i] (nullable = all into 0; indices >= nsegments are skipped), and writes them as
 * nsegments back-to-back shard records (encoded aggregate share OUT x FB || report count u64 LE ||
 * ReportIdChecksum 32 B, see jx_shard_record_bytes) to out_records. Nothing in the engine changes: the
 * batch stays resident and the running aggregations are untouched, so the call can be repeated with
 * the same or another mask (a retried run_tx closure, aggregator_core/src/datastore.rs:225-282) and the
 * host merges each record into the batch-aggregation row it read at its shard `ord`
 * (BatchAggregation::merged_with, aggregation_job_writer.rs:527,615-690). */
int32_t jx_batch_aggregate_records(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* accept_mask,
                                   const uint32_t* segment_index, uint32_t nsegments, uint8_t* out_records);
/* Same with device arrays and a device output (asynchronous on the engine stream). */
int32_t jx_batch_aggregate_records_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_accept_mask,
                                          const void* d_segment_index, uint32_t nsegments, void* d_out_records);

/* ---- Leader role: the leader side of the same ping-pong exchange.
 * jx_leader_prep_init_batch replaces the per-report vdaf.leader_initialized(verify_key, agg_param,
 * nonce = report id, public_share, leader_input_share) of step_aggregation_job_aggregate_init
 * (aggregator/src/aggregator/aggregation_job_driver.rs:344-362): prepare_init with agg_id 0 on the
 * explicit leader input share (meas share || proofs share || [k_blind], LIS bytes each, see
 * jx_engine_leader_sizes). out_prep_shares[n x LPS] receives the prep_share that goes into
 * PingPongMessage::Initialize; out_verdicts[n]: JX_FINISHED (0) = initialized, or
 * JX_PREPARE_INIT_FAILURE (an input-share element >= p, or t a P-th root of unity). The prepare
 * state (output share + corrected joint-rand seed) stays on the device in the new batch.
 * jx_leader_prep_finish_batch replaces leader_continued on the helper's Finish{prep_msg}
 * (aggregation_job_driver.rs:588-602): prepare_next fails (JX_PREPARE_NEXT_FAILURE) unless prep_msg
 * equals the corrected seed. prep_msgs: n x PM (PM = 0: nullable). out_output_shares nullable.
 * *out_batch_id names the leader batch; finish, records and accumulate pass it back. A batch is
 * finished once (a second finish returns JX_E_STATE); its records / accumulation need the finish. */
int32_t jx_engine_leader_sizes(const jx_engine* e, uint32_t* leader_input_share);
int32_t jx_leader_prep_init_batch(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                  const uint8_t* leader_input_shares, uint8_t* out_prep_shares, uint8_t* out_verdicts,
                                  uint64_t* out_batch_id);
int32_t jx_leader_prep_finish_batch(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* prep_msgs,
                                    uint8_t* out_verdicts, uint8_t* out_output_shares);
/* Device-pointer leader role (inputs resident in HBM; asynchronous on the engine stream, n <= the
 * engine capacity, grown on demand; the report ids are copied into the batch). For Prio3Sum, SumVec
 * and FixedPointBoundedL2VecSum the FLP kernels read the measurement share in place from
 * d_leader_input_shares in 16-byte vectors: that pointer must be 16-byte aligned (JX_E_INVALID
 * otherwise); the stride LIS is a multiple of 16 for every Field128 instance.
 * d_out_verdicts nullable. Finish: d_peer_verdicts (nullable) are the helper's verdicts; a report
 * the helper rejected gets JX_HELPER_STEP_FAILURE. */
int32_t jx_leader_prep_init_device(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                   const void* d_leader_input_shares, void* d_out_prep_shares, void* d_out_verdicts,
                                   uint64_t* out_batch_id);
int32_t jx_leader_prep_finish_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_prep_msgs,
                                     const void* d_peer_verdicts, void* d_out_verdicts);
/* jx_leader_prep_init_device with an explicit row stride of d_leader_input_shares (0 = LIS; otherwise
 * >= LIS and a multiple of 16). The leader assembles these rows after HPKE open, so it can pad them for
 * free: with a stride that is a multiple of 128 the in-place FLP kernels read whole cache lines. */
int32_t jx_leader_prep_init_device_ex(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                      const void* d_leader_input_shares, uint64_t lis_stride, void* d_out_prep_shares,
                                      void* d_out_verdicts, uint64_t* out_batch_id);

/* ---- The leader's upload path: handle_upload_generic's per-report loop (aggregator/src/aggregator.rs:1513-1694) on
 * the device, producing the rows jx_leader_prep_init_device_ex reads. Per report: hpke::open of
 * leader_encrypted_input_share under (InputShare, Client -> Leader) with keypairs[key_index[2i]] and, if that fails to
 * decrypt, keypairs[key_index[2i + 1]] (the task's keypair, then the global one of the same config id, :1602-1637);
 * PlaintextInputShare::get_decoded (:1653); A::InputShare::get_decoded_with_param(&(&vdaf, 0), payload) (:1659-1662):
 * the payload's length must equal jx_engine_leader_sizes' LIS exactly and every element of its measurement-share and
 * proofs-share parts must be < p (the blind is opaque), for every algo id 0-5. The three time checks of the handler
 * are the caller's (they need no report bytes). Arguments as in jx_helper_prep_encrypted_batch2:
 *   report_ids[n x 16], times[n], public_shares[n x PS] (fixed-length rows: a report with another length is the
 *   caller's to reject), task_id, keypairs (contexts created with the (InputShare, Client -> Leader) application
 *   info; their keys are read from the device's key registry, the call uploads no key material), key_index[n x 2]
 *   (JX_KEY_NONE / JX_KEY_MALFORMED as there), encs with enc_offsets[n + 1] (NULL: n x 32 bytes), payloads with
 *   payload_offsets[n + 1] (each ciphertext < 2^32 bytes). The associated data, the encoded InputShareAad, is built
 *   on the device.
 * out_status[i] reuses the JX_OPEN_* codes: JX_OPEN_UNKNOWN_CONFIG is Janus's ReportRejectionReason::
 * OutdatedHpkeConfig, JX_OPEN_HPKE_DECRYPT_ERROR is DecryptFailure, JX_OPEN_PLAINTEXT_DECODE_FAILURE (the framing: a
 * truncated list, an unknown extension type, bytes after the payload) and JX_OPEN_INPUT_SHARE_DECODE_FAILURE (the
 * payload: its length, an element >= p) are both DecodeFailure and stay distinct for the logs; JX_OPEN_OK the rest.
 * The upload handler makes no duplicate-extension and no taskprov checks (:1653-1678), so codes 3-5
 * (JX_OPEN_DUPLICATE_EXTENSION, JX_OPEN_UNEXPECTED_TASKPROV, JX_OPEN_MISSING_TASKPROV) never occur here.
 * An accepted report's payload goes to row i of the output (host call: rows of LIS bytes; device call: rows of
 * lis_stride bytes, 0 = LIS, else >= LIS and a multiple of 16, zero padded; d_out_rows 16-byte aligned); a rejected
 * report's row is zeros. Report i's extension list, without its u16 length prefix, goes to out_extensions +
 * payload_offsets[i] (the buffer is as long as payloads) with its length in out_ext_len[i] (0 for a rejected report).
 * The call runs on the engine's stream with scratch from the device's arena and is not coalesced (upload batches
 * come from the report writer's own batcher). The device call takes device pointers for the bulk data (report ids,
 * public shares, encapsulated keys, payloads, the four outputs) and HOST arrays for times, key_index and the two
 * offset arrays; it returns once its launches are queued. */
int32_t jx_leader_upload_open_batch(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                                    const uint8_t* public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                    uint32_t nkeypairs, const uint8_t* key_index, const uint8_t* encs,
                                    const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                                    uint8_t* out_leader_input_shares, uint8_t* out_extensions, uint32_t* out_ext_len,
                                    uint8_t* out_status);
int32_t jx_leader_upload_open_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                     const void* d_public_shares, const uint8_t task_id[32], jx_hpke* const* keypairs,
                                     uint32_t nkeypairs, const uint8_t* key_index, const void* d_encs,
                                     const uint64_t* enc_offsets, const void* d_payloads, const uint64_t* payload_offsets,
                                     void* d_out_rows, uint64_t lis_stride, void* d_out_extensions, void* d_out_ext_len,
                                     void* d_out_status);

/* ---- The client: Prio3.shard (VDAF-08 §7.2.1) for n measurements, the first of the VDAF's four algorithms and the
 * source of the rows every prepare call above takes. Per report: the helper's measurement and proof shares are
 * expanded from its two seeds, the leader's measurement share is enc(measurement) - the helper's, the joint
 * randomness is derived from both shares' parts, FlpGeneric.prove runs on the whole measurement (the gadget
 * polynomial through number-theoretic transforms), and the leader's proof share is the proof minus the helper's.
 * Every XOF stream is rejection-sampled exactly.
 *   measurements  uint64: one per report for Count ({0, 1}), Sum (< 2^bits) and Histogram (a bucket index <
 *                 length); `length` per report for SumVec (each < 2^bits)
 *   nonces        n x 16
 *   rands         n x jx_client_rand_bytes: k_helper_meas || k_helper_proofs || k_prove || [blind_leader ||
 *                 blind_helper], 16 bytes each, the blinds only for instances with joint randomness. The engine
 *                 never generates randomness: the caller owns the CSPRNG. The engine's verify key is not used.
 * Outputs, fixed-stride rows in the encodings the prepare calls take: public shares n x PS, leader input shares
 * (measurement share || proof share || [blind]; host call: rows of LIS bytes; device call: rows of lis_stride
 * bytes, 0 = LIS, else >= LIS and a multiple of 16, zero padded, 16-byte aligned), helper input shares n x HIS.
 * out_status (nullable): 0, or JX_SHARD_INVALID_MEASUREMENT for a report whose measurement is out of range, as
 * prio's encode_measurement refuses it; its three rows are zeros.
 * The device call is asynchronous on the engine stream under the ordering contract of the Conventions, takes its
 * scratch from the device's arena, is cut into launches when n exceeds one launch's scratch, and is not coalesced.
 * n == 0 is JX_OK. Algo ids 0-3 only: the multiproof (4) and FixedPoint (5) instances return JX_E_UNSUPPORTED, and so
 * does an instance whose transform size P = next_pow2(1 + gadget calls) exceeds JX_SHARD_MAX_P. */
#define JX_SHARD_INVALID_MEASUREMENT 1
#define JX_SHARD_MAX_P 1024u
int32_t jx_client_shard_batch(jx_engine* e, uint64_t n, const uint64_t* measurements, const uint8_t* nonces,
                              const uint8_t* rands, uint8_t* out_public_shares, uint8_t* out_leader_input_shares,
                              uint8_t* out_helper_input_shares, uint8_t* out_status);
int32_t jx_client_shard_device(jx_engine* e, uint64_t n, const void* d_measurements, const void* d_nonces,
                               const void* d_rands, void* d_out_public_shares, void* d_out_leader_input_shares,
                               uint64_t lis_stride, void* d_out_helper_input_shares, void* d_out_status);
int32_t jx_client_rand_bytes(const jx_engine* e, uint32_t* bytes);

/* ---- The client's second half: the two hpke::seal calls of the reference client's prepare_report (client/src/
 * lib.rs:339-383; core/src/hpke.rs:167) for the n reports whose rows jx_client_shard_* wrote. Per report, under RFC
 * 9180 base mode (single shot: sequence number 0): the leader's PlaintextInputShare, u16 0 (no extensions) || u32 LIS ||
 * leader row (read in place at lis_stride), is sealed for the leader, and the helper's, u16 0 || u32 HIS || helper
 * input share, for the helper, each under its own recipient context and its own ephemeral key, with the encoded
 * InputShareAad, task_id || report_id || time (u64 BE) || u32 PS || public_share, built on the device.
 *   report_ids[n x 16], times[n] (a HOST array in both forms), public_shares[n x PS] (NULL when PS is 0), leader rows
 *   (lis_stride apart; 0 = LIS), helper rows [n x HIS], task_id, leader / helper: X25519 contexts created with the
 *   (InputShare, Client -> Leader) and (InputShare, Client -> Helper) application infos, normally sender contexts
 *   (jx_hpke_create_sender; their keys are read from the device's key registry), ephemeral_sks[n x 64]: the leader
 *   seal's X25519 private key, then the helper seal's, clamped by the engine (the engine draws no randomness: the
 *   caller owns the CSPRNG, as for jx_client_shard_*'s rands), shard_status (nullable): jx_client_shard_*'s
 *   out_status, a non-zero entry leaves that report's outputs zero.
 * Outputs: leader encapsulated keys [n x 32] and ciphertext rows [n x (6 + LIS + 16)], the helper's [n x 32] and
 * [n x (6 + HIS + 16)] (jx_client_seal_sizes gives the two row lengths), and out_status[n]: JX_SEAL_OK,
 * JX_SEAL_SKIPPED (shard_status was non-zero: all four outputs zero), or JX_SEAL_ZERO_DH (a recipient key of low
 * order: X25519(skE, pkR) was all zero; that share's encapsulated key and ciphertext are zeros). The ciphertext rows
 * are what jx_leader_upload_open_device and jx_helper_prep_aggregate_encrypted_device read with payload_offsets[i] =
 * i x row length and enc_offsets = NULL.
 * The device call is asynchronous on the engine stream under the ordering contract of the Conventions, takes its
 * scratch from the device's arena, is cut into launches (debug option 11) and is not coalesced. It only reads rows,
 * so it works for every algo id 0-5. n == 0 is JX_OK. A P-256 context returns JX_E_UNSUPPORTED. */
#define JX_SEAL_OK 0
#define JX_SEAL_SKIPPED 1
#define JX_SEAL_ZERO_DH 2
int32_t jx_client_seal_sizes(const jx_engine* e, uint32_t* leader_ct_len, uint32_t* helper_ct_len);
int32_t jx_client_seal_batch(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                             const uint8_t* public_shares, const uint8_t* leader_input_shares, uint64_t lis_stride,
                             const uint8_t* helper_input_shares, const uint8_t task_id[32], jx_hpke* leader,
                             jx_hpke* helper, const uint8_t* ephemeral_sks, const uint8_t* shard_status,
                             uint8_t* out_leader_encs, uint8_t* out_leader_cts, uint8_t* out_helper_encs,
                             uint8_t* out_helper_cts, uint8_t* out_status);
int32_t jx_client_seal_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                              const void* d_public_shares, const void* d_leader_input_shares, uint64_t lis_stride,
                              const void* d_helper_input_shares, const uint8_t task_id[32], jx_hpke* leader,
                              jx_hpke* helper, const void* d_ephemeral_sks, const void* d_shard_status,
                              void* d_out_leader_encs, void* d_out_leader_cts, void* d_out_helper_encs,
                              void* d_out_helper_cts, void* d_out_status);

/* ---- Wire in, wire out: the helper's aggregate-init exchange from the bytes it receives to the bytes it answers.
 * jx_init_req_decode* cuts an AggregationJobInitializeReq body (u32 + aggregation parameter || PartialBatchSelector ||
 * u32 + PrepareInits; messages/src/lib.rs:2482-2553) on the device into the arrays the sealed fused call reads, and
 * jx_init_resp_encode* writes the AggregationJobResp body (u32 + PrepareResps) from that call's outputs. The request
 * is decoded as the reference's get_decoded does: any framing error fails the whole request, and so does a repeated
 * report id (aggregator.rs:1748-1758); what the reference's loop fails per report stays per report (wire_status).
 *
 * Decode returns a handle also for a request it refuses (jx_init_req_info says why); a refused request has no arrays
 * and queues nothing. The body is copied to the device once (host form) or read in place (device form, asynchronous
 * inputs ordered by the Conventions; the call itself waits for its own results, since n is one of them). After the
 * call the body is no longer read. A handle holds device memory of the engine's arena until jx_init_req_release,
 * which must come before jx_engine_destroy.
 *   expected_query_type  JX_QUERY_TIME_INTERVAL or JX_QUERY_FIXED_SIZE: the task's (decode_expecting_value)
 *   key_first/second     two 256-entry tables, config id -> keypair index of the request's keypairs as the sealed
 *                        calls take them (first trial, second trial; JX_KEY_NONE where there is none)
 *   report_deadline      NULL, or the latest report time that is not too early (aggregator.rs:1929-1940)
 * Per report i the arrays hold: report id, time (native u64), public-share row (PS bytes), leader prep-share row (LPS
 * bytes), the encapsulated keys and payloads packed with enc_offsets[n + 1] / payload_offsets[n + 1], key_index[2i..],
 * wire_status[i] and route[i]. wire_status: 0; JX_WIRE_REPORT_ODD_PUBLIC_SHARE (the public share is not PS bytes: the
 * row is zeros, both key indices are JX_KEY_NONE, and the host resolves the report from the body);
 * JX_WIRE_REPORT_NOT_INITIALIZE (the ping-pong message is not Initialize) and JX_WIRE_REPORT_ODD_PREP_SHARE (its prep
 * share is not LPS bytes) ride with a zero prep-share row. route[i] is 0, or 0xFFFFFFFF for a report that must not
 * reach an aggregation (wire_status != 0, or its time is after the deadline): pass it as d_segment with one segment id.
 * The host pointers of jx_init_req_arrays are one pinned copy made by the decode. */
#define JX_WIRE_OK 0
#define JX_WIRE_MALFORMED 1        /* info.error_offset: the read that failed */
#define JX_WIRE_WRONG_QUERY_TYPE 2 /* info.error_offset: the query-type byte */
#define JX_WIRE_DUPLICATE_ID 3     /* info.duplicate_index: the lowest index with an equal id at a lower index */
#define JX_WIRE_REPORT_ODD_PUBLIC_SHARE 1
#define JX_WIRE_REPORT_NOT_INITIALIZE 2
#define JX_WIRE_REPORT_ODD_PREP_SHARE 3
#define JX_QUERY_TIME_INTERVAL 1
#define JX_QUERY_FIXED_SIZE 2
#define JX_WIRE_NO_ERROR 0xFF /* host_errors[i]: no host-resolved error */
typedef struct jx_init_req jx_init_req;
typedef struct jx_wire_record { /* one PrepareInit: absolute offsets into the body and lengths of its fields */
  uint64_t off, len;
  uint64_t public_share_off, enc_off, payload_off, message_off, prep_msg_off, prep_share_off;
  uint32_t public_share_len, enc_len, payload_len, message_len, prep_msg_len, prep_share_len;
  uint8_t config_id, ping_pong_type, pad_[6];
} jx_wire_record;
typedef struct jx_init_req_info_t {
  uint32_t status;          /* JX_WIRE_* */
  uint32_t has_batch_id;    /* FixedSize */
  uint64_t error_offset;    /* JX_WIRE_MALFORMED / JX_WIRE_WRONG_QUERY_TYPE */
  uint64_t duplicate_index; /* JX_WIRE_DUPLICATE_ID */
  uint64_t n;               /* PrepareInits (0 unless status is JX_WIRE_OK or JX_WIRE_DUPLICATE_ID) */
  uint64_t agg_param_off, agg_param_len;
  uint64_t fallback_iterations; /* iterations of the index's fallback loop: 0 for a uniform body */
  uint64_t odd_public_shares;   /* reports of wire_status JX_WIRE_REPORT_ODD_PUBLIC_SHARE */
  uint64_t enc_bytes, payload_bytes;
  uint8_t batch_id[32];
} jx_init_req_info_t;
typedef struct jx_init_req_arrays_t {
  const void *d_report_ids, *d_times, *d_public_shares, *d_leader_prep_shares, *d_encs, *d_enc_offsets, *d_payloads,
      *d_payload_offsets, *d_key_index, *d_wire_status, *d_route, *d_records;
  const uint64_t *times, *enc_offsets, *payload_offsets;
  const jx_wire_record* records;
  const uint8_t *report_ids, *key_index, *wire_status;
} jx_init_req_arrays_t;
int32_t jx_init_req_decode(jx_engine* e, const uint8_t* body, uint64_t len, uint32_t expected_query_type,
                           const uint8_t key_first[256], const uint8_t key_second[256], const uint64_t* report_deadline,
                           jx_init_req** out);
int32_t jx_init_req_decode_device(jx_engine* e, const void* d_body, uint64_t len, uint32_t expected_query_type,
                                  const uint8_t key_first[256], const uint8_t key_second[256],
                                  const uint64_t* report_deadline, jx_init_req** out);
int32_t jx_init_req_info(const jx_init_req* r, jx_init_req_info_t* out);
/* JX_E_STATE unless the request's status is JX_WIRE_OK. */
int32_t jx_init_req_arrays(const jx_init_req* r, jx_init_req_arrays_t* out);
/* Route the reports with exclude[i] != 0 (a host array of n) away from every aggregation: route[i] = 0xFFFFFFFF. For
 * reports the caller knows before the prepare call that it will not accept, such as replayed ones. */
int32_t jx_init_req_exclude(jx_init_req* r, const uint8_t* exclude);
/* Route the reports of a time-interval request to their batch buckets on the device, as the reference's aggregation
 * job writer indexes them (aggregation_job_writer.rs:557-605, :608-708). A report's bucket starts at its time rounded
 * down to time_precision (> 0; exact for every u64). The table that comes back holds the distinct bucket starts over
 * all n reports, ascending, at most JX_ROUTE_MAX_BUCKETS of them: min_time, max_time and reports cover every report of
 * the bucket, the excluded and failed ones too (the writer widens the batch's client-timestamp interval with all of
 * them); routed counts the reports this call routes to the bucket; collected is 1 when the start is among
 * collected_starts (a host array in any order, repeats allowed; a start that is no bucket of the request matches
 * nothing). Per report, route[i] becomes its bucket's index in the table when it was 0 and the bucket is not
 * collected, and 0xFFFFFFFF otherwise: pass it as d_segment with segment_ids[k] the aggregation of bucket k. The
 * response encode answers the otherwise finished reports of a collected bucket with BatchCollected (code point 0),
 * which ranks below ReportReplayed. jx_init_req_exclude may still follow: it routes out as before, and the table's
 * `routed` counts, which are this call's, are not updated by it. The call waits for its table.
 * JX_E_INVALID: time_precision 0, or a request with a batch id (FixedSize: its one batch needs no route). JX_E_STATE: a
 * refused request, or a handle that is routed already. *out_status JX_ROUTE_TOO_MANY_BUCKETS: more than
 * JX_ROUTE_MAX_BUCKETS distinct buckets; route and the handle are as they were, and it may be routed again. */
#define JX_ROUTE_MAX_BUCKETS 1024
#define JX_ROUTE_OK 0
#define JX_ROUTE_TOO_MANY_BUCKETS 1
typedef struct jx_route_bucket {
  uint64_t start, min_time, max_time;
  uint32_t reports, routed, collected, pad_;
} jx_route_bucket;
int32_t jx_init_req_route(jx_engine* e, jx_init_req* r, uint64_t time_precision, const uint64_t* collected_starts,
                          uint64_t ncollected, uint32_t* out_status, uint32_t* out_nbuckets,
                          jx_route_bucket* out_buckets /* [JX_ROUTE_MAX_BUCKETS] */);
/* A routed handle's per-report device arrays: bucket_index u32[n], bucket_collected u8[n] (either pointer nullable).
 * JX_E_STATE unless the handle is routed. */
int32_t jx_init_req_route_arrays(const jx_init_req* r, const void** d_bucket_index, const void** d_bucket_collected);
/* The AggregationJobResp body of the request: per report, by the helper loop's precedence (aggregator.rs:1781-2013,
 * :2127-2132): host_errors[i] (a PrepareError code point, JX_WIRE_NO_ERROR: none) for reports the host resolved; the
 * open status (1: HpkeDecryptError, 2-6: InvalidMessage, 7: HpkeUnknownConfigId); a time after the decode's deadline:
 * ReportTooEarly; wire_status 2 or 3: VdafPrepError; a verdict other than 0: VdafPrepError; replayed[i] != 0:
 * ReportReplayed; otherwise Continue{Finish{prep_msg}}: id || 00 || u32(5 + S) || 02 || u32(S) || prep_msg[S], S the
 * engine's prep-message length. d_verdicts, d_open_status, d_prep_msgs (rows prep_msg_stride apart, 0: S; NULL when S
 * is 0): the device arrays the sealed calls wrote; host_errors, replayed: host arrays of n, nullable. The body goes to
 * out (capacity bytes; 4 + n x (26 + S) always suffices, JX_E_INVALID when it does not fit), its length to *out_len,
 * and finished[i] = 1 for exactly the reports answered with Continue (d_out_finished / out_finished, nullable). Both
 * calls wait for their result: the length is part of it. */
int32_t jx_init_resp_encode_device(jx_engine* e, jx_init_req* r, const void* d_verdicts, const void* d_open_status,
                                   const void* d_prep_msgs, uint64_t prep_msg_stride, const uint8_t* host_errors,
                                   const uint8_t* replayed, void* d_out, uint64_t capacity, uint64_t* out_len,
                                   void* d_out_finished);
int32_t jx_init_resp_encode(jx_engine* e, jx_init_req* r, const void* d_verdicts, const void* d_open_status,
                            const void* d_prep_msgs, uint64_t prep_msg_stride, const uint8_t* host_errors,
                            const uint8_t* replayed, uint8_t* out, uint64_t capacity, uint64_t* out_len,
                            uint8_t* out_finished);
void jx_init_req_release(jx_init_req* r);

/* ---- The leader's end of the same exchange: step_aggregation_job_aggregate_init's request written and
 * process_response_from_helper's response read (aggregation_job_driver.rs:296-425, :540-701), with the prep shares
 * staying on the device between jx_leader_prep_init_device* and the body, and the response's prep messages going
 * straight into the rows jx_leader_prep_finish_device reads.
 *
 * jx_init_req_encode* writes the AggregationJobInitializeReq body: u32 + aggregation parameter || PartialBatchSelector
 * (query type, and the 32-byte batch id under FixedSize) || u32 + PrepareInits. Report i is sent iff verdicts[i] ==
 * JX_FINISHED and exclude[i] == 0 (exclude nullable): a report whose leader init failed, or that the caller knows it
 * must not send (a collected batch, duplicate extensions), takes no room in the body. The reports sent keep their order:
 * the response is matched by position. Per sent report: id[16] || time u64 || u32 PS || public share || config id ||
 * u16 + encapsulated key || u32 + payload || u32 (5 + LPS) || 00 || u32 LPS || prep share.
 *   device form  device pointers for report ids [n x 16], public shares [n x PS] (NULL when PS is 0), encapsulated
 *                keys and payloads (packed by their offset arrays), prep shares (rows prep_share_stride apart, 0 = LPS:
 *                jx_leader_prep_init_device*'s d_out_prep_shares) and that call's d_out_verdicts, all of any alignment;
 *                HOST arrays for times[n], config_ids[n], enc_offsets[n + 1] (NULL: n x 32 bytes), payload_offsets
 *                [n + 1] and exclude[n]; the aggregation parameter, the query type and batch_id (FixedSize) on the host.
 *   host form    host pointers throughout, and the body in host memory.
 * Refused before a byte is written: an encapsulated key of 2^16 bytes or more, a payload of 2^32 bytes or more,
 * decreasing offsets (JX_E_INVALID); PrepareInits of more than 2^32 - 1 bytes together (JX_E_UNSUPPORTED); a body longer
 * than `capacity` (JX_E_INVALID). jx_init_req_encode_bound gives the body's length if every report were sent, from the
 * host arrays alone. Both forms wait for their result, since the length is part of it (inputs written on another
 * stream are ordered by the Conventions). n_sent == 0 is JX_OK with a body that holds an empty vector; the reference
 * then sends nothing (aggregation_job_driver.rs:388-423), which is the caller's choice.
 * The handle remembers which reports were sent (jx_leader_req_sent: the compaction list, sent_index[k] = i, as a pinned
 * host array and on the device, n_sent entries) and their ids. It holds arena memory until jx_leader_req_release,
 * which must come before jx_engine_destroy.
 *
 * jx_init_resp_decode reads the helper's AggregationJobResp body (host memory) for the handle's request. The body is
 * walked on the host (a response is ~42 bytes per report and a dependent chain), as AggregationJobResp::get_decoded
 * does: a framing error anywhere (a truncation, a length that overruns, a tag above 2, a PrepareError above 9, a
 * ping-pong type above 2, bytes left over) refuses the response with JX_WIRE_MALFORMED and the offset of the read that
 * failed; a response whose PrepareResps are not exactly the sent reports in order is JX_WIRE_RESP_MISMATCH with the
 * first position that differs. A refused response queues nothing and writes nothing; the call can be repeated with
 * another body. Otherwise out_result[k] / out_error[k] (n_sent entries, host) say what a one-round leader makes of
 * response k (aggregation_job_driver.rs:584-663): JX_RESP_CONTINUED (Continue{Finish{prep_msg}} with a prep message of
 * PM bytes; error JX_WIRE_NO_ERROR), JX_RESP_REJECTED (error: the helper's PrepareError), JX_RESP_FINISHED and
 * JX_RESP_MESSAGE_MISMATCH (a Continue carrying another message, or a prep message of another length; error 5,
 * VdafPrepError). One upload and one kernel on the engine stream then write, for every row i < n of the leader batch,
 * d_out_prep_msgs row i (prep_msg_stride apart, 0 = PM; NULL when PM is 0) and d_out_peer_verdicts[i]: the prep message
 * and 0 where the row's response continued, zeros and a non-zero verdict everywhere else, rows never sent included, so
 * jx_leader_prep_finish_device(e, batch_id, n, d_out_prep_msgs, d_out_peer_verdicts, ..) can never finish such a row.
 * The device outputs are queued, not waited for. */
#define JX_WIRE_RESP_MISMATCH 4 /* info.mismatch_index */
#define JX_RESP_CONTINUED 0
#define JX_RESP_REJECTED 1
#define JX_RESP_FINISHED 2
#define JX_RESP_MESSAGE_MISMATCH 3
typedef struct jx_leader_req jx_leader_req;
typedef struct jx_leader_req_info_t {
  uint64_t n, n_sent, body_len;
} jx_leader_req_info_t;
typedef struct jx_init_resp_info_t {
  uint32_t status; /* JX_WIRE_OK, JX_WIRE_MALFORMED or JX_WIRE_RESP_MISMATCH */
  uint32_t pad_;
  uint64_t error_offset;   /* JX_WIRE_MALFORMED */
  uint64_t mismatch_index; /* JX_WIRE_RESP_MISMATCH */
  uint64_t n;              /* PrepareResps in the body (0 when malformed) */
} jx_init_resp_info_t;
int32_t jx_init_req_encode_bound(const jx_engine* e, uint64_t n, const uint64_t* enc_offsets, const uint64_t* payload_offsets,
                                 uint64_t agg_param_len, uint32_t query_type, uint64_t* out_bound);
int32_t jx_init_req_encode_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                  const void* d_public_shares, const uint8_t* config_ids, const void* d_encs,
                                  const uint64_t* enc_offsets, const void* d_payloads, const uint64_t* payload_offsets,
                                  const void* d_prep_shares, uint64_t prep_share_stride, const void* d_verdicts,
                                  const uint8_t* exclude, const uint8_t* agg_param, uint64_t agg_param_len,
                                  uint32_t query_type, const uint8_t* batch_id, void* d_out, uint64_t capacity,
                                  uint64_t* out_len, jx_leader_req** out_req);
int32_t jx_init_req_encode(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                           const uint8_t* public_shares, const uint8_t* config_ids, const uint8_t* encs,
                           const uint64_t* enc_offsets, const uint8_t* payloads, const uint64_t* payload_offsets,
                           const uint8_t* prep_shares, uint64_t prep_share_stride, const uint8_t* verdicts,
                           const uint8_t* exclude, const uint8_t* agg_param, uint64_t agg_param_len, uint32_t query_type,
                           const uint8_t* batch_id, uint8_t* out, uint64_t capacity, uint64_t* out_len,
                           jx_leader_req** out_req);
int32_t jx_leader_req_info(const jx_leader_req* r, jx_leader_req_info_t* out);
int32_t jx_leader_req_sent(const jx_leader_req* r, const uint32_t** sent_index, const void** d_sent_index);
int32_t jx_init_resp_decode(jx_engine* e, jx_leader_req* r, const uint8_t* body, uint64_t len, void* d_out_prep_msgs,
                            uint64_t prep_msg_stride, void* d_out_peer_verdicts, uint8_t* out_result, uint8_t* out_error,
                            jx_init_resp_info_t* info);
void jx_leader_req_release(jx_leader_req* r);

/* ---- The upload message on the device: the DAP Report a client sends the leader (messages/src/lib.rs:1353-1432),
 *   id[16] || time u64 BE || u32 + public share || config id u8 || u16 + encapsulated key || u32 + payload ||
 *   config id u8 || u16 + encapsulated key || u32 + payload     (the leader's ciphertext, then the helper's),
 * written from the rows jx_client_seal_* left on the device and cut into the arrays jx_leader_upload_open_device and
 * jx_init_req_encode_device read, so that a report's 100+ KB never cross the host one report at a time.
 *
 * jx_report_encode* (the client) writes n Report bodies back to back into out (capacity bytes) from report ids
 * [n x 16], times[n] (a HOST array in both forms, as in the seal), public-share rows [n x PS] (NULL when PS is 0),
 * leader and helper encapsulated-key rows [n x leader_enc_len] / [n x helper_enc_len], the two ciphertext row arrays
 * of jx_client_seal_sizes' lengths, one config id per recipient and the seal's status (nullable). Report i lies at
 * out + offsets[i], offsets[n] is the total (also *out_len); a report whose status is non-zero takes no room
 * (offsets[i + 1] == offsets[i]). The offsets go to d_out_offsets (device, n + 1, nullable) and out_offsets (host,
 * n + 1, nullable). An encapsulated key of 2^16 bytes or more, or bodies longer than `capacity`, are JX_E_INVALID
 * before a byte is written; jx_report_encode_bound gives the length if every report takes room. The calls wait for
 * their result: the length is part of it.
 *
 * jx_upload_decode* (the leader) takes n upload bodies back to back (len bytes) with the HOST array body_offsets
 * [n + 1]: every upload is an HTTP body of its own, so the boundaries are known. Per upload, first failing check first:
 * the parse (Report::get_decoded: every field inside the body, nothing left over), the handler's three time checks in
 * its order (aggregator.rs:1544-1573; both sums saturate at 2^64 - 1, which decides as the unbounded sum does), the
 * public share's length against the engine's PS (the reference's DecodeFailure, :1580-1593). There is no duplicate-id
 * check: the reference's upload has none (the report writer's unique constraint does it). key_first / key_second map
 * the LEADER ciphertext's config id to keypair slots, as in jx_init_req_decode.
 * The handle gives, for all n: report id, time, upload_status and row_of (JX_UPLOAD_NO_ROW when not accepted; id and
 * time are zeros when the body has fewer than 24 bytes); and for the m accepted reports, dense and in order, exactly
 * what jx_leader_upload_open_device and jx_init_req_encode_device take: index[m] (accepted report k is upload
 * index[k]), ids, times, public-share rows, key_index[m x 2], the leader's encapsulated keys and payloads packed with
 * their offset arrays [m + 1], the helper's config_ids[m], encapsulated keys and payloads packed with theirs. The host
 * pointers of jx_upload_req_arrays are one pinned copy made by the decode. After the call the bodies are no longer
 * read. Decreasing body_offsets or an offset past len: JX_E_INVALID; n >= 2^31 - 1: JX_E_UNSUPPORTED; both with
 * nothing queued. The device form's inputs are ordered by the Conventions; the call waits for its own results (m is
 * one). A handle holds arena memory until jx_upload_req_release, which must come before jx_engine_destroy. */
#define JX_UPLOAD_OK 0
#define JX_UPLOAD_MALFORMED 1         /* the reference answers that upload with invalidMessage */
#define JX_UPLOAD_TOO_EARLY 2         /* time > now + tolerable_clock_skew */
#define JX_UPLOAD_TASK_EXPIRED 3      /* time > task_expiration */
#define JX_UPLOAD_EXPIRED 4           /* now > time + report_expiry_age */
#define JX_UPLOAD_ODD_PUBLIC_SHARE 5  /* the public share is not PS bytes */
#define JX_UPLOAD_NO_ROW 0xFFFFFFFFu
typedef struct jx_upload_req jx_upload_req;
typedef struct jx_upload_checks {
  uint64_t now, tolerable_clock_skew;
  uint32_t has_task_expiration;
  uint64_t task_expiration;
  uint32_t has_report_expiry_age;
  uint64_t report_expiry_age;
} jx_upload_checks;
typedef struct jx_upload_req_info_t {
  uint64_t n, m; /* uploads; accepted */
  uint64_t leader_enc_bytes, leader_payload_bytes, helper_enc_bytes, helper_payload_bytes;
  uint64_t status_count[6]; /* uploads by JX_UPLOAD_* */
} jx_upload_req_info_t;
typedef struct jx_upload_req_arrays_t {
  /* on the device; the m accepted reports */
  const void *d_index, *d_report_ids, *d_times, *d_public_shares, *d_key_index, *d_leader_encs, *d_leader_enc_offsets,
      *d_leader_payloads, *d_leader_payload_offsets, *d_helper_config_ids, *d_helper_encs, *d_helper_enc_offsets,
      *d_helper_payloads, *d_helper_payload_offsets;
  /* on the device; all n uploads */
  const void *d_all_report_ids, *d_all_times, *d_upload_status, *d_row_of;
  /* the pinned host copy */
  const uint32_t* index;
  const uint64_t* times;
  const uint8_t* key_index;
  const uint64_t *leader_enc_offsets, *leader_payload_offsets, *helper_enc_offsets, *helper_payload_offsets;
  const uint8_t* helper_config_ids;
  const uint8_t* all_report_ids;
  const uint64_t* all_times;
  const uint8_t* upload_status;
  const uint32_t* row_of;
} jx_upload_req_arrays_t;
int32_t jx_report_encode_bound(const jx_engine* e, uint64_t n, uint32_t leader_enc_len, uint32_t helper_enc_len,
                               uint64_t* out_bound);
int32_t jx_report_encode_device(jx_engine* e, uint64_t n, const void* d_report_ids, const uint64_t* times,
                                const void* d_public_shares, const void* d_leader_encs, uint32_t leader_enc_len,
                                const void* d_leader_cts, const void* d_helper_encs, uint32_t helper_enc_len,
                                const void* d_helper_cts, uint8_t leader_config_id, uint8_t helper_config_id,
                                const void* d_seal_status, void* d_out, uint64_t capacity, void* d_out_offsets,
                                uint64_t* out_offsets, uint64_t* out_len);
int32_t jx_report_encode(jx_engine* e, uint64_t n, const uint8_t* report_ids, const uint64_t* times,
                         const uint8_t* public_shares, const uint8_t* leader_encs, uint32_t leader_enc_len,
                         const uint8_t* leader_cts, const uint8_t* helper_encs, uint32_t helper_enc_len,
                         const uint8_t* helper_cts, uint8_t leader_config_id, uint8_t helper_config_id,
                         const uint8_t* seal_status, uint8_t* out, uint64_t capacity, uint64_t* out_offsets,
                         uint64_t* out_len);
int32_t jx_upload_decode_device(jx_engine* e, const void* d_bodies, uint64_t len, uint64_t n, const uint64_t* body_offsets,
                                const jx_upload_checks* checks, const uint8_t key_first[256],
                                const uint8_t key_second[256], jx_upload_req** out);
int32_t jx_upload_decode(jx_engine* e, const uint8_t* bodies, uint64_t len, uint64_t n, const uint64_t* body_offsets,
                         const jx_upload_checks* checks, const uint8_t key_first[256], const uint8_t key_second[256],
                         jx_upload_req** out);
int32_t jx_upload_req_info(const jx_upload_req* r, jx_upload_req_info_t* out);
int32_t jx_upload_req_arrays(const jx_upload_req* r, jx_upload_req_arrays_t* out);
void jx_upload_req_release(jx_upload_req* r);

/* Accumulate the output shares of the resident batch `batch_id` (helper, or leader after finish) into
 * the engine's running batch aggregations (the engine as one shard, §8e): report i is added iff
 * verdict == FINISHED and accept_mask[i] != 0 (accept_mask nullable = all), into aggregation
 * `segment[i]` (any u32 batch-aggregation id; segment nullable = 0). Adds to the aggregate share, the
 * report count and the ReportIdChecksum (XOR of SHA-256(report id)). Any number of segments is handled
 * in one pass over the batch (device counting sort by segment). The batch is released: it is
 * accumulated at most once (a second call returns JX_E_STATE). The call returns once the accumulation is
 * queued on the engine stream (the host arrays are consumed before it returns); later calls on the engine
 * see its result (jx_aggregate_read / jx_engine_sync wait for it). A job-sized batch (<= 1,024 reports, no
 * accept_mask, one segment) is deferred: the engine keeps it and adds up to 64 such batches per aggregation
 * in one launch, when its queue is full or at the next call that reads, exports, resets or orders work
 * against the aggregations (jx_aggregate_*, jx_shard_record_export_device, jx_engine_sync,
 * jx_engine_record_event, jx_engine_join_stream, jx_engine_stream). */
int32_t jx_accumulate(jx_engine* e, uint64_t batch_id, uint64_t n, const uint8_t* accept_mask,
                      const uint32_t* segment);
/* Same with device arrays: d_accept_mask (nullable) and d_segment (nullable = all reports into
 * segment_ids[0]) holding, per report, an index into the host array segment_ids[nsegments]; reports
 * whose index is >= nsegments are skipped. segment_ids must not repeat an id (JX_E_INVALID).
 * Asynchronous on the engine stream. */
int32_t jx_accumulate_device(jx_engine* e, uint64_t batch_id, uint64_t n, const void* d_accept_mask,
                             const void* d_segment, const uint32_t* segment_ids, uint32_t nsegments);

/* Fused prep + accumulate (the metric's unit of work): prepare n reports and add every
 * finished one into aggregation `segment`. Host buffers; processed in capacity-sized chunks.
 * out_prep_msgs / out_verdicts nullable. */
int32_t jx_helper_prep_aggregate(jx_engine* e, uint64_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                 const uint8_t* helper_input_shares, const uint8_t* leader_prep_shares,
                                 uint32_t segment, uint8_t* out_prep_msgs, uint8_t* out_verdicts);

/* Same with DEVICE pointers (inputs already resident in HBM, e.g. from a torch tensor).
 * Report i goes to aggregation segment_ids[d_segment[i]] (d_segment nullable: all into
 * segment_ids[0]; indices >= nsegments are skipped; ids must not repeat); every finished report is
 * added. No batch is created (staging holds one launch at a time).
 * d_out_prep_msgs / d_out_verdicts are device pointers (nullable). Asynchronous on the engine
 * stream; call jx_engine_sync before reading results. */
int32_t jx_helper_prep_aggregate_device(jx_engine* e, uint64_t n, const void* d_nonces, const void* d_public_shares,
                                        const void* d_helper_input_shares, const void* d_leader_prep_shares,
                                        const void* d_segment, const uint32_t* segment_ids, uint32_t nsegments,
                                        void* d_out_prep_msgs, void* d_out_verdicts);

/* Read aggregation `segment`: encoded aggregate share (OUT x FB, LE), report count, checksum. */
int32_t jx_aggregate_read(jx_engine* e, uint32_t segment, uint8_t* out_agg, uint64_t* count);
int32_t jx_aggregate_checksum(jx_engine* e, uint32_t segment, uint8_t out_checksum[32]);
/* Zero every aggregation. */
int32_t jx_aggregate_reset(jx_engine* e);

/* Multi-GPU combine (compute_aggregate_share, aggregate_share.rs:87-95): write the encoded
 * aggregate share of `segment` to device buffer d_dst (OUT x FB bytes), and sum `nparts`
 * encoded shares laid out back to back at d_parts into d_out (mod p; RCCL's sum is not
 * field addition). Both asynchronous on the engine stream. */
int32_t jx_aggregate_export_device(jx_engine* e, uint32_t segment, void* d_dst);
int32_t jx_aggregate_combine_device(jx_engine* e, const void* d_parts, uint32_t nparts, void* d_out);

/* Shard records for the multi-GPU combine. A record is the encoded aggregate
 * share (OUT x FB) || report count (u64 LE) || checksum (32 B) of one aggregation: the state of
 * one batch_aggregations shard row that compute_aggregate_share merges
 * (aggregator/src/aggregator/aggregate_share.rs:55-96). Export writes this engine's record for
 * `segment` to device memory; combine merges `nrecords` records laid out back to back (e.g. the
 * output of an RCCL all-gather) into one: mod-p sum, count sum, checksum XOR. Both asynchronous
 * on the engine stream. jx_shard_record_bytes gives the record size. */
int32_t jx_shard_record_bytes(const jx_engine* e, uint32_t* bytes);
int32_t jx_shard_record_export_device(jx_engine* e, uint32_t segment, void* d_dst);
int32_t jx_shard_record_combine_device(jx_engine* e, const void* d_records, uint32_t nrecords, void* d_out);

/* ---- Collection, the protocol's last stage, at all three roles. Only NoDifferentialPrivacy is covered: no noise is
 * added to a share.
 *
 * jx_collect_seal* is the helper's handle_aggregate_share_generic (aggregator/src/aggregator.rs:2766-2965) and the
 * leader's collection step (collection_job_driver.rs) for njobs collection jobs in one call: per job, merge the shard
 * records it names (compute_aggregate_share, aggregate_share.rs:55-110: mod-p sum of the shares, sum of the counts, XOR
 * of the checksums), check the result, and seal the merged share to the collector (hpke::seal under
 * HpkeApplicationInfo(AggregateShare, Helper or Leader, Collector), associated data the job's encoded
 * AggregateShareAad). The records are the state of batch_aggregations rows as jx_shard_record_bytes /
 * jx_shard_record_export_device define them; a row without a share (count 0) is passed as a zero share.
 *   records          nrecords x jx_shard_record_bytes, back to back
 *   record_offsets   [njobs + 1], record_index[]: job j's records are records[record_index[k]] for k in
 *                    [record_offsets[j], record_offsets[j + 1]). Jobs may share records and name them in any order.
 *   expect_counts    [njobs] and expect_checksums [njobs x 32]: the other aggregator's report count and checksum (the
 *                    helper: from the AggregateShareReq); both NULL for the leader, which has nothing to compare against
 *   min_batch_size, max_batch_size   the task's (max 0 = none): task.validate_batch_size (task.rs:365-377)
 *   aads, aad_offsets [njobs + 1]    the encoded AggregateShareAad of each job, in the layout of jx_hpke_seal_*
 *   ephemeral_sks    njobs x 32: one X25519 private key per seal, from the caller's CSPRNG (jx_hpke.h)
 *   sender           a context of jx_hpke_create_sender holding the collector's public key
 *   out_status [njobs], out_counts [njobs] (u64), out_checksums [njobs x 32], out_encs [njobs x 32],
 *   out_cts [njobs x (OUT x FB + 16)], out_shares [njobs x OUT x FB] (nullable): the merged share unencrypted, which
 *                    Janus keeps in its AggregateShareJob so that a repeated request is served without a merge
 * out_status[j] is decided in Janus's order: JX_COLLECT_BAD_RECORD, an element of a record of the job is >= p (the
 * datastore's decode fails); JX_COLLECT_INVALID_BATCH_SIZE, the job names no record or its count is below
 * min_batch_size or above a non-zero max_batch_size; JX_COLLECT_BATCH_MISMATCH, expectations were given and the count or
 * the checksum differs (aggregator.rs:2927-2939); JX_COLLECT_SEAL_FAILED, X25519(skE, pkR) was all zero (a low-order
 * collector key); else JX_COLLECT_OK. The count and the checksum of every job are reported (BatchMismatch carries
 * them); enc, ciphertext and share of a job whose status is not JX_COLLECT_OK are zeros.
 * Refused before anything is queued, with nothing written: decreasing offsets, a record index >= nrecords, a record
 * named twice by one job, a context that is no sender context or lives on another device (JX_E_INVALID); a context of
 * the P-256 KEM (JX_E_UNSUPPORTED). njobs == 0 is JX_OK.
 * The host form waits for its results. The device form takes the records, the ephemeral keys and every output as
 * device pointers (8-byte aligned but for the status bytes) and the small arrays (offsets, indices, expectations, aads)
 * from the host: they are consumed before the call returns, and the kernels stay queued on the engine stream (one merge
 * launch for all jobs, one decision launch, the long seal's two, one that zeroes the refused jobs' outputs). */
#define JX_COLLECT_OK 0
#define JX_COLLECT_INVALID_BATCH_SIZE 1
#define JX_COLLECT_BATCH_MISMATCH 2
#define JX_COLLECT_BAD_RECORD 3
#define JX_COLLECT_SEAL_FAILED 4
int32_t jx_collect_seal(jx_engine* e, uint64_t njobs, const uint8_t* records, uint64_t nrecords,
                        const uint64_t* record_offsets, const uint32_t* record_index, const uint64_t* expect_counts,
                        const uint8_t* expect_checksums, uint64_t min_batch_size, uint64_t max_batch_size,
                        const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* ephemeral_sks, jx_hpke* sender,
                        uint8_t* out_status, uint64_t* out_counts, uint8_t* out_checksums, uint8_t* out_encs,
                        uint8_t* out_cts, uint8_t* out_shares);
int32_t jx_collect_seal_device(jx_engine* e, uint64_t njobs, const void* d_records, uint64_t nrecords,
                               const uint64_t* record_offsets, const uint32_t* record_index,
                               const uint64_t* expect_counts, const uint8_t* expect_checksums, uint64_t min_batch_size,
                               uint64_t max_batch_size, const uint8_t* aads, const uint64_t* aad_offsets,
                               const void* d_ephemeral_sks, jx_hpke* sender, void* d_out_status, void* d_out_counts,
                               void* d_out_checksums, void* d_out_encs, void* d_out_cts, void* d_out_shares);
/* jx_collect_open* is the collector (collector/src/lib.rs:573-629) for n collections: open the leader's and the
 * helper's encrypted aggregate share of each, decode both and add them mod p (Prio3.unshard before the decode of the
 * result).
 *   leader_opener, helper_opener   recipient contexts holding the collector's keypair with the
 *                    (AggregateShare, Leader -> Collector) and (AggregateShare, Helper -> Collector) application infos
 *   leader_encs, helper_encs       n x jx_hpke_enc_len of the context
 *   leader_cts / helper_cts with leader_ct_offsets / helper_ct_offsets [n + 1]   the ciphertexts, back to back
 *   aads, aad_offsets [n + 1]      the encoded AggregateShareAad of each collection, the same for both shares
 *   out_aggregates [n x OUT x FB]  the aggregate as canonical little-endian elements
 *   out_status [n]   JX_COLLECT_OPEN_OK; _LEADER / _HELPER: that share did not open; JX_COLLECT_DECODE_LEADER /
 *                    _HELPER: that share is not OUT x FB bytes, or holds an element >= p (Error::AggregateShareDecode)
 * The lengths are read from the offsets on the host: a collection with a share of another length than OUT x FB + 16
 * gets its status there (the leader's share first) and neither of its shares is opened. Of the others the leader's
 * open failing comes first, then the helper's, then the leader's decode, then the helper's. The row of a collection
 * whose status is not JX_COLLECT_OPEN_OK is zeros. A sender context, or a context on another device, is JX_E_INVALID
 * before anything is queued; n == 0 is JX_OK. The device form takes the encapsulated keys, the ciphertexts and the two
 * outputs as device pointers (out_aggregates 8-byte aligned) and the offsets and aads from the host; it stays queued
 * on the engine stream (per share the long open's two launches, then the check-and-add and the status launch). */
#define JX_COLLECT_OPEN_OK 0
#define JX_COLLECT_OPEN_LEADER 1
#define JX_COLLECT_OPEN_HELPER 2
#define JX_COLLECT_DECODE_LEADER 3
#define JX_COLLECT_DECODE_HELPER 4
int32_t jx_collect_open(jx_engine* e, jx_hpke* leader_opener, jx_hpke* helper_opener, uint64_t n,
                        const uint8_t* leader_encs, const uint8_t* leader_cts, const uint64_t* leader_ct_offsets,
                        const uint8_t* helper_encs, const uint8_t* helper_cts, const uint64_t* helper_ct_offsets,
                        const uint8_t* aads, const uint64_t* aad_offsets, uint8_t* out_aggregates, uint8_t* out_status);
int32_t jx_collect_open_device(jx_engine* e, jx_hpke* leader_opener, jx_hpke* helper_opener, uint64_t n,
                               const void* d_leader_encs, const void* d_leader_cts, const uint64_t* leader_ct_offsets,
                               const void* d_helper_encs, const void* d_helper_cts, const uint64_t* helper_ct_offsets,
                               const uint8_t* aads, const uint64_t* aad_offsets, void* d_out_aggregates,
                               void* d_out_status);

/* Wait for all work on the engine stream. Returns JX_E_INVALID if a combine since the last sync
 * met a non-canonical field element (>= p) in its inputs (the host merge rejects those too). */
int32_t jx_engine_sync(jx_engine* e);
/* The engine's HIP stream (hipStream_t), for callers that order their own work after it. */
int32_t jx_engine_stream(jx_engine* e, void** stream);

/* Producer / consumer ordering of the device-pointer entry points (see Conventions). None blocks the
 * host; all are stream-ordered.
 * jx_engine_wait_stream: engine work queued after this call starts only after all work queued on
 *   `stream` (hipStream_t; NULL = the null stream) so far has completed.
 * jx_engine_join_stream: work queued on `stream` after this call starts only after all engine work
 *   queued so far has completed.
 * jx_engine_wait_event / jx_engine_record_event: the same with a caller-owned hipEvent_t (the engine
 *   stream waits on the event's last record / records the event). With several host threads on one
 *   engine, a wait or join issued by one thread may also order another thread's calls: that only
 *   adds ordering, never removes it.
 * The reference needs none of this: Janus calls prio synchronously on owned values
 * (aggregator/src/aggregator.rs:1945-1967). */
int32_t jx_engine_wait_stream(jx_engine* e, void* stream);
int32_t jx_engine_join_stream(jx_engine* e, void* stream);
int32_t jx_engine_wait_event(jx_engine* e, void* event);
int32_t jx_engine_record_event(jx_engine* e, void* event);

/* Kernel timing with HIP events recorded on the engine stream around each stage.
 * enable != 0 starts collecting (and clears the totals). ms[0] = XOF stage (K1),
 * ms[1] = FLP stage (K3), ms[2] = accumulate (K4), ms[3] = slow-path kernel;
 * launches[0..3] = launch counts. Reading synchronizes the stream. */
int32_t jx_engine_timing(jx_engine* e, int32_t enable);
int32_t jx_engine_timing_read(jx_engine* e, float ms[4], uint64_t launches[4]);

/* Debug knobs (tests and measurements); any other option returns JX_E_INVALID.
 *   option 1: value != 0 routes every report through the slow XOF kernel K1';
 *   option 2: accumulate report chunks, 1..4096 (frees the staging);
 *   option 3: helper K1 kernel: 0 automatic (the fused two-sponge kernel; the lane-split kernel for
 *             launches under one fused wave per SIMD; the lane-pair kernel under one lane-split wave
 *             per SIMD; a word per lane up to one report-wave per SIMD), 3 lane-split, 5 fused,
 *             6 lane pairs, 7 a word per lane (6 and 7: bits <= 32).
 *   option 4: pipelines of jx_helper_prep_aggregate_device / jx_helper_prep_aggregate: 0 automatic
 *             (when a call of one segment spans two or more launches: 2 for the device form, 3 for the
 *             host form), 1 one stream, 2..4 that many (each with its own stream and staging; the
 *             launches alternate over them, their accumulations stay in launch order). A call runs with
 *             fewer when the arena cannot stage them all at once (jx_engine_memory: last_pipelines);
 *   option 5: reports per launch of the fused paths: 0 automatic (whole K1 rounds within ~48 GiB of
 *             staging), else >= 64 (rounded down to a multiple of 64);
 *   option 6: lane-split K1 workgroups per CU (its placement for chain-latency-bound launches): 2 default
 *             (at most two waves per SIMD), 0 no cap, 1..8;
 *   option 7: tests: the device coalescer's gathers wait, up to their window, until `value` jobs have joined
 *             (0: off); needs coalescing on (JX_E_STATE otherwise). Applies to the whole device coalescer;
 *   option 8: jx_accumulate of job-sized batches: 1 deferred and added together (default), 0 one launch per call
 *             (queued deferrals run first);
 *   option 9: run the deferred accumulations now;
 *   option 10: reports per launch of jx_client_shard_batch / _device: 0 automatic (what 4 GiB of scratch hold, at
 *             least 64), else that many;
 *   option 11: reports per launch of jx_client_seal_batch / _device: 0 automatic (2^20), else that many;
 *   option 12: waves per report of the gather of jx_upload_decode* and the pack of jx_report_encode*: 0 automatic
 *             (one, or more when few reports with long fields would leave the device idle), else 1..64. */
int32_t jx_engine_debug(jx_engine* e, int32_t option, int64_t value);

const char* jx_status_str(int32_t status);
const char* jx_last_error(const jx_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* JX_PRIO3_H */
