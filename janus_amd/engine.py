"""Batched Prio3 helper preparation + aggregation on one MI355X (wrapper of include/jx_prio3.h).

This is the host-side mirror of the prio `vdaf::Aggregator` + ping-pong surface that
Janus calls per report at /root/reference/aggregator/src/aggregator.rs:1945-1967:

    vdaf.helper_initialized(verify_key, agg_param, nonce, public_share, input_share,
                            leader_message).and_then(|t| t.evaluate(&vdaf))

`HelperEngine.helper_initialized_batch` does that for a whole batch and returns, per
report, either the outbound `PingPongMessage::Finish{prep_msg}` or a verdict naming the
`PingPongError` variant (labels of aggregator/src/aggregator/error.rs:379-424), plus the
handle of the new resident batch (one per aggregation job in flight; any number can be
resident). `aggregate_records` turns a batch into per-batch-identifier deltas
(BatchAggregation rows to merge with `merged_with`, aggregator_core/src/datastore/
models.rs:1275-1330) without changing the engine, so a retried datastore transaction can
recompute them; `accumulate` merges a batch into the engine's running aggregations (the
engine as one shard) and releases it.

Device-pointer methods (`*_device`) order themselves against a torch stream (default: the current
stream of the engine's device): the engine's work waits for everything queued on that stream before
the call (the producer of the inputs), and work queued on that stream afterwards waits for the
engine's (the consumer of the outputs, and torch's allocator reusing the inputs). So tensors produced
and consumed on torch's current stream need no `sync()`. Pass `stream=False` to order by hand
(`wait_stream` / `join_stream` / events), e.g. to keep two engines' jobs overlapping.

Resident batches hold device memory until released: `helper_initialized_batch(keep=False)` drops the
batch at once, `resident(batch_id)` is a context manager that releases it on exit, and the aggregator
paths release in `finally`.

All compute runs in the HIP kernels of libjanus_prio3.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes
import threading
import weakref
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import EngineError, JxParams, check
from .vdaf import Prio3

FINISHED = 0
PREPARE_INIT_FAILURE = 1
PREP_SHARE_DECODE_FAILURE = 2
PREPARE_MESSAGE_FAILURE = 3
PREPARE_NEXT_FAILURE = 4
HELPER_STEP_FAILURE = 5  # leader only: the helper rejected the report
OPEN_FAILURE = 6  # encrypted inputs: the report never reached helper_initialized (see open_status)
VERDICT_LABELS = {
    FINISHED: "finished",
    PREPARE_INIT_FAILURE: "prepare_init_failure",
    PREP_SHARE_DECODE_FAILURE: "leader_prep_share_decode_failure",
    PREPARE_MESSAGE_FAILURE: "prepare_message_failure",
    PREPARE_NEXT_FAILURE: "prepare_next_failure",
    HELPER_STEP_FAILURE: "helper_step_failure",
}
# open status of an encrypted input share (include/jx_prio3.h JX_OPEN_*; aggregator.rs:1781-1910):
# (janus_step_failures label, PrepareError value)
OPEN_OK = 0
SHARD_INVALID_MEASUREMENT = 1  # jx_client_shard_*: the measurement is out of range (JX_SHARD_INVALID_MEASUREMENT)
SEAL_OK, SEAL_SKIPPED, SEAL_ZERO_DH = 0, 1, 2  # jx_client_seal_*: JX_SEAL_* (include/jx_prio3.h)
SHARD_MAX_P = 1024             # JX_SHARD_MAX_P: the largest transform size (gadget-call points) the prover holds
KEY_NONE, KEY_MALFORMED = 0xFF, 0xFE
ENC_REQUIRE_TASKPROV = 1
OPEN_STATUS = {
    1: ("decrypt_failure", 4),                           # HpkeDecryptError
    2: ("plaintext_input_share_decode_failure", 8),      # InvalidMessage
    3: ("duplicate_extension", 8),
    4: ("unexpected_taskprov_extension", 8),
    5: ("missing_or_malformed_taskprov_extension", 8),
    6: ("input_share_decode_failure", 8),
    7: ("unknown_hpke_config_id", 3),                    # HpkeUnknownConfigId
}


def _ptr(a: np.ndarray | None):
    if a is None:
        return None
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return a.ctypes.data_as(ctypes.c_void_p)


def _u8(a, n: int, width: int, what: str) -> np.ndarray:
    arr = np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a,
                               dtype=np.uint8)
    if width == 0:
        return np.zeros((max(n, 1), 1), np.uint8)
    arr = arr.reshape(n, width) if arr.size == n * width else None
    if arr is None:
        raise ValueError(f"{what}: expected {n} x {width} bytes")
    return arr


_U64P = ctypes.POINTER(ctypes.c_uint64)


def _u64p(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(_U64P)


def _items(a, n: int, dtype, *row) -> np.ndarray:
    """n items (rows of shape `row`) of dtype, contiguous; a 1-item dummy the call never reads when n is 0."""
    if not n:
        return np.zeros((1, *row), dtype)
    return np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(n, *row))


def _offs(a, n: int) -> np.ndarray:
    """n + 1 uint64 offsets, contiguous."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(n + 1))


def _packed(items) -> tuple[np.ndarray, np.ndarray]:
    """Byte strings laid back to back (one zero byte when there are none) and their len(items) + 1 offsets."""
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(x) for x in items) or b"\0", np.uint8).copy(), off


def _seg_table(segment_ids):
    ids = np.ascontiguousarray(np.asarray(segment_ids, dtype=np.uint32).reshape(-1))
    if ids.size == 0:
        raise ValueError("at least one segment id")
    return ids, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


@dataclass
class LeaderInit:
    verdicts: np.ndarray       # uint8[n]: 0 initialized, 1 prepare_init_failure
    prep_shares: np.ndarray    # uint8[n, LPS]: payloads of PingPongMessage::Initialize
    batch_id: int = 0          # the resident leader batch (finish / records / accumulate / release)


@dataclass
class BatchResult:
    verdicts: np.ndarray       # uint8[n]
    prep_msgs: np.ndarray      # uint8[n, PM]
    out_shares: np.ndarray | None  # uint8[n, OUT*FB]
    batch_id: int = 0          # the resident batch these results belong to (records / accumulate / release)

    def finished(self) -> np.ndarray:
        return self.verdicts == FINISHED


@dataclass
class EncryptedResult:
    verdicts: np.ndarray       # uint8[n]: as BatchResult, OPEN_FAILURE where the share did not open / decode
    prep_msgs: np.ndarray      # uint8[n, PM]
    open_status: np.ndarray    # uint8[n]: OPEN_OK or an OPEN_STATUS key
    batch_id: int = 0


@dataclass
class UploadOpen:
    status: np.ndarray         # uint8[n]: OPEN_OK or an OPEN_STATUS key (never 3-5: the upload path has no such checks)
    extensions: list           # per report: its extension list's bytes, without the u16 prefix (b"" when rejected)
    rows: object               # torch uint8[n, lis_stride] on the device: the leader input shares, zeros when rejected
    lis_stride: int


@dataclass
class ShardResult:
    public_shares: np.ndarray        # uint8[n, PS]
    leader_input_shares: np.ndarray  # uint8[n, LIS]: measurement share || proof share || [blind]
    helper_input_shares: np.ndarray  # uint8[n, HIS]: k_meas || k_proofs || [blind]
    status: np.ndarray               # uint8[n]: 0, or SHARD_INVALID_MEASUREMENT (the report's rows are zeros)


@dataclass
class SealResult:
    leader_encs: np.ndarray   # uint8[n, 32]
    leader_cts: np.ndarray    # uint8[n, 6 + LIS + 16]
    helper_encs: np.ndarray   # uint8[n, 32]
    helper_cts: np.ndarray    # uint8[n, 6 + HIS + 16]
    status: np.ndarray        # uint8[n]: SEAL_OK, SEAL_SKIPPED or SEAL_ZERO_DH


# jx_collect_seal*: JX_COLLECT_* (include/jx_prio3.h), in the order they are decided but for the numbering
COLLECT_OK, COLLECT_INVALID_BATCH_SIZE, COLLECT_BATCH_MISMATCH, COLLECT_BAD_RECORD, COLLECT_SEAL_FAILED = 0, 1, 2, 3, 4
# jx_collect_open*: JX_COLLECT_OPEN_* / JX_COLLECT_DECODE_*
COLLECT_OPEN_OK, COLLECT_OPEN_LEADER, COLLECT_OPEN_HELPER, COLLECT_DECODE_LEADER, COLLECT_DECODE_HELPER = 0, 1, 2, 3, 4


@dataclass
class CollectSeal:
    status: np.ndarray        # uint8[njobs]: COLLECT_*
    counts: np.ndarray        # uint64[njobs]: the merged report counts
    checksums: np.ndarray     # uint8[njobs, 32]: the merged checksums
    encs: np.ndarray          # uint8[njobs, 32]
    cts: np.ndarray           # uint8[njobs, OUT * FB + 16]
    shares: np.ndarray | None  # uint8[njobs, OUT * FB]: the merged shares, unencrypted (want_shares)


@dataclass
class CollectOpen:
    aggregates: np.ndarray    # uint8[n, OUT * FB]: canonical little-endian elements, zeros where status != 0
    status: np.ndarray        # uint8[n]: COLLECT_OPEN_* / COLLECT_DECODE_*


WIRE_OK, WIRE_MALFORMED, WIRE_WRONG_QUERY_TYPE, WIRE_DUPLICATE_ID = 0, 1, 2, 3  # JX_WIRE_* (request status)
WIRE_REPORT_ODD_PUBLIC_SHARE, WIRE_REPORT_NOT_INITIALIZE, WIRE_REPORT_ODD_PREP_SHARE = 1, 2, 3  # wire_status
WIRE_NO_ERROR = 0xFF           # JX_WIRE_NO_ERROR: no host-resolved error for the report
ROUTE_OUT = 0xFFFFFFFF         # route[i] of a report that must not reach an aggregation
ROUTE_OK, ROUTE_TOO_MANY_BUCKETS, ROUTE_MAX_BUCKETS = 0, 1, 1024  # JX_ROUTE_*
ROUTE_BUCKET = np.dtype([("start", "<u8"), ("min_time", "<u8"), ("max_time", "<u8"), ("reports", "<u4"), ("routed", "<u4"),
                         ("collected", "<u4"), ("pad_", "<u4")])  # jx_route_bucket
WIRE_RECORD = np.dtype([(name, "<u8") for name in ("off", "len", "public_share_off", "enc_off", "payload_off", "message_off",
                                                    "prep_msg_off", "prep_share_off")] +
                       [(name, "<u4") for name in ("public_share_len", "enc_len", "payload_len", "message_len",
                                                    "prep_msg_len", "prep_share_len")] +
                       [("config_id", "u1"), ("ping_pong_type", "u1"), ("pad_", "u1", 6)])


class _DeviceBytes:
    """Device memory as torch sees it (__cuda_array_interface__): no copy, no ownership."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class _Req:
    """What the request handles share: a C handle that owns device arrays and a pinned host copy of the small ones.
    A subclass names its release symbol (_RELEASE) and the attributes whose memory goes with the handle (_VIEWS)."""

    def __init__(self, engine: "HelperEngine", handle):
        self._engine, self._h = engine, handle

    @staticmethod
    def view(ptr, dtype, count):  # count items at ptr, the handle's pinned host memory, without a copy
        if count == 0:
            return np.zeros(0, dtype)
        buf = (ctypes.c_uint8 * (np.dtype(dtype).itemsize * count)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=count)

    def _device_tensor(self, name: str, size: int):  # d.d_<name> as torch uint8[size]; empty when there is none
        import torch

        dev = torch.device("cuda", self._engine.device)
        ptr = getattr(self.d, "d_" + name) if self.d is not None else None
        if not size or not ptr:
            return torch.zeros(0, dtype=torch.uint8, device=dev)
        return torch.as_tensor(_DeviceBytes(ptr, size), device=dev)

    def release(self):
        if self._h:
            for name in self._VIEWS:  # the views' memory goes with the handle
                setattr(self, name, None)
            getattr(self._engine._L, self._RELEASE)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()


class InitReq(_Req):
    """A decoded AggregationJobInitializeReq (jx_init_req): the request's status, and for an accepted one the device
    arrays the sealed fused call reads (`d`, a _lib.JxInitReqArrays of device pointers) with the pinned host copy of
    the small ones as numpy views: times, enc_offsets, payload_offsets, key_index, wire_status, report_ids, records
    (WIRE_RECORD). Holds device memory until release() (or the end of a `with`), which must come before the engine's
    close()."""

    _RELEASE = "jx_init_req_release"
    _VIEWS = ("times", "enc_offsets", "payload_offsets", "records", "report_ids", "key_index", "wire_status", "d")

    def __init__(self, engine: "HelperEngine", handle):
        super().__init__(engine, handle)
        L = engine._L
        info = _lib.JxInitReqInfo()
        check(L.jx_init_req_info(handle, ctypes.byref(info)), engine._h, "jx_init_req_info")
        self.status, self.error_offset, self.duplicate_index = int(info.status), int(info.error_offset), int(info.duplicate_index)
        self.n = int(info.n)
        self.batch_id = bytes(info.batch_id) if info.has_batch_id else None
        self.agg_param_span = (int(info.agg_param_off), int(info.agg_param_len))
        self.fallback_iterations, self.odd_public_shares = int(info.fallback_iterations), int(info.odd_public_shares)
        self.enc_bytes, self.payload_bytes = int(info.enc_bytes), int(info.payload_bytes)
        self.d = None
        n = self.n
        if self.status == WIRE_OK and n:
            a = _lib.JxInitReqArrays()
            check(L.jx_init_req_arrays(handle, ctypes.byref(a)), engine._h, "jx_init_req_arrays")
            self.d, view = a, self.view
            self.times = view(a.times, np.uint64, n)
            self.enc_offsets = view(a.enc_offsets, np.uint64, n + 1)
            self.payload_offsets = view(a.payload_offsets, np.uint64, n + 1)
            self.records = view(a.records, WIRE_RECORD, n)
            self.report_ids = view(a.report_ids, np.uint8, 16 * n).reshape(n, 16)
            self.key_index = view(a.key_index, np.uint8, 2 * n).reshape(n, 2)
            self.wire_status = view(a.wire_status, np.uint8, n)
        else:
            self.n = n if self.status == WIRE_DUPLICATE_ID else 0
            self.times, self.enc_offsets, self.payload_offsets = np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
            self.records, self.report_ids = np.zeros(0, WIRE_RECORD), np.zeros((0, 16), np.uint8)
            self.key_index, self.wire_status = np.zeros((0, 2), np.uint8), np.zeros(0, np.uint8)

    def device_bytes(self, name: str):
        """One of the device arrays (report_ids, times, public_shares, leader_prep_shares, encs, enc_offsets, payloads,
        payload_offsets, key_index, wire_status, route, records; bucket_index, bucket_collected once the request is
        routed) as a torch uint8 tensor over the handle's memory."""
        e, n = self._engine, self.n
        if name in ("bucket_index", "bucket_collected"):
            import torch

            ptrs = (ctypes.c_void_p(), ctypes.c_void_p())
            check(e._L.jx_init_req_route_arrays(self._h, ctypes.byref(ptrs[0]), ctypes.byref(ptrs[1])), e._h,
                  "jx_init_req_route_arrays")
            ptr, size = (ptrs[0].value, 4 * n) if name == "bucket_index" else (ptrs[1].value, n)
            dev = torch.device("cuda", e.device)
            if not size or not ptr:
                return torch.zeros(0, dtype=torch.uint8, device=dev)
            return torch.as_tensor(_DeviceBytes(ptr, size), device=dev)
        size = {"report_ids": 16 * n, "times": 8 * n, "public_shares": n * e.public_share_len,
                "leader_prep_shares": n * e.prep_share_len, "encs": self.enc_bytes, "enc_offsets": 8 * (n + 1),
                "payloads": self.payload_bytes, "payload_offsets": 8 * (n + 1), "key_index": 2 * n, "wire_status": n,
                "route": 4 * n, "records": WIRE_RECORD.itemsize * n}[name]
        return self._device_tensor(name, size)

    def exclude(self, mask):
        """Route the reports with mask[i] away from every aggregation (jx_init_req_exclude)."""
        m = _items(np.asarray(mask).astype(np.uint8), self.n, np.uint8)
        check(self._engine._L.jx_init_req_exclude(self._h, _ptr(m)), self._engine._h, "jx_init_req_exclude")

    def route(self, time_precision: int, collected=()):
        """Route the reports to their batch buckets, the report time rounded down to time_precision, on the GPU
        (jx_init_req_route). collected: the starts of the batches that no longer accept aggregations, in any order.
        Returns (ROUTE_OK, the bucket table as a ROUTE_BUCKET array, ascending by start): route[i] is then the index of
        report i's bucket in the table, or ROUTE_OUT; or (ROUTE_TOO_MANY_BUCKETS, an empty table) for a request of
        more than ROUTE_MAX_BUCKETS buckets, which leaves the request as it was."""
        e = self._engine
        col = np.ascontiguousarray(np.asarray(list(collected), dtype=np.uint64))
        table = np.zeros(ROUTE_MAX_BUCKETS, ROUTE_BUCKET)
        status, nb = ctypes.c_uint32(), ctypes.c_uint32()
        check(e._L.jx_init_req_route(e._h, self._h, time_precision, _u64p(col) if col.size else None, col.size,
                                     ctypes.byref(status), ctypes.byref(nb), _ptr(table)), e._h, "jx_init_req_route")
        return int(status.value), table[:nb.value].copy()


WIRE_RESP_MISMATCH = 4         # JX_WIRE_RESP_MISMATCH: the response's PrepareResps are not the sent reports in order
RESP_CONTINUED, RESP_REJECTED, RESP_FINISHED, RESP_MESSAGE_MISMATCH = 0, 1, 2, 3  # JX_RESP_*


class LeaderReq(_Req):
    """An encoded AggregationJobInitializeReq (jx_leader_req): `body` (bytes; the device form copies it from its
    device buffer `d_body`, a torch uint8 tensor, when first asked), `body_len`, `n` (rows of the leader batch),
    `n_sent` and `sent_index` (numpy uint32[n_sent]: sent report k is row sent_index[k]; `d_sent_index` is the same
    list on the device). Holds device memory until release() (or the end of a `with`), which must come before the
    engine's close()."""

    _RELEASE = "jx_leader_req_release"
    _VIEWS = ("d_sent_index",)

    def __init__(self, engine: "HelperEngine", handle, body: bytes | None = None, d_body=None):
        super().__init__(engine, handle)
        L = engine._L
        info = _lib.JxLeaderReqInfo()
        check(L.jx_leader_req_info(handle, ctypes.byref(info)), engine._h, "jx_leader_req_info")
        self.n, self.n_sent, self.body_len = int(info.n), int(info.n_sent), int(info.body_len)
        hp, dp = ctypes.c_void_p(), ctypes.c_void_p()
        check(L.jx_leader_req_sent(handle, ctypes.byref(hp), ctypes.byref(dp)), engine._h, "jx_leader_req_sent")
        self.d_sent_index = dp.value
        self.sent_index = self.view(hp.value, np.uint32, self.n_sent).copy()
        self._body, self.d_body = body, d_body

    @property
    def body(self) -> bytes:
        if self._body is None:
            self._body = self.d_body[:self.body_len].cpu().numpy().tobytes()
        return self._body


@dataclass
class InitRespDecode:
    status: int                # WIRE_OK, WIRE_MALFORMED or WIRE_RESP_MISMATCH
    results: np.ndarray        # uint8[n_sent]: RESP_* per response (meaningful when status is WIRE_OK)
    errors: np.ndarray         # uint8[n_sent]: the PrepareError code point, WIRE_NO_ERROR where continued
    error_offset: int = 0      # WIRE_MALFORMED: the read that failed
    mismatch_index: int = 0    # WIRE_RESP_MISMATCH: the first position that differs
    n: int = 0                 # PrepareResps in the body


# JX_UPLOAD_*: upload_status of jx_upload_decode
UPLOAD_OK, UPLOAD_MALFORMED, UPLOAD_TOO_EARLY, UPLOAD_TASK_EXPIRED, UPLOAD_EXPIRED, UPLOAD_ODD_PUBLIC_SHARE = range(6)
UPLOAD_NO_ROW = 0xFFFFFFFF     # row_of[i] of an upload that is not accepted


class UploadReq(_Req):
    """A batch of decoded upload bodies (jx_upload_req). For all n uploads, numpy views of the pinned host copy:
    status (UPLOAD_*), row_of (UPLOAD_NO_ROW where not accepted), report_ids (n x 16) and all_times. For the m accepted
    reports, dense and in order: index (accepted report k is upload index[k]), times, key_index (m x 2),
    leader_enc_offsets / leader_payload_offsets / helper_enc_offsets / helper_payload_offsets (m + 1 each) and
    helper_config_ids; `d` holds the device pointers (a _lib.JxUploadReqArrays), in the form leader_upload_open's device
    call and encode_init_req take. Holds device memory until release() (or the end of a `with`), which must come before
    the engine's close()."""

    _VIEWS = ("status", "row_of", "report_ids", "all_times", "index", "times", "key_index", "leader_enc_offsets",
              "leader_payload_offsets", "helper_enc_offsets", "helper_payload_offsets", "helper_config_ids", "d")
    _RELEASE = "jx_upload_req_release"

    def __init__(self, engine: "HelperEngine", handle):
        super().__init__(engine, handle)
        L = engine._L
        info = _lib.JxUploadReqInfo()
        check(L.jx_upload_req_info(handle, ctypes.byref(info)), engine._h, "jx_upload_req_info")
        self.n, self.m = int(info.n), int(info.m)
        self.leader_enc_bytes, self.leader_payload_bytes = int(info.leader_enc_bytes), int(info.leader_payload_bytes)
        self.helper_enc_bytes, self.helper_payload_bytes = int(info.helper_enc_bytes), int(info.helper_payload_bytes)
        self.status_count = [int(x) for x in info.status_count]
        n, m = self.n, self.m
        a = _lib.JxUploadReqArrays()  # all null for a call of no uploads
        check(L.jx_upload_req_arrays(handle, ctypes.byref(a)), engine._h, "jx_upload_req_arrays")
        self.d, view = (a if n else None), self.view
        offs = (lambda p: view(p, np.uint64, m + 1)) if n else (lambda p: np.zeros(1, np.uint64))
        self.status = view(a.upload_status, np.uint8, n)
        self.row_of = view(a.row_of, np.uint32, n)
        self.report_ids = view(a.all_report_ids, np.uint8, 16 * n).reshape(n, 16)
        self.all_times = view(a.all_times, np.uint64, n)
        self.index = view(a.index, np.uint32, m)
        self.times = view(a.times, np.uint64, m)
        self.key_index = view(a.key_index, np.uint8, 2 * m).reshape(m, 2)
        self.leader_enc_offsets, self.leader_payload_offsets = offs(a.leader_enc_offsets), offs(a.leader_payload_offsets)
        self.helper_enc_offsets, self.helper_payload_offsets = offs(a.helper_enc_offsets), offs(a.helper_payload_offsets)
        self.helper_config_ids = view(a.helper_config_ids, np.uint8, m)

    def device_bytes(self, name: str):
        """One of the device arrays of the accepted reports (report_ids, public_shares, leader_encs, leader_payloads,
        helper_encs, helper_payloads) as a torch uint8 tensor over the handle's memory."""
        e, m = self._engine, self.m
        size = {"report_ids": 16 * m, "public_shares": m * e.public_share_len, "leader_encs": self.leader_enc_bytes,
                "leader_payloads": self.leader_payload_bytes, "helper_encs": self.helper_enc_bytes,
                "helper_payloads": self.helper_payload_bytes}[name]
        return self._device_tensor(name, size)


class HelperEngine:
    """One engine per (Prio3 instance, verify key, GPU). Serves the helper role (the north-star
    path) and the leader role of the same ping-pong exchange."""

    _leader_n = 0
    _leader_id = 0

    def __init__(self, vdaf: Prio3, verify_key: bytes, device: int = 0):
        # guards the per-instance defaults (last leader batch) when threads share the engine; the
        # C engine serializes the calls themselves
        self._lock = threading.Lock()
        self._init_reqs = weakref.WeakSet()  # live request handles: they hold the engine's arena memory
        if len(verify_key) != vdaf.verify_key_len:
            raise ValueError(f"verify key must be {vdaf.verify_key_len} bytes for {vdaf.name()} "
                             "(VERIFY_KEY_LENGTH / VERIFY_KEY_LENGTH_HMACSHA256_AES128, core/src/vdaf.rs:16,24)")
        self.vdaf = vdaf
        self.device = device
        L = _lib.load()
        self._L = L
        p = JxParams(vdaf.algo_id, vdaf.bits, vdaf.length, vdaf.chunk_length, vdaf.num_proofs)
        h = ctypes.c_void_p()
        vk = (ctypes.c_uint8 * len(verify_key)).from_buffer_copy(verify_key)
        st = L.jx_engine_create_ex(ctypes.byref(p), ctypes.cast(vk, ctypes.c_void_p), len(verify_key), device,
                                   ctypes.byref(h))
        if st != 0:  # no engine to ask: the reason a parameter set was refused is this thread's last error
            why = L.jx_last_error(None).decode()
            raise EngineError(f"jx_engine_create({vdaf.name()}): {L.jx_status_str(st).decode()} ({st}) {why}".strip())
        self._h = h
        sizes = [ctypes.c_uint32() for _ in range(6)]
        check(L.jx_engine_sizes(h, *[ctypes.byref(s) for s in sizes]), h, "jx_engine_sizes")
        self.public_share_len, self.helper_input_share_len, self.prep_share_len, self.prep_msg_len, \
            self.output_len, self.field_bytes = (s.value for s in sizes)
        lis = ctypes.c_uint32()
        check(L.jx_engine_leader_sizes(h, ctypes.byref(lis)), h, "jx_engine_leader_sizes")
        self.leader_input_share_len = lis.value

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            for r in list(self._init_reqs):
                r.release()
            self._L.jx_engine_destroy(self._h)
            self._h = None

    def _track(self, req):
        """Remember a request handle so that close() releases it if its owner has not."""
        with self._lock:
            self._init_reqs.add(req)
        return req

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # ------------------------------------------------------------------ stream ordering
    def _stream_handle(self, stream):
        """hipStream_t of `stream` (None: torch's current stream on the engine's device; a torch
        stream; or an integer handle); None when the caller orders by hand (stream=False)."""
        if stream is False:
            return None
        if stream is None:
            try:
                import torch
            except ImportError:  # raw device pointers without torch: the caller orders by hand
                return None
            stream = torch.cuda.current_stream(self.device)
        return int(getattr(stream, "cuda_stream", stream))

    def wait_stream(self, stream=None):
        """Engine work queued from now on waits for all work queued on `stream` so far."""
        h = self._stream_handle(stream)
        check(self._L.jx_engine_wait_stream(self._h, h or None), self._h, "jx_engine_wait_stream")

    def join_stream(self, stream=None):
        """Work queued on `stream` from now on waits for all engine work queued so far."""
        h = self._stream_handle(stream)
        check(self._L.jx_engine_join_stream(self._h, h or None), self._h, "jx_engine_join_stream")

    def wait_event(self, event):
        """The engine stream waits on a torch.cuda.Event (or hipEvent_t handle) recorded by the caller."""
        check(self._L.jx_engine_wait_event(self._h, int(getattr(event, "cuda_event", event))), self._h,
              "jx_engine_wait_event")

    def record_event(self, event):
        """Record a torch.cuda.Event (or hipEvent_t handle) on the engine stream."""
        h = int(getattr(event, "cuda_event", event))
        if h == 0 and hasattr(event, "record"):  # torch creates its event on the first record
            event.record()
            h = int(event.cuda_event)
        check(self._L.jx_engine_record_event(self._h, h), self._h, "jx_engine_record_event")

    @contextlib.contextmanager
    def _ordered(self, stream):
        h = self._stream_handle(stream)
        if h is None:  # stream=False (ordered by hand), or no torch to order against
            yield
            return
        check(self._L.jx_engine_wait_stream(self._h, h or None), self._h, "jx_engine_wait_stream")
        try:
            yield
        except BaseException:
            # the join still orders whatever the failed call queued; its own error must not hide the call's
            self._L.jx_engine_join_stream(self._h, h or None)
            raise
        check(self._L.jx_engine_join_stream(self._h, h or None), self._h, "jx_engine_join_stream")

    # ------------------------------------------------------------------ prepare
    def helper_initialized_batch(self, nonces, public_shares, helper_input_shares, leader_prep_shares,
                                 want_out_shares: bool = False, keep: bool = True) -> BatchResult:
        """prio ping-pong helper_initialized + evaluate for n reports (host buffers).

        leader_prep_shares are the prep_share payloads of the leaders'
        PingPongMessage::Initialize (fixed length; the aggregator layer rejects other
        lengths as leader_prep_share_decode_failure before calling this). keep=False releases the
        new resident batch before returning (callers that want only verdicts / prep messages /
        output shares); the result's batch_id is then 0."""
        n = len(nonces) // 16 if isinstance(nonces, (bytes, bytearray)) else int(np.asarray(nonces).shape[0])
        nn = _u8(nonces, n, 16, "nonces")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        his = _u8(helper_input_shares, n, self.helper_input_share_len, "helper_input_shares")
        lps = _u8(leader_prep_shares, n, self.prep_share_len, "leader_prep_shares")
        verdicts = np.zeros(max(n, 1), np.uint8)
        msgs = np.zeros((max(n, 1), max(self.prep_msg_len, 1)), np.uint8)
        outs = np.zeros((max(n, 1), self.output_len * self.field_bytes), np.uint8) if want_out_shares else None
        bid = ctypes.c_uint64()
        st = self._L.jx_helper_prep_batch(self._h, n, _ptr(nn), _ptr(ps) if self.public_share_len else None,
                                          _ptr(his), _ptr(lps), _ptr(msgs) if self.prep_msg_len else None,
                                          _ptr(verdicts), _ptr(outs), ctypes.byref(bid))
        check(st, self._h, "jx_helper_prep_batch")
        if not keep:
            self.release(bid.value)
            bid.value = 0
        return BatchResult(verdicts[:n], msgs[:n, : self.prep_msg_len], outs[:n] if outs is not None else None,
                           bid.value)

    def helper_initialized_encrypted_batch(self, nonces, times, public_shares, task_id: bytes, keypairs,
                                           key_index, encs, payloads: list[bytes], leader_prep_shares,
                                           require_taskprov: bool = False, keep: bool = True) -> "EncryptedResult":
        """The helper's per-report loop from the encrypted report share to helper_initialized + evaluate
        (aggregator.rs:1763-1967), on the GPU for the whole job (jx_helper_prep_encrypted_batch2): report i
        is opened with keypairs[key_index[i][0]] (then keypairs[key_index[i][1]] if that fails to decrypt;
        KEY_NONE: none), its PlaintextInputShare decoded and checked, and prepared. encs: an (n, 32) array, or a
        list of the reports' encapsulated keys of any lengths (32 bytes under X25519, 65 under P-256); a trial of
        a keypair whose KEM has another length fails without an open. keypairs: janus_amd.hpke.HpkeOpener contexts on this engine's
        device. Returns verdicts (OPEN_FAILURE where the share did not open / decode), prep messages, the
        open status per report (OPEN_STATUS) and the batch handle."""
        n = int(np.asarray(nonces).reshape(-1, 16).shape[0])
        nn = _u8(nonces, n, 16, "nonces")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        lps = _u8(leader_prep_shares, n, self.prep_share_len, "leader_prep_shares")
        tm = _items(times, n, np.uint64)
        ki = _items(key_index, n, np.uint8, 2)
        if isinstance(encs, (list, tuple)):
            if len(encs) != n:
                raise ValueError("one encapsulated key per report")
            en, eoff = _packed(encs)
        else:
            en = _u8(encs, n, 32, "encs") if n else np.zeros((1, 32), np.uint8)
            eoff = np.arange(n + 1, dtype=np.uint64) * 32
        if len(task_id) != 32 or len(payloads) != n:
            raise ValueError("task id is 32 bytes; one payload per report")
        ct, off = _packed(payloads)
        task = np.frombuffer(task_id, np.uint8).copy()
        hs = (ctypes.c_void_p * max(1, len(keypairs)))(*[k.handle for k in keypairs])
        verdicts = np.zeros(max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        msgs = np.zeros((max(n, 1), max(self.prep_msg_len, 1)), np.uint8)
        bid = ctypes.c_uint64()
        st = self._L.jx_helper_prep_encrypted_batch2(
            self._h, n, _ptr(nn), _u64p(tm), _ptr(ps) if self.public_share_len else None, _ptr(task), hs, len(keypairs),
            _ptr(ki), _ptr(en), _u64p(eoff), _ptr(ct), _u64p(off), ENC_REQUIRE_TASKPROV if require_taskprov else 0,
            _ptr(lps), _ptr(msgs) if self.prep_msg_len else None, _ptr(verdicts), _ptr(status), ctypes.byref(bid))
        check(st, self._h, "jx_helper_prep_encrypted_batch2")
        if not keep:
            self.release(bid.value)
            bid.value = 0
        return EncryptedResult(verdicts[:n], msgs[:n, : self.prep_msg_len], status[:n], bid.value)

    def batch_id(self) -> int:
        """Handle of the most recently prepared batch if still resident (0 otherwise)."""
        b = ctypes.c_uint64()
        check(self._L.jx_engine_batch_id(self._h, ctypes.byref(b)), self._h, "jx_engine_batch_id")
        return b.value

    def resident_batches(self) -> tuple[int, int]:
        """(resident batches, device bytes they hold)."""
        n, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._L.jx_engine_batches(self._h, ctypes.byref(n), ctypes.byref(b)), self._h, "jx_engine_batches")
        return n.value, b.value

    def release(self, batch_id: int, missing_ok: bool = False):
        """Drop a resident batch (an aggregation job that is done or abandoned). missing_ok: a batch
        that is no longer resident (already accumulated or released) is not an error."""
        st = self._L.jx_batch_release(self._h, batch_id)
        if st == -5 and missing_ok:  # JX_E_STATE
            return
        check(st, self._h, "jx_batch_release")

    @contextlib.contextmanager
    def resident(self, batch_id: int):
        """Scope of a resident batch: released on exit unless accumulate already consumed it."""
        try:
            yield batch_id
        finally:
            if batch_id:
                self.release(batch_id, missing_ok=True)

    def aggregate_records(self, batch_id: int, n: int, accept_mask: np.ndarray | None = None,
                          segment_index: np.ndarray | None = None, nsegments: int = 1) -> list[tuple[bytes, int, bytes]]:
        """Per-batch-identifier deltas of a resident batch: for each of nsegments aggregations, the
        (encoded aggregate share, report count, checksum) of the finished reports i with
        accept_mask[i] and segment_index[i] == that index. Changes nothing on the engine: repeatable
        (a retried transaction recomputes the same rows), the batch stays resident."""
        m = None if accept_mask is None else np.ascontiguousarray(accept_mask, dtype=np.uint8)
        s = None if segment_index is None else np.ascontiguousarray(segment_index, dtype=np.uint32)
        rb = self.record_bytes()
        out = np.zeros(nsegments * rb, np.uint8)
        check(self._L.jx_batch_aggregate_records(self._h, batch_id, n, _ptr(m), _ptr(s), nsegments, _ptr(out)),
              self._h, "jx_batch_aggregate_records")
        from .distributed import unpack_record
        return [unpack_record(out[k * rb:(k + 1) * rb], self.field_bytes) for k in range(nsegments)]

    def aggregate_records_device(self, batch_id: int, n: int, d_accept_mask: int | None, d_segment_index: int | None,
                                 nsegments: int, d_out_records: int, stream=None):
        """aggregate_records with device arrays; asynchronous on the engine stream, ordered against
        `stream`."""
        with self._ordered(stream):
            check(self._L.jx_batch_aggregate_records_device(self._h, batch_id, n, d_accept_mask, d_segment_index,
                                                            nsegments, d_out_records),
                  self._h, "jx_batch_aggregate_records_device")

    # ------------------------------------------------------------------ leader role
    def leader_initialized_batch(self, nonces, public_shares, leader_input_shares) -> "LeaderInit":
        """prio ping-pong leader_initialized for n reports (aggregation_job_driver.rs:344-362):
        prepare_init with agg_id 0 on the explicit leader input shares. Returns the verdicts
        (0 = initialized, 1 = prepare_init_failure) and the prep shares that go into each
        PingPongMessage::Initialize. The prepare states stay on the device for
        leader_continued_batch."""
        n = int(np.asarray(nonces).reshape(-1, 16).shape[0])
        nn = _u8(nonces, n, 16, "nonces")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        lis = _u8(leader_input_shares, n, self.leader_input_share_len, "leader_input_shares")
        verdicts = np.zeros(max(n, 1), np.uint8)
        shares = np.zeros((max(n, 1), self.prep_share_len), np.uint8)
        bid = ctypes.c_uint64()
        st = self._L.jx_leader_prep_init_batch(self._h, n, _ptr(nn), _ptr(ps) if self.public_share_len else None,
                                               _ptr(lis), _ptr(shares), _ptr(verdicts), ctypes.byref(bid))
        check(st, self._h, "jx_leader_prep_init_batch")
        with self._lock:
            self._leader_n, self._leader_id = n, bid.value
        return LeaderInit(verdicts[:n], shares[:n], bid.value)

    def leader_continued_batch(self, prep_msgs, want_out_shares: bool = False,
                               init: "LeaderInit | None" = None) -> BatchResult:
        """prio ping-pong leader_continued on the helper's Finish{prep_msg} (aggregation_job_driver.rs:
        588-602): prepare_next for the batch of `init` (default: the last leader_initialized_batch).
        Raises EngineError (JX_E_STATE) if that batch was released or already finished."""
        if init is None:  # the last leader batch: callers sharing the engine across threads pass `init`
            with self._lock:
                n, bid = self._leader_n, self._leader_id
        else:
            n, bid = len(init.verdicts), init.batch_id
        msgs = None
        if self.prep_msg_len:
            msgs = _u8(prep_msgs, n, self.prep_msg_len, "prep_msgs") if n else np.zeros((1, self.prep_msg_len), np.uint8)
        verdicts = np.zeros(max(n, 1), np.uint8)
        outs = np.zeros((max(n, 1), self.output_len * self.field_bytes), np.uint8) if want_out_shares else None
        st = self._L.jx_leader_prep_finish_batch(self._h, bid, n, _ptr(msgs), _ptr(verdicts), _ptr(outs))
        check(st, self._h, "jx_leader_prep_finish_batch")
        return BatchResult(verdicts[:n], msgs[:n] if msgs is not None else np.zeros((n, 0), np.uint8),
                           outs[:n] if outs is not None else None, bid)

    def accumulate(self, n: int, accept_mask: np.ndarray | None = None, segments: np.ndarray | None = None,
                   batch_id: int | None = None):
        """Merge the finished output shares of a prepared batch into the engine's running batch
        aggregations and release the batch (at most once per batch). segments[i]: the
        batch-aggregation id (any u32) of report i. batch_id defaults to the last prepared batch,
        which is only meaningful on an engine one thread uses: threads sharing an engine pass it."""
        m = None if accept_mask is None else np.ascontiguousarray(accept_mask, dtype=np.uint8)
        s = None if segments is None else np.ascontiguousarray(segments, dtype=np.uint32)
        bid = self.batch_id() if batch_id is None else batch_id
        check(self._L.jx_accumulate(self._h, bid, n, _ptr(m), _ptr(s)), self._h, "jx_accumulate")

    # ------------------------------------------------------------------ the client (Prio3.shard)
    def client_rand_bytes(self) -> int:
        """Bytes of client randomness per report: k_helper_meas || k_helper_proofs || k_prove || [blind_leader ||
        blind_helper], 16 bytes each."""
        b = ctypes.c_uint32()
        check(self._L.jx_client_rand_bytes(self._h, ctypes.byref(b)), self._h, "jx_client_rand_bytes")
        return b.value

    def _measurements(self, measurements, n: int) -> np.ndarray:
        width = self.vdaf.length if self.vdaf.algo_id in (2, 4, 5) else 1  # the vector instances
        m = np.ascontiguousarray(np.asarray(measurements, dtype=np.uint64))
        if m.size != n * width:
            raise ValueError(f"measurements: expected {n} x {width} uint64")
        return m.reshape(n, width) if n else np.zeros((1, width), np.uint64)

    def shard_batch(self, measurements, nonces, rands=None) -> ShardResult:
        """Prio3.shard for n measurements on the GPU (jx_client_shard_batch; Count, Sum, SumVec, Histogram).
        measurements: n uint64 (SumVec: n x length); nonces: n x 16; rands: n x client_rand_bytes() of client
        randomness, drawn from os.urandom when None. The rows go into leader_initialized_batch /
        helper_initialized_batch unchanged. A report whose measurement is out of range gets status
        SHARD_INVALID_MEASUREMENT and zero rows."""
        n = len(nonces) // 16 if isinstance(nonces, (bytes, bytearray)) else int(np.asarray(nonces).reshape(-1, 16).shape[0])
        rb = self.client_rand_bytes()
        if rands is None:
            import os
            rands = os.urandom(n * rb)
        nn = _u8(nonces, n, 16, "nonces")
        rd = _u8(rands, n, rb, "rands")
        m = self._measurements(measurements, n)
        ps = np.zeros((n, self.public_share_len), np.uint8)
        lis = np.zeros((n, self.leader_input_share_len), np.uint8)
        his = np.zeros((n, self.helper_input_share_len), np.uint8)
        status = np.zeros(n, np.uint8)
        check(self._L.jx_client_shard_batch(self._h, n, _ptr(m), _ptr(nn), _ptr(rd),
                                            _ptr(ps) if self.public_share_len and n else None, _ptr(lis), _ptr(his),
                                            _ptr(status)),
              self._h, "jx_client_shard_batch")
        return ShardResult(ps, lis, his, status)

    def shard_device(self, n: int, d_measurements: int, d_nonces: int, d_rands: int, d_out_public_shares: int | None,
                     d_out_leader_input_shares: int, d_out_helper_input_shares: int, d_out_status: int | None = None,
                     lis_stride: int = 0, stream=None):
        """Prio3.shard with everything in HBM (jx_client_shard_device). Asynchronous, ordered against `stream`
        (module docstring). lis_stride: the row stride of the leader input shares written (0: packed rows; else at
        least leader_input_share_len and a multiple of 16, zero padded), as leader_init_device reads them; the rows
        must be 16-byte aligned."""
        with self._ordered(stream):
            check(self._L.jx_client_shard_device(self._h, n, d_measurements, d_nonces, d_rands, d_out_public_shares,
                                                 d_out_leader_input_shares, lis_stride, d_out_helper_input_shares,
                                                 d_out_status),
                  self._h, "jx_client_shard_device")

    # ------------------------------------------------------------------ the client (the two hpke::seal calls)
    def client_seal_sizes(self) -> tuple[int, int]:
        """(leader, helper) ciphertext row lengths of seal_reports: 6 + LIS + 16 and 6 + HIS + 16."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        check(self._L.jx_client_seal_sizes(self._h, ctypes.byref(a), ctypes.byref(b)), self._h, "jx_client_seal_sizes")
        return a.value, b.value

    def seal_reports(self, report_ids, times, public_shares, leader_input_shares, helper_input_shares, task_id: bytes,
                     leader_sealer, helper_sealer, ephemeral_sks, shard_status=None) -> SealResult:
        """The second half of the reference client's prepare_report for n reports (jx_client_seal_batch): the rows of
        shard_batch sealed for the leader and the helper, each share under its own ephemeral key. leader_sealer /
        helper_sealer: janus_amd.hpke.HpkeSealer (or HpkeOpener) contexts with the (InputShare, Client -> Leader /
        Helper) application infos; ephemeral_sks: n x 64 bytes from the caller's CSPRNG (the leader seal's X25519
        private key, then the helper seal's); leader_input_shares: an (n, stride) array with stride >=
        leader_input_share_len; shard_status: shard_batch's status, a non-zero entry leaves the report's outputs zero."""
        n = int(np.asarray(report_ids).reshape(-1, 16).shape[0]) if not isinstance(report_ids, (bytes, bytearray)) \
            else len(report_ids) // 16
        ids = _u8(report_ids, n, 16, "report_ids")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        lis = np.ascontiguousarray(np.asarray(leader_input_shares, dtype=np.uint8)).reshape(max(n, 1), -1)
        stride = lis.shape[1]
        if n and stride < self.leader_input_share_len:
            raise ValueError("leader_input_shares: rows shorter than the leader input share")
        his = _u8(helper_input_shares, n, self.helper_input_share_len, "helper_input_shares")
        sks = _u8(ephemeral_sks, n, 64, "ephemeral_sks")
        tm = _items(times, n, np.uint64)
        ss = None if shard_status is None else _u8(shard_status, n, 1, "shard_status")
        if len(task_id) != 32:
            raise ValueError("task id is 32 bytes")
        task = np.frombuffer(task_id, np.uint8).copy()
        lct, hct = self.client_seal_sizes()
        out = SealResult(np.zeros((n, 32), np.uint8), np.zeros((n, lct), np.uint8), np.zeros((n, 32), np.uint8),
                         np.zeros((n, hct), np.uint8), np.zeros(n, np.uint8))
        check(self._L.jx_client_seal_batch(self._h, n, _ptr(ids), _u64p(tm),
                                           _ptr(ps) if self.public_share_len and n else None, _ptr(lis), stride,
                                           _ptr(his), _ptr(task), leader_sealer.handle, helper_sealer.handle, _ptr(sks),
                                           _ptr(ss), _ptr(out.leader_encs), _ptr(out.leader_cts), _ptr(out.helper_encs),
                                           _ptr(out.helper_cts), _ptr(out.status)),
              self._h, "jx_client_seal_batch")
        return out

    def seal_reports_device(self, n: int, d_report_ids: int, times, d_public_shares: int | None,
                            d_leader_input_shares: int, d_helper_input_shares: int, task_id: bytes, leader_sealer,
                            helper_sealer, d_ephemeral_sks: int, d_out_leader_encs: int, d_out_leader_cts: int,
                            d_out_helper_encs: int, d_out_helper_cts: int, d_out_status: int,
                            d_shard_status: int | None = None, lis_stride: int = 0, stream=None):
        """seal_reports with everything in HBM but `times`, a host array (jx_client_seal_device). Asynchronous, ordered
        against `stream` (module docstring): it reads the rows shard_device wrote, at the same lis_stride, and writes
        the ciphertext rows jx_leader_upload_open_device and jx_helper_prep_aggregate_encrypted_device read with
        payload offsets i x client_seal_sizes()."""
        tm = _items(times, n, np.uint64)
        if len(task_id) != 32:
            raise ValueError("task id is 32 bytes")
        task = np.frombuffer(task_id, np.uint8).copy()
        with self._ordered(stream):
            check(self._L.jx_client_seal_device(self._h, n, d_report_ids, _u64p(tm),
                                                d_public_shares, d_leader_input_shares, lis_stride, d_helper_input_shares,
                                                _ptr(task), leader_sealer.handle, helper_sealer.handle, d_ephemeral_sks,
                                                d_shard_status, d_out_leader_encs, d_out_leader_cts, d_out_helper_encs,
                                                d_out_helper_cts, d_out_status),
                  self._h, "jx_client_seal_device")

    # ------------------------------------------------------------------ device-pointer paths (inputs in HBM)
    def leader_init_device(self, n: int, d_nonces: int, d_public_shares: int | None, d_leader_input_shares: int,
                           d_out_prep_shares: int, d_out_verdicts: int | None = None, stream=None,
                           lis_stride: int = 0) -> int:
        """leader_initialized for n reports resident in HBM; returns the batch id. Asynchronous,
        ordered against `stream` (module docstring). lis_stride: the row stride of the leader input
        shares (0: packed rows of leader_input_share_len; a multiple of 128 lets the in-place FLP
        kernels read whole cache lines)."""
        bid = ctypes.c_uint64()
        with self._ordered(stream):
            st = self._L.jx_leader_prep_init_device_ex(self._h, n, d_nonces, d_public_shares, d_leader_input_shares,
                                                       lis_stride, d_out_prep_shares, d_out_verdicts, ctypes.byref(bid))
            check(st, self._h, "jx_leader_prep_init_device_ex")
        return bid.value

    def leader_upload_open(self, report_ids, times, public_shares, task_id: bytes, keypairs, key_index, encs,
                           payloads: list[bytes], lis_stride: int = 0, stream=None) -> "UploadOpen":
        """The leader's upload loop for n reports (handle_upload_generic, aggregator.rs:1513-1694) on the GPU
        (jx_leader_upload_open_device): report i's leader_encrypted_input_share is opened with
        keypairs[key_index[i][0]] (then keypairs[key_index[i][1]] if that fails to decrypt; KEY_NONE: none), its
        PlaintextInputShare decoded, its payload checked as the leader input share (exact length, every element
        < p) and laid out as row i of a device tensor. keypairs: janus_amd.hpke.HpkeOpener contexts created with
        the (InputShare, Client -> Leader) application info on this engine's device; encs: an (n, 32) array or a
        list of encapsulated keys of any lengths. lis_stride: 0 (rows of leader_input_share_len) or a multiple of
        16 that is at least that. Returns the status per report (OPEN_OK or an OPEN_STATUS key), each report's
        extension bytes and the rows, which `leader_init_device(n, ..., rows.data_ptr(), ..., lis_stride=...)`
        reads in place (rejected reports: zeros). The inputs go through torch tensors on the engine's device;
        the call is ordered against `stream` like the other device-pointer methods and waits for its results."""
        import torch

        n = int(np.asarray(report_ids).reshape(-1, 16).shape[0])
        ids = _u8(report_ids, n, 16, "report_ids")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        tm = _items(times, n, np.uint64)
        ki = _items(key_index, n, np.uint8, 2)
        if isinstance(encs, (list, tuple)):
            if len(encs) != n:
                raise ValueError("one encapsulated key per report")
            en, eoff = _packed(encs)
        else:
            en = _u8(encs, n, 32, "encs").reshape(-1) if n else np.zeros(32, np.uint8)
            eoff = np.arange(n + 1, dtype=np.uint64) * 32
        if len(task_id) != 32 or len(payloads) != n:
            raise ValueError("task id is 32 bytes; one payload per report")
        ct, off = _packed(payloads)
        task = np.frombuffer(task_id, np.uint8).copy()
        hs = (ctypes.c_void_p * max(1, len(keypairs)))(*[k.handle for k in keypairs])
        stride = lis_stride or self.leader_input_share_len
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_ids, d_ps, d_en, d_ct = (torch.from_numpy(a.reshape(-1).copy()).to(dev) for a in (ids, ps, en, ct))
            # 16 spare bytes: the rows start at the tensor's next 16-byte boundary whatever the allocator gives
            d_rows = torch.zeros(max(n, 1) * stride + 16, dtype=torch.uint8, device=dev)
            skew = (-d_rows.data_ptr()) % 16
            rows = d_rows[skew:skew + max(n, 1) * stride].view(max(n, 1), stride)
            d_ext = torch.zeros(ct.size, dtype=torch.uint8, device=dev)
            d_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            d_st = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            with self._ordered(stream):
                st = self._L.jx_leader_upload_open_device(
                    self._h, n, d_ids.data_ptr(), _u64p(tm), d_ps.data_ptr() if self.public_share_len else None,
                    _ptr(task), hs, len(keypairs), _ptr(ki), d_en.data_ptr(), _u64p(eoff), d_ct.data_ptr(), _u64p(off),
                    rows.data_ptr(), lis_stride, d_ext.data_ptr(), d_len.data_ptr(), d_st.data_ptr())
                check(st, self._h, "jx_leader_upload_open_device")
            status, ext_len, ext = d_st.cpu().numpy()[:n], d_len.cpu().numpy()[:n], d_ext.cpu().numpy()
        exts = [ext[int(off[i]):int(off[i]) + int(ext_len[i])].tobytes() for i in range(n)]
        return UploadOpen(status, exts, rows[:n], stride)

    def leader_finish_device(self, batch_id: int, n: int, d_prep_msgs: int | None, d_peer_verdicts: int | None = None,
                             d_out_verdicts: int | None = None, stream=None):
        """leader_continued on the helper's prep messages in HBM; reports the helper rejected
        (d_peer_verdicts != 0) fail with helper_step_failure. Asynchronous, ordered against `stream`."""
        with self._ordered(stream):
            check(self._L.jx_leader_prep_finish_device(self._h, batch_id, n, d_prep_msgs, d_peer_verdicts,
                                                       d_out_verdicts),
                  self._h, "jx_leader_prep_finish_device")

    def accumulate_device(self, batch_id: int, n: int, d_accept_mask: int | None = None, d_segments: int | None = None,
                          segment_ids=(0,), stream=None):
        """accumulate with device arrays: d_segments[i] indexes segment_ids. Asynchronous, ordered
        against `stream`."""
        ids, ptr = _seg_table(segment_ids)
        with self._ordered(stream):
            check(self._L.jx_accumulate_device(self._h, batch_id, n, d_accept_mask, d_segments, ptr, ids.size),
                  self._h, "jx_accumulate_device")

    def prep_and_aggregate(self, nonces, public_shares, helper_input_shares, leader_prep_shares,
                           segment: int = 0, want_results: bool = True):
        """Fused prep_init + aggregate of n reports (the benchmark's unit of work), host buffers."""
        n = int(np.asarray(nonces).reshape(-1, 16).shape[0])
        nn = _u8(nonces, n, 16, "nonces")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        his = _u8(helper_input_shares, n, self.helper_input_share_len, "helper_input_shares")
        lps = _u8(leader_prep_shares, n, self.prep_share_len, "leader_prep_shares")
        verdicts = np.zeros(max(n, 1), np.uint8) if want_results else None
        msgs = np.zeros((max(n, 1), self.prep_msg_len), np.uint8) if (want_results and self.prep_msg_len) else None
        st = self._L.jx_helper_prep_aggregate(self._h, n, _ptr(nn), _ptr(ps) if self.public_share_len else None,
                                              _ptr(his), _ptr(lps), segment, _ptr(msgs), _ptr(verdicts))
        check(st, self._h, "jx_helper_prep_aggregate")
        if want_results:
            return verdicts[:n], (msgs[:n] if msgs is not None else np.zeros((n, 0), np.uint8))
        return None

    def prep_and_aggregate_device(self, d_nonces: int, d_public_shares: int | None, d_helper_input_shares: int,
                                  d_leader_prep_shares: int, n: int, segment: int = 0,
                                  d_out_prep_msgs: int | None = None, d_out_verdicts: int | None = None,
                                  d_segments: int | None = None, segment_ids=None, stream=None):
        """Same, with inputs already resident in HBM (device pointers, e.g. tensor.data_ptr()).
        Every report goes to `segment`, or, with d_segments, report i to segment_ids[d_segments[i]].
        Asynchronous, ordered against `stream` (default: torch's current stream), so outputs read on
        that stream need no sync(); with stream=False call sync() (or join_stream) first."""
        ids, ptr = _seg_table([segment] if segment_ids is None else segment_ids)
        with self._ordered(stream):
            st = self._L.jx_helper_prep_aggregate_device(self._h, n, d_nonces, d_public_shares, d_helper_input_shares,
                                                         d_leader_prep_shares, d_segments, ptr, ids.size,
                                                         d_out_prep_msgs, d_out_verdicts)
            check(st, self._h, "jx_helper_prep_aggregate_device")

    def _sealed_inputs(self, n: int, times, task_id: bytes, keypairs, key_index, encs, payloads, payload_offsets):
        """The sealed-share arguments of the fused calls as host arrays (the conventions of
        helper_initialized_encrypted_batch): times, key-index pairs, the encapsulated keys packed with their
        offsets (None: n x 32), the payloads packed with theirs, the task id and the keypair handles."""
        tm = _items(times, n, np.uint64)
        ki = _items(key_index, n, np.uint8, 2)
        if isinstance(encs, (list, tuple)):
            if len(encs) != n:
                raise ValueError("one encapsulated key per report")
            en, eoff = _packed(encs)
        else:
            en = _u8(encs, n, 32, "encs").reshape(-1) if n else np.zeros(32, np.uint8)
            eoff = None
        if isinstance(payloads, (list, tuple)):
            if len(payloads) != n or payload_offsets is not None:
                raise ValueError("one payload per report (a list carries its own offsets)")
            ct, off = _packed(payloads)
        else:
            if payload_offsets is None:
                raise ValueError("packed payloads need payload_offsets (n + 1)")
            off = _offs(payload_offsets, n)
            ct = np.ascontiguousarray(np.frombuffer(payloads, np.uint8) if isinstance(payloads, (bytes, bytearray))
                                      else payloads, dtype=np.uint8).reshape(-1)
            if ct.size == 0:
                ct = np.zeros(1, np.uint8)
        if len(task_id) != 32:
            raise ValueError("task id is 32 bytes")
        task = np.frombuffer(task_id, np.uint8).copy()
        hs = (ctypes.c_void_p * max(1, len(keypairs)))(*[k.handle for k in keypairs])
        return tm, ki, en, eoff, ct, off, task, hs

    def prep_and_aggregate_encrypted(self, nonces, times, public_shares, task_id: bytes, keypairs, key_index, encs,
                                     payloads, leader_prep_shares, payload_offsets=None, segment: int = 0,
                                     require_taskprov: bool = False) -> "EncryptedResult":
        """prep_and_aggregate from report shares still under HPKE, host buffers
        (jx_helper_prep_aggregate_encrypted): every launch of the fused call opens its own reports, as
        helper_initialized_encrypted_batch does for a job, and exactly the finished reports are accumulated into
        `segment`. encs: an (n, 32) array or a list of keys of any lengths; payloads: a list of ciphertexts, or a
        packed array with payload_offsets (n + 1, which may start above 0). Returns verdicts (OPEN_FAILURE where
        the share did not open / decode), prep messages and the open status per report."""
        n = int(np.asarray(nonces).reshape(-1, 16).shape[0])
        nn = _u8(nonces, n, 16, "nonces")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        lps = _u8(leader_prep_shares, n, self.prep_share_len, "leader_prep_shares")
        tm, ki, en, eoff, ct, off, task, hs = self._sealed_inputs(n, times, task_id, keypairs, key_index, encs, payloads,
                                                                  payload_offsets)
        verdicts = np.zeros(max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        msgs = np.zeros((max(n, 1), max(self.prep_msg_len, 1)), np.uint8)
        st = self._L.jx_helper_prep_aggregate_encrypted(
            self._h, n, _ptr(nn), _u64p(tm), _ptr(ps) if self.public_share_len else None, _ptr(task), hs, len(keypairs),
            _ptr(ki), _ptr(en), _u64p(eoff), _ptr(ct), _u64p(off), ENC_REQUIRE_TASKPROV if require_taskprov else 0,
            _ptr(lps), segment, _ptr(msgs) if self.prep_msg_len else None, _ptr(verdicts), _ptr(status))
        check(st, self._h, "jx_helper_prep_aggregate_encrypted")
        return EncryptedResult(verdicts[:n], msgs[:n, : self.prep_msg_len], status[:n], 0)

    def prep_and_aggregate_encrypted_device(self, d_nonces: int, times, d_public_shares: int | None, task_id: bytes,
                                            keypairs, key_index, d_encs: int, d_payloads: int, payload_offsets,
                                            d_leader_prep_shares: int, n: int, enc_offsets=None, segment: int = 0,
                                            require_taskprov: bool = False, d_out_prep_msgs: int | None = None,
                                            d_out_verdicts: int | None = None, d_out_open_status: int | None = None,
                                            d_segments: int | None = None, segment_ids=None, stream=None):
        """Same, with the bulk data resident in HBM (jx_helper_prep_aggregate_encrypted_device): device pointers
        for the report ids, public shares, encapsulated keys (packed; enc_offsets None: n x 32 bytes), payloads
        (packed, report i's at payload_offsets[i]) and leader prep shares and for the three optional outputs; host
        arrays for times, key_index and the two offset arrays. The ciphertexts and keys are read in place.
        Segments and stream ordering as prep_and_aggregate_device."""
        tm = _items(times, n, np.uint64)
        ki = _items(key_index, n, np.uint8, 2)
        off = _offs(payload_offsets, n)
        eoff = None if enc_offsets is None else _offs(enc_offsets, n)
        if len(task_id) != 32:
            raise ValueError("task id is 32 bytes")
        task = np.frombuffer(task_id, np.uint8).copy()
        hs = (ctypes.c_void_p * max(1, len(keypairs)))(*[k.handle for k in keypairs])
        ids, ptr = _seg_table([segment] if segment_ids is None else segment_ids)
        with self._ordered(stream):
            st = self._L.jx_helper_prep_aggregate_encrypted_device(
                self._h, n, d_nonces, _u64p(tm), d_public_shares, _ptr(task), hs, len(keypairs), _ptr(ki), d_encs,
                _u64p(eoff), d_payloads, _u64p(off), ENC_REQUIRE_TASKPROV if require_taskprov else 0,
                d_leader_prep_shares, d_segments, ptr, ids.size, d_out_prep_msgs, d_out_verdicts, d_out_open_status)
            check(st, self._h, "jx_helper_prep_aggregate_encrypted_device")

    # ------------------------------------------------------------------ wire in, wire out
    def decode_init_req(self, body, query_type: int, key_first, key_second, report_deadline: int | None = None,
                        length: int | None = None, stream=None) -> InitReq:
        """Decode an AggregationJobInitializeReq body on the GPU (jx_init_req_decode / _device). body: bytes (copied to
        the device once) or, with `length`, a device pointer or torch tensor holding the body (ordered against `stream`
        like the other device-pointer methods). query_type: the task's (messages.QUERY_TIME_INTERVAL / _FIXED_SIZE).
        key_first / key_second: 256 keypair indices by HPKE config id (KEY_NONE: none). report_deadline: the latest
        report time that is not too early. Returns an InitReq also for a request that is refused: see its status."""
        kf = np.ascontiguousarray(np.asarray(key_first, dtype=np.uint8).reshape(256))
        ks = np.ascontiguousarray(np.asarray(key_second, dtype=np.uint8).reshape(256))
        dl = None if report_deadline is None else ctypes.byref(ctypes.c_uint64(report_deadline))
        h = ctypes.c_void_p()
        if length is None:
            b = np.frombuffer(bytes(body) or b"\0", np.uint8)
            st = self._L.jx_init_req_decode(self._h, _ptr(b), len(body), query_type, _ptr(kf), _ptr(ks), dl, ctypes.byref(h))
            check(st, self._h, "jx_init_req_decode")
        else:
            ptr = int(body.data_ptr()) if hasattr(body, "data_ptr") else int(body)
            with self._ordered(stream):
                st = self._L.jx_init_req_decode_device(self._h, ptr, length, query_type, _ptr(kf), _ptr(ks), dl,
                                                       ctypes.byref(h))
                check(st, self._h, "jx_init_req_decode_device")
        return self._track(InitReq(self, h))

    def encode_init_resp(self, req: InitReq, d_verdicts: int | None, d_open_status: int | None, d_prep_msgs: int | None,
                         host_errors=None, replayed=None, prep_msg_stride: int = 0, d_out: int | None = None,
                         capacity: int = 0, d_out_finished: int | None = None, stream=None):
        """The AggregationJobResp body of a decoded request from the device arrays the sealed calls wrote
        (jx_init_resp_encode / _device). host_errors: uint8[n] PrepareError code points of reports the host resolved
        (WIRE_NO_ERROR: none); replayed: a mask of n. Returns (body bytes, finished mask); with d_out (a device buffer of
        `capacity` bytes) the body is written there and its length is returned."""
        n = req.n
        he = None if host_errors is None else np.ascontiguousarray(np.asarray(host_errors, dtype=np.uint8).reshape(n))
        rp = None if replayed is None else np.ascontiguousarray(np.asarray(replayed).astype(np.uint8).reshape(n))
        ln = ctypes.c_uint64()
        with self._ordered(stream):
            if d_out is not None:
                st = self._L.jx_init_resp_encode_device(self._h, req._h, d_verdicts, d_open_status, d_prep_msgs,
                                                        prep_msg_stride, _ptr(he), _ptr(rp), d_out, capacity,
                                                        ctypes.byref(ln), d_out_finished)
                check(st, self._h, "jx_init_resp_encode_device")
                return ln.value
            cap = 4 + n * (26 + self.prep_msg_len)
            out = np.zeros(cap, np.uint8)
            fin = np.zeros(max(n, 1), np.uint8)
            st = self._L.jx_init_resp_encode(self._h, req._h, d_verdicts, d_open_status, d_prep_msgs, prep_msg_stride,
                                             _ptr(he), _ptr(rp), _ptr(out), cap, ctypes.byref(ln), _ptr(fin))
            check(st, self._h, "jx_init_resp_encode")
        return out[:ln.value].tobytes(), fin[:n].astype(bool)

    # ------------------------------------------------------------------ the leader's end of the wire
    def _req_host_arrays(self, n: int, times, config_ids, enc_offsets, payload_offsets, exclude, agg_param, query_type,
                         batch_id):
        tm = _items(times, n, np.uint64)
        cf = _items(config_ids, n, np.uint8)
        off = _offs(payload_offsets, n)
        eoff = None if enc_offsets is None else _offs(enc_offsets, n)
        ex = None if exclude is None or not n else np.ascontiguousarray(np.asarray(exclude).astype(np.uint8).reshape(n))
        par = np.frombuffer(bytes(agg_param) or b"\0", np.uint8)
        if query_type == 2 and (batch_id is None or len(batch_id) != 32):
            raise ValueError("FixedSize carries a 32-byte batch id")
        bid = None if batch_id is None else np.frombuffer(bytes(batch_id), np.uint8)
        return (_u64p(tm), _ptr(cf), _u64p(eoff), _u64p(off), _ptr(ex), _ptr(par), len(agg_param), query_type,
                _ptr(bid)), (tm, cf, off, eoff, ex, par, bid)

    def init_req_bound(self, n: int, payload_offsets, agg_param_len: int, query_type: int, enc_offsets=None) -> int:
        """The length of the request body if every report were sent (jx_init_req_encode_bound)."""
        off = _offs(payload_offsets, n)
        eoff = None if enc_offsets is None else _offs(enc_offsets, n)
        out = ctypes.c_uint64()
        check(self._L.jx_init_req_encode_bound(self._h, n, _u64p(eoff), _u64p(off), agg_param_len, query_type,
                                               ctypes.byref(out)),
              self._h, "jx_init_req_encode_bound")
        return out.value

    def encode_init_req(self, n: int, d_report_ids: int, times, d_public_shares: int | None, config_ids, d_encs: int,
                        d_payloads: int, payload_offsets, d_prep_shares: int, d_verdicts: int, agg_param: bytes = b"",
                        query_type: int = 1, batch_id: bytes | None = None, enc_offsets=None, exclude=None,
                        prep_share_stride: int = 0, d_out: int | None = None, capacity: int = 0, stream=None) -> LeaderReq:
        """The AggregationJobInitializeReq body of a leader job, written on the GPU (jx_init_req_encode_device) from
        the arrays the leader holds: device pointers for the report ids, public shares, encapsulated keys and payloads
        (packed; enc_offsets None: n x 32 bytes), the prep shares and verdicts leader_init_device wrote; host arrays
        for times, config_ids, the offset arrays and exclude (a mask of reports not to send). Report i is sent iff its
        verdict is FINISHED and it is not excluded. Without d_out the body goes to a device buffer of the bound that
        the returned LeaderReq keeps (d_body); with d_out (a device buffer of `capacity` bytes) it is written there.
        Ordered against `stream` like the other device-pointer methods; waits for its result."""
        args, keep = self._req_host_arrays(n, times, config_ids, enc_offsets, payload_offsets, exclude, agg_param,
                                           query_type, batch_id)
        d_body = None
        if d_out is None:
            import torch

            capacity = self.init_req_bound(n, payload_offsets, len(agg_param), query_type, enc_offsets)
            d_body = torch.empty(capacity, dtype=torch.uint8, device=torch.device("cuda", self.device))
            d_out = d_body.data_ptr()
        ln, h = ctypes.c_uint64(), ctypes.c_void_p()
        tm, cf, eoff, off, ex, par, plen, q, bid = args
        with self._ordered(stream):
            st = self._L.jx_init_req_encode_device(self._h, n, d_report_ids, tm, d_public_shares, cf, d_encs, eoff,
                                                   d_payloads, off, d_prep_shares, prep_share_stride, d_verdicts, ex,
                                                   par, plen, q, bid, d_out, capacity, ctypes.byref(ln), ctypes.byref(h))
            check(st, self._h, "jx_init_req_encode_device")
        del keep
        if d_body is None and ln.value:  # the caller's buffer, as torch sees it
            import torch

            d_body = torch.as_tensor(_DeviceBytes(d_out, ln.value), device=torch.device("cuda", self.device))
        return self._track(LeaderReq(self, h, None, d_body))

    def encode_init_req_host(self, report_ids, times, public_shares, config_ids, encs, payloads, payload_offsets,
                             prep_shares, verdicts, agg_param: bytes = b"", query_type: int = 1,
                             batch_id: bytes | None = None, enc_offsets=None, exclude=None) -> LeaderReq:
        """The same from host arrays (jx_init_req_encode): encs and payloads are the packed byte arrays the offset
        arrays index, prep_shares rows of prep_share_len bytes. The body is returned in host memory."""
        if isinstance(report_ids, (bytes, bytearray)):
            report_ids = np.frombuffer(report_ids, np.uint8)
        n = int(np.asarray(report_ids).size // 16)
        ids = _u8(report_ids, n, 16, "report_ids") if n else np.zeros((1, 16), np.uint8)
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        lps = _u8(prep_shares, n, self.prep_share_len, "prep_shares")
        vd = _items(verdicts, n, np.uint8)
        en = np.ascontiguousarray(np.frombuffer(bytes(encs) or b"\0", np.uint8))
        pay = np.ascontiguousarray(np.frombuffer(bytes(payloads) or b"\0", np.uint8))
        args, keep = self._req_host_arrays(n, times, config_ids, enc_offsets, payload_offsets, exclude, agg_param,
                                           query_type, batch_id)
        tm, cf, eoff, off, ex, par, plen, q, bid = args
        cap = self.init_req_bound(n, payload_offsets, len(agg_param), query_type, enc_offsets)
        out = np.zeros(cap, np.uint8)
        ln, h = ctypes.c_uint64(), ctypes.c_void_p()
        st = self._L.jx_init_req_encode(self._h, n, _ptr(ids), tm, _ptr(ps) if self.public_share_len else None, cf,
                                        _ptr(en), eoff, _ptr(pay), off, _ptr(lps), 0, _ptr(vd), ex, par, plen, q, bid,
                                        _ptr(out), cap, ctypes.byref(ln), ctypes.byref(h))
        check(st, self._h, "jx_init_req_encode")
        del keep
        return self._track(LeaderReq(self, h, out[:ln.value].tobytes()))

    def decode_init_resp(self, req: LeaderReq, body: bytes, d_out_prep_msgs: int | None, d_out_peer_verdicts: int | None,
                         prep_msg_stride: int = 0, stream=None) -> InitRespDecode:
        """The helper's AggregationJobResp body for an encoded request (jx_init_resp_decode): the body is walked and
        matched against the sent reports on the host; for an accepted one the prep messages and peer verdicts of all
        req.n rows are queued into the device arrays leader_finish_device reads. Raises nothing for a refused
        response (see the status); a refused response writes nothing."""
        b = np.frombuffer(bytes(body) or b"\0", np.uint8)
        res = np.full(max(req.n_sent, 1), 0xFF, np.uint8)
        err = np.full(max(req.n_sent, 1), 0xFF, np.uint8)
        info = _lib.JxInitRespInfo()
        with self._ordered(stream):
            st = self._L.jx_init_resp_decode(self._h, req._h, _ptr(b), len(body), d_out_prep_msgs, prep_msg_stride,
                                             d_out_peer_verdicts, _ptr(res), _ptr(err), ctypes.byref(info))
            check(st, self._h, "jx_init_resp_decode")
        return InitRespDecode(int(info.status), res[:req.n_sent], err[:req.n_sent], int(info.error_offset),
                              int(info.mismatch_index), int(info.n))

    # ------------------------------------------------------------------ the upload message
    def report_bound(self, n: int, leader_enc_len: int = 32, helper_enc_len: int = 32) -> int:
        """The length of n Report bodies if every report takes room (jx_report_encode_bound)."""
        out = ctypes.c_uint64()
        check(self._L.jx_report_encode_bound(self._h, n, leader_enc_len, helper_enc_len, ctypes.byref(out)), self._h,
              "jx_report_encode_bound")
        return out.value

    def encode_reports(self, n: int, d_report_ids: int, times, d_public_shares: int | None, d_leader_encs: int,
                       d_leader_cts: int, d_helper_encs: int, d_helper_cts: int, leader_config_id: int,
                       helper_config_id: int, d_seal_status: int | None = None, leader_enc_len: int = 32,
                       helper_enc_len: int = 32, d_out: int | None = None, capacity: int = 0, stream=None):
        """The DAP Report bodies of n sealed reports, written back to back on the GPU (jx_report_encode_device) from
        the arrays seal_reports_device wrote: device pointers for the report ids, public-share rows, encapsulated-key
        rows (leader_enc_len / helper_enc_len bytes each) and ciphertext rows (client_seal_sizes() bytes each), `times`
        a host array, one config id per recipient. A report whose d_seal_status entry is non-zero takes no room.
        Returns (bodies, offsets): offsets is numpy uint64[n + 1], report i lies at bodies[offsets[i]:offsets[i + 1]];
        bodies is a torch uint8 tensor on the device (the caller's d_out of `capacity` bytes when given, else a buffer
        of report_bound). Ordered against `stream` like the other device-pointer methods; waits for its result."""
        import torch

        tm = _items(times, n, np.uint64)
        dev = torch.device("cuda", self.device)
        keep = None
        if d_out is None:
            capacity = self.report_bound(n, leader_enc_len, helper_enc_len)
            keep = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
            d_out = keep.data_ptr()
        offs = np.zeros(n + 1, np.uint64)
        ln = ctypes.c_uint64()
        with self._ordered(stream):
            st = self._L.jx_report_encode_device(self._h, n, d_report_ids, _u64p(tm), d_public_shares,
                                                 d_leader_encs, leader_enc_len, d_leader_cts, d_helper_encs, helper_enc_len,
                                                 d_helper_cts, leader_config_id, helper_config_id, d_seal_status, d_out,
                                                 capacity, None, _u64p(offs), ctypes.byref(ln))
            check(st, self._h, "jx_report_encode_device")
        if keep is not None:
            bodies = keep[:ln.value]
        elif ln.value:
            bodies = torch.as_tensor(_DeviceBytes(d_out, ln.value), device=dev)
        else:
            bodies = torch.zeros(0, dtype=torch.uint8, device=dev)
        return bodies, offs

    def encode_reports_host(self, report_ids, times, public_shares, leader_encs, leader_cts, helper_encs, helper_cts,
                            leader_config_id: int, helper_config_id: int, seal_status=None):
        """The same from host arrays (jx_report_encode), as seal_reports returns them: rows of n, the encapsulated
        keys' lengths taken from the rows. Returns (bodies bytes, offsets numpy uint64[n + 1])."""
        ids = np.ascontiguousarray(np.asarray(report_ids, dtype=np.uint8)).reshape(-1, 16)
        n = ids.shape[0]
        rows = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint8)).reshape(max(n, 1), -1)  # noqa: E731
        le, lc, he, hc = rows(leader_encs), rows(leader_cts), rows(helper_encs), rows(helper_cts)
        if n and (lc.shape[1], hc.shape[1]) != self.client_seal_sizes():
            raise ValueError("ciphertext rows of client_seal_sizes() bytes")
        ps = _u8(public_shares, n, self.public_share_len, "public_shares")
        tm = _items(times, n, np.uint64)
        ss = None if seal_status is None else _u8(seal_status, n, 1, "seal_status")
        le_len, he_len = (le.shape[1], he.shape[1]) if n else (32, 32)
        cap = self.report_bound(n, le_len, he_len)
        out, offs, ln = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.uint64), ctypes.c_uint64()
        st = self._L.jx_report_encode(self._h, n, _ptr(ids), _u64p(tm), _ptr(ps) if self.public_share_len else None,
                                      _ptr(le), le_len, _ptr(lc), _ptr(he), he_len, _ptr(hc), leader_config_id,
                                      helper_config_id, _ptr(ss), _ptr(out), cap, _u64p(offs), ctypes.byref(ln))
        check(st, self._h, "jx_report_encode")
        return out[:ln.value].tobytes(), offs

    def decode_uploads(self, bodies, body_offsets, now: int, key_first, key_second, tolerable_clock_skew: int = 0,
                       task_expiration: int | None = None, report_expiry_age: int | None = None,
                       length: int | None = None, stream=None) -> UploadReq:
        """Decode n upload bodies lying back to back on the GPU (jx_upload_decode / _device). bodies: bytes (copied to
        the device once) or, with `length`, a device pointer or torch tensor (ordered against `stream`). body_offsets:
        n + 1, upload i is bodies[body_offsets[i]:body_offsets[i + 1]]. now, tolerable_clock_skew, task_expiration,
        report_expiry_age: the upload handler's three time checks (None: the task has no such limit). key_first /
        key_second: 256 keypair indices by the leader ciphertext's HPKE config id (KEY_NONE: none). Per upload the
        UploadReq says whether it was accepted (status); the accepted reports' fields are its device arrays."""
        off = np.ascontiguousarray(np.asarray(body_offsets, dtype=np.uint64).reshape(-1))
        n = off.size - 1
        if n < 0:
            raise ValueError("body_offsets holds n + 1 offsets")
        tab = lambda k: np.frombuffer(bytes(k), np.uint8) if isinstance(k, (bytes, bytearray)) else np.asarray(k, dtype=np.uint8)  # noqa: E731
        kf, ks = (np.ascontiguousarray(tab(k).reshape(256)) for k in (key_first, key_second))
        ck = _lib.JxUploadChecks(now, tolerable_clock_skew, task_expiration is not None, task_expiration or 0,
                                 report_expiry_age is not None, report_expiry_age or 0)
        h = ctypes.c_void_p()
        if length is None:
            b = np.frombuffer(bytes(bodies) or b"\0", np.uint8)
            st = self._L.jx_upload_decode(self._h, _ptr(b), len(bodies), n, _u64p(off), ctypes.byref(ck),
                                          _ptr(kf), _ptr(ks), ctypes.byref(h))
            check(st, self._h, "jx_upload_decode")
        else:
            ptr = int(bodies.data_ptr()) if hasattr(bodies, "data_ptr") else int(bodies)
            with self._ordered(stream):
                st = self._L.jx_upload_decode_device(self._h, ptr, length, n, _u64p(off), ctypes.byref(ck),
                                                     _ptr(kf), _ptr(ks), ctypes.byref(h))
                check(st, self._h, "jx_upload_decode_device")
        return self._track(UploadReq(self, h))

    # ------------------------------------------------------------------ aggregation state
    def aggregate_share(self, segment: int = 0) -> tuple[bytes, int, bytes]:
        """(encoded aggregate share, report count, checksum) of one batch aggregation."""
        out = np.zeros(self.output_len * self.field_bytes, np.uint8)
        cnt = ctypes.c_uint64()
        check(self._L.jx_aggregate_read(self._h, segment, _ptr(out), ctypes.byref(cnt)), self._h,
              "jx_aggregate_read")
        cs = np.zeros(32, np.uint8)
        check(self._L.jx_aggregate_checksum(self._h, segment, _ptr(cs)), self._h, "jx_aggregate_checksum")
        return out.tobytes(), cnt.value, cs.tobytes()

    def reset_aggregates(self):
        check(self._L.jx_aggregate_reset(self._h), self._h, "jx_aggregate_reset")

    def export_aggregate_device(self, segment: int, d_dst: int, stream=None):
        with self._ordered(stream):
            check(self._L.jx_aggregate_export_device(self._h, segment, d_dst), self._h, "jx_aggregate_export_device")

    def combine_device(self, d_parts: int, nparts: int, d_out: int, stream=None):
        with self._ordered(stream):
            check(self._L.jx_aggregate_combine_device(self._h, d_parts, nparts, d_out), self._h,
                  "jx_aggregate_combine_device")

    def record_bytes(self) -> int:
        b = ctypes.c_uint32()
        check(self._L.jx_shard_record_bytes(self._h, ctypes.byref(b)), self._h, "jx_shard_record_bytes")
        return b.value

    def export_record_device(self, segment: int, d_dst: int, stream=None):
        """Write this engine's shard record (agg share || count || checksum) to device memory."""
        with self._ordered(stream):
            check(self._L.jx_shard_record_export_device(self._h, segment, d_dst), self._h,
                  "jx_shard_record_export_device")

    def combine_records_device(self, d_records: int, nrecords: int, d_out: int, stream=None):
        """Merge nrecords back-to-back shard records on the device (compute_aggregate_share)."""
        with self._ordered(stream):
            check(self._L.jx_shard_record_combine_device(self._h, d_records, nrecords, d_out), self._h,
                  "jx_shard_record_combine_device")

    # ------------------------------------------------------------------ collection
    def _collect_jobs(self, jobs, nrecords: int, expect, aads, njobs_keys: int):
        """The host arrays jx_collect_seal* takes: the jobs' record lists as a CSR, the expectations, the aads."""
        njobs = len(jobs)
        if not (len(aads) == njobs and njobs_keys == njobs) or (expect is not None and len(expect) != njobs):
            raise ValueError("one aad, one 32-byte ephemeral key and (when given) one expectation per job")
        off = np.zeros(njobs + 1, np.uint64)
        off[1:] = np.cumsum([len(j) for j in jobs], dtype=np.uint64)
        idx = np.ascontiguousarray(np.asarray([r for j in jobs for r in j] or [0], dtype=np.int64))
        if idx.min() < 0 or idx.max() >= 2**32:
            raise ValueError("record indices are u32")
        idx = idx.astype(np.uint32)
        aad, ao = _packed(aads)
        ec = ecs = None
        if expect is not None:
            ec = np.ascontiguousarray(np.asarray([c for c, _ in expect] or [0], dtype=np.uint64))
            if any(len(cs) != 32 for _, cs in expect):
                raise ValueError("a checksum is 32 bytes")
            ecs = np.frombuffer(b"".join(cs for _, cs in expect) or bytes(32), np.uint8).copy()
        return off, idx, ec, ecs, aad, ao

    def collect_seal(self, records, jobs, aads, ephemeral_sks, sender, min_batch_size: int, max_batch_size: int = 0,
                     expect=None, want_shares: bool = False) -> CollectSeal:
        """Merge, check and seal many collection jobs in one call (jx_collect_seal): the helper's
        handle_aggregate_share_generic and the leader's collection step. records: nrecords x record_bytes() shard records
        (bytes or array; the state of batch_aggregations rows); jobs[j]: the indices of job j's records; aads[j]: its
        encoded AggregateShareAad; ephemeral_sks: njobs x 32 bytes from the caller's CSPRNG; sender: an HpkeSealer with
        the collector's public key and the (AggregateShare, this role -> Collector) info; expect: per job (report count,
        checksum) of the other aggregator, None for the leader. A job whose status is not COLLECT_OK has zeros for
        enc, ciphertext and share; its count and checksum are reported all the same."""
        rb, njobs = self.record_bytes(), len(jobs)
        rec = np.ascontiguousarray(np.frombuffer(records, np.uint8) if isinstance(records, (bytes, bytearray))
                                   else np.asarray(records, dtype=np.uint8)).reshape(-1)
        if rec.size % rb:
            raise ValueError(f"records: a multiple of {rb} bytes")
        nrecords = rec.size // rb
        sks = _u8(ephemeral_sks, njobs, 32, "ephemeral_sks")
        off, idx, ec, ecs, aad, ao = self._collect_jobs(jobs, nrecords, expect, aads, njobs)
        pt = self.output_len * self.field_bytes
        out = CollectSeal(np.zeros(njobs, np.uint8), np.zeros(njobs, np.uint64), np.zeros((njobs, 32), np.uint8),
                          np.zeros((njobs, 32), np.uint8), np.zeros((njobs, pt + 16), np.uint8),
                          np.zeros((njobs, pt), np.uint8) if want_shares else None)
        check(self._L.jx_collect_seal(self._h, njobs, _ptr(rec) if nrecords else None, nrecords, _u64p(off),
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _u64p(ec), _ptr(ecs),
                                      min_batch_size, max_batch_size, _ptr(aad), _u64p(ao), _ptr(sks), sender.handle,
                                      _ptr(out.status), _u64p(out.counts), _ptr(out.checksums), _ptr(out.encs),
                                      _ptr(out.cts), _ptr(out.shares)),
              self._h, "jx_collect_seal")
        return out

    def collect_seal_device(self, d_records: int, nrecords: int, jobs, aads, d_ephemeral_sks: int, sender,
                            min_batch_size: int, max_batch_size: int, d_out_status: int, d_out_counts: int,
                            d_out_checksums: int, d_out_encs: int, d_out_cts: int, d_out_shares: int | None = None,
                            expect=None, stream=None):
        """collect_seal with the records, the ephemeral keys and every output in HBM (jx_collect_seal_device; 8-byte
        aligned pointers); the jobs' record lists, the aads and the expectations stay host arrays. Asynchronous, ordered
        against `stream` (module docstring)."""
        njobs = len(jobs)
        off, idx, ec, ecs, aad, ao = self._collect_jobs(jobs, nrecords, expect, aads, njobs)
        with self._ordered(stream):
            check(self._L.jx_collect_seal_device(self._h, njobs, d_records, nrecords, _u64p(off),
                                                 idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _u64p(ec),
                                                 _ptr(ecs), min_batch_size, max_batch_size, _ptr(aad), _u64p(ao),
                                                 d_ephemeral_sks, sender.handle, d_out_status, d_out_counts,
                                                 d_out_checksums, d_out_encs, d_out_cts, d_out_shares),
                  self._h, "jx_collect_seal_device")

    def collect_open(self, leader_opener, helper_opener, leader_shares, helper_shares, aads) -> CollectOpen:
        """The collector for n collections (jx_collect_open): open both encrypted aggregate shares of each and add them
        mod p. leader_opener / helper_opener: HpkeOpener contexts holding the collector's keypair with the
        (AggregateShare, Leader / Helper -> Collector) infos; leader_shares / helper_shares: per collection (enc,
        ciphertext); aads: per collection the encoded AggregateShareAad. An encapsulated key of another length than the
        KEM's never reaches the GPU: that share did not open."""
        n = len(aads)
        if not len(leader_shares) == len(helper_shares) == n:
            raise ValueError("one leader share, one helper share and one aad per collection")
        pt = self.output_len * self.field_bytes
        out = CollectOpen(np.zeros((n, pt), np.uint8), np.zeros(n, np.uint8))
        pre = {i: code for i in range(n) for code, op, sh in ((COLLECT_OPEN_HELPER, helper_opener, helper_shares),
                                                               (COLLECT_OPEN_LEADER, leader_opener, leader_shares))
               if len(sh[i][0]) != op.enc_len}
        keep = [i for i in range(n) if i not in pre]
        for i, code in pre.items():
            out.status[i] = code
        if not keep:
            return out
        m = len(keep)
        arrs = []
        for sh in (leader_shares, helper_shares):
            encs = np.frombuffer(b"".join(sh[i][0] for i in keep), np.uint8).copy()
            arrs += [encs, *_packed([sh[i][1] for i in keep])]
        aad, ao = _packed([aads[i] for i in keep])
        agg, st = np.zeros((m, pt), np.uint8), np.zeros(m, np.uint8)
        check(self._L.jx_collect_open(self._h, leader_opener.handle, helper_opener.handle, m, _ptr(arrs[0]), _ptr(arrs[1]),
                                      _u64p(arrs[2]), _ptr(arrs[3]), _ptr(arrs[4]),
                                      _u64p(arrs[5]), _ptr(aad), _u64p(ao), _ptr(agg), _ptr(st)),
              self._h, "jx_collect_open")
        out.aggregates[keep] = agg
        out.status[keep] = st
        return out

    def collect_open_device(self, leader_opener, helper_opener, n: int, d_leader_encs: int, d_leader_cts: int,
                            leader_ct_offsets, d_helper_encs: int, d_helper_cts: int, helper_ct_offsets, aads,
                            d_out_aggregates: int, d_out_status: int, stream=None):
        """collect_open with the encapsulated keys (n x enc_len rows), the ciphertexts and both outputs in HBM
        (jx_collect_open_device); the ciphertext offsets [n + 1] and the aads stay on the host. Asynchronous, ordered
        against `stream` (module docstring)."""
        lo = _offs(leader_ct_offsets, n)
        ho = _offs(helper_ct_offsets, n)
        if len(aads) != n:
            raise ValueError("one aad per collection")
        aad, ao = _packed(aads)
        with self._ordered(stream):
            check(self._L.jx_collect_open_device(self._h, leader_opener.handle, helper_opener.handle, n, d_leader_encs,
                                                 d_leader_cts, _u64p(lo), d_helper_encs, d_helper_cts, _u64p(ho),
                                                 _ptr(aad), _u64p(ao), d_out_aggregates, d_out_status),
                  self._h, "jx_collect_open_device")

    def set_capacity(self, reports: int):
        check(self._L.jx_engine_set_capacity(self._h, reports), self._h, "jx_engine_set_capacity")

    def sync(self):
        check(self._L.jx_engine_sync(self._h), self._h, "jx_engine_sync")

    def stream(self) -> int:
        s = ctypes.c_void_p()
        check(self._L.jx_engine_stream(self._h, ctypes.byref(s)), self._h, "jx_engine_stream")
        return s.value or 0

    # ------------------------------------------------------------------ coalescing and memory
    def coalesce(self, enable: bool = True, window_us: int = 0):
        """Coalesced prepares: helper_initialized_batch / leader_initialized_batch of small jobs join the
        device's next shared launch with the concurrent jobs of every coalescing engine of this Prio3
        instance on the device (each report keeps its own engine's verify key). window_us = 0: automatic."""
        check(self._L.jx_engine_coalesce(self._h, int(bool(enable)), int(window_us)), self._h, "jx_engine_coalesce")

    def memory(self) -> dict:
        """This engine's resident batches and the device arena / coalescer counters (jx_engine_memory)."""
        m = _lib.JxMemoryStats()
        check(self._L.jx_engine_memory(self._h, ctypes.byref(m)), self._h, "jx_engine_memory")
        return {name: int(getattr(m, name)) for name, _ in m._fields_}

    # ------------------------------------------------------------------ instrumentation
    def timing(self, enable: bool):
        check(self._L.jx_engine_timing(self._h, int(enable)), self._h, "jx_engine_timing")

    def timing_read(self) -> dict:
        ms = (ctypes.c_float * 4)()
        ln = (ctypes.c_uint64 * 4)()
        check(self._L.jx_engine_timing_read(self._h, ms, ln), self._h, "jx_engine_timing_read")
        names = ("xof", "flp", "accumulate", "slow")
        return {k: {"ms": float(ms[i]), "launches": int(ln[i])} for i, k in enumerate(names)}

    def debug(self, option: int, value: int):
        check(self._L.jx_engine_debug(self._h, option, value), self._h, "jx_engine_debug")


Prio3Engine = HelperEngine

__all__ = ["HelperEngine", "Prio3Engine", "BatchResult", "EncryptedResult", "LeaderInit", "EngineError", "InitReq",
           "VERDICT_LABELS", "FINISHED", "OPEN_STATUS"]
