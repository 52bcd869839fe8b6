"""DAP message codecs on the hot path (subset of /root/reference/messages/src/lib.rs).

Only what the helper's aggregate-init loop touches: PingPongMessage (prio's
topology::ping_pong framing, KATs at messages/src/lib.rs:4232-4240, 4289-4297,
4321-4333), PrepareInit (:2114-2228), PrepareResp / PrepareStepResult / PrepareError
(:2237-2349). Encodings are big-endian length-prefixed as in the DAP codec.
"""
from __future__ import annotations

import enum
import struct
from dataclasses import dataclass


class CodecError(ValueError):
    pass


class _Reader:
    def __init__(self, b: bytes):
        self.b, self.i = memoryview(b), 0

    def take(self, n: int) -> bytes:
        if self.i + n > len(self.b):
            raise CodecError("short read")
        v = bytes(self.b[self.i:self.i + n])
        self.i += n
        return v

    def u8(self) -> int:
        return self.take(1)[0]

    def u16(self) -> int:
        return struct.unpack(">H", self.take(2))[0]

    def u32(self) -> int:
        return struct.unpack(">I", self.take(4))[0]

    def u64(self) -> int:
        return struct.unpack(">Q", self.take(8))[0]

    def opaque16(self) -> bytes:
        return self.take(self.u16())

    def opaque32(self) -> bytes:
        return self.take(self.u32())

    def done(self):
        if self.i != len(self.b):
            raise CodecError("trailing bytes")


def _o16(b: bytes) -> bytes:
    return struct.pack(">H", len(b)) + b


def _o32(b: bytes) -> bytes:
    return struct.pack(">I", len(b)) + b


# ----------------------------------------------------------------------------- PingPongMessage


@dataclass(frozen=True)
class PingPongMessage:
    """Initialize{prep_share} (0), Continue{prep_msg, prep_share} (1), Finish{prep_msg} (2)."""

    kind: int
    prep_msg: bytes = b""
    prep_share: bytes = b""

    INITIALIZE, CONTINUE, FINISH = 0, 1, 2

    @classmethod
    def initialize(cls, prep_share: bytes) -> "PingPongMessage":
        return cls(cls.INITIALIZE, prep_share=prep_share)

    @classmethod
    def finish(cls, prep_msg: bytes) -> "PingPongMessage":
        return cls(cls.FINISH, prep_msg=prep_msg)

    def encode(self) -> bytes:
        if self.kind == self.INITIALIZE:
            return b"\x00" + _o32(self.prep_share)
        if self.kind == self.CONTINUE:
            return b"\x01" + _o32(self.prep_msg) + _o32(self.prep_share)
        return b"\x02" + _o32(self.prep_msg)

    @classmethod
    def decode(cls, b: bytes) -> "PingPongMessage":
        r = _Reader(b)
        k = r.u8()
        if k == 0:
            m = cls(0, prep_share=r.opaque32())
        elif k == 1:
            pm = r.opaque32()
            m = cls(1, prep_msg=pm, prep_share=r.opaque32())
        elif k == 2:
            m = cls(2, prep_msg=r.opaque32())
        else:
            raise CodecError("unexpected PingPongMessage type")
        r.done()
        return m


# ----------------------------------------------------------------------------- Prepare*


class PrepareError(enum.IntEnum):  # messages/src/lib.rs:2338-2349
    BatchCollected = 0
    ReportReplayed = 1
    ReportDropped = 2
    HpkeUnknownConfigId = 3
    HpkeDecryptError = 4
    VdafPrepError = 5
    BatchSaturated = 6
    TaskExpired = 7
    InvalidMessage = 8
    ReportTooEarly = 9


@dataclass(frozen=True)
class ReportMetadata:
    report_id: bytes
    time: int

    def encode(self) -> bytes:
        return self.report_id + struct.pack(">Q", self.time)


@dataclass(frozen=True)
class HpkeCiphertext:
    config_id: int
    encapsulated_key: bytes
    payload: bytes

    def encode(self) -> bytes:
        return bytes([self.config_id]) + _o16(self.encapsulated_key) + _o32(self.payload)

    @classmethod
    def decode_from(cls, r: _Reader) -> "HpkeCiphertext":
        return cls(r.u8(), r.opaque16(), r.opaque32())


@dataclass(frozen=True)
class Report:
    """A client report as uploaded to the leader (messages/src/lib.rs:1353-1432): metadata || u32-prefixed public
    share || leader_encrypted_input_share || helper_encrypted_input_share."""

    metadata: ReportMetadata
    public_share: bytes
    leader_encrypted_input_share: HpkeCiphertext
    helper_encrypted_input_share: HpkeCiphertext

    MEDIA_TYPE = "application/dap-report"

    def encode(self) -> bytes:
        return (self.metadata.encode() + _o32(self.public_share) + self.leader_encrypted_input_share.encode() +
                self.helper_encrypted_input_share.encode())

    @classmethod
    def decode(cls, b: bytes) -> "Report":
        r = _Reader(b)
        md = ReportMetadata(r.take(16), r.u64())
        ps = r.opaque32()
        leader = HpkeCiphertext.decode_from(r)
        helper = HpkeCiphertext.decode_from(r)
        r.done()
        return cls(md, ps, leader, helper)


@dataclass(frozen=True)
class ReportShare:
    metadata: ReportMetadata
    public_share: bytes
    encrypted_input_share: HpkeCiphertext

    def encode(self) -> bytes:
        return self.metadata.encode() + _o32(self.public_share) + self.encrypted_input_share.encode()

    @classmethod
    def decode_from(cls, r: _Reader) -> "ReportShare":
        md = ReportMetadata(r.take(16), r.u64())
        ps = r.opaque32()
        cfg = r.u8()
        enc = r.opaque16()
        payload = r.opaque32()
        return cls(md, ps, HpkeCiphertext(cfg, enc, payload))


@dataclass(frozen=True)
class PrepareInit:
    report_share: ReportShare
    message: PingPongMessage

    def encode(self) -> bytes:
        return self.report_share.encode() + _o32(self.message.encode())

    @classmethod
    def decode(cls, b: bytes) -> "PrepareInit":
        r = _Reader(b)
        rs = ReportShare.decode_from(r)
        msg = PingPongMessage.decode(r.opaque32())
        r.done()
        return cls(rs, msg)


@dataclass(frozen=True)
class PrepareStepResult:
    """Continue{message} (0), Finished (1), Reject(PrepareError) (2)."""

    kind: int
    message: PingPongMessage | None = None
    error: PrepareError | None = None

    def encode(self) -> bytes:
        if self.kind == 0:
            return b"\x00" + _o32(self.message.encode())
        if self.kind == 1:
            return b"\x01"
        return b"\x02" + bytes([int(self.error)])


@dataclass(frozen=True)
class PrepareResp:
    report_id: bytes
    result: PrepareStepResult

    def encode(self) -> bytes:
        return self.report_id + self.result.encode()

    @classmethod
    def decode(cls, b: bytes) -> "PrepareResp":
        r = _Reader(b)
        rid = r.take(16)
        k = r.u8()
        if k == 0:
            res = PrepareStepResult(0, message=PingPongMessage.decode(r.opaque32()))
        elif k == 1:
            res = PrepareStepResult(1)
        elif k == 2:
            res = PrepareStepResult(2, error=PrepareError(r.u8()))
        else:
            raise CodecError("unexpected PrepareStepResult")
        r.done()
        return cls(rid, res)


# ----------------------------------------------------------------------------- PlaintextInputShare

EXTENSION_TBD, EXTENSION_TASKPROV = 0x0000, 0xFF00  # messages/src/lib.rs:924-927


@dataclass(frozen=True)
class Extension:
    extension_type: int
    extension_data: bytes = b""

    def encode(self) -> bytes:
        return struct.pack(">H", self.extension_type) + _o16(self.extension_data)


@dataclass(frozen=True)
class PlaintextInputShare:
    """extensions (u16-length-prefixed list) || payload (u32-length-prefixed), the HPKE plaintext
    of a report share (messages/src/lib.rs:1323-1326)."""

    extensions: tuple = ()
    payload: bytes = b""

    def encode(self) -> bytes:
        ext = b"".join(e.encode() for e in self.extensions)
        return _o16(ext) + _o32(self.payload)

    @classmethod
    def decode(cls, b: bytes) -> "PlaintextInputShare":
        r = _Reader(b)
        er = _Reader(r.opaque16())
        exts = []
        while er.i < len(er.b):
            t = er.u16()
            if t not in (EXTENSION_TBD, EXTENSION_TASKPROV):
                raise CodecError("unknown extension type")
            exts.append(Extension(t, er.opaque16()))
        payload = r.opaque32()
        r.done()
        return cls(tuple(exts), payload)


# ----------------------------------------------------------------------------- aggregate-init request / response

QUERY_TIME_INTERVAL, QUERY_FIXED_SIZE = 1, 2  # messages/src/query_type.rs: the query-type code points


@dataclass(frozen=True)
class PartialBatchSelector:
    """query type byte, then the batch id (32 bytes) under FixedSize and nothing under TimeInterval
    (messages/src/lib.rs:1606-1700). Decoding expects the task's query type (decode_expecting_value, :1659-1666)."""

    query_type: int
    batch_id: bytes | None = None

    @classmethod
    def time_interval(cls) -> "PartialBatchSelector":
        return cls(QUERY_TIME_INTERVAL)

    @classmethod
    def fixed_size(cls, batch_id: bytes) -> "PartialBatchSelector":
        return cls(QUERY_FIXED_SIZE, bytes(batch_id))

    def encode(self) -> bytes:
        if self.query_type == QUERY_TIME_INTERVAL:
            return b"\x01"
        if self.query_type != QUERY_FIXED_SIZE or self.batch_id is None or len(self.batch_id) != 32:
            raise CodecError("FixedSize carries a 32-byte batch id; no other query type is known")
        return b"\x02" + self.batch_id

    @classmethod
    def decode_from(cls, r: _Reader, query_type: int) -> "PartialBatchSelector":
        if query_type not in (QUERY_TIME_INTERVAL, QUERY_FIXED_SIZE):
            raise ValueError("unknown query type")
        if r.u8() != query_type:
            raise CodecError("unexpected query type")
        return cls(query_type, r.take(32) if query_type == QUERY_FIXED_SIZE else None)

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "PartialBatchSelector":
        r = _Reader(b)
        s = cls.decode_from(r, query_type)
        r.done()
        return s


def _prepare_init_from(r: _Reader) -> PrepareInit:
    rs = ReportShare.decode_from(r)
    return PrepareInit(rs, PingPongMessage.decode(r.opaque32()))


@dataclass(frozen=True)
class AggregationJobInitializeReq:
    """u32-prefixed aggregation parameter || PartialBatchSelector || u32 byte length of the PrepareInits || the
    PrepareInits (messages/src/lib.rs:2482-2553)."""

    aggregation_parameter: bytes
    partial_batch_selector: PartialBatchSelector
    prepare_inits: tuple

    MEDIA_TYPE = "application/dap-aggregation-job-init-req"

    def encode(self) -> bytes:
        items = b"".join(p.encode() for p in self.prepare_inits)
        return _o32(self.aggregation_parameter) + self.partial_batch_selector.encode() + _o32(items)

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "AggregationJobInitializeReq":
        r = _Reader(b)
        param = r.opaque32()
        sel = PartialBatchSelector.decode_from(r, query_type)
        ir = _Reader(r.opaque32())
        r.done()
        inits = []
        while ir.i < len(ir.b):
            inits.append(_prepare_init_from(ir))
        return cls(param, sel, tuple(inits))


def _prepare_resp_from(r: _Reader) -> PrepareResp:
    rid = r.take(16)
    k = r.u8()
    if k == 0:
        return PrepareResp(rid, PrepareStepResult(0, message=PingPongMessage.decode(r.opaque32())))
    if k == 1:
        return PrepareResp(rid, PrepareStepResult(1))
    if k == 2:
        e = r.u8()
        if e not in PrepareError._value2member_map_:
            raise CodecError("unexpected PrepareError")
        return PrepareResp(rid, PrepareStepResult(2, error=PrepareError(e)))
    raise CodecError("unexpected PrepareStepResult")


@dataclass(frozen=True)
class AggregationJobResp:
    """u32 byte length of the PrepareResps || the PrepareResps (messages/src/lib.rs:2669-2700)."""

    prepare_resps: tuple

    MEDIA_TYPE = "application/dap-aggregation-job-resp"

    def encode(self) -> bytes:
        return _o32(b"".join(p.encode() for p in self.prepare_resps))

    @classmethod
    def decode(cls, b: bytes) -> "AggregationJobResp":
        r = _Reader(b)
        ir = _Reader(r.opaque32())
        r.done()
        resps = []
        while ir.i < len(ir.b):
            resps.append(_prepare_resp_from(ir))
        return cls(tuple(resps))


# ----------------------------------------------------------------------------- collection

from .batch_aggregation import Interval  # noqa: E402  (the DAP Interval; its codec is below)

_U64_MAX = (1 << 64) - 1


def _interval_encode(iv: Interval) -> bytes:
    """Interval (messages/src/lib.rs:219-260): u64 start || u64 duration, seconds."""
    return struct.pack(">QQ", iv.start, iv.duration)


def _interval_from(r: _Reader) -> Interval:
    start, duration = r.u64(), r.u64()
    if start + duration > _U64_MAX:  # Interval::new refuses an end past u64 (:232-240)
        raise CodecError("interval end overflows u64")
    return Interval(start, duration)


def encode_interval(iv: Interval) -> bytes:
    return _interval_encode(iv)


def decode_interval(b: bytes) -> Interval:
    r = _Reader(b)
    iv = _interval_from(r)
    r.done()
    return iv


def _expect_query_type(r: _Reader, query_type: int) -> None:
    if query_type not in (QUERY_TIME_INTERVAL, QUERY_FIXED_SIZE):
        raise ValueError("unknown query type")
    if r.u8() != query_type:  # query_type::Code::decode_expecting_value
        raise CodecError("unexpected query type")


@dataclass(frozen=True)
class BatchSelector:
    """query type byte, then the batch interval under TimeInterval and the 32-byte batch id under FixedSize
    (messages/src/lib.rs:2711-2777). Decoding expects the task's query type."""

    query_type: int
    batch_interval: Interval | None = None
    batch_id: bytes | None = None

    @classmethod
    def time_interval(cls, batch_interval: Interval) -> "BatchSelector":
        return cls(QUERY_TIME_INTERVAL, batch_interval=batch_interval)

    @classmethod
    def fixed_size(cls, batch_id: bytes) -> "BatchSelector":
        return cls(QUERY_FIXED_SIZE, batch_id=bytes(batch_id))

    def encode(self) -> bytes:
        if self.query_type == QUERY_TIME_INTERVAL and self.batch_interval is not None:
            return b"\x01" + _interval_encode(self.batch_interval)
        if self.query_type != QUERY_FIXED_SIZE or self.batch_id is None or len(self.batch_id) != 32:
            raise CodecError("TimeInterval carries an interval, FixedSize a 32-byte batch id; no other query type is known")
        return b"\x02" + self.batch_id

    @classmethod
    def decode_from(cls, r: _Reader, query_type: int) -> "BatchSelector":
        _expect_query_type(r, query_type)
        if query_type == QUERY_TIME_INTERVAL:
            return cls(query_type, batch_interval=_interval_from(r))
        return cls(query_type, batch_id=r.take(32))

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "BatchSelector":
        r = _Reader(b)
        s = cls.decode_from(r, query_type)
        r.done()
        return s


FIXED_SIZE_BY_BATCH_ID, FIXED_SIZE_CURRENT_BATCH = 0, 1  # FixedSizeQuery (messages/src/lib.rs:1422-1476)


@dataclass(frozen=True)
class Query:
    """query type byte, then the query body (messages/src/lib.rs:1479-1550): the batch interval under TimeInterval; under
    FixedSize a FixedSizeQuery, ByBatchId (0) with its batch id or CurrentBatch (1)."""

    query_type: int
    batch_interval: Interval | None = None
    fixed_size_kind: int | None = None
    batch_id: bytes | None = None

    @classmethod
    def time_interval(cls, batch_interval: Interval) -> "Query":
        return cls(QUERY_TIME_INTERVAL, batch_interval=batch_interval)

    @classmethod
    def by_batch_id(cls, batch_id: bytes) -> "Query":
        return cls(QUERY_FIXED_SIZE, fixed_size_kind=FIXED_SIZE_BY_BATCH_ID, batch_id=bytes(batch_id))

    @classmethod
    def current_batch(cls) -> "Query":
        return cls(QUERY_FIXED_SIZE, fixed_size_kind=FIXED_SIZE_CURRENT_BATCH)

    def encode(self) -> bytes:
        if self.query_type == QUERY_TIME_INTERVAL and self.batch_interval is not None:
            return b"\x01" + _interval_encode(self.batch_interval)
        if self.query_type == QUERY_FIXED_SIZE and self.fixed_size_kind == FIXED_SIZE_CURRENT_BATCH:
            return b"\x02\x01"
        if self.query_type != QUERY_FIXED_SIZE or self.fixed_size_kind != FIXED_SIZE_BY_BATCH_ID or \
                self.batch_id is None or len(self.batch_id) != 32:
            raise CodecError("not a TimeInterval query nor a FixedSize one (ByBatchId with 32 bytes, CurrentBatch)")
        return b"\x02\x00" + self.batch_id

    @classmethod
    def decode_from(cls, r: _Reader, query_type: int) -> "Query":
        _expect_query_type(r, query_type)
        if query_type == QUERY_TIME_INTERVAL:
            return cls(query_type, batch_interval=_interval_from(r))
        kind = r.u8()
        if kind == FIXED_SIZE_BY_BATCH_ID:
            return cls(query_type, fixed_size_kind=kind, batch_id=r.take(32))
        if kind == FIXED_SIZE_CURRENT_BATCH:
            return cls(query_type, fixed_size_kind=kind)
        raise CodecError("unexpected FixedSizeQueryType value")

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "Query":
        r = _Reader(b)
        q = cls.decode_from(r, query_type)
        r.done()
        return q


@dataclass(frozen=True)
class CollectionReq:
    """Query || u32-prefixed aggregation parameter (messages/src/lib.rs:1551-1600)."""

    query: Query
    aggregation_parameter: bytes = b""

    MEDIA_TYPE = "application/dap-collect-req"

    def encode(self) -> bytes:
        return self.query.encode() + _o32(self.aggregation_parameter)

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "CollectionReq":
        r = _Reader(b)
        q = Query.decode_from(r, query_type)
        param = r.opaque32()
        r.done()
        return cls(q, param)


@dataclass(frozen=True)
class AggregateShareReq:
    """BatchSelector || u32-prefixed aggregation parameter || u64 report count || 32-byte ReportIdChecksum
    (messages/src/lib.rs:2783-2864)."""

    batch_selector: BatchSelector
    aggregation_parameter: bytes
    report_count: int
    checksum: bytes

    MEDIA_TYPE = "application/dap-aggregate-share-req"

    def encode(self) -> bytes:
        if len(self.checksum) != 32:
            raise CodecError("a ReportIdChecksum is 32 bytes")
        return (self.batch_selector.encode() + _o32(self.aggregation_parameter) + struct.pack(">Q", self.report_count) +
                self.checksum)

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "AggregateShareReq":
        r = _Reader(b)
        sel = BatchSelector.decode_from(r, query_type)
        param = r.opaque32()
        count = r.u64()
        checksum = r.take(32)
        r.done()
        return cls(sel, param, count, checksum)


@dataclass(frozen=True)
class AggregateShare:
    """One HpkeCiphertext: the helper's encrypted aggregate share (messages/src/lib.rs:2869-2908)."""

    encrypted_aggregate_share: HpkeCiphertext

    MEDIA_TYPE = "application/dap-aggregate-share"

    def encode(self) -> bytes:
        return self.encrypted_aggregate_share.encode()

    @classmethod
    def decode(cls, b: bytes) -> "AggregateShare":
        r = _Reader(b)
        ct = HpkeCiphertext.decode_from(r)
        r.done()
        return cls(ct)


@dataclass(frozen=True)
class Collection:
    """PartialBatchSelector || u64 report count || Interval || the leader's HpkeCiphertext || the helper's
    (messages/src/lib.rs:1726-1817)."""

    partial_batch_selector: PartialBatchSelector
    report_count: int
    interval: Interval
    leader_encrypted_agg_share: HpkeCiphertext
    helper_encrypted_agg_share: HpkeCiphertext

    MEDIA_TYPE = "application/dap-collection"

    def encode(self) -> bytes:
        return (self.partial_batch_selector.encode() + struct.pack(">Q", self.report_count) +
                _interval_encode(self.interval) + self.leader_encrypted_agg_share.encode() +
                self.helper_encrypted_agg_share.encode())

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "Collection":
        r = _Reader(b)
        sel = PartialBatchSelector.decode_from(r, query_type)
        count = r.u64()
        iv = _interval_from(r)
        leader = HpkeCiphertext.decode_from(r)
        helper = HpkeCiphertext.decode_from(r)
        r.done()
        return cls(sel, count, iv, leader, helper)


@dataclass(frozen=True)
class AggregateShareAad:
    """The associated data of an encrypted aggregate share: task id || u32-prefixed aggregation parameter ||
    BatchSelector (messages/src/lib.rs:1887-1952)."""

    task_id: bytes
    aggregation_parameter: bytes
    batch_selector: BatchSelector

    def encode(self) -> bytes:
        if len(self.task_id) != 32:
            raise CodecError("a task id is 32 bytes")
        return self.task_id + _o32(self.aggregation_parameter) + self.batch_selector.encode()

    @classmethod
    def decode(cls, b: bytes, query_type: int) -> "AggregateShareAad":
        r = _Reader(b)
        task_id = r.take(32)
        param = r.opaque32()
        sel = BatchSelector.decode_from(r, query_type)
        r.done()
        return cls(task_id, param, sel)
