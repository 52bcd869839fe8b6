"""The collector's last step on the GPU: open the two encrypted aggregate shares of a Collection and unshard them.

Mirror of Collector::poll_once's tail (collector/src/lib.rs:573-629): hpke::open of the leader's share
under HpkeApplicationInfo(AggregateShare, Leader, Collector) and of the helper's under (AggregateShare, Helper,
Collector), both with the AggregateShareAad of what the collector asked for (task id, aggregation parameter, batch
selector), then Prio3.unshard. The opens and the element-wise sum run in one engine call
(HelperEngine.collect_open, jx_collect_open); the decode of the result into the VDAF's aggregate type stays here. Only
NoDifferentialPrivacy is covered.
"""
from __future__ import annotations

from dataclasses import dataclass

from .engine import COLLECT_DECODE_HELPER, COLLECT_DECODE_LEADER, COLLECT_OPEN_HELPER, COLLECT_OPEN_LEADER, HelperEngine
from .hpke import (AEAD_AES_128_GCM, KDF_HKDF_SHA256, KEM_X25519_HKDF_SHA256, LABEL_AGGREGATE_SHARE, ROLE_COLLECTOR,
                   ROLE_HELPER, ROLE_LEADER, HpkeOpener, application_info)
from .messages import AggregateShareAad, BatchSelector, Collection, Interval
from .vdaf import PRIO3_COUNT, PRIO3_FIXEDPOINT_L2, PRIO3_SUM, Prio3


class HpkeOpenError(ValueError):
    """An encrypted aggregate share did not open (Error::Hpke)."""


class AggregateShareDecode(ValueError):
    """An opened aggregate share has the wrong length or holds an element >= p (Error::AggregateShareDecode)."""


@dataclass(frozen=True)
class CollectionResult:
    """collector/src/lib.rs Collection: what the collector gets out of a collection job."""

    partial_batch_selector: object
    report_count: int
    interval: Interval
    aggregate_result: object  # an int (Count, Sum), a list of ints (SumVec, Histogram, multiproof SumVec) or floats


class Collector:
    """One task's collector on one GPU: the VDAF, the task id and the collector's HPKE keypair (private key 32 bytes;
    public key 32 bytes under X25519, 65 under P-256)."""

    def __init__(self, v: Prio3, task_id: bytes, keypair: tuple[bytes, bytes], device: int = 0,
                 kem_id: int = KEM_X25519_HKDF_SHA256, kdf_id: int = KDF_HKDF_SHA256, aead_id: int = AEAD_AES_128_GCM):
        if len(task_id) != 32:
            raise ValueError("task id is 32 bytes")
        self.vdaf, self.task_id = v, task_id
        sk, pk = keypair
        suite = dict(device=device, kem_id=kem_id, kdf_id=kdf_id, aead_id=aead_id)
        self._leader = HpkeOpener(sk, pk, application_info(LABEL_AGGREGATE_SHARE, ROLE_LEADER, ROLE_COLLECTOR), **suite)
        self._helper = HpkeOpener(sk, pk, application_info(LABEL_AGGREGATE_SHARE, ROLE_HELPER, ROLE_COLLECTOR), **suite)
        # the engine runs no preparation here: its verify key is never read
        self._engine = HelperEngine(v, bytes(v.verify_key_len), device=device)

    def close(self):
        for c in (self._engine, self._leader, self._helper):
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _result(self, row: bytes, report_count: int):
        v, fb = self.vdaf, self.vdaf.field_bytes
        if v.algo_id == PRIO3_FIXEDPOINT_L2:
            return v.decode_fixedpoint_result(row, report_count)
        vals = [int.from_bytes(row[i:i + fb], "little") for i in range(0, len(row), fb)]
        return vals[0] if v.algo_id in (PRIO3_COUNT, PRIO3_SUM) else vals

    def unshard_batch(self, collections: list) -> list[CollectionResult]:
        """Many collections in one engine call. collections: (Collection body, the BatchSelector the collector asked
        for, the aggregation parameter) each. Raises for the first collection that fails, as unshard does."""
        decoded = [Collection.decode(body, sel.query_type) for body, sel, _ in collections]
        aads = [AggregateShareAad(self.task_id, param, sel).encode() for _, sel, param in collections]
        shares = lambda ct: (ct.encapsulated_key, ct.payload)  # noqa: E731
        out = self._engine.collect_open(self._leader, self._helper, [shares(c.leader_encrypted_agg_share) for c in decoded],
                                        [shares(c.helper_encrypted_agg_share) for c in decoded], aads)
        results = []
        for i, c in enumerate(decoded):
            st = int(out.status[i])
            if st in (COLLECT_OPEN_LEADER, COLLECT_OPEN_HELPER):
                raise HpkeOpenError(f"collection {i}: the {'leader' if st == COLLECT_OPEN_LEADER else 'helper'}'s "
                                    "aggregate share did not open")
            if st in (COLLECT_DECODE_LEADER, COLLECT_DECODE_HELPER):
                raise AggregateShareDecode(f"collection {i}: the {'leader' if st == COLLECT_DECODE_LEADER else 'helper'}"
                                           "'s aggregate share does not decode")
            results.append(CollectionResult(c.partial_batch_selector, c.report_count, c.interval,
                                            self._result(out.aggregates[i].tobytes(), c.report_count)))
        return results

    def unshard(self, collection_body: bytes, batch_selector: BatchSelector, agg_param: bytes = b"") -> CollectionResult:
        """Decode the Collection, build the aad from what the collector asked for, open both shares and unshard."""
        return self.unshard_batch([(collection_body, batch_selector, agg_param)])[0]
