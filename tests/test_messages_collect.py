"""The collection messages of janus_amd/messages.py against the reference's own test vectors
(tests/golden/wire/dap_collect_kats.json: values and hex copied from messages/src/lib.rs, with their line numbers):
both directions, a truncation of each, and a wrong query-type code."""
import json
import os

import pytest

from janus_amd import messages as M
from janus_amd.messages import (AggregateShare, AggregateShareAad, AggregateShareReq, BatchSelector, CodecError, Collection,
                                CollectionReq, HpkeCiphertext, Interval, PartialBatchSelector, Query)

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "wire", "dap_collect_kats.json")))


def ids(name):
    return [f"{name}:{k['lines']}" for k in KATS[name]]


def iv(d):
    return Interval(d["start"], d["duration"])


def ct(d):
    return HpkeCiphertext(d["config_id"], bytes.fromhex(d["encapsulated_key"]), bytes.fromhex(d["payload"]))


def selector(k):
    return BatchSelector.time_interval(iv(k["interval"])) if k["query_type"] == 1 else \
        BatchSelector.fixed_size(bytes.fromhex(k["batch_id"]))


def query(k):
    if k["query_type"] == 1:
        return Query.time_interval(iv(k["interval"]))
    return Query.by_batch_id(bytes.fromhex(k["batch_id"])) if k["fixed_size"] == "by_batch_id" else Query.current_batch()


def other(query_type):
    return 3 - query_type


def roundtrip(value, hexstr, decode):
    """encode gives the vector; decode gives the value back; every proper prefix is refused; so is a byte more."""
    want = bytes.fromhex(hexstr)
    assert value.encode() == want
    assert decode(want) == value
    for cut in range(len(want)):
        with pytest.raises(CodecError):
            decode(want[:cut])
    with pytest.raises(CodecError):
        decode(want + b"\0")


@pytest.mark.parametrize("k", KATS["interval"], ids=ids("interval"))
def test_interval(k):
    want = bytes.fromhex(k["hex"])
    assert M.encode_interval(iv(k)) == want
    if not k["decodes"]:  # an end past u64: Interval::get_decoded refuses what the struct literal encoded
        with pytest.raises(CodecError):
            M.decode_interval(want)
        return
    assert M.decode_interval(want) == iv(k)
    for cut in range(len(want)):
        with pytest.raises(CodecError):
            M.decode_interval(want[:cut])
    with pytest.raises(CodecError):
        M.decode_interval(want + b"\0")


@pytest.mark.parametrize("k", KATS["query"], ids=ids("query"))
def test_query(k):
    roundtrip(query(k), k["hex"], lambda b: Query.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        Query.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))


def test_query_unknown_fixed_size_kind():
    with pytest.raises(CodecError):
        Query.decode(b"\x02\x02" + bytes(32), 2)


@pytest.mark.parametrize("k", KATS["collection_req"], ids=ids("collection_req"))
def test_collection_req(k):
    v = CollectionReq(query(k), bytes.fromhex(k["aggregation_parameter"]))
    roundtrip(v, k["hex"], lambda b: CollectionReq.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        CollectionReq.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))


@pytest.mark.parametrize("k", KATS["collection"], ids=ids("collection"))
def test_collection(k):
    sel = PartialBatchSelector.time_interval() if k["query_type"] == 1 else \
        PartialBatchSelector.fixed_size(bytes.fromhex(k["batch_id"]))
    v = Collection(sel, k["report_count"], iv(k["interval"]), ct(k["leader"]), ct(k["helper"]))
    roundtrip(v, k["hex"], lambda b: Collection.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        Collection.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))


@pytest.mark.parametrize("k", KATS["batch_selector"], ids=ids("batch_selector"))
def test_batch_selector(k):
    roundtrip(selector(k), k["hex"], lambda b: BatchSelector.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        BatchSelector.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))
    bad = bytearray(bytes.fromhex(k["hex"]))
    bad[0] = 3  # a code point no query type has
    with pytest.raises(CodecError):
        BatchSelector.decode(bytes(bad), k["query_type"])


@pytest.mark.parametrize("k", KATS["aggregate_share_req"], ids=ids("aggregate_share_req"))
def test_aggregate_share_req(k):
    v = AggregateShareReq(selector(k), bytes.fromhex(k["aggregation_parameter"]), k["report_count"],
                          bytes.fromhex(k["checksum"]))
    roundtrip(v, k["hex"], lambda b: AggregateShareReq.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        AggregateShareReq.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))


@pytest.mark.parametrize("k", KATS["aggregate_share"], ids=ids("aggregate_share"))
def test_aggregate_share(k):
    roundtrip(AggregateShare(ct(k)), k["hex"], AggregateShare.decode)


@pytest.mark.parametrize("k", KATS["aggregate_share_aad"], ids=ids("aggregate_share_aad"))
def test_aggregate_share_aad(k):
    v = AggregateShareAad(bytes.fromhex(k["task_id"]), bytes.fromhex(k["aggregation_parameter"]), selector(k))
    roundtrip(v, k["hex"], lambda b: AggregateShareAad.decode(b, k["query_type"]))
    with pytest.raises(CodecError):
        AggregateShareAad.decode(bytes.fromhex(k["hex"]), other(k["query_type"]))
