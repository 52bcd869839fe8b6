"""The aggregate-init request and response codecs (janus_amd.messages) against the reference's own hex KATs
(tests/golden/wire/dap_wire_kats.json, copied as data from messages/src/lib.rs with their line numbers; in a folder of
its own because test_gpu_parity replays every tests/golden/*.json as a Prio3 fixture), and round trips."""
from __future__ import annotations

import json
import os
import random

import pytest

from janus_amd.messages import (AggregationJobInitializeReq, AggregationJobResp, CodecError, HpkeCiphertext,
                                PartialBatchSelector, PingPongMessage, PrepareError, PrepareInit, PrepareResp,
                                PrepareStepResult, ReportMetadata, ReportShare)

with open(os.path.join(os.path.dirname(__file__), "golden", "wire", "dap_wire_kats.json"), encoding="utf-8") as fh:
    KATS = json.load(fh)
H = bytes.fromhex


def _msg(m) -> PingPongMessage:
    return PingPongMessage(m["kind"], H(m["prep_msg"]), H(m["prep_share"]))


def _req(k) -> AggregationJobInitializeReq:
    sel = PartialBatchSelector(k["query_type"], H(k["batch_id"]) if k["batch_id"] else None)
    inits = tuple(PrepareInit(ReportShare(ReportMetadata(H(p["report_id"]), p["time"]), H(p["public_share"]),
                                          HpkeCiphertext(p["config_id"], H(p["encapsulated_key"]), H(p["payload"]))),
                              _msg(p["message"])) for p in k["prepare_inits"])
    return AggregationJobInitializeReq(H(k["aggregation_parameter"]), sel, inits)


@pytest.mark.parametrize("k", KATS["aggregation_job_initialize_req"], ids=lambda k: f"lines{k['lines']}")
def test_init_req_kats(k):
    req = _req(k)
    assert req.encode().hex() == k["hex"]
    assert AggregationJobInitializeReq.decode(H(k["hex"]), k["query_type"]) == req
    with pytest.raises(CodecError):  # decode_expecting_value: the task's query type
        AggregationJobInitializeReq.decode(H(k["hex"]), 3 - k["query_type"])
    for cut in range(len(k["hex"]) // 2):
        with pytest.raises(CodecError):
            AggregationJobInitializeReq.decode(H(k["hex"])[:cut], k["query_type"])
    with pytest.raises(CodecError):
        AggregationJobInitializeReq.decode(H(k["hex"]) + b"\0", k["query_type"])


@pytest.mark.parametrize("k", KATS["aggregation_job_resp"], ids=lambda k: f"lines{k['lines']}")
def test_resp_kats(k):
    resps = tuple(PrepareResp(H(p["report_id"]), PrepareStepResult(0, message=_msg(p["message"])) if p["kind"] == 0
                              else PrepareStepResult(1)) for p in k["prepare_resps"])
    resp = AggregationJobResp(resps)
    assert resp.encode().hex() == k["hex"]
    assert AggregationJobResp.decode(H(k["hex"])) == resp
    for bad in (H(k["hex"])[:-1], H(k["hex"]) + b"\0"):
        with pytest.raises(CodecError):
            AggregationJobResp.decode(bad)


def test_round_trips():
    rnd = random.Random(7)
    for trial in range(40):
        n = rnd.choice([0, 1, 2, 7])
        inits = []
        for _ in range(n):
            kind = rnd.randrange(3)
            msg = PingPongMessage(kind, rnd.randbytes(rnd.randrange(5)) if kind else b"",
                                  rnd.randbytes(rnd.randrange(40)) if kind < 2 else b"")
            inits.append(PrepareInit(ReportShare(ReportMetadata(rnd.randbytes(16), rnd.getrandbits(64)),
                                                 rnd.randbytes(rnd.choice([0, 16, 33])),
                                                 HpkeCiphertext(rnd.randrange(256), rnd.randbytes(rnd.choice([0, 32, 65])),
                                                                rnd.randbytes(rnd.randrange(80)))), msg))
        sel = PartialBatchSelector.fixed_size(rnd.randbytes(32)) if trial % 2 else PartialBatchSelector.time_interval()
        req = AggregationJobInitializeReq(rnd.randbytes(rnd.randrange(9)), sel, tuple(inits))
        assert AggregationJobInitializeReq.decode(req.encode(), sel.query_type) == req
        assert PartialBatchSelector.decode(sel.encode(), sel.query_type) == sel
        resps = []
        for p in inits:
            k = rnd.randrange(3)
            res = (PrepareStepResult(0, message=PingPongMessage.finish(rnd.randbytes(rnd.choice([0, 16, 32])))) if k == 0
                   else PrepareStepResult(1) if k == 1 else PrepareStepResult(2, error=PrepareError(rnd.randrange(10))))
            resps.append(PrepareResp(p.report_share.metadata.report_id, res))
        resp = AggregationJobResp(tuple(resps))
        assert AggregationJobResp.decode(resp.encode()) == resp
    with pytest.raises(CodecError):
        AggregationJobResp.decode(b"\0\0\0\x12" + bytes(16) + b"\x02\x0a")  # PrepareError 10 does not exist
    with pytest.raises(CodecError):
        PartialBatchSelector.fixed_size(bytes(31)).encode()
