#!/usr/bin/env python3
"""Time the aggregate-init codec on the GPU (jx_init_req_decode_device, jx_init_resp_encode_device) next to the sealed
fused call on the same reports and next to the host work it replaces.

Workload: one AggregationJobInitializeReq of n (default 16,384) sealed Prio3SumVec 8 x 1000 / 88 PrepareInits, all
distinct (the C oracle's reports, each helper share sealed once under one task keypair as tools/bench_sealed_fused.py
seals its pool), in three bodies: `uniform` (every message the same length: the index's fast pass alone),
`alternating` (32- and 65-byte encapsulated keys alternating, as two KEMs' reports would: the fallback loop, a wave's
worth of messages per iteration) and `irregular` (encapsulated keys of 32 + 7 i mod 13 bytes, so no message has the
length of the one two before it: the fallback loop's worst case, one message per iteration). The keys of other
lengths than 32 are random bytes: those reports do not open.

  check     before any timing, for every body: every decoded array, both offset arrays, key_index, wire_status and
            the records' chain equal what janus_amd.messages extracts from the same bytes, and the response body the device
            encodes from the sealed call's verdicts and prep messages equals the Python codec's; the tool fails
            otherwise
  decode    jx_init_req_decode_device on the body resident in HBM, device events on the engine stream around the call
            and the host clock, the median of five runs after two warm-ups; the host form (the body's copy included)
            by the host clock
  encode    jx_init_resp_encode_device, the same way
  fused     jx_helper_prep_aggregate_encrypted_device on the decoded arrays, the same way
  host      tools/wire_split.cpp: one thread walking and splitting the same body (median of five after two warm-ups)

  --route   the route leg alone (jx_init_req_route): a request of the same lengths filled with random bytes (the route
            reads nothing but the times), its times spread over 1, 8 and 1,024 batch buckets of an hour. Checked first
            against what a caller of the decode did before there was a route: np.unique(times - times % P,
            return_inverse=True) on the pinned times, whose inverse is the route and whose values are the table. Timed
            with device events around the call on a freshly decoded handle (a handle routes once) and by the host
            clock; the caller's way, the np.unique and the copy of the n x 4-byte route to the device, by the host clock

No threshold: the ratios are written down as found.

  python tools/bench_wire.py --out profiles/wire_decode.json
  python tools/bench_wire.py --route --out profiles/wire_route.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def split_exe() -> str:
    src = os.path.join(ROOT, "tools", "wire_split.cpp")
    exe = os.path.join(ROOT, "tools", "bin", "wire_split")
    deps = [src, os.path.join(ROOT, "janus_amd", "csrc", "jx_wire.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, src], check=True)
        os.replace(tmp, exe)
    return exe


def route_leg(a) -> int:
    import random

    import torch

    from janus_amd.engine import KEY_NONE, ROUTE_OK, WIRE_OK, HelperEngine
    from janus_amd.messages import (QUERY_TIME_INTERVAL, AggregationJobInitializeReq, HpkeCiphertext, PartialBatchSelector,
                                    PingPongMessage, PrepareInit, ReportMetadata, ReportShare)
    from janus_amd.vdaf import Prio3

    if not torch.cuda.is_available():
        raise SystemExit("bench_wire needs a GPU (there is no CPU path)")
    n, P = a.n, 3600
    v = Prio3.sum_vec(8, 1000, 88)
    rnd = random.Random(12)
    t0 = 1_700_000_000 - 1_700_000_000 % P
    parts = [(rnd.randbytes(16), rnd.randbytes(v.public_share_len), rnd.randbytes(32),
              rnd.randbytes(22 + v.helper_input_share_len), rnd.randbytes(v.prep_share_len)) for _ in range(n)]
    dev = torch.device("cuda", 0)
    kf, ks = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    kf[7] = 0
    result = {"tool": "tools/bench_wire.py --route", "vdaf": v.name(), "n": n, "time_precision": P,
              "device": torch.cuda.get_device_name(0),
              "timing": f"medians of {a.runs} runs after {a.warmups} warm-ups; the route by device events on the engine "
                        "stream around the call and by the host clock, the caller's way by the host clock", "buckets": {}}
    with HelperEngine(v, bytes(range(16))) as eng:
        s_eng = torch.cuda.ExternalStream(eng.stream())
        for B in (1, 8, 1024):
            times = np.array([t0 + (i * B // n) * P + i % P for i in range(n)], np.uint64)
            body = AggregationJobInitializeReq(b"", PartialBatchSelector.time_interval(), tuple(
                PrepareInit(ReportShare(ReportMetadata(rid, int(t)), ps, HpkeCiphertext(7, enc, pay)),
                            PingPongMessage.initialize(lps)) for (rid, ps, enc, pay, lps), t in zip(parts, times))).encode()
            d_body = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(dev)
            torch.cuda.synchronize()

            def decode():
                req = eng.decode_init_req(d_body, QUERY_TIME_INTERVAL, kf, ks, length=len(body))
                assert req.status == WIRE_OK and req.n == n
                return req

            # ---- check: the device route against the caller's np.unique
            with decode() as req:
                starts, inverse = np.unique(req.times - req.times % np.uint64(P), return_inverse=True)
                status, table = req.route(P)
                route = req.device_bytes("route").cpu().numpy().view(np.uint32)
                lo, hi = np.full(len(starts), np.iinfo(np.uint64).max, np.uint64), np.zeros(len(starts), np.uint64)
                np.minimum.at(lo, inverse, req.times)
                np.maximum.at(hi, inverse, req.times)
                ok = (status == ROUTE_OK and np.array_equal(table["start"], starts) and np.array_equal(route, inverse)
                      and np.array_equal(table["reports"], np.bincount(inverse)) and np.array_equal(table["routed"], table["reports"])
                      and np.array_equal(table["min_time"], lo) and np.array_equal(table["max_time"], hi) and len(starts) == B)
            if not ok:
                raise SystemExit(f"bench_wire: the device route over {B} buckets differs from np.unique's")
            # ---- timings
            ev, host, caller = [], [], []
            d_route = torch.zeros(n, dtype=torch.int32, device=dev)
            for i in range(a.warmups + a.runs):
                with decode() as req:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    e0.record(s_eng)
                    req.route(P)
                    e1.record(s_eng)
                    e1.synchronize()
                    t_route = (time.perf_counter() - t) * 1e3
                    t = time.perf_counter()
                    _, inverse = np.unique(req.times - req.times % np.uint64(P), return_inverse=True)
                    d_route.copy_(torch.from_numpy(inverse.astype(np.int32)))
                    torch.cuda.synchronize()
                    t_caller = (time.perf_counter() - t) * 1e3
                    if i >= a.warmups:
                        ev.append(e0.elapsed_time(e1))
                        host.append(t_route)
                        caller.append(t_caller)
            r = {"body_bytes": len(body), "equals_np_unique": True,
                 "route_device_ms_median": round(float(np.median(ev)), 3),
                 "route_host_clock_ms_median": round(float(np.median(host)), 3),
                 "caller_np_unique_and_copy_ms_median": round(float(np.median(caller)), 3),
                 "route_device_ms": [round(x, 3) for x in ev]}
            result["buckets"][str(B)] = r
            print(f"{B} buckets: " + json.dumps(r), flush=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--pool", default=None, help="an .npz to keep the reports in: read when it is there, written when not")
    ap.add_argument("--out", default=None)
    ap.add_argument("--route", action="store_true", help="the route leg alone")
    a = ap.parse_args()
    if a.route:
        return route_leg(a)
    n = a.n

    import torch

    import bench
    from bench_sealed_fused import seal_pool
    from janus_amd import hpke
    from janus_amd.engine import KEY_NONE, WIRE_OK, HelperEngine
    from janus_amd.messages import (QUERY_TIME_INTERVAL, AggregationJobInitializeReq, AggregationJobResp, HpkeCiphertext,
                                    PartialBatchSelector, PingPongMessage, PrepareError, PrepareInit, PrepareResp,
                                    PrepareStepResult, ReportMetadata, ReportShare)
    from janus_amd.vdaf import Prio3

    if not torch.cuda.is_available():
        raise SystemExit("bench_wire needs a GPU (there is no CPU path)")
    v = Prio3.sum_vec(8, 1000, 88)
    vk = bytes(range(16))
    t0 = time.perf_counter()
    if a.pool and os.path.exists(a.pool):
        d = np.load(a.pool)
        nonces, ps, his, lps = d["nonces"], d["ps"], d["his"], d["lps"]
        assert nonces.shape[0] == n, "the pool file holds another number of reports"
    else:
        _, nonces, ps, his, lps, _ = bench.make_pool(v, vk, n, threads=16, expect=False)
        if a.pool:
            np.savez(a.pool, nonces=nonces, ps=ps, his=his, lps=lps)
    task = bytes(range(32, 64))
    sk, pk, info, times, encs, cts = seal_pool(task, nonces, ps, his)
    rng = np.random.default_rng(11)
    fake = rng.integers(0, 256, size=(n, 65), dtype=np.uint8)
    enc_len = {"uniform": lambda i: 32, "alternating": lambda i: 65 if i % 2 else 32, "irregular": lambda i: 32 + 7 * i % 13}

    def inits(name: str):
        return [PrepareInit(ReportShare(ReportMetadata(nonces[i].tobytes(), int(times[i])), ps[i].tobytes(),
                                        HpkeCiphertext(7, encs[i].tobytes() if enc_len[name](i) == 32 else
                                                       fake[i, :enc_len[name](i)].tobytes(), cts[i].tobytes())),
                            PingPongMessage.initialize(lps[i].tobytes())) for i in range(n)]

    real = {name: sum(enc_len[name](i) == 32 for i in range(n)) for name in enc_len}
    bodies = {name: AggregationJobInitializeReq(b"", PartialBatchSelector.time_interval(), tuple(inits(name))).encode()
              for name in enc_len}
    print(f"{n} reports made, sealed and framed in {time.perf_counter() - t0:.1f} s; bodies of "
          f"{[len(b) for b in bodies.values()]} bytes", flush=True)
    dev = torch.device("cuda", 0)
    kf, ks = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
    kf[7] = 0
    S = v.prep_msg_len
    result = {"tool": "tools/bench_wire.py", "vdaf": v.name(), "n": n, "device": torch.cuda.get_device_name(0),
              "timing": f"device events on the engine stream around the call and the host clock, medians of {a.runs} runs "
                        f"after {a.warmups} warm-ups", "bodies": {}}

    def timed(fn, stream):
        ev, host = [], []
        for i in range(a.warmups + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmups:
                host.append((time.perf_counter() - t) * 1e3)
                ev.append(e0.elapsed_time(e1))
        return {"device_ms_median": round(float(np.median(ev)), 3), "host_clock_ms_median": round(float(np.median(host)), 3),
                "device_ms": [round(x, 3) for x in ev]}

    with hpke.HpkeOpener(sk, pk, info) as op, HelperEngine(v, vk) as eng:
        s_eng = torch.cuda.ExternalStream(eng.stream())
        for name, body in bodies.items():
            d_body = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            # ---- check: the decode against the Python codec
            want = AggregationJobInitializeReq.decode(body, QUERY_TIME_INTERVAL).prepare_inits
            req = eng.decode_init_req(d_body, QUERY_TIME_INTERVAL, kf, ks, length=len(body))
            assert req.status == WIRE_OK and req.n == n, (req.status, req.error_offset)
            get = lambda k: req.device_bytes(k).cpu().numpy()  # noqa: E731
            w_enc = [p.report_share.encrypted_input_share.encapsulated_key for p in want]
            w_pay = [p.report_share.encrypted_input_share.payload for p in want]
            ok = (get("report_ids").tobytes() == b"".join(p.report_share.metadata.report_id for p in want)
                  and np.array_equal(get("times").view(np.uint64), [p.report_share.metadata.time for p in want])
                  and get("public_shares").tobytes() == b"".join(p.report_share.public_share for p in want)
                  and get("leader_prep_shares").tobytes() == b"".join(p.message.prep_share for p in want)
                  and get("encs").tobytes() == b"".join(w_enc) and get("payloads").tobytes() == b"".join(w_pay)
                  and np.array_equal(req.enc_offsets[1:], np.cumsum([len(x) for x in w_enc]))
                  and np.array_equal(req.payload_offsets[1:], np.cumsum([len(x) for x in w_pay]))
                  and np.array_equal(get("enc_offsets").view(np.uint64), req.enc_offsets)
                  and np.array_equal(get("payload_offsets").view(np.uint64), req.payload_offsets)
                  and (req.key_index == [0, KEY_NONE]).all() and not req.wire_status.any()
                  and not get("route").any() and np.array_equal(req.records["off"][1:], req.records["off"][:-1] + req.records["len"][:-1]))
            if not ok:
                raise SystemExit(f"bench_wire: the decoded arrays of the {name} body differ from the Python codec's")
            # ---- the sealed fused call on the decoded arrays, and the response against the Python codec
            d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_m = torch.zeros((n, S), dtype=torch.uint8, device=dev)
            ad = req.d

            def fused():
                eng.prep_and_aggregate_encrypted_device(ad.d_report_ids, req.times, ad.d_public_shares, task, [op],
                                                        req.key_index, ad.d_encs, ad.d_payloads, req.payload_offsets,
                                                        ad.d_leader_prep_shares, n, enc_offsets=req.enc_offsets,
                                                        d_out_prep_msgs=d_m.data_ptr(), d_out_verdicts=d_v.data_ptr(),
                                                        d_out_open_status=d_st.data_ptr(), d_segments=ad.d_route,
                                                        segment_ids=[0], stream=False)

            fused()
            eng.sync()
            body_out, fin = eng.encode_init_resp(req, d_v.data_ptr(), d_st.data_ptr(), d_m.data_ptr())
            vd, st, mm = d_v.cpu().numpy(), d_st.cpu().numpy(), d_m.cpu().numpy()
            err = {1: PrepareError.HpkeDecryptError, 7: PrepareError.HpkeUnknownConfigId}
            resps = [PrepareResp(p.report_share.metadata.report_id,
                                 PrepareStepResult(2, error=err.get(int(st[i]), PrepareError.InvalidMessage)) if st[i] else
                                 PrepareStepResult(2, error=PrepareError.VdafPrepError) if vd[i] else
                                 PrepareStepResult(0, message=PingPongMessage.finish(mm[i].tobytes())))
                     for i, p in enumerate(want)]
            if body_out != AggregationJobResp(tuple(resps)).encode():
                raise SystemExit(f"bench_wire: the response body of the {name} body differs from the Python codec's")
            finished = int(fin.sum())  # the pool's reports but its 1% with a flipped leader prep share; the fake keys' none
            assert finished == int(((vd == 0) & (st == 0)).sum()) and finished >= real[name] * 98 // 100
            r = {"body_bytes": len(body), "response_bytes": len(body_out), "finished": finished,
                 "fallback_iterations": req.fallback_iterations, "equals_python_codec": True}
            req.release()
            # ---- timings
            d_out = torch.zeros(len(body_out), dtype=torch.uint8, device=dev)
            held = []

            def decode():
                held.append(eng.decode_init_req(d_body, QUERY_TIME_INTERVAL, kf, ks, length=len(body), stream=False))
                if len(held) > 1:
                    held.pop(0).release()

            r["decode_device"] = timed(decode, s_eng)
            req = held[-1]
            ad = req.d
            t_host = []
            for i in range(a.warmups + a.runs):
                t = time.perf_counter()
                eng.decode_init_req(body, QUERY_TIME_INTERVAL, kf, ks).release()
                if i >= a.warmups:
                    t_host.append((time.perf_counter() - t) * 1e3)
            r["decode_host_body_ms_median"] = round(float(np.median(t_host)), 3)
            r["encode_device"] = timed(lambda: eng.encode_init_resp(req, d_v.data_ptr(), d_st.data_ptr(), d_m.data_ptr(),
                                                                    d_out=d_out.data_ptr(), capacity=len(body_out),
                                                                    stream=False), s_eng)
            r["sealed_fused_call"] = timed(lambda: (fused(), eng.sync()), s_eng)
            req.release()
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "body.bin")
                with open(path, "wb") as fh:
                    fh.write(body)
                out = subprocess.run([split_exe(), path, "1", str(v.public_share_len), str(v.prep_share_len), str(a.runs),
                                      str(a.warmups)], check=True, capture_output=True, text=True, timeout=600)
            r["host_wire_split_cpp"] = json.loads(out.stdout)
            dec, enc = r["decode_device"]["host_clock_ms_median"], r["encode_device"]["host_clock_ms_median"]
            r["decode_gb_per_s"] = round(len(body) / dec / 1e6, 2)
            r["host_split_over_device_decode"] = round(r["host_wire_split_cpp"]["ms_median"] / dec, 2)
            r["codec_over_sealed_fused_call"] = round((dec + enc) / r["sealed_fused_call"]["host_clock_ms_median"], 4)
            result["bodies"][name] = r
            print(name + ": " + json.dumps(r), flush=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
