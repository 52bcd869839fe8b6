#!/usr/bin/env python3
"""Time the leader's end of the aggregate-init exchange on the GPU (jx_init_req_encode[_device], jx_init_resp_decode)
next to the leader's prepare-init on the same reports and next to the host work it replaces.

Workload: as tools/bench_wire.py, one request of n (default 16,384) sealed Prio3SumVec 8 x 1000 / 88 reports, here
sharded and sealed by the engine's own client calls, in two bodies: `uniform` (32-byte encapsulated keys) and
`alternating` (32- and 65-byte keys alternating, as two KEMs' reports would; the 65-byte keys are random bytes, so
the helper rejects those reports and the response is half two-byte rejections).

  check     before any timing, for every body: the device body equals janus_amd.messages' encoding and
            tools/wire_join.cpp's byte for byte; the helper's real response (handle_aggregate_init_wire on a second
            engine) decodes into the prep-message rows and peer verdicts aggregator.leader_process_helper_response
            derives from the same responses; the tool fails otherwise
  encode    jx_init_req_encode_device, device events on the engine stream around the call and the host clock, the
            median of five runs after two warm-ups; the host form (every array uploaded, the body copied back) by
            the host clock
  decode    jx_init_resp_decode, the same way (the call queues its kernel; the events bracket it)
  init      jx_leader_prep_init_device_ex on the same reports, the same way
  copy      the device-to-host copy of the prep shares (into pinned memory) that the object path needs
  host      tools/wire_join.cpp: one thread packing the same body from the same arrays

No threshold: the ratios are written down as found.

  python tools/bench_wire_leader.py --out profiles/wire_encode.json
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def join_exe() -> str:
    src = os.path.join(ROOT, "tools", "wire_join.cpp")
    exe = os.path.join(ROOT, "tools", "bin", "wire_join")
    deps = [src, os.path.join(ROOT, "janus_amd", "csrc", "jx_wire.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, src], check=True)
        os.replace(tmp, exe)
    return exe


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n

    import torch

    from janus_amd import hpke
    from janus_amd.aggregator import handle_aggregate_init_wire
    from janus_amd.engine import RESP_CONTINUED, WIRE_OK, HelperEngine
    from janus_amd.messages import (QUERY_TIME_INTERVAL, AggregationJobInitializeReq, AggregationJobResp, HpkeCiphertext,
                                    PartialBatchSelector, PingPongMessage, PrepareInit, ReportMetadata, ReportShare)
    from janus_amd.vdaf import Prio3
    from oracle import hpke_oracle as H

    if not torch.cuda.is_available():
        raise SystemExit("bench_wire_leader needs a GPU (there is no CPU path)")
    v = Prio3.sum_vec(8, 1000, 88)
    vk, task = bytes(range(16)), bytes(range(32, 64))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0x5EED)
    t0 = time.perf_counter()
    meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    eph = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    times = np.arange(n, dtype=np.uint64) + np.uint64(1_700_000_000)
    skl, skh = rng.bytes(32), rng.bytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    info_l, info_h = H.dap_info(recipient=hpke.ROLE_LEADER), H.dap_info(recipient=hpke.ROLE_HELPER)
    PS, LPS, PM, LIS = v.public_share_len, v.prep_share_len, v.prep_msg_len, v.leader_input_share_len
    result = {"tool": "tools/bench_wire_leader.py", "vdaf": v.name(), "n": n, "device": torch.cuda.get_device_name(0),
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

    with hpke.HpkeSealer(pkl, info_l) as sl, hpke.HpkeSealer(pkh, info_h) as sh, hpke.HpkeOpener(skh, pkh, info_h) as oh, \
            HelperEngine(v, vk) as eng, HelperEngine(v, vk) as helper:
        rows = eng.shard_batch(meas, nonces, rands)
        sealed = eng.seal_reports(nonces, times, rows.public_shares, rows.leader_input_shares, rows.helper_input_shares,
                                  task, sl, sh, eph.tobytes(), shard_status=rows.status)
        assert not sealed.status.any() and not rows.status.any()
        ps, cts = rows.public_shares, sealed.helper_cts
        print(f"{n} reports sharded and sealed in {time.perf_counter() - t0:.1f} s", flush=True)
        s_eng = torch.cuda.ExternalStream(eng.stream())
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to(dev)  # noqa: E731
        d_ids, d_ps, d_lis, d_pay = up(nonces), up(ps), up(rows.leader_input_shares), up(cts)
        d_lps = torch.zeros(n * LPS, dtype=torch.uint8, device=dev)
        d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
        assert d_lis.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        bids = []

        def init():
            bids.append(eng.leader_init_device(n, d_ids.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(), d_lps.data_ptr(),
                                               d_v.data_ptr(), stream=False))
            if len(bids) > 1:
                eng.release(bids.pop(0))

        result["leader_prep_init_device_ex"] = timed(init, s_eng)
        eng.sync()
        lps = d_lps.cpu().numpy().reshape(n, LPS)
        assert not d_v.cpu().numpy().any()
        # on torch's own stream: torch remembers which stream last used a pinned tensor and records an event on it when
        # the tensor is freed, which must not be the engine's stream once the engine is gone
        pinned = torch.empty(n * LPS, dtype=torch.uint8).pin_memory()
        result["prep_share_copy_to_host"] = dict(timed(lambda: pinned.copy_(d_lps, non_blocking=True),
                                                       torch.cuda.current_stream()), bytes=n * LPS)
        del pinned
        cfg = np.full(n, 7, np.uint8)
        poff = np.arange(n + 1, dtype=np.uint64) * np.uint64(cts.shape[1])
        fake = rng.integers(0, 256, size=(n, 65), dtype=np.uint8)
        enc_len = {"uniform": lambda i: 32, "alternating": lambda i: 65 if i % 2 else 32}
        sel = PartialBatchSelector.time_interval()
        for name, el in enc_len.items():
            encs = [sealed.helper_encs[i].tobytes() if el(i) == 32 else fake[i].tobytes() for i in range(n)]
            eoff = np.concatenate([[0], np.cumsum([len(x) for x in encs])]).astype(np.uint64)
            enc_bytes = np.frombuffer(b"".join(encs), np.uint8)
            d_en = up(enc_bytes)
            torch.cuda.synchronize()
            # ---- check: the body against the Python codec and the one-thread packer
            want = AggregationJobInitializeReq(b"", sel, tuple(
                PrepareInit(ReportShare(ReportMetadata(nonces[i].tobytes(), int(times[i])), ps[i].tobytes(),
                                        HpkeCiphertext(7, encs[i], cts[i].tobytes())),
                            PingPongMessage.initialize(lps[i].tobytes())) for i in range(n))).encode()

            def encode(d_out=None, capacity=0):
                return eng.encode_init_req(n, d_ids.data_ptr(), times, d_ps.data_ptr(), cfg, d_en.data_ptr(), d_pay.data_ptr(),
                                           poff, d_lps.data_ptr(), d_v.data_ptr(), b"", QUERY_TIME_INTERVAL,
                                           enc_offsets=eoff, d_out=d_out, capacity=capacity, stream=False)

            req = encode()
            if req.body != want or req.n_sent != n:
                raise SystemExit(f"bench_wire_leader: the {name} body differs from the Python codec's")
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "arrays.bin")
                with open(path, "wb") as fh:
                    fh.write(struct.pack("<QIIII", n, PS, LPS, QUERY_TIME_INTERVAL, 0) + bytes(32) + nonces.tobytes() +
                             times.tobytes() + cfg.tobytes() + ps.tobytes() + eoff.tobytes() + enc_bytes.tobytes() +
                             poff.tobytes() + cts.tobytes() + lps.tobytes())
                out = subprocess.run([join_exe(), path, path + ".body", str(a.runs), str(a.warmups)], check=True,
                                     capture_output=True, text=True, timeout=600)
                with open(path + ".body", "rb") as fh:
                    if fh.read() != want:
                        raise SystemExit(f"bench_wire_leader: wire_join's {name} body differs from the Python codec's")
            r = {"body_bytes": len(want), "equals_python_codec": True, "equals_wire_join": True,
                 "host_wire_join_cpp": json.loads(out.stdout)}
            # ---- the helper's real response, and its decode against the object path's derivation
            resp_body, hfin, _ = handle_aggregate_init_wire(helper, want, task, oh, 7, QUERY_TIME_INTERVAL)
            resps = AggregationJobResp.decode(resp_body).prepare_resps
            msgs, cont = np.zeros((n, PM), np.uint8), np.zeros(n, bool)
            for k, p in enumerate(resps):  # as leader_process_helper_response fills them
                m = p.result.message
                if p.result.kind == 0 and m.kind == PingPongMessage.FINISH and len(m.prep_msg) == PM:
                    msgs[k], cont[k] = np.frombuffer(m.prep_msg, np.uint8), True
            d_m = torch.full((n, PM), 0xA5, dtype=torch.uint8, device=dev)
            d_p = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
            dec = eng.decode_init_resp(req, resp_body, d_m.data_ptr(), d_p.data_ptr(), stream=False)
            eng.sync()
            if not (dec.status == WIRE_OK and np.array_equal(d_m.cpu().numpy(), msgs) and
                    np.array_equal(d_p.cpu().numpy() == 0, cont) and np.array_equal(dec.results == RESP_CONTINUED, cont)
                    and np.array_equal(cont, hfin)):
                raise SystemExit(f"bench_wire_leader: the decoded response of the {name} body differs from the object path's")
            r.update(response_bytes=len(resp_body), continued=int(cont.sum()), response_equals_object_path=True)
            # ---- timings
            d_out = torch.zeros(len(want), dtype=torch.uint8, device=dev)
            held = [req]

            def enc_dev():
                held.append(encode(d_out.data_ptr(), len(want)))
                held.pop(0).release()

            r["encode_device"] = timed(enc_dev, s_eng)
            t_host = []
            for i in range(a.warmups + a.runs):
                t = time.perf_counter()
                eng.encode_init_req_host(nonces, times, ps, cfg, enc_bytes, cts.reshape(-1), poff, lps, np.zeros(n, np.uint8),
                                         b"", QUERY_TIME_INTERVAL, enc_offsets=eoff).release()
                if i >= a.warmups:
                    t_host.append((time.perf_counter() - t) * 1e3)
            r["encode_host_form_ms_median"] = round(float(np.median(t_host)), 3)
            r["response_decode"] = timed(lambda: eng.decode_init_resp(held[-1], resp_body, d_m.data_ptr(), d_p.data_ptr(),
                                                                      stream=False), s_eng)
            held.pop().release()
            enc = r["encode_device"]["host_clock_ms_median"]
            join = r["host_wire_join_cpp"]["ms_median"]
            copy = result["prep_share_copy_to_host"]["host_clock_ms_median"]
            r["encode_gb_per_s"] = round(len(want) / enc / 1e6, 2)
            r["encode_device_kernels_gb_per_s"] = round(len(want) / r["encode_device"]["device_ms_median"] / 1e6, 2)
            r["host_join_plus_copy_over_device_encode"] = round((join + copy) / enc, 2)
            r["encode_over_leader_prep_init"] = round(enc / result["leader_prep_init_device_ex"]["host_clock_ms_median"], 4)
            result["bodies"][name] = r
            print(name + ": " + json.dumps(r), flush=True)
        eng.release(bids.pop())
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
