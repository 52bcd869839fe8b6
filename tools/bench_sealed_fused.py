#!/usr/bin/env python3
"""Time the fused prepare + aggregate from SEALED helper input shares (jx_helper_prep_aggregate_encrypted_device:
every launch of every pipeline lays out its rows, opens its reports and masks its verdicts) against the plaintext
jx_helper_prep_aggregate_device on the same reports, in one process, alternating, after warming both. A step is the
call plus jx_engine_sync, timed with the host clock; the time each call takes to return is kept too. The host forms
(pageable buffers; tools/bench_host_path.py's figure for the plaintext one) are timed the same way.

Workload: SumVec 8 x 1000 / 88, 1.25M reports: bench.py's pool (4,096 distinct reports), each pool report sealed
once under one task keypair of the default suite (16 ephemeral keys round-robin, key schedules from the Python
reference, AEAD by tools/upload_seal.cpp in 16 threads, one report pinned against the Python reference) and the
sealed pool tiled as the plaintext one is. Before anything is timed, the sealed call's verdicts, prep messages, aggregate, count and checksum
must equal the plaintext call's, and every report must have opened: the tool fails otherwise.

    python tools/bench_sealed_fused.py --out profiles/sealed_fused.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def seal_pool(task: bytes, nonces, ps, his, seed: int = 7):
    """Every pool report's helper input share sealed once: (sk, pk, info, times, encs (K x 32), cts (K x ct_len))."""
    import hpke_suites_ref as S
    from bench_upload import seal_lib
    from janus_amd import hpke
    from oracle import hpke_oracle as H

    rng = np.random.default_rng(seed)
    info = H.dap_info()
    sk = rng.bytes(32)
    pk = H.x25519_base(sk)
    ctxs = []
    for _ in range(16):  # an X25519 in Python takes milliseconds; the device decapsulates every report
        ss, enc = H.encap(rng.bytes(32), pk)
        ctxs.append((enc,) + S.key_schedule(1, 1, ss, info))
    K, hl = his.shape
    times = np.arange(K, dtype=np.uint64) + np.uint64(1_700_000_000)
    pts = np.zeros((K, 6 + hl), np.uint8)  # PlaintextInputShare: no extensions, u32-prefixed payload
    pts[:, 2:6] = np.frombuffer(hl.to_bytes(4, "big"), np.uint8)
    pts[:, 6:] = his
    cts = np.zeros((K, 6 + hl + 16), np.uint8)
    aads = [hpke.input_share_aad(task, nonces[i].tobytes(), int(times[i]), ps[i].tobytes()) for i in range(K)]
    L = seal_lib()

    def seal(i):
        enc, key, nonce = ctxs[i % 16]
        L.us_seal(1, key, nonce, aads[i], len(aads[i]), pts[i].ctypes.data, pts.shape[1], cts[i].ctypes.data)

    with ThreadPoolExecutor(16) as pool:
        list(pool.map(seal, range(K)))
    enc, key, nonce = ctxs[0]  # the sealing code is the kernels' own: pin one report against the Python reference
    assert cts[0].tobytes() == S.aead_seal(1, key, nonce, aads[0], pts[0].tobytes()), \
        "host sealing disagrees with the Python reference"
    encs = np.frombuffer(b"".join(ctxs[i % 16][0] for i in range(K)), np.uint8).reshape(K, 32).copy()
    return sk, pk, info, times, encs, cts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reports", type=int, default=1_250_000)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=2, help="steps of each host form (0: skip them)")
    ap.add_argument("--pipes", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, help="reports per launch (debug option 5; 0: automatic)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench
    from janus_amd import hpke
    from janus_amd.engine import KEY_NONE, HelperEngine
    from janus_amd.vdaf import Prio3

    vdaf = Prio3.sum_vec(8, 1000, 88)
    vk = bytes(range(16))
    t0 = time.perf_counter()
    orc, nonces, ps, his, lps, want, how = bench.load_or_make_pool(vdaf, vk, a.pool, 16, 0, expect=False)
    task = bytes(range(32, 64))
    sk, pk, info, times, encs, cts = seal_pool(task, nonces, ps, his)
    print(f"pool of {a.pool} reports {how} and sealed in {time.perf_counter() - t0:.1f} s", flush=True)
    R, K, ct_len = a.reports, a.pool, cts.shape[1]
    idx = np.arange(R) % K
    dev = torch.device("cuda", 0)
    d_idx = torch.from_numpy(idx).to(dev)

    def dev_tile(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev).index_select(0, d_idx).contiguous()

    d_n, d_ps, d_his, d_lps, d_enc, d_ct = (dev_tile(x) for x in (nonces, ps, his, lps, encs, cts))
    del d_idx
    h_times = np.ascontiguousarray(times[idx])
    h_off = np.arange(R + 1, dtype=np.uint64) * np.uint64(ct_len)
    h_ki = np.zeros((R, 2), np.uint8)
    h_ki[:, 1] = KEY_NONE
    out = {k: (torch.empty(R, dtype=torch.uint8, device=dev), torch.empty((R, 16), dtype=torch.uint8, device=dev))
           for k in ("plain", "sealed")}
    d_status = torch.empty(R, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    result = {"workload": f"{R} x {vdaf.name()} helper reports, pool of {K} tiled, sealed shares of {ct_len} bytes",
              "reports": R}
    with hpke.HpkeOpener(sk, pk, info) as op, HelperEngine(vdaf, vk) as ep, HelperEngine(vdaf, vk) as es:
        for e in (ep, es):
            if a.pipes:
                e.debug(4, a.pipes)
            if a.chunk:
                e.debug(5, a.chunk)

        def plain():
            t = time.perf_counter()
            ep.prep_and_aggregate_device(d_n.data_ptr(), d_ps.data_ptr(), d_his.data_ptr(), d_lps.data_ptr(), R, 0,
                                         out["plain"][1].data_ptr(), out["plain"][0].data_ptr(), stream=False)
            back = time.perf_counter() - t
            ep.sync()
            return time.perf_counter() - t, back

        def sealed():
            t = time.perf_counter()
            es.prep_and_aggregate_encrypted_device(d_n.data_ptr(), h_times, d_ps.data_ptr(), task, [op], h_ki,
                                                   d_enc.data_ptr(), d_ct.data_ptr(), h_off, d_lps.data_ptr(), R,
                                                   d_out_prep_msgs=out["sealed"][1].data_ptr(),
                                                   d_out_verdicts=out["sealed"][0].data_ptr(),
                                                   d_out_open_status=d_status.data_ptr(), stream=False)
            back = time.perf_counter() - t
            es.sync()
            return time.perf_counter() - t, back

        # ---- verification: one call each on fresh aggregations; the plaintext call is the reference
        plain()
        sealed()
        pv, pm = (t.cpu().numpy() for t in out["plain"])
        sv, sm = (t.cpu().numpy() for t in out["sealed"])
        st = d_status.cpu().numpy()
        fin = pv == 0
        assert (st == 0).all(), f"{int((st != 0).sum())} reports did not open"
        assert np.array_equal(sv, pv), "verdicts differ from the plaintext call's"
        assert np.array_equal(sm[fin], pm[fin]), "prep messages differ from the plaintext call's"
        assert ep.aggregate_share(0) == es.aggregate_share(0), "aggregate, count or checksum differ"
        assert int(fin.sum()) == ep.aggregate_share(0)[1] > 0
        result["verified"] = {"reports": R, "finished": int(fin.sum()), "opened": int((st == 0).sum()),
                              "pipelines": es.memory()["last_pipelines"]}
        print("verified: " + json.dumps(result["verified"]), flush=True)
        # ---- the device forms, alternating
        for _ in range(max(a.warmup - 1, 0)):
            plain()
            sealed()
        pairs = [(plain(), sealed()) for _ in range(a.pairs)]
        p_s = [p[0][0] for p in pairs]
        s_s = [p[1][0] for p in pairs]
        ratios = [x / y for x, y in zip(p_s, s_s)]  # sealed rate over plaintext rate, pair by pair
        result["device"] = {
            "plaintext_reports_per_s": round(R / float(np.median(p_s)), 1),
            "sealed_reports_per_s": round(R / float(np.median(s_s)), 1),
            "plaintext_ms": [round(x * 1e3, 2) for x in p_s], "sealed_ms": [round(x * 1e3, 2) for x in s_s],
            "ratio_sealed_over_plaintext": round(float(np.median(ratios)), 4),
            "ratio_spread": [round(min(ratios), 4), round(max(ratios), 4)],
            "plaintext_call_returns_ms": round(float(np.median([p[0][1] for p in pairs])) * 1e3, 2),
            "sealed_call_returns_ms": round(float(np.median([p[1][1] for p in pairs])) * 1e3, 2),
        }
        print(json.dumps(result["device"]), flush=True)
        # ---- the host forms (pageable buffers), as tools/bench_host_path.py times the plaintext one
        if a.host_steps:
            h = [np.ascontiguousarray(x[idx]) for x in (nonces, ps, his, lps, encs, cts)]

            def host_plain():
                return ep.prep_and_aggregate(h[0], h[1], h[2], h[3])

            def host_sealed():
                r = es.prep_and_aggregate_encrypted(h[0], h_times, h[1], task, [op], h_ki, h[4], h[5].reshape(-1), h[3],
                                                    payload_offsets=h_off)
                return r.verdicts, r.prep_msgs

            res = {}
            for name, fn in (("plaintext", host_plain), ("sealed", host_sealed)):
                fn()  # warm-up (staging allocation)
                t = time.perf_counter()
                for _ in range(a.host_steps):
                    v, m = fn()
                el = (time.perf_counter() - t) / a.host_steps
                assert np.array_equal(v, pv) and np.array_equal(m[fin], pm[fin]), f"host {name}: results differ"
                res[name + "_reports_per_s"] = round(R / el, 1)
                res[name + "_ms"] = round(el * 1e3, 2)
            res["ratio_sealed_over_plaintext"] = round(res["sealed_reports_per_s"] / res["plaintext_reports_per_s"], 4)
            result["host"] = res
            print(json.dumps(res), flush=True)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
