#!/usr/bin/env python3
"""Time the client's seal on the GPU (jx_client_seal_device) against the opens of the same bytes.

Workload: n (default 16,384) all-distinct Prio3SumVec 8 x 1000 / 88 reports resident in HBM, every share under its own
ephemeral key: rows of random bytes (what is timed does not depend on their values), DHKEM(X25519, HKDF-SHA256) /
HKDF-SHA256 / AES-128-GCM for both recipients.

  check         before any timing: every sealed report opens (the leader's through jx_leader_upload_open_device, the
                helper's through jx_hpke_open_batch_device) and equals its row; the tool fails otherwise
  seal          seal_reports_device by device events around the call, the median of five runs after two warm-ups
  kernels       per-kernel times from one `rocprofv3 --kernel-trace --stats` run of this tool (--profile: a child
                process running --timed-only, started before this process touches the GPU)
  open          in the same process, over the same bytes: jx_leader_upload_open_device (the leader's ciphertexts) and
                jx_hpke_open_batch_device (the helper's), the same way
  host sealer   tools/upload_seal.cpp (the AEAD alone, no X25519) on 16 threads over --host-n of the leader plaintexts

No threshold: the ratio of seal time to open time of the same bytes is what is written down.

  python tools/bench_seal.py --profile --out profiles/seal.json
"""
from __future__ import annotations

import argparse
import csv
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

THREADS = 16
T0 = 1_700_000_000


def kernel_stats(n: int, seed: int) -> dict:
    """One traced run of the timed part in a child process; per kernel of the seal and the opens: calls and times."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "seal", "--",
               sys.executable, os.path.abspath(__file__), "--timed-only", "--n", str(n), "--seed", str(seed),
               "--runs", "1", "--warmups", "0"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel stats")
        out = {}
        with open(files[0], newline="") as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"(\w+_kernel(?:<[^>]*>)?)", r["Name"])
                if m and any(k in m.group(1) for k in ("seal_", "upload_", "hpke_open")):
                    name = m.group(1)
                    out[name] = {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                 "mean_ms": round(float(r["AverageNs"]) / 1e6, 3)}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--host-n", type=int, default=512)
    ap.add_argument("--timed-only", action="store_true", help="the device calls alone (what --profile traces)")
    ap.add_argument("--profile", action="store_true", help="add per-kernel times from a traced child run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n

    kernels = None
    if a.profile:  # before this process opens the GPU
        kernels = kernel_stats(n, a.seed)

    import torch

    from janus_amd import hpke
    from janus_amd.engine import KEY_NONE, HelperEngine
    from janus_amd.vdaf import Prio3
    from oracle import hpke_oracle as H

    if not torch.cuda.is_available():
        raise SystemExit("bench_seal needs a GPU (there is no CPU path)")
    v = Prio3.sum_vec(8, 1000, 88)
    lis, his, psl = v.leader_input_share_len, v.helper_input_share_len, v.public_share_len
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)  # noqa: E731
    d_ids, d_ps, d_lis, d_his, d_sks = rnd(n, 16), rnd(n, psl), rnd(n, lis), rnd(n, his), rnd(n, 64)
    # every 16 bytes of a row an element < p with probability 1 - 2^-59; the top byte cleared makes it certain
    d_lis.view(n, -1, 16)[:, :, 15] = 0
    assert len({bytes(r) for r in d_sks.cpu().numpy().reshape(2 * n, 32)}) == 2 * n, "ephemeral keys repeat"
    times = np.arange(T0, T0 + n, dtype=np.uint64)
    rng = np.random.default_rng(a.seed)
    task = rng.bytes(32)
    skl, skh = rng.bytes(32), rng.bytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    info_l, info_h = H.dap_info(recipient=hpke.ROLE_LEADER), H.dap_info(recipient=hpke.ROLE_HELPER)
    eng = HelperEngine(v, bytes(16))
    lct, hct = eng.client_seal_sizes()
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    d_lenc, d_lcts, d_henc, d_hcts, d_st = u8(n, 32), u8(n, lct), u8(n, 32), u8(n, hct), u8(n)
    d_rows, d_ext, d_open = u8(n, lis), u8(n * lct), u8(n)
    d_extlen = torch.zeros(n, dtype=torch.int32, device=dev)
    d_hpt, d_hok = u8(n, hct - 16), u8(n)
    sl, sh = hpke.HpkeSealer(pkl, info_l), hpke.HpkeSealer(pkh, info_h)
    ol, oh = hpke.HpkeOpener(skl, pkl, info_l), hpke.HpkeOpener(skh, pkh, info_h)
    # the helper's associated data, as jx_hpke_open_batch_device takes it
    ids_h, ps_h = d_ids.cpu().numpy(), d_ps.cpu().numpy()
    aads = np.concatenate([np.broadcast_to(np.frombuffer(task, np.uint8), (n, 32)), ids_h,
                           times.astype(">u8").view(np.uint8).reshape(n, 8),
                           np.broadcast_to(np.frombuffer(psl.to_bytes(4, "big"), np.uint8), (n, 4)), ps_h], axis=1)
    d_aads = torch.from_numpy(np.ascontiguousarray(aads)).to(dev)
    d_aoff = torch.arange(n + 1, dtype=torch.int64, device=dev) * aads.shape[1]
    d_hoff = torch.arange(n + 1, dtype=torch.int64, device=dev) * hct
    l_off = np.arange(n + 1, dtype=np.uint64) * lct
    key_index = np.array([[0, KEY_NONE]] * n, np.uint8)
    taskb = np.frombuffer(task, np.uint8).copy()
    u64p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    L = eng._L
    es = ctypes.c_void_p()
    assert L.jx_engine_stream(eng.handle, ctypes.byref(es)) == 0
    s_eng, s_hpke = torch.cuda.ExternalStream(es.value or 0), torch.cuda.ExternalStream(oh.stream)
    torch.cuda.synchronize()

    def seal():
        eng.seal_reports_device(n, d_ids.data_ptr(), times, d_ps.data_ptr(), d_lis.data_ptr(), d_his.data_ptr(), task, sl, sh,
                                d_sks.data_ptr(), d_lenc.data_ptr(), d_lcts.data_ptr(), d_henc.data_ptr(), d_hcts.data_ptr(),
                                d_st.data_ptr(), stream=False)

    def open_leader():
        st = L.jx_leader_upload_open_device(
            eng.handle, n, d_ids.data_ptr(), times.ctypes.data_as(u64p), d_ps.data_ptr(), taskb.ctypes.data_as(vp),
            (vp * 1)(ol.handle), 1, key_index.ctypes.data_as(vp), d_lenc.data_ptr(), None, d_lcts.data_ptr(),
            l_off.ctypes.data_as(u64p), d_rows.data_ptr(), 0, d_ext.data_ptr(), d_extlen.data_ptr(), d_open.data_ptr())
        assert st == 0, L.jx_last_error(eng.handle)

    def open_helper():
        st = oh._L.jx_hpke_open_batch_device(oh.handle, n, d_henc.data_ptr(), d_hcts.data_ptr(), d_hoff.data_ptr(),
                                             d_aads.data_ptr(), d_aoff.data_ptr(), d_hpt.data_ptr(), d_hok.data_ptr())
        assert st == 0, oh._L.jx_hpke_last_error(oh.handle)

    def timed(fn, stream, runs, warmups):
        ms = []
        for i in range(warmups + runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= warmups:
                ms.append(e0.elapsed_time(e1))
        return ms

    if a.timed_only:
        for fn, s in ((seal, s_eng), (open_leader, s_eng), (open_helper, s_hpke)):
            timed(fn, s, a.runs, a.warmups)
        for x in (eng, sl, sh, ol, oh):
            x.close()
        print(json.dumps({"n": n}))
        return

    # ---- before any timing: every sealed report opens and equals its row
    seal()
    open_leader()
    eng.sync()
    open_helper()
    torch.cuda.synchronize()
    want_hpt = torch.cat([torch.tensor(list(bytes(2) + his.to_bytes(4, "big")), dtype=torch.uint8, device=dev).expand(n, 6),
                          d_his], dim=1)
    ok = (not d_st.any().item() and not d_open.any().item() and torch.equal(d_rows, d_lis) and d_hok.all().item()
          and torch.equal(d_hpt, want_hpt))
    if not ok:
        raise SystemExit("bench_seal: a sealed report does not open to its row")

    def summary(ms):
        med = float(np.median(ms))
        return {"ms": [round(x, 3) for x in ms], "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
                "reports_per_s_median": round(n / med * 1e3, 1)}

    how = f"device events around the call, the median of {a.runs} runs after {a.warmups} warm-ups"
    res = {"tool": "tools/bench_seal.py", "vdaf": v.name(), "n": n, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "suite": "DHKEM(X25519, HKDF-SHA256), HKDF-SHA256, AES-128-GCM", "all_distinct_ephemeral_keys": True,
           "leader_ciphertext_bytes": lct, "helper_ciphertext_bytes": hct, "timing": how,
           "every_sealed_report_opens_to_its_row": bool(ok)}
    res["seal_reports_device"] = summary(timed(seal, s_eng, a.runs, a.warmups))
    res["leader_upload_open_device"] = summary(timed(open_leader, s_eng, a.runs, a.warmups))
    res["hpke_open_batch_device_helper"] = summary(timed(open_helper, s_hpke, a.runs, a.warmups))
    seal_ms = res["seal_reports_device"]["ms_median"]
    open_ms = res["leader_upload_open_device"]["ms_median"] + res["hpke_open_batch_device_helper"]["ms_median"]
    res["seal_over_open_of_the_same_bytes"] = round(seal_ms / open_ms, 3)
    res["seal_gb_per_s"] = round(n * (lct + hct) / seal_ms / 1e6, 1)
    if kernels is not None:
        res["kernels_one_call_each"] = kernels
        ctx_seal = kernels.get("client_seal_ctx_kernel", {}).get("total_ms")
        ctx_open = kernels.get("upload_ctx_kernel<false>", {}).get("total_ms")
        if ctx_seal and ctx_open:
            # the seal's context stage runs 4n ladders (two shares, two points each), the upload open's 2n (two trials)
            res["ctx_stage_seal_over_upload_open"] = round(ctx_seal / ctx_open, 3)

    # ---- the host sealer of the tools: the AEAD alone over the leader plaintexts, 16 threads
    from bench_upload import seal_lib

    k = min(a.host_n, n)
    US = seal_lib()
    pts = np.zeros((k, lct - 16), np.uint8)
    pts[:, 2:6] = np.frombuffer(lis.to_bytes(4, "big"), np.uint8)
    pts[:, 6:] = d_lis[:k].cpu().numpy()
    out = np.zeros((k, lct), np.uint8)
    key, nonce = rng.bytes(16) + bytes(16), rng.bytes(12)
    aad_h = [aads[i].tobytes() for i in range(k)]
    US.us_seal(1, key, nonce, aad_h[0], len(aad_h[0]), pts[0].ctypes.data, lct - 16, out[0].ctypes.data)  # loads, warms
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(lambda i: US.us_seal(1, key, nonce, aad_h[i], len(aad_h[i]), pts[i].ctypes.data, lct - 16,
                                           out[i].ctypes.data), range(k)))
    dt = time.perf_counter() - t0
    res["host_upload_seal_cpp"] = {"threads": THREADS, "reports": k, "seconds": round(dt, 3),
                                   "reports_per_s": round(k / dt, 1), "what": "AES-128-GCM of the leader share alone, no X25519"}
    res["device_over_host_sealer"] = round(res["seal_reports_device"]["reports_per_s_median"] / (k / dt), 1)
    for x in (eng, sl, sh, ol, oh):
        x.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
