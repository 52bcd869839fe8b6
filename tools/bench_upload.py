#!/usr/bin/env python3
"""Time the leader's upload path on the GPU: jx_leader_upload_open_device (HPKE open one wave per report, decode,
range check, row layout) against jx_hpke_open_batch_device (one report per lane: the only way to open these shares
before) on the same device buffers, with HIP events.

Workload: n (default 1,024) Prio3SumVec 8 x 1000 / 88 leader input shares (134,912 bytes each; 134,934 with the
PlaintextInputShare framing and the tag) under DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM, packed back to
back. The shares are random bytes (every 16 bytes an element < p with probability 1 - 2^-59): what is timed does not
depend on their values. They are sealed on the host by the kernels' own AES / GHASH code (tools/upload_seal.cpp);
the key schedules come from the Python references. Five alternating pairs after two warm-ups; AES-256-GCM and
ChaCha20Poly1305 are timed for the record (one warm-up, three runs each).

  python tools/bench_upload.py --probe-old      # one old call alone: run it first, under its own time limit
  python tools/bench_upload.py --out profiles/upload_open.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0


def seal_lib():
    src = os.path.join(ROOT, "tools", "upload_seal.cpp")
    so = os.path.join(ROOT, "tools", "bin", "libupload_seal.so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.us_seal.argtypes = [ctypes.c_uint32, vp, vp, vp, u64, vp, u64, vp]
    L.us_seal.restype = None
    return L


def make_inputs(n: int, aead: int, lis: int, ps_len: int, seed: int = 1):
    """n sealed leader shares under one recipient key: (sk, pk, ids, times, ps, encs, cts (n x ct_len), aads)."""
    import hpke_suites_ref as S
    from janus_amd import hpke
    from oracle import hpke_oracle as H

    rng = np.random.default_rng(seed)
    info = H.dap_info(recipient=hpke.ROLE_LEADER)
    sk = rng.bytes(32)
    pk = H.x25519_base(sk)
    task = rng.bytes(32)
    # 16 ephemeral keys, reused round-robin (an X25519 in Python takes milliseconds; the device decapsulates every report)
    ctxs = []
    for _ in range(16):
        ss, enc = H.encap(rng.bytes(32), pk)
        ctxs.append((enc,) + S.key_schedule(1, aead, ss, info))
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ps = rng.integers(0, 256, (n, ps_len), dtype=np.uint8)
    times = np.arange(n, dtype=np.uint64) + 1_700_000_000
    pt_len = 2 + 4 + lis
    pts = rng.integers(0, 256, (n, pt_len), dtype=np.uint8)
    pts[:, :2] = 0
    pts[:, 2:6] = np.frombuffer(lis.to_bytes(4, "big"), np.uint8)
    cts = np.zeros((n, pt_len + 16), np.uint8)
    aads = [hpke.input_share_aad(task, ids[i].tobytes(), int(times[i]), ps[i].tobytes()) for i in range(n)]
    L = seal_lib()

    def seal(i):
        enc, key, nonce = ctxs[i % 16]
        L.us_seal(aead, key, nonce, aads[i], len(aads[i]), pts[i].ctypes.data, pt_len, cts[i].ctypes.data)

    with ThreadPoolExecutor(16) as pool:
        list(pool.map(seal, range(n)))
    # the sealing code is the kernels' own: pin one report against the Python reference
    enc, key, nonce = ctxs[0]
    want = S.aead_seal(aead, key, nonce, aads[0], pts[0, :600].tobytes())
    got = np.zeros(616, np.uint8)
    L.us_seal(aead, key, nonce, aads[0], len(aads[0]), pts[0].ctypes.data, 600, got.ctypes.data)
    assert got.tobytes() == want, "host sealing disagrees with the Python reference"
    encs = np.frombuffer(b"".join(ctxs[i % 16][0] for i in range(n)), np.uint8).reshape(n, 32).copy()
    return sk, pk, info, task, ids, times, ps, encs, cts, aads, pts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--probe-old", action="store_true", help="one old call alone, then exit")
    ap.add_argument("--skip-old", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from janus_amd import hpke
    from janus_amd.engine import HelperEngine
    from janus_amd.vdaf import Prio3

    v = Prio3.sum_vec(8, 1000, 88)
    lis, n = v.leader_input_share_len, a.n
    dev = torch.device("cuda", 0)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    result = {"workload": f"{n} x {v.name()} leader input shares ({lis} bytes)", "n": n}

    def run_suite(aead: int, with_old: bool, pairs: int, warmup: int):
        t0 = time.time()
        sk, pk, info, task, ids, times, ps, encs, cts, aads, pts = make_inputs(n, aead, lis, v.public_share_len)
        ct_len = cts.shape[1]
        print(f"aead {aead}: sealed {n} x {ct_len} bytes in {time.time() - t0:.1f} s", flush=True)
        off = (np.arange(n + 1, dtype=np.uint64) * ct_len)
        aoff = np.zeros(n + 1, np.uint64)
        aoff[1:] = np.cumsum([len(x) for x in aads])
        d = {k: torch.from_numpy(x.reshape(-1)).to(dev) for k, x in
             dict(ids=ids, ps=ps, encs=encs, cts=cts, aads=np.frombuffer(b"".join(aads), np.uint8).copy()).items()}
        d_off, d_aoff = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(aoff.astype(np.int64)).to(dev)
        d_rows = torch.zeros(n * lis, dtype=torch.uint8, device=dev)
        d_ext = torch.zeros(n * ct_len, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        d_pt = torch.zeros(n * (ct_len - 16), dtype=torch.uint8, device=dev)
        d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        assert d_rows.data_ptr() % 16 == 0
        ki = np.zeros((n, 2), np.uint8)
        ki[:, 1] = 0xFF
        taskb = np.frombuffer(task, np.uint8).copy()
        torch.cuda.synchronize()
        with hpke.HpkeOpener(sk, pk, info, aead_id=aead) as op, HelperEngine(v, bytes(16)) as eng:
            hs = (ctypes.c_void_p * 1)(op.handle)
            L = eng._L
            es = ctypes.c_void_p()
            assert L.jx_engine_stream(eng.handle, ctypes.byref(es)) == 0
            s_new, s_old = torch.cuda.ExternalStream(es.value or 0), torch.cuda.ExternalStream(op.stream)

            def new_call():
                st = L.jx_leader_upload_open_device(
                    eng.handle, n, d["ids"].data_ptr(), times.ctypes.data_as(u64p), d["ps"].data_ptr(),
                    taskb.ctypes.data_as(ctypes.c_void_p), hs, 1, ki.ctypes.data_as(ctypes.c_void_p), d["encs"].data_ptr(),
                    None, d["cts"].data_ptr(), off.ctypes.data_as(u64p), d_rows.data_ptr(), 0, d_ext.data_ptr(),
                    d_len.data_ptr(), d_st.data_ptr())
                assert st == 0, L.jx_last_error(eng.handle)

            def old_call():
                st = op._L.jx_hpke_open_batch_device(op.handle, n, d["encs"].data_ptr(), d["cts"].data_ptr(), d_off.data_ptr(),
                                                     d["aads"].data_ptr(), d_aoff.data_ptr(), d_pt.data_ptr(), d_ok.data_ptr())
                assert st == 0, op._L.jx_hpke_last_error(op.handle)

            def timed(fn, stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            if a.probe_old:
                ms = timed(old_call, s_old)
                assert d_ok.cpu().numpy().all()
                print(json.dumps({"probe_old_ms": ms, "n": n}), flush=True)
                return None
            for _ in range(warmup):
                timed(new_call, s_new)
                if with_old:
                    timed(old_call, s_old)
            # both calls open every report, to the same bytes
            assert (d_st.cpu().numpy() == 0).all(), "the new call rejected a report"
            rows = d_rows.cpu().numpy().reshape(n, lis)
            assert rows.tobytes() == pts[:, 6:].tobytes(), "rows differ from the sealed shares"
            if with_old:
                assert d_ok.cpu().numpy().all()
                assert d_pt.cpu().numpy().tobytes() == pts.tobytes()
            new_ms, old_ms = [], []
            for _ in range(pairs):
                new_ms.append(timed(new_call, s_new))
                if with_old:
                    old_ms.append(timed(old_call, s_old))
            return new_ms, old_ms, n * ct_len

    if a.probe_old:
        run_suite(1, True, 0, 0)
        return 0
    new_ms, old_ms, ct_bytes = run_suite(1, not a.skip_old, a.pairs, a.warmup)
    best = min(new_ms)
    result["aes128gcm"] = {
        "new_ms": new_ms, "old_ms": old_ms, "ciphertext_bytes": ct_bytes,
        "new_gb_per_s": ct_bytes / best / 1e6, "fraction_of_hbm_peak": ct_bytes / best / 1e6 / HBM_PEAK_GBS,
    }
    if old_ms:
        result["aes128gcm"]["ratio_old_over_new"] = [o / x for o, x in zip(old_ms, new_ms)]
        result["aes128gcm"]["new_faster_in_all_pairs"] = all(x < o for o, x in zip(old_ms, new_ms))
    for name, aead in (("aes256gcm", 2), ("chacha20poly1305", 3)):
        ms, _, _ = run_suite(aead, False, 3, 1)
        result[name] = {"new_ms": ms, "new_gb_per_s": ct_bytes / min(ms) / 1e6}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if result["aes128gcm"].get("new_faster_in_all_pairs", True) else 1


if __name__ == "__main__":
    sys.exit(main())
