#!/usr/bin/env python3
"""Cost of the batched HPKE open under DHKEM(P-256, HKDF-SHA256) on one MI355X (janus_amd/csrc/jx_hpke_p256.hip:
hpke_open_p256_kernel) against the X25519 default suite (hpke_open_kernel), and the run-to-run spread of the
X25519 default suite on another build of the library (the parent commit's), which is what the unchanged path has
to stay within.

As tools/bench_hpke_suites.py: a pool of DAP-sized report shares (248-byte payload, 92-byte InputShareAad) sealed
by the Python references and tiled on the device; n = 1,024 and n = 65,536 opened with jx_hpke_open_batch_device
(inputs resident in HBM), timed by HIP events on the context's stream; the contexts are interleaved within every
repetition and the figure is the median.

    python tools/bench_hpke_p256.py [--reps 7] [--pool 64] [--parent-root DIR] [--out profiles/hpke_p256.json]

--parent-root: a checkout of the parent commit with its library built. The X25519 default suite is measured there
three times, each in a fresh child process (--x25519-only --root DIR), before this process touches the GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 65536)
KDF = {1: "HKDF-SHA256", 2: "HKDF-SHA384", 3: "HKDF-SHA512"}
AEAD = {1: "AES-128-GCM", 2: "AES-256-GCM", 3: "ChaCha20Poly1305"}
P256, X25519 = 0x0010, 0x0020


def measure(root: str, x25519_only: bool, reps: int, pool: int) -> dict:
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))  # the references (this checkout's, whatever library is measured)
    import numpy as np
    import torch

    import hpke_p256_ref as R
    import hpke_suites_ref as S
    from janus_amd import hpke
    from oracle import hpke_oracle as H

    hpke._declare(hpke._lib.load())
    # the HIP runtime this process already holds (the engine library's and torch's), not a second copy
    loaded = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
    vp = ctypes.c_void_p
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]

    def chk(st):
        if st != 0:
            raise RuntimeError(f"HIP error {st}")

    ev0, ev1 = vp(), vp()
    chk(hip.hipEventCreate(ctypes.byref(ev0)))
    chk(hip.hipEventCreate(ctypes.byref(ev1)))

    rnd = random.Random(1)
    info = hpke.application_info()
    task = rnd.randbytes(32)
    dev = torch.device("cuda", 0)
    nmax = max(SIZES)
    xsk = rnd.randbytes(32)
    xpk = H.x25519_base(xsk)
    psk = rnd.randrange(1, R.N).to_bytes(32, "big")
    ppk = R.public_key(psk)
    todo = [(X25519, 1, 1)] if x25519_only else [(X25519, 1, 1), (P256, 1, 1), (P256, 3, 3)]
    ctxs = {}
    cl, al = 248 + 16, 92
    for kem, kdf, aead in todo:
        encs, cts, aads, pts = [], [], [], []
        for i in range(pool):
            aad = hpke.input_share_aad(task, rnd.randbytes(16), 1_700_000_000 + i, rnd.randbytes(32))
            pt = (0).to_bytes(2, "big") + (242).to_bytes(4, "big") + rnd.randbytes(242)  # 248 bytes
            if kem == P256:
                enc, ct = R.seal_base(kdf, aead, ppk, info, aad, pt, rnd.randrange(1, R.N).to_bytes(32, "big"))
            else:
                enc, ct = S.seal_base(kdf, aead, xpk, info, aad, pt, rnd.randbytes(32))
            encs.append(enc)
            cts.append(ct)
            aads.append(aad)
            pts.append(pt)
        tiles = -(-nmax // pool)
        tile = lambda xs: torch.from_numpy(np.frombuffer(b"".join(xs), np.uint8).copy()).to(dev).repeat(tiles)[  # noqa: E731
            : nmax * len(xs[0])].contiguous()
        assert (len(cts[0]), len(aads[0])) == (cl, al)
        if kem == P256:
            op = hpke.HpkeOpener(psk, ppk, info, kem_id=kem, kdf_id=kdf, aead_id=aead)
        else:
            op = hpke.HpkeOpener(xsk, xpk, info, kdf_id=kdf, aead_id=aead)
        ctxs[(kem, kdf, aead)] = {"op": op, "enc": tile(encs), "ct": tile(cts), "aad": tile(aads), "pts": b"".join(pts),
                                  "ms": {n: [] for n in SIZES}}
    d_co = torch.arange(nmax + 1, dtype=torch.int64, device=dev) * cl
    d_ao = torch.arange(nmax + 1, dtype=torch.int64, device=dev) * al
    d_pt = torch.empty(nmax * (cl - 16), dtype=torch.uint8, device=dev)
    d_ok = torch.empty(nmax, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run(s, n) -> float:
        op = s["op"]
        stream = op.stream
        chk(hip.hipEventRecord(ev0, stream))
        st = op._L.jx_hpke_open_batch_device(op.handle, n, s["enc"].data_ptr(), s["ct"].data_ptr(), d_co.data_ptr(),
                                             s["aad"].data_ptr(), d_ao.data_ptr(), d_pt.data_ptr(), d_ok.data_ptr())
        assert st == 0, st
        chk(hip.hipEventRecord(ev1, stream))
        chk(hip.hipEventSynchronize(ev1))
        ms = ctypes.c_float()
        chk(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1))
        return ms.value

    verified = True
    for n in SIZES:
        for rep in range(reps + 1):  # repetition 0 warms up (and is verified), the rest are kept
            for s in ctxs.values():
                ms = run(s, n)
                if rep == 0:
                    good = bool(d_ok[:n].all().item()) and d_pt[: pool * (cl - 16)].cpu().numpy().tobytes() == s["pts"]
                    verified = verified and good
                else:
                    s["ms"][n].append(ms)
    rows = []
    base = {n: statistics.median(ctxs[(X25519, 1, 1)]["ms"][n]) for n in SIZES}
    for (kem, kdf, aead), s in ctxs.items():
        row = {"kem_id": kem, "kdf_id": kdf, "aead_id": aead,
               "suite": f"{'P-256' if kem == P256 else 'X25519'} / {KDF[kdf]} / {AEAD[aead]}"}
        for n in SIZES:
            med = statistics.median(s["ms"][n])
            row[f"ms_{n}"] = round(med, 4)
            row[f"min_ms_{n}"] = round(min(s["ms"][n]), 4)
            row[f"ratio_{n}"] = round(med / base[n], 3)
        rows.append(row)
        s["op"].close()
    return {"verified": verified, "device": torch.cuda.get_device_name(0), "suites": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--x25519-only", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose janus_amd (and library) is measured")
    a = ap.parse_args()
    if a.x25519_only:
        print(json.dumps(measure(a.root, True, a.reps, a.pool)))
        return 0
    parent_runs = []
    if a.parent_root:
        for _ in range(3):  # fresh processes, one at a time, before this one opens the GPU
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--x25519-only", "--root", a.parent_root,
                                "--reps", str(a.reps), "--pool", str(a.pool)], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                return 1
            parent_runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = measure(a.root, False, a.reps, a.pool)
    out = {"metric": "HPKE open_batch_device, ms per batch (median of interleaved repetitions, HIP events)",
           "payload_bytes": 248, "aad_bytes": 92, "reps": a.reps, "sizes": list(SIZES), "verified": res["verified"],
           "device": res["device"], "suites": res["suites"]}
    if parent_runs:
        xs = [r["suites"][0] for r in parent_runs]
        out["parent_x25519_default"] = {
            "verified": all(r["verified"] for r in parent_runs),
            **{f"ms_{n}": [x[f"ms_{n}"] for x in xs] for n in SIZES},
            **{f"spread_{n}": round(max(x[f"ms_{n}"] for x in xs) / min(x[f"ms_{n}"] for x in xs), 3) for n in SIZES}}
        now = res["suites"][0]
        out["x25519_default_now_over_parent_median"] = {
            str(n): round(now[f"ms_{n}"] / statistics.median(x[f"ms_{n}"] for x in xs), 3) for n in SIZES}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if res["verified"] and all(r["verified"] for r in parent_runs) else 1


if __name__ == "__main__":
    sys.exit(main())
