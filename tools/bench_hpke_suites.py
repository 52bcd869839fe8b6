#!/usr/bin/env python3
"""Cost of the batched HPKE open under each of the nine X25519 suites on one MI355X (janus_amd/csrc/jx_hpke.hip:
hpke_open_kernel for the default suite, hpke_open_suite_kernel for the rest).

For each suite a pool of DAP-sized report shares (248-byte payload, 92-byte InputShareAad) is sealed by
tests/hpke_suites_ref.py and tiled on the device to n ciphertexts. One process opens n = 1,024 and n = 65,536 with
jx_hpke_open_batch_device (inputs resident in HBM), timed by HIP events on the context's stream. The suites are
interleaved (every repetition visits all nine in turn), so that clock drift falls on all of them; the figure per
suite is the median over the repetitions, and the ratio is to the default suite of the same run.

    python tools/bench_hpke_suites.py [--reps 7] [--pool 64] [--out profiles/hpke_suites.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1024, 65536)
KDF = {1: "HKDF-SHA256", 2: "HKDF-SHA384", 3: "HKDF-SHA512"}
AEAD = {1: "AES-128-GCM", 2: "AES-256-GCM", 3: "ChaCha20Poly1305"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

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
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    info = hpke.application_info()
    task = rnd.randbytes(32)
    dev = torch.device("cuda", 0)
    nmax = max(SIZES)
    suites = {}
    for kdf, aead in S.SUITES:
        encs, cts, aads, pts = [], [], [], []
        for i in range(a.pool):
            aad = hpke.input_share_aad(task, rnd.randbytes(16), 1_700_000_000 + i, rnd.randbytes(32))
            pt = (0).to_bytes(2, "big") + (242).to_bytes(4, "big") + rnd.randbytes(242)  # 248 bytes
            enc, ct = S.seal_base(kdf, aead, pk, info, aad, pt, rnd.randbytes(32))
            encs.append(enc)
            cts.append(ct)
            aads.append(aad)
            pts.append(pt)
        reps = -(-nmax // a.pool)
        tile = lambda xs: torch.from_numpy(np.frombuffer(b"".join(xs), np.uint8).copy()).to(dev).repeat(reps)[  # noqa: E731
            : nmax * len(xs[0])].contiguous()
        cl, al = len(cts[0]), len(aads[0])
        assert (cl, al) == (248 + 16, 92)
        suites[(kdf, aead)] = {
            "op": hpke.HpkeOpener(sk, pk, info, kdf_id=kdf, aead_id=aead), "enc": tile(encs), "ct": tile(cts),
            "aad": tile(aads), "pts": b"".join(pts), "ms": {n: [] for n in SIZES}}
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
        for rep in range(a.reps + 1):  # repetition 0 warms up (and is verified), the rest are kept
            for key, s in suites.items():
                ms = run(s, n)
                if rep == 0:
                    good = bool(d_ok[:n].all().item()) and d_pt[: a.pool * (cl - 16)].cpu().numpy().tobytes() == s["pts"]
                    verified = verified and good
                else:
                    s["ms"][n].append(ms)
    rows = []
    base = {n: statistics.median(suites[(1, 1)]["ms"][n]) for n in SIZES}
    for (kdf, aead), s in suites.items():
        row = {"kdf_id": kdf, "aead_id": aead, "suite": f"{KDF[kdf]} / {AEAD[aead]}"}
        for n in SIZES:
            med = statistics.median(s["ms"][n])
            row[f"ms_{n}"] = round(med, 4)
            row[f"min_ms_{n}"] = round(min(s["ms"][n]), 4)
            row[f"ratio_{n}"] = round(med / base[n], 3)
        rows.append(row)
        s["op"].close()
    out = {"metric": "HPKE open_batch_device, ms per batch (median of interleaved repetitions, HIP events)",
           "payload_bytes": 248, "aad_bytes": 92, "reps": a.reps, "sizes": list(SIZES), "verified": verified,
           "device": torch.cuda.get_device_name(0), "suites": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
