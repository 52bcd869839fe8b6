"""Time the collection merge-and-seal on one GPU: 64 collection jobs of 32 shard records each on Prio3SumVec 8x1000/88
(a record is 16,040 bytes, a share 16,000), three ways over the same records:

  collect_seal_device   one jx_collect_seal_device call: everything in HBM (device events around the call)
  collect_seal_host     one jx_collect_seal call: records in, ciphertexts out through host memory
  per_job               what the code before this call would do: one jx_shard_record_combine_device per job, the merged
                        shares copied out, one HpkeSealer.seal_long_batch over them (host clock, ends synchronised)
  python_ints           one host thread merging the same records with Python integers (no seal)

Prints one JSON line: per way the median, the minimum and the maximum of `--steps` timed calls after `--warmup`
untimed ones, in milliseconds. The three GPU ways must give the same shares, and the first two the same ciphertexts as
the third: checked before anything is timed.

    python tools/bench_collect.py [--steps 20] [--warmup 3] [--out profiles/collect.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NJOBS, PER_JOB = 64, 32
P128 = 2**128 - 28 * 2**64 + 1


def summary(ms: list[float]) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "calls": len(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--python-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from janus_amd import hpke
    from janus_amd.engine import HelperEngine
    from janus_amd.vdaf import Prio3

    if not torch.cuda.is_available():
        raise SystemExit("bench_collect needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    v = Prio3.sum_vec(8, 1000, 88)
    pt = v.output_len * v.field_bytes
    rb = pt + 40
    nrec = NJOBS * PER_JOB
    rng = np.random.default_rng(2024)
    # canonical elements: the high word below P_HI is enough (p = P_HI * 2^64 + 1)
    rec = np.zeros((nrec, rb), np.uint8)
    words = rng.integers(0, 2**63, size=(nrec, 2 * v.output_len), dtype=np.uint64)
    rec[:, :pt] = words.view(np.uint8).reshape(nrec, pt)
    rec[:, pt:pt + 8] = rng.integers(1, 100, size=(nrec, 1), dtype=np.uint64).view(np.uint8)
    rec[:, pt + 8:] = rng.integers(0, 256, size=(nrec, 32), dtype=np.uint8)
    jobs = [list(range(j * PER_JOB, (j + 1) * PER_JOB)) for j in range(NJOBS)]
    aads = [bytes([j]) * 57 for j in range(NJOBS)]  # the length of a time-interval AggregateShareAad without a parameter
    sks = rng.integers(0, 256, size=(NJOBS, 32), dtype=np.uint8)
    pk = bytes(range(9, 41))  # any X25519 public key: nothing is opened here
    info = hpke.application_info(hpke.LABEL_AGGREGATE_SHARE, hpke.ROLE_HELPER, hpke.ROLE_COLLECTOR)

    d_rec, d_sk = torch.from_numpy(rec).to(dev), torch.from_numpy(sks).to(dev)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    d_st, d_cnt, d_cs, d_enc, d_ct, d_pt = u8(NJOBS), u8(NJOBS, 8), u8(NJOBS, 32), u8(NJOBS, 32), u8(NJOBS, pt + 16), u8(NJOBS, pt)
    d_merged = u8(NJOBS, rb)

    with HelperEngine(v, bytes(16)) as eng, hpke.HpkeSealer(pk, info) as sender:
        def device_form():
            eng.collect_seal_device(d_rec.data_ptr(), nrec, jobs, aads, d_sk.data_ptr(), sender, 1, 0, d_st.data_ptr(),
                                    d_cnt.data_ptr(), d_cs.data_ptr(), d_enc.data_ptr(), d_ct.data_ptr(), d_pt.data_ptr())

        def host_form():
            return eng.collect_seal(rec, jobs, aads, sks, sender, 1, 0, want_shares=True)

        def per_job():
            for j in range(NJOBS):
                eng.combine_records_device(d_rec.data_ptr() + j * PER_JOB * rb, PER_JOB, d_merged.data_ptr() + j * rb)
            merged = d_merged.cpu().numpy()
            shares = [merged[j, :pt].tobytes() for j in range(NJOBS)]
            return shares, sender.seal_long_batch([sks[j].tobytes() for j in range(NJOBS)], shares, aads)

        def python_ints():
            out = []
            for job in jobs:
                total = [0] * v.output_len
                for r in job:
                    row = rec[r, :pt].tobytes()
                    for i in range(v.output_len):
                        total[i] += int.from_bytes(row[16 * i:16 * i + 16], "little")
                out.append(b"".join((t % P128).to_bytes(16, "little") for t in total))
            return out

        # the same results every way, before anything is timed
        device_form()
        torch.cuda.synchronize()
        host = host_form()
        shares, sealed = per_job()
        assert not d_st.cpu().numpy().any() and not host.status.any()
        assert [host.shares[j].tobytes() for j in range(NJOBS)] == shares == [bytes(r) for r in d_pt.cpu().numpy()]
        assert [(host.encs[j].tobytes(), host.cts[j].tobytes()) for j in range(NJOBS)] == sealed
        assert np.array_equal(d_ct.cpu().numpy(), host.cts) and np.array_equal(d_enc.cpu().numpy(), host.encs)
        py = python_ints()
        assert py == shares

        res = {}
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for _ in range(args.warmup):
            device_form()
        torch.cuda.synchronize()
        wall = []
        for e0, e1 in ev:
            t = time.perf_counter()
            e0.record()
            device_form()
            e1.record()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t))
        res["collect_seal_device"] = {"device_events": summary([e0.elapsed_time(e1) for e0, e1 in ev]),
                                      "host_clock_synchronised": summary(wall)}
        for name, fn, steps, warm in (("collect_seal_host", host_form, args.steps, args.warmup),
                                      ("per_job", per_job, args.steps, args.warmup),
                                      ("python_ints", python_ints, args.python_steps, 0)):
            for _ in range(warm):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(steps):
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t))
            res[name] = {"host_clock_synchronised": summary(ms)}

    doc = {"bench": "collect", "vdaf": v.name(), "jobs": NJOBS, "records_per_job": PER_JOB, "record_bytes": rb,
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "results": res,
           "note": "per_job = one jx_shard_record_combine_device per job + a device-to-host copy + one "
                   "HpkeSealer.seal_long_batch; python_ints merges only (no seal), one host thread"}
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
