#!/usr/bin/env python3
"""Time Prio3.shard on the GPU (jx_client_shard_device) and close the loop on what it makes.

Workload: n (default 16,384) all-distinct Prio3SumVec 8 x 1000 / 88 reports: random measurements, nonces and client
randomness from a seed, resident in HBM.

  device call   reports/s of jx_client_shard_device by device events around the call, five runs after two warm-ups
  kernels       per-kernel times from one `rocprofv3 --kernel-trace --stats` run of this tool (--profile: a child
                process running --timed-only, started before this process touches the GPU)
  oracle        the C oracle's jo_shard on 16 threads of the same box, over --oracle-n of the same reports
  end to end    the same n reports through leader init -> helper prepare + aggregate -> leader finish -> leader
                accumulate; every verdict is checked, and Prio3.unshard of the two aggregate shares against the numpy
                column sums of the measurements; the first --oracle-n reports' rows against the oracle byte for byte

  python tools/bench_shard.py --profile --out profiles/shard.json
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BITS, LENGTH, CHUNK = 8, 1000, 88
THREADS = 16


def inputs(n: int, seed: int):
    rng = np.random.default_rng(seed)
    meas = rng.integers(0, 1 << BITS, size=(n, LENGTH), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    return meas, nonces, rands


def kernel_stats(n: int, seed: int) -> dict:
    """One traced run of the timed part in a child process; per shard kernel: calls, total and mean time."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "shard", "--",
               sys.executable, os.path.abspath(__file__), "--timed-only", "--n", str(n), "--seed", str(seed),
               "--runs", "1", "--warmups", "0"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel stats")
        out = {}
        with open(files[0], newline="") as fh:
            for r in csv.DictReader(fh):
                if "shard_" in r["Name"]:
                    name = r["Name"].split("(")[0].split("::")[-1]
                    out[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                 "mean_ms": float(r["AverageNs"]) / 1e6}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--oracle-n", type=int, default=512)
    ap.add_argument("--timed-only", action="store_true", help="the device calls alone (what --profile traces)")
    ap.add_argument("--profile", action="store_true", help="add per-kernel times from a traced child run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n

    kernels = None
    if a.profile:  # before this process opens the GPU
        kernels = kernel_stats(n, a.seed)

    import torch

    from janus_amd.engine import HelperEngine
    from janus_amd.vdaf import Prio3

    if not torch.cuda.is_available():
        raise SystemExit("bench_shard needs a GPU (there is no CPU path)")
    v = Prio3.sum_vec(BITS, LENGTH, CHUNK)
    vk = bytes(range(16))
    meas, nonces, rands = inputs(n, a.seed)
    dev = torch.device("cuda", 0)
    lis_len = v.leader_input_share_len
    stride = (lis_len + 127) // 128 * 128
    d_m = torch.from_numpy(meas.view(np.int64)).to(dev)
    d_n, d_r = torch.from_numpy(nonces).to(dev), torch.from_numpy(rands).to(dev)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    d_ps, d_lis, d_his, d_st = u8(n, v.public_share_len), u8(n, stride), u8(n, v.helper_input_share_len), u8(n)
    leader, helper = HelperEngine(v, vk), HelperEngine(v, vk)

    def shard():
        leader.shard_device(n, d_m.data_ptr(), d_n.data_ptr(), d_r.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(),
                            d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)

    for _ in range(a.warmups):
        shard()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        shard()  # ordered behind e0 and ahead of e1 through torch's current stream
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    if a.timed_only:
        leader.close()
        helper.close()
        print(json.dumps({"n": n, "ms": ms}))
        return
    best = min(ms)
    res = {"tool": "tools/bench_shard.py", "vdaf": v.name(), "n": n, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "leader_input_share_bytes": lis_len, "lis_stride": stride,
           "device_call": {"ms": [round(x, 3) for x in ms], "ms_min": round(best, 3),
                           "ms_median": round(float(np.median(ms)), 3),
                           "reports_per_s_best": round(n / best * 1e3, 1),
                           "reports_per_s_median": round(n / float(np.median(ms)) * 1e3, 1),
                           "timing": f"device events around the call, {a.runs} runs after {a.warmups} warm-ups"}}
    if kernels is not None:
        res["kernels_one_call"] = kernels

    # ---- the loop closed on the same reports
    d_lps, d_msgs = u8(n, v.prep_share_len), u8(n, v.prep_msg_len)
    d_lver, d_hver, d_fver = u8(n), u8(n), u8(n)
    t0 = time.perf_counter()
    bid = leader.leader_init_device(n, d_n.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(), d_lps.data_ptr(),
                                    d_lver.data_ptr(), lis_stride=stride)
    helper.prep_and_aggregate_device(d_n.data_ptr(), d_ps.data_ptr(), d_his.data_ptr(), d_lps.data_ptr(), n,
                                     d_out_prep_msgs=d_msgs.data_ptr(), d_out_verdicts=d_hver.data_ptr())
    leader.leader_finish_device(bid, n, d_msgs.data_ptr(), d_hver.data_ptr(), d_fver.data_ptr())
    leader.accumulate_device(bid, n)
    st, lver, hver, fver = (t.cpu().numpy() for t in (d_st, d_lver, d_hver, d_fver))
    agg_l, cnt_l, cs_l = leader.aggregate_share(0)
    agg_h, cnt_h, cs_h = helper.aggregate_share(0)
    e2e_s = time.perf_counter() - t0
    sums = [int(x) for x in meas.sum(axis=0, dtype=np.uint64)]
    ok = (not st.any() and not lver.any() and not hver.any() and not fver.any() and cnt_l == cnt_h == n and cs_l == cs_h
          and v.unshard([agg_l, agg_h], n) == sums)
    res["end_to_end"] = {"reports": n, "all_verdicts_finished": bool(not (lver.any() or hver.any() or fver.any())),
                         "shard_status_nonzero": int(np.count_nonzero(st)), "report_counts": [cnt_l, cnt_h],
                         "unshard_equals_column_sums": bool(v.unshard([agg_l, agg_h], n) == sums),
                         "prepare_and_aggregate_wall_s": round(e2e_s, 3), "ok": bool(ok)}

    # ---- the oracle: the same reports, 16 threads (ctypes releases the GIL inside jo_shard)
    from oracle import oracle as O

    k = min(a.oracle_n, n)
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length)
    orc.shard(meas[0], nonces[0].tobytes(), rands[0].tobytes())  # loads the library
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        rows = list(pool.map(lambda i: orc.shard(meas[i], nonces[i].tobytes(), rands[i].tobytes()), range(k)))
    dt = time.perf_counter() - t0
    got = [t[:k].cpu().numpy() for t in (d_ps, d_lis, d_his)]
    same = all(rows[i][0] == got[0][i].tobytes() and rows[i][1] == got[1][i, :lis_len].tobytes()
               and rows[i][2] == got[2][i].tobytes() for i in range(k))
    res["oracle_jo_shard"] = {"threads": THREADS, "reports": k, "seconds": round(dt, 3),
                              "reports_per_s": round(k / dt, 1), "device_rows_equal_oracle": bool(same)}
    res["device_over_oracle"] = round(res["device_call"]["reports_per_s_median"] / (k / dt), 1)
    leader.close()
    helper.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    if not (ok and same):
        raise SystemExit("bench_shard: the end-to-end check or the oracle comparison failed")


if __name__ == "__main__":
    main()
