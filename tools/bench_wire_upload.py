#!/usr/bin/env python3
"""Time the upload message on the GPU (jx_report_encode_device, jx_upload_decode_device) next to the upload open on the
same reports and next to the host work it replaces.

Workload: n (default 16,384) Prio3SumVec 8 x 1000 / 88 reports, sharded and sealed by the engine's own client calls on
the device; a Report body is about 135 KB, of which 132 KB are the leader's ciphertext.

  check     before any timing, on a 512-report prefix: the encoded bodies equal janus_amd.messages' encoding byte for
            byte, and the decoded arrays equal what messages.py extracts (tests/test_wire_upload_host.expected_decode);
            the tool fails otherwise
  encode    jx_report_encode_device, device events on the engine stream around the call and the host clock, the
            median of five runs after two warm-ups
  decode    jx_upload_decode_device, the same way
  open      jx_leader_upload_open_device over the decoded handle's arrays, the same way
  parts     the encode and the decode again with 1, 2, 4 and 8 waves per report forced (debug option 12), and on a
            512-report prefix automatic against one wave per report: is one wave per report enough?
  host      tools/upload_split.cpp: one thread doing the decode's split of the same bodies
  object    aggregator.handle_upload (Report.decode per report, the Python loop, the joins, one upload open) on a
            prefix small enough to finish, by the host clock

No threshold: the ratios are written down as found.

  python tools/bench_wire_upload.py --out profiles/wire_upload.json
"""
from __future__ import annotations

import argparse
import ctypes
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


def split_exe() -> str:
    src = os.path.join(ROOT, "tools", "upload_split.cpp")
    exe = os.path.join(ROOT, "tools", "bin", "upload_split")
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
    ap.add_argument("--object-n", type=int, default=256, help="reports of the object path's prefix")
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host split")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n

    import torch

    import test_wire_upload_host as U
    from janus_amd import hpke
    from janus_amd._lib import check
    from janus_amd.aggregator import UploadTask, handle_upload
    from janus_amd.engine import KEY_NONE, HelperEngine
    from janus_amd.messages import HpkeCiphertext, Report, ReportMetadata
    from janus_amd.vdaf import Prio3
    from oracle import hpke_oracle as H

    if not torch.cuda.is_available():
        raise SystemExit("bench_wire_upload needs a GPU (there is no CPU path)")
    v = Prio3.sum_vec(8, 1000, 88)
    vk, task = bytes(range(16)), bytes(range(32, 64))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0x5EED)
    t0 = time.perf_counter()
    meas = rng.integers(0, 1 << v.bits, size=(n, v.length), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8)
    eph = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    now = 1_700_000_000 + n
    times = np.arange(n, dtype=np.uint64) + np.uint64(1_700_000_000)
    skl, skh = rng.bytes(32), rng.bytes(32)
    pkl, pkh = H.x25519_base(skl), H.x25519_base(skh)
    info_l, info_h = H.dap_info(recipient=hpke.ROLE_LEADER), H.dap_info(recipient=hpke.ROLE_HELPER)
    PS, LIS, HIS = v.public_share_len, v.leader_input_share_len, v.helper_input_share_len
    result = {"tool": "tools/bench_wire_upload.py", "vdaf": v.name(), "n": n, "device": torch.cuda.get_device_name(0),
              "timing": f"device events on the engine stream around the call and the host clock, medians of {a.runs} runs "
                        f"after {a.warmups} warm-ups"}

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

    u64p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    with hpke.HpkeSealer(pkl, info_l) as sl, hpke.HpkeSealer(pkh, info_h) as sh, hpke.HpkeOpener(skl, pkl, info_l) as ol, \
            HelperEngine(v, vk) as eng:
        L = eng._L
        stride = (LIS + 15) // 16 * 16
        lct, hct = eng.client_seal_sizes()
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to(dev)  # noqa: E731
        z = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)  # noqa: E731
        d_meas, d_ids, d_rd, d_eph = torch.from_numpy(meas.view(np.int64)).to(dev), up(nonces), up(rands), up(eph)
        d_ps, d_lis, d_his, d_st = z(n * PS), z(n * stride), z(n * HIS), z(n)
        d_le, d_lc, d_he, d_hc, d_seal = z(n * 32), z(n * lct), z(n * 32), z(n * hct), z(n)
        eng.shard_device(n, d_meas.data_ptr(), d_ids.data_ptr(), d_rd.data_ptr(), d_ps.data_ptr(), d_lis.data_ptr(),
                         d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)
        eng.seal_reports_device(n, d_ids.data_ptr(), times, d_ps.data_ptr(), d_lis.data_ptr(), d_his.data_ptr(), task, sl, sh,
                                d_eph.data_ptr(), d_le.data_ptr(), d_lc.data_ptr(), d_he.data_ptr(), d_hc.data_ptr(),
                                d_seal.data_ptr(), d_shard_status=d_st.data_ptr(), lis_stride=stride)
        assert not d_seal.cpu().numpy().any()
        del d_meas, d_rd, d_lis, d_his
        print(f"{n} reports sharded and sealed in {time.perf_counter() - t0:.1f} s", flush=True)
        s_eng = torch.cuda.ExternalStream(eng.stream())
        total = eng.report_bound(n)
        d_body = z(total)
        key_first, key_second = np.full(256, KEY_NONE, np.uint8), np.full(256, KEY_NONE, np.uint8)
        key_first[5] = 0

        def encode(count=n):
            return eng.encode_reports(count, d_ids.data_ptr(), times[:count], d_ps.data_ptr(), d_le.data_ptr(), d_lc.data_ptr(),
                                      d_he.data_ptr(), d_hc.data_ptr(), 5, 6, d_seal_status=d_seal.data_ptr(),
                                      d_out=d_body.data_ptr(), capacity=total, stream=False)

        held = []

        def decode(count=n, offs=None):
            held.append(eng.decode_uploads(d_body, offs, now, key_first, key_second, length=int(offs[count]), stream=False))
            while len(held) > 1:
                held.pop(0).release()

        # ---- check: a 512-report prefix against the Python codec
        k = min(512, n)
        host = lambda t, w: t[:k * w].cpu().numpy().reshape(k, w)  # noqa: E731
        ids_h, ps_h, le_h, lc_h, he_h, hc_h = host(d_ids, 16), host(d_ps, PS), host(d_le, 32), host(d_lc, lct), host(d_he, 32), host(d_hc, hct)
        reports = [Report(ReportMetadata(ids_h[i].tobytes(), int(times[i])), ps_h[i].tobytes(),
                          HpkeCiphertext(5, le_h[i].tobytes(), lc_h[i].tobytes()),
                          HpkeCiphertext(6, he_h[i].tobytes(), hc_h[i].tobytes())) for i in range(k)]
        enc = [r.encode() for r in reports]
        bodies, offs_k = encode(k)
        eng.sync()
        if bodies.cpu().numpy().tobytes() != b"".join(enc) or offs_k.tolist() != np.concatenate([[0], np.cumsum([len(x) for x in enc])]).tolist():
            raise SystemExit("bench_wire_upload: the encoded bodies differ from the Python codec's")
        decode(k, offs_k)
        req = held[-1]
        want = U.expected_decode(enc, PS, now, 0, None, None, bytes(key_first), bytes(key_second))
        db = lambda name: req.device_bytes(name).cpu().numpy().tobytes()  # noqa: E731
        got = dict(status=req.status, row_of=req.row_of, ids_all=req.report_ids, times_all=req.all_times, m=req.m, index=req.index,
                   ids=db("report_ids"), times=req.times, ps=db("public_shares"), key_index=req.key_index.tobytes(),
                   config_ids=req.helper_config_ids.tobytes(),
                   offs=[req.leader_enc_offsets, req.leader_payload_offsets, req.helper_enc_offsets, req.helper_payload_offsets],
                   packed=[db("leader_encs"), db("leader_payloads"), db("helper_encs"), db("helper_payloads")])
        U.assert_decode_equal(got, want)  # raises when anything differs
        result["check"] = {"prefix": k, "bodies_equal_python_codec": True, "arrays_equal_python_codec": True}
        print("check: " + json.dumps(result["check"]), flush=True)

        # ---- the object path on a small prefix, by the host clock
        ko = min(a.object_n, k)
        t = time.perf_counter()
        up_obj = handle_upload(eng, UploadTask(task, {5: ol}), enc[:ko], now)
        obj_ms = (time.perf_counter() - t) * 1e3
        assert not up_obj.status
        result["object_path_handle_upload"] = {"n": ko, "host_clock_ms": round(obj_ms, 3), "ms_per_report": round(obj_ms / ko, 4)}
        del up_obj

        # ---- timings
        _, offs = encode()
        eng.sync()
        assert int(offs[-1]) == total
        result["body_bytes"] = total
        result["encode_device"] = timed(encode, s_eng)
        result["decode_device"] = timed(lambda: decode(n, offs), s_eng)
        req = held[-1]
        assert req.m == n
        m, A = req.m, req.d
        d_rows, d_ext = z(m * stride), z(req.leader_payload_bytes)
        d_len, d_ost = torch.zeros(m, dtype=torch.int32, device=dev), z(m)
        task_b = np.frombuffer(task, np.uint8).copy()
        hs = (vp * 1)(ol.handle)
        kidx = np.ascontiguousarray(req.key_index)

        def open_leader():
            check(L.jx_leader_upload_open_device(eng.handle, m, A.d_report_ids, req.times.ctypes.data_as(u64p), A.d_public_shares,
                                                 task_b.ctypes.data_as(vp), hs, 1, kidx.ctypes.data_as(vp), A.d_leader_encs,
                                                 req.leader_enc_offsets.ctypes.data_as(u64p), A.d_leader_payloads,
                                                 req.leader_payload_offsets.ctypes.data_as(u64p), d_rows.data_ptr(), stride,
                                                 d_ext.data_ptr(), d_len.data_ptr(), d_ost.data_ptr()), eng.handle, "open")

        result["leader_upload_open_device"] = timed(open_leader, s_eng)
        eng.sync()
        assert not d_ost.cpu().numpy().any()
        del d_rows, d_ext

        # ---- one wave per report, or several?
        sweep = {}
        for parts in (1, 2, 4, 8):
            eng.debug(12, parts)
            sweep[str(parts)] = {"encode_device_ms": timed(encode, s_eng)["device_ms_median"],
                                 "decode_device_ms": timed(lambda: decode(n, offs), s_eng)["device_ms_median"]}
        small = {}
        for label, parts in (("automatic", 0), ("one_wave", 1)):
            eng.debug(12, parts)
            small[label] = {"encode_device_ms": timed(lambda: encode(k), s_eng)["device_ms_median"],
                            "decode_device_ms": timed(lambda: decode(k, offs_k), s_eng)["device_ms_median"]}
        eng.debug(12, 0)
        result["waves_per_report"] = {f"n_{n}": sweep, f"n_{k}": small}
        encode()
        eng.sync()
        while held:
            held.pop().release()

        # ---- one host thread doing the decode's split
        if not a.no_host:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "bodies.bin")
                with open(path, "wb") as fh:
                    d_body.cpu().numpy().tofile(fh)
                with open(path + ".off", "wb") as fh:
                    fh.write(offs.astype("<u8").tobytes())
                out = subprocess.run([split_exe(), path, path + ".off", str(PS), str(now), str(a.runs), str(a.warmups)], check=True,
                                     capture_output=True, text=True, timeout=900)
            result["host_upload_split_cpp"] = json.loads(out.stdout)
            assert result["host_upload_split_cpp"]["accepted"] == n

    enc_ms, dec_ms = result["encode_device"]["host_clock_ms_median"], result["decode_device"]["host_clock_ms_median"]
    open_ms = result["leader_upload_open_device"]["host_clock_ms_median"]
    result["encode_gb_per_s"] = round(total / enc_ms / 1e6, 2)
    result["decode_gb_per_s"] = round(total / dec_ms / 1e6, 2)
    result["encode_kernels_gb_per_s"] = round(total / result["encode_device"]["device_ms_median"] / 1e6, 2)
    result["decode_kernels_gb_per_s"] = round(total / result["decode_device"]["device_ms_median"] / 1e6, 2)
    result["encode_over_upload_open"] = round(enc_ms / open_ms, 4)
    result["decode_over_upload_open"] = round(dec_ms / open_ms, 4)
    if "host_upload_split_cpp" in result:
        result["host_split_over_device_decode"] = round(result["host_upload_split_cpp"]["ms_median"] / dec_ms, 2)
    result["object_path_ms_per_report_over_device_decode"] = round(result["object_path_handle_upload"]["ms_per_report"] / (dec_ms / n), 1)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
