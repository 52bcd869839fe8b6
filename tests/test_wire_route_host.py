"""The batch-bucket rule of the aggregate-init route (janus_amd/csrc/jx_wire.h: wire_bucket_start, the claim / rank /
assign passes, wire_outcome_routed) on the CPU: tests/csrc/hosttest_route.cpp, a stand-alone program built with
-fsanitize=address,undefined and run directly. It replays the three passes of the kernels with one loop iteration per
thread in a shuffled order; whatever the order, the result must be the Python model's: the sorted set of
t - t % P, and per bucket the minimum, the maximum and the counts."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = 0xFFFFFFFF
MAX_BUCKETS = 1024
U64 = (1 << 64) - 1


def build_exe() -> str:
    src = os.path.join(HERE, "csrc", "hosttest_route.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_route")
    deps = [src] + [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_wire.h", "jx_field.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", "-o", tmp, src], check=True)
        os.replace(tmp, exe)
    return exe


def run(mode: str, payload: bytes | None, tmp_path) -> list[str]:
    args = [build_exe(), mode]
    if payload is not None:
        path = os.path.join(str(tmp_path), mode + ".bin")
        with open(path, "wb") as fh:
            fh.write(payload)
        args.append(path)
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def route_model(times, route, P, collected):
    """(status, table rows (start, min, max, reports, routed, collected), route, bucket_index, bucket_collected)."""
    starts = sorted({t - t % P for t in times})
    if len(starts) > MAX_BUCKETS:
        return 1, [], list(route), None, None
    at = {s: k for k, s in enumerate(starts)}
    col = set(collected)
    index = [at[t - t % P] for t in times]
    in_col = [int(starts[k] in col) for k in index]
    new = [k if r == 0 and not c else OUT for k, r, c in zip(index, route, in_col)]
    rows = []
    for k, s in enumerate(starts):
        mine = [i for i in range(len(times)) if index[i] == k]
        rows.append((s, min(times[i] for i in mine), max(times[i] for i in mine), len(mine),
                     sum(new[i] != OUT for i in mine), int(s in col)))
    return 0, rows, new, index, in_col


EDGE_TIMES = lambda P: [0, P - 1, P, (P + 1) & U64, 1 << 63, U64 - 1, U64]  # noqa: E731
EDGE_PRECISIONS = [1, 3, 3600, 1 << 63, (1 << 63) + 1, U64]


def test_bucket_start_at_the_u64_edges(tmp_path):
    pairs = [(t, P) for P in EDGE_PRECISIONS for t in EDGE_TIMES(P)]
    got = run("start", struct.pack("<I", len(pairs)) + b"".join(struct.pack("<QQ", t, P) for t, P in pairs), tmp_path)
    assert [int(x) for x in got] == [t - t % P for t, P in pairs]


def test_outcome_routed_over_the_full_product(tmp_path):
    """wire_outcome_routed equals wire_outcome except exactly where that returns none (0xFF) and the bucket is
    collected: there it is BatchCollected, code point 0. So BatchCollected ranks below every other error."""
    rows = [tuple(int(x) for x in line.split()) for line in run("outcome", None, tmp_path)]
    assert len(rows) == 11 * 9 * 2 * 4 * 7 * 2 * 2 and len(set(r[:7] for r in rows)) == len(rows)
    changed = 0
    for *_, collected, routed, plain in rows:
        if plain == 0xFF and collected:
            assert routed == 0
            changed += 1
        else:
            assert routed == plain
    # finished without the route: no host error, opened, not early, wire_status 0 or 1, verdict 0, not replayed
    assert changed == 2


def route_cases() -> list[tuple[str, list[int], list[int], int, list[int]]]:
    rnd = random.Random(557)
    T0 = 1_700_000_000 - 1_700_000_000 % 64
    C = []

    def add(name, times, P, collected=(), out=()):
        route = [OUT if i in out else 0 for i in range(len(times))]
        C.append((name, list(times), route, P, list(collected)))

    add("empty", [], 7)
    for n in (1, 64, 65, 193):
        for P in (64, 50, 3600):
            add(f"ramp{n}/{P}", [T0 + i for i in range(n)], P)
    add("descending130", [T0 + 129 - i for i in range(130)], 1)
    ramp = [T0 + i for i in range(193)]
    starts = sorted({t - t % 50 for t in ramp})
    add("collected_all", ramp, 50, starts)
    add("collected_subset", ramp, 50, starts[1:3], out={0, 60, 61, 192})
    add("collected_no_bucket", ramp, 50, [starts[0] + 1, starts[-1] + 50, 0, U64])
    add("collected_unsorted_repeats", ramp, 50, [starts[3], starts[0], starts[3], starts[0], 5])
    add("random", [rnd.randrange(1 << 20) for _ in range(300)], 4096, [8192, 0], out=set(range(0, 300, 7)))
    add("all_out", ramp, 50, (), out=set(range(193)))
    add("cap_1024", [(i % 1024) * 10 + i // 1024 for i in range(2100)], 10, [10, 10230])
    add("cap_1025", [(i % 1025) * 10 + i // 1025 for i in range(2100)], 10, [10], out={3})
    for P in EDGE_PRECISIONS:
        add(f"edges/{P}", EDGE_TIMES(P) * 2, P, [0, (1 << 63) - (1 << 63) % P], out={2})
    return C


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_route_passes_in_any_thread_order(tmp_path, seed):
    C = route_cases()
    blob = struct.pack("<I", len(C))
    for _, times, route, P, collected in C:
        blob += struct.pack("<QQQQ", len(times), P, len(collected), seed)
        blob += struct.pack(f"<{len(times)}Q", *times) + struct.pack(f"<{len(times)}I", *route)
        blob += struct.pack(f"<{len(collected)}Q", *collected)
    lines = run("route", blob, tmp_path)
    assert len(lines) == len(C)
    seen = set()
    for (name, times, route, P, collected), line in zip(C, lines):
        head, table, per = line.split("|")
        status, nb = int(head.split()[3]), int(head.split()[5])
        t = [int(x) for x in table.split()]
        p = [int(x) for x in per.split()]
        w_status, w_rows, w_route, w_index, w_col = route_model(times, route, P, collected)
        assert status == w_status, name
        assert p[0::3] == w_route, name
        seen.add(status)
        if status:
            assert nb == 0 and name == "cap_1025"
            continue
        assert [tuple(t[6 * k:6 * k + 6]) for k in range(nb)] == w_rows, name
        assert p[1::3] == w_index and p[2::3] == w_col, name
        if name.startswith("ramp"):
            n, prec = (int(x) for x in name[4:].split("/"))
            assert nb == {(193, 64): 4, (193, 50): 4, (193, 3600): 1}.get((n, prec), nb)
        if name == "descending130":
            assert nb == 130
        if name == "cap_1024":
            assert nb == 1024
    assert seen == {0, 1}
