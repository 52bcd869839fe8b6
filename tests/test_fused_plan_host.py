"""The fused call's launch plan (janus_amd/csrc/jx_fused_plan.h: the reports per launch of a fused prepare + aggregate
call, its launches and the pipelines that run them), on the CPU: tests/csrc/hosttest_fused_plan.cpp, a stand-alone
program built with -fsanitize=address,undefined and run directly. Its expectations were worked out from the engine's
launch_chunk and pipes_for as they stood before the plan moved into the header; the empty call is new."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = 20


def test_fused_plan_under_sanitizers():
    src = os.path.join(HERE, "csrc", "hosttest_fused_plan.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_fused_plan")
    deps = [src, os.path.join(HERE, "..", "janus_amd", "csrc", "jx_fused_plan.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        # the sanitizers' runtimes linked into the program itself: it runs as it is, whatever else the loader brings
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", tmp, src],
                       check=True)
        os.replace(tmp, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines[-1] == "all ok" and len(lines) == CHECKS + 1, r.stdout
    assert all(line.endswith(": ok") for line in lines[:-1]), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
