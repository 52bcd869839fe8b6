"""The slab carver (janus_amd/csrc/jx_carve.h: the one rule by which staging, resident batches and per-call scratch
are laid out of an arena slab), on the CPU: tests/csrc/hosttest_carve.cpp, a stand-alone program built with
-fsanitize=address,undefined and run directly. The batch offsets it expects were worked out from batch_new's offset
chain as it stood before the carver."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = 17


def test_carve_under_sanitizers():
    src = os.path.join(HERE, "csrc", "hosttest_carve.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_carve")
    deps = [src, os.path.join(HERE, "..", "janus_amd", "csrc", "jx_carve.h")]
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
