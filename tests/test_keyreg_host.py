"""The HPKE key registry's slot bookkeeping (janus_amd/csrc/jx_keyreg.h: take, exhaustion at 16,384, reuse, 16-bit
slots in an EncRow) and the X25519 ladder with masked swaps (janus_amd/csrc/jx_hpke.h: RFC 7748 §5.2, the all-zero
output, 200 pairs recorded from oracle/hpke_oracle.py), on the CPU: tests/csrc/hosttest_keyreg.cpp, a stand-alone
program built with -fsanitize=address,undefined and run directly."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = 12


def test_keyreg_and_ladder_under_sanitizers():
    src = os.path.join(HERE, "csrc", "hosttest_keyreg.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_keyreg")
    deps = [src, os.path.join(HERE, "csrc", "hosttest_keyreg_vectors.h")]
    deps += [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_keyreg.h", "jx_hpke.h", "jx_sha_aes.h",
                                                                         "jx_sha256.h", "jx_field.h")]
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
