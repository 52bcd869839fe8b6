"""The one rule that lays a sealed report out as an EncRow (janus_amd/csrc/jx_enc_rows.h: flags, registry slots, 32-
and 65-byte encapsulated keys), on the CPU: tests/csrc/hosttest_enc_rows.cpp, a stand-alone program built with
-fsanitize=address,undefined and run directly. 400 seeded random jobs (both KEMs among the keypairs, keys of other
lengths, JX_KEY_NONE, JX_KEY_MALFORMED, fallbacks of the other KEM, the taskprov flag, payload offsets that do not
start at 0) through the host loop and through the kernel's lane body must equal fill_enc_rows as it was before the
rule was shared, byte for byte."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = 5


def test_enc_row_rule_under_sanitizers():
    src = os.path.join(HERE, "csrc", "hosttest_enc_rows.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_enc_rows")
    deps = [src] + [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_enc_rows.h", "jx_keyreg.h", "jx_field.h")]
    deps += [os.path.join(HERE, "..", "include", h) for h in ("jx_prio3.h", "jx_hpke.h")]
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
