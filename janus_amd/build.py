"""Build the gfx950 engine library in-tree: janus_amd/lib/libjanus_prio3.so.

hipcc cross-compiles for gfx950 without a GPU. Run: ``python -m janus_amd.build``.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(_HERE, "csrc", f) for f in ("jx_hpke_p256.hip", "jx_hpke_long.hip", "jx_kernels.hip", "jx_hpke_suite.hip",
                                                  "jx_hpke_default.hip", "jx_flp.hip", "jx_accumulate.hip",
                                                  "jx_mp64.hip", "jx_engine.cpp", "jx_coalesce.cpp", "jx_arena.cpp",
                                                  "jx_hpke.hip")]  # the slowest to compile first
HEADERS = [os.path.join(_HERE, "csrc", f) for f in ("jx_field.h", "jx_keccak.h", "jx_sha256.h", "jx_kernels.h",
                                                  "jx_hpke.h", "jx_sha_aes.h", "jx_engine_internal.h", "jx_sha512.h",
                                                  "jx_chapoly.h", "jx_hpke_suites.h", "jx_p256.h", "jx_keyreg.h",
                                                  "jx_hpke_open.h", "jx_k1_plan.h", "jx_fused_plan.h", "jx_ghash_lanes.h",
                                                  "jx_hpke_long.h", "jx_upload.h", "jx_chapoly_lanes.h")]
OUT = os.path.join(_HERE, "lib", "libjanus_prio3.so")
# jx_mp64.hip: keep the LDS for the AES table (the AMDGPU backend would otherwise move a small private
# array of the out-of-line helpers into LDS, +16 KiB per workgroup, one workgroup less per CU)
EXTRA_FLAGS = {"jx_mp64.hip": ["-mllvm", "-disable-promote-alloca-to-lds"]}
ARCH = os.environ.get("JX_OFFLOAD_ARCH", "gfx950")


def _stale() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = SOURCES + HEADERS + [os.path.join(_HERE, "..", "include", h) for h in ("jx_prio3.h", "jx_hpke.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Build the library (measurement variants live in tools/kernel_probe.hip, not here)."""
    out = OUT
    if not force and not _stale():
        return OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [os.path.join(os.path.dirname(out), os.path.basename(src) + ".o") for src in SOURCES]

    def compile_one(src, obj):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", src, "-o", obj]
        cmd += EXTRA_FLAGS.get(os.path.basename(src), [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return p.returncode, p.stdout.decode(), cmd

    # one hipcc per translation unit, at most 16 at a time
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), 16)) as pool:
        results = list(pool.map(compile_one, SOURCES, objs))
    for rc, log, cmd in results:
        if rc != 0:
            sys.stderr.write(log)
            raise RuntimeError(f"hipcc failed: {' '.join(cmd)}")
        if verbose and log:
            sys.stderr.write(log)
    tmp = f"{out}.{os.getpid()}.tmp"  # link aside, then rename: a reader never sees a partial library
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    for o in objs:
        os.remove(o)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
