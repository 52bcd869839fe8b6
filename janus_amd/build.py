"""Build the gfx950 engine library in-tree: janus_amd/lib/libjanus_prio3.so, and the test-only device harness
tests/csrc/libjx_devtest.so (the arithmetic headers one case per lane, for tests/test_gpu_device_math.py).

hipcc cross-compiles for gfx950 without a GPU. Run: ``python -m janus_amd.build``.
"""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(_HERE, "csrc", f) for f in ("jx_hpke_p256.hip", "jx_hpke_long.hip", "jx_kernels.hip", "jx_hpke_suite.hip", "jx_hpke_seal.hip",
                                                  "jx_hpke_default.hip", "jx_flp.hip", "jx_accumulate.hip",
                                                  "jx_mp64.hip", "jx_shard.hip", "jx_collect.hip", "jx_engine.cpp", "jx_engine_cfg.cpp", "jx_engine_prep.cpp",
                                                  "jx_engine_acc.cpp", "jx_engine_fused.cpp", "jx_engine_upload.cpp",
                                                  "jx_engine_shard.cpp", "jx_engine_seal.cpp", "jx_engine_collect.cpp", "jx_engine_wire.cpp", "jx_wire.hip",
                                                  "jx_engine_wire_upload.cpp", "jx_wire_upload.hip", "jx_coalesce.cpp",
                                                  "jx_arena.cpp",
                                                  "jx_hpke.hip")]  # the slowest to compile first
HEADERS = [os.path.join(_HERE, "csrc", f) for f in ("jx_field.h", "jx_keccak.h", "jx_sha256.h", "jx_kernels.h",
                                                  "jx_hpke.h", "jx_sha_aes.h", "jx_engine_internal.h", "jx_sha512.h",
                                                  "jx_chapoly.h", "jx_hpke_suites.h", "jx_p256.h", "jx_keyreg.h",
                                                  "jx_hpke_open.h", "jx_k1_plan.h", "jx_fused_plan.h", "jx_ghash_lanes.h",
                                                  "jx_hpke_long.h", "jx_upload.h", "jx_chapoly_lanes.h", "jx_enc_rows.h",
                                                  "jx_ntt.h", "jx_shard.h", "jx_sample.h", "jx_carve.h", "jx_hpke_seal.h",
                                                  "jx_wire.h", "jx_wire_dev.h", "jx_collect.h", "jx_engine_call.h")]
OUT = os.path.join(_HERE, "lib", "libjanus_prio3.so")
# jx_mp64.hip: keep the LDS for the AES table (the AMDGPU backend would otherwise move a small private
# array of the out-of-line helpers into LDS, +16 KiB per workgroup, one workgroup less per CU)
EXTRA_FLAGS = {"jx_mp64.hip": ["-mllvm", "-disable-promote-alloca-to-lds"]}
ARCH = os.environ.get("JX_OFFLOAD_ARCH", "gfx950")

_TESTS_CSRC = os.path.join(_HERE, "..", "tests", "csrc")
DEVTEST_SRC = os.path.join(_TESTS_CSRC, "devtest.hip")
DEVTEST_OUT = os.path.join(_TESTS_CSRC, "libjx_devtest.so")


def _stale() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = SOURCES + HEADERS + [os.path.join(_HERE, "..", "include", h) for h in ("jx_prio3.h", "jx_hpke.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def hipcc_path() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_and_link(sources, out: str, extra_flags=None, defines=(), verbose: bool = False) -> str:
    """The one hipcc invocation of the project: every source to an object beside `out` (one hipcc per
    translation unit, at most 16 at a time), then the shared library, linked aside and renamed into place."""
    extra_flags = extra_flags or {}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hipcc = hipcc_path()
    objs = [os.path.join(os.path.dirname(out), os.path.basename(src) + ".o") for src in sources]

    def compile_one(src, obj):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", src, "-o", obj]
        cmd += [f"-D{d}" for d in defines]
        cmd += extra_flags.get(os.path.basename(src), [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return p.returncode, p.stdout.decode(), cmd

    with ThreadPoolExecutor(max_workers=min(len(sources), 16)) as pool:
        results = list(pool.map(compile_one, sources, objs))
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


_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def devtest_sources() -> list:
    """devtest.hip and every project header it includes, directly or not, in a fixed order."""
    seen, todo = [], [os.path.normpath(DEVTEST_SRC)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.append(f)
        with open(f, encoding="utf-8") as fh:
            for inc in _INCLUDE.findall(fh.read()):
                p = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                if os.path.exists(p):
                    todo.append(p)
    return sorted(seen)


def devtest_source_hash() -> str:
    """File times do not survive a copy between machines: the harness is stale when this differs from the
    dt_source_hash() it was built with."""
    h = hashlib.sha256()
    for f in devtest_sources():
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(hashlib.sha256(fh.read()).digest())
    return h.hexdigest()[:32]


def build_devtest(verbose: bool = False) -> str:
    """Build tests/csrc/libjx_devtest.so (test-only; needs neither torch nor the engine library)."""
    return compile_and_link([DEVTEST_SRC], DEVTEST_OUT, defines=[f'DT_SRC_HASH="{devtest_source_hash()}"'], verbose=verbose)


def devtest_built_hash():
    """The hash libjx_devtest.so was built with, read from the file (no GPU, no load); None when there is none."""
    if not os.path.exists(DEVTEST_OUT):
        return None
    with open(DEVTEST_OUT, "rb") as fh:
        m = re.search(rb"DT_SRC_HASH=([0-9a-f]{32})\0", fh.read())
    return m.group(1).decode() if m else None


def build(force: bool = False, verbose: bool = False) -> str:
    """Build the library (measurement variants live in tools/kernel_probe.hip, not here), then the device harness
    of the tests when its sources changed."""
    if force or _stale():
        compile_and_link(SOURCES, OUT, extra_flags=EXTRA_FLAGS, verbose=verbose)
    if force or devtest_built_hash() != devtest_source_hash():
        build_devtest(verbose=verbose)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(DEVTEST_OUT)
