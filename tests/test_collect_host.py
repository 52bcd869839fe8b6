"""janus_amd/csrc/jx_collect.h (the per-element and per-job pieces of the collection kernels), compiled for the host,
against Python integers."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
P64 = 2**64 - 2**32 + 1
P128 = 2**128 - 28 * 2**64 + 1
M64 = 2**64 - 1
OK, INVALID_BATCH_SIZE, BATCH_MISMATCH, BAD_RECORD, SEAL_FAILED = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def ch():
    src = os.path.join(HERE, "csrc", "collect_hosttest.cpp")
    so = os.path.join(HERE, "csrc", "libjx_collect_hosttest.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_collect.h", "jx_field.h")]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    u64, u32, vp, i = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    L.ch_decode64.argtypes = [u64, ctypes.POINTER(u64)]
    L.ch_decode128.argtypes = [u64, u64, ctypes.POINTER(u64 * 2)]
    L.ch_add64.argtypes = [u64, u64]
    L.ch_add64.restype = u64
    L.ch_add128.argtypes = [ctypes.POINTER(u64 * 2)] * 3
    L.ch_status.argtypes = [u64, i, u64, vp, u64, vp, u64, u64]
    L.ch_status.restype = u32
    L.ch_seal_status.argtypes = [u32, i]
    L.ch_seal_status.restype = u32
    L.ch_open_status.argtypes = [i, i, i, i]
    L.ch_open_status.restype = u32
    return L


def pair(v):
    return (ctypes.c_uint64 * 2)(v & M64, v >> 64)


def add128(ch, a, b):
    out = (ctypes.c_uint64 * 2)()
    ch.ch_add128(ctypes.byref(pair(a)), ctypes.byref(pair(b)), ctypes.byref(out))
    return out[0] | (out[1] << 64)


@pytest.mark.parametrize("v", [0, 1, P64 - 1, P64, P64 + 1, M64])
def test_decode64(ch, v):
    out = ctypes.c_uint64()
    assert bool(ch.ch_decode64(v, ctypes.byref(out))) == (v < P64)
    assert out.value == v


P_HI = P128 >> 64
@pytest.mark.parametrize("v", [0, 1, P128 - 1, P128, P128 + 1, 2**128 - 1, P_HI << 64, (P_HI << 64) | 1,
                               ((P_HI - 1) << 64) | M64, ((P_HI + 1) << 64)])
def test_decode128(ch, v):
    out = (ctypes.c_uint64 * 2)()
    assert bool(ch.ch_decode128(v & M64, v >> 64, ctypes.byref(out))) == (v < P128)
    assert out[0] | (out[1] << 64) == v


def test_p128_halves():
    assert P128 == (P_HI << 64) | 1  # hi = P_HI with lo = 0 is the largest element, with lo = 1 it is p


def test_add64(ch):
    rng = random.Random(64)
    edge = [0, 1, 2**32 - 1, 2**32, P64 - 2**32, P64 - 2, P64 - 1, (P64 - 1) // 2, (P64 + 1) // 2]
    cases = list(itertools.product(edge, edge)) + [(rng.randrange(P64), rng.randrange(P64)) for _ in range(2000)]
    cases += [(a, P64 - a) for a in edge[1:]]  # sums that land exactly on p
    cases += [(a, P64 - a) for a in (rng.randrange(1, P64) for _ in range(200))]
    wrapped = 0
    for a, b in cases:
        assert ch.ch_add64(a, b) == (a + b) % P64, (a, b)
        wrapped += a + b >= 2**64
    assert wrapped > 100  # sums past 2^64, not only past p


def test_add128(ch):
    rng = random.Random(128)
    edge = [0, 1, M64, 2**64, P128 - 2**64, P128 - 2, P128 - 1, (P128 - 1) // 2, (P128 + 1) // 2, P_HI << 64]
    cases = list(itertools.product(edge, edge)) + [(rng.randrange(P128), rng.randrange(P128)) for _ in range(2000)]
    cases += [(a, P128 - a) for a in edge[1:]]
    cases += [(a, P128 - a) for a in (rng.randrange(1, P128) for _ in range(200))]
    wrapped = 0
    for a, b in cases:
        assert add128(ch, a, b) == (a + b) % P128, (a, b)
        wrapped += a + b >= 2**128
    assert wrapped > 100


def want_status(nrecords, bad, count, cs, expect, lo, hi):
    """Janus's order: the datastore's decode, validate_batch_size, then the count and checksum comparison."""
    if bad:
        return BAD_RECORD
    if nrecords == 0 or count < lo or (hi != 0 and count > hi):
        return INVALID_BATCH_SIZE
    if expect is not None and (expect[0] != count or expect[1] != cs):
        return BATCH_MISMATCH
    return OK


def test_status_every_combination(ch):
    lo, hi = 10, 20
    cs = bytes(range(32))
    flipped = [cs[:31] + bytes([cs[31] ^ (1 << b)]) for b in range(8)] + [bytes([cs[0] ^ 1]) + cs[1:]]
    seen = set()
    for nrecords, bad, count, maxb in itertools.product([0, 1, 33], [0, 1], [0, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 2**63],
                                                        [0, hi, lo]):
        expects = [None, (count, cs), (count + 1, cs), (count - 1 if count else 5, cs)] + [(count, f) for f in flipped]
        for expect in expects:
            want = want_status(nrecords, bad, count, cs, expect, lo, maxb)
            got = ch.ch_status(nrecords, bad, count, cs, expect[0] if expect else 0, expect[1] if expect else None, lo, maxb)
            assert got == want, (nrecords, bad, count, maxb, expect)
            seen.add(got)
    assert seen == {OK, INVALID_BATCH_SIZE, BATCH_MISMATCH, BAD_RECORD}
    # the named cases, spelled out
    assert ch.ch_status(0, 0, 15, cs, 15, cs, lo, hi) == INVALID_BATCH_SIZE  # an empty job
    assert ch.ch_status(1, 0, lo - 1, cs, lo - 1, cs, lo, hi) == INVALID_BATCH_SIZE
    assert ch.ch_status(1, 0, lo, cs, lo, cs, lo, hi) == OK
    assert ch.ch_status(1, 0, hi, cs, hi, cs, lo, hi) == OK
    assert ch.ch_status(1, 0, hi + 1, cs, hi + 1, cs, lo, hi) == INVALID_BATCH_SIZE
    assert ch.ch_status(1, 0, hi + 1, cs, hi + 1, cs, lo, 0) == OK  # no maximum
    assert ch.ch_status(1, 0, 15, cs, 16, cs, lo, hi) == BATCH_MISMATCH
    assert ch.ch_status(1, 0, 15, cs, 15, flipped[0], lo, hi) == BATCH_MISMATCH
    assert ch.ch_status(1, 0, 15, cs, 16, None, lo, hi) == OK  # the leader: nothing to compare against
    assert ch.ch_status(1, 1, 15, cs, 16, cs, lo, hi) == BAD_RECORD  # before everything else
    assert ch.ch_status(0, 1, 0, cs, 0, cs, lo, hi) == BAD_RECORD


def test_seal_and_open_status(ch):
    for st in (OK, INVALID_BATCH_SIZE, BATCH_MISMATCH, BAD_RECORD):
        assert ch.ch_seal_status(st, 1) == st
        assert ch.ch_seal_status(st, 0) == (SEAL_FAILED if st == OK else st)
    for lo_, ho, lb, hb in itertools.product([0, 1], repeat=4):
        want = 1 if not lo_ else 2 if not ho else 3 if lb else 4 if hb else 0
        assert ch.ch_open_status(lo_, ho, lb, hb) == want
