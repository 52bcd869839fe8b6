"""The staged form of a ParallelSum call's coefficients (pack_cd26 / unpack_cd26, janus_amd/csrc/jx_field.h),
compiled for the host: K1 writes (c_k, d_k) as ten 26-bit limbs and the FLP kernels multiply from them without
splitting a coefficient again. unpack(pack(c, d)) must be to_limbs26 of each value, and wacc_mac fed from the
unpacked words must give the nine columns it gives from to_limbs26; both against Python integers."""
import ctypes
import os
import random
import subprocess

import pytest

import math_vectors as V

HERE = os.path.dirname(os.path.abspath(__file__))
M26 = 2**26 - 1


@pytest.fixture(scope="module")
def cl():
    src = os.path.join(HERE, "csrc", "hosttest_coef_limbs.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_coef_limbs.so")
    hdr = os.path.join(HERE, "..", "janus_amd", "csrc", "jx_field.h")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr, os.path.join(HERE, "csrc", "jx_testops.h"))):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.cl_to_limbs.argtypes = [vp, vp]
    L.cl_pack.argtypes = [vp, vp, vp]
    L.cl_unpack.argtypes = [vp, vp, vp]
    L.cl_mac.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    assert L.cl_words() == 10
    return L


def limbs(a):
    """Five limbs of a 128-bit value: 26, 26, 26, 26 and the remaining 24 bits."""
    return [(a >> (26 * i)) & M26 for i in range(4)] + [a >> 104]


def _b(x):
    return ctypes.create_string_buffer(x.to_bytes(16, "little"), 16)


_values = V.coef_limb_values


def test_unpack_of_pack_is_to_limbs26(cl):
    vals = _values()
    rnd = random.Random(27)
    for i, c in enumerate(vals):
        d = vals[(i * 7 + 3) % len(vals)] if i % 3 else rnd.choice(vals[:9])
        w = (ctypes.c_uint32 * 10)()
        cl.cl_pack(_b(c), _b(d), w)
        # the staged layout: row A = c's limbs 0-3, row B = d's limbs 0-3, half-row C = the two top limbs
        assert list(w) == limbs(c)[:4] + limbs(d)[:4] + [limbs(c)[4], limbs(d)[4]], hex(c)
        gc, gd = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
        cl.cl_unpack(w, gc, gd)
        tc, td = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
        cl.cl_to_limbs(_b(c), tc)
        cl.cl_to_limbs(_b(d), td)
        assert list(gc) == list(tc) == limbs(c), hex(c)
        assert list(gd) == list(td) == limbs(d), hex(d)


@pytest.mark.parametrize("n", [1, 5, 512])
def test_wacc_mac_from_unpacked_rows(cl, n):
    """n calls of one slot (512: the most between two normalisations), operands drawn from the edge values
    and random ones: the same nine columns from the staged words as from to_limbs26, == Python's."""
    draws = V.coef_mac_operands(n)
    assert len(draws) == 40
    for xs, cs, ds in draws:
        bx, bc, bd = (ctypes.create_string_buffer(b"".join(v.to_bytes(16, "little") for v in a), 16 * n)
                      for a in (xs, cs, ds))
        got = {}
        for packed in (0, 1):
            ce, co = (ctypes.c_uint64 * 9)(), (ctypes.c_uint64 * 9)()
            cl.cl_mac(bx, bc, bd, n, packed, ce, co)
            got[packed] = (list(ce), list(co))
        want_e, want_o = [0] * 9, [0] * 9
        for x, c, d in zip(xs, cs, ds):
            xl, cl_, dl = limbs(x), limbs(c), limbs(d)
            for i in range(5):
                for j in range(5):
                    want_e[i + j] += xl[i] * dl[j]
                    want_o[i + j] += xl[i] * cl_[j]
        assert max(want_e + want_o) < 2**64
        assert got[1] == got[0] == (want_e, want_o)
        # the columns are the products themselves: sum_s col[s] 2^(26 s) == sum_k x_k c_k
        assert sum(v << (26 * s) for s, v in enumerate(got[1][1])) == sum(x * c for x, c in zip(xs, cs))
