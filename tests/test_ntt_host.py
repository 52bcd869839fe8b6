"""janus_amd/csrc/jx_ntt.h (the prover's Field128 transforms), compiled for the host, against Python integers."""
import ctypes
import os
import random
import subprocess

import pytest

import math_vectors as V
from math_vectors import P128, dft, horner, interpolate, rand_vals, rev, root  # shared with the device test

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def nt():
    src = os.path.join(HERE, "csrc", "ntt_hosttest.cpp")
    so = os.path.join(HERE, "csrc", "libjx_ntt_hosttest.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_ntt.h", "jx_field.h")]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.nt_table.argtypes = [u32, vp]
    L.nt_transform.argtypes = [ctypes.c_int, u32, vp]
    L.nt_gpoly.argtypes = [u32, u32, vp, vp]
    return L


def pack(vals):
    return ctypes.create_string_buffer(b"".join(v.to_bytes(16, "little") for v in vals), 16 * len(vals))


def unpack(buf, n):
    return [int.from_bytes(buf.raw[16 * i:16 * i + 16], "little") for i in range(n)]


@pytest.mark.parametrize("log_p", range(1, 12))
def test_table(nt, log_p):
    n = 1 << log_p
    buf = ctypes.create_string_buffer(16 * (3 * n + 1))
    nt.nt_table(log_p, buf)
    t = unpack(buf, 3 * n + 1)
    alpha, beta = root(log_p), root(log_p + 1)
    assert beta * beta % P128 == alpha and pow(alpha, n, P128) == 1 and pow(alpha, n // 2, P128) == P128 - 1
    ninv = pow(n, P128 - 2, P128)
    for k in range(0, n // 2, max(1, n // 64)):
        assert t[k] == pow(alpha, k, P128)
        assert t[n // 2 + k] == pow(alpha, P128 - 1 - k, P128)
    for i in range(0, n, max(1, n // 64)):
        j = rev(i, log_p)
        assert t[n + i] == pow(beta, j, P128) * ninv % P128
        assert t[2 * n + i] == pow(beta, (P128 - 1 - j) % (P128 - 1), P128)
    # the final scale R / (2P), stored in Montgomery form and read back out of it: (1 / 2P) R
    assert t[3 * n] == pow(2 * n, P128 - 2, P128) * (1 << 128) % P128


@pytest.mark.parametrize("log_p", range(1, 12))
def test_forward_and_inverse(nt, log_p):
    """Sizes 2 to 2048: the inverse (DIF) against the direct sum up to 64 points and against the Python fast
    transform above it; the forward (DIT) undoes it up to the factor P."""
    rng = random.Random(100 + log_p)
    n = 1 << log_p
    x = rand_vals(rng, n)
    buf = pack(x)
    nt.nt_transform(0, log_p, buf)
    got = unpack(buf, n)
    if n <= 64:
        want = dft(x, pow(root(log_p), P128 - 2, P128))
        assert [got[rev(m, log_p)] for m in range(n)] == want
    coef = interpolate(x, log_p)
    assert [got[rev(j, log_p)] * pow(n, P128 - 2, P128) % P128 for j in range(n)] == coef
    nt.nt_transform(1, log_p, buf)  # bit-reversed in, natural out
    assert unpack(buf, n) == [v * n % P128 for v in x]
    if n <= 64:
        y = [x[rev(i, log_p)] for i in range(n)]
        buf = pack(y)
        nt.nt_transform(1, log_p, buf)
        assert unpack(buf, n) == dft(x, root(log_p))


@pytest.mark.parametrize("log_p", [1, 2, 3, 5, 6, 7, 9, 10])
def test_odd_points_against_horner(nt, log_p):
    rng = random.Random(200 + log_p)
    n = 1 << log_p
    x = rand_vals(rng, n)
    coef = interpolate(x, log_p)
    alpha, beta = root(log_p), root(log_p + 1)
    for k in rng.sample(range(n), min(n, 8)):  # the interpolated polynomial does pass through the wire values
        assert horner(coef, pow(alpha, k, P128)) == x[k]
    buf = pack(x)
    nt.nt_transform(2, log_p, buf)
    got = unpack(buf, n)
    for k in (range(n) if n <= 64 else rng.sample(range(n), 24)):
        assert got[k] == horner(coef, pow(beta, 2 * k + 1, P128))


@pytest.mark.parametrize("log_p,npairs", [(1, 1), (2, 3), (5, 2), (7, 3), (10, 1)])
def test_gadget_poly(nt, log_p, npairs):
    """G's coefficients from random wires: the top one, 2P - 1, is zero, and G takes the values sum a_i b_i at
    the even points and agrees with the product of the interpolated wire polynomials at a random point."""
    rng = random.Random(300 + log_p)
    n = 1 << log_p
    wires = [rand_vals(rng, n) for _ in range(2 * npairs)]
    out = ctypes.create_string_buffer(16 * 2 * n)
    nt.nt_gpoly(log_p, npairs, pack([v for w in wires for v in w]), out)
    g = unpack(out, 2 * n)
    assert g[2 * n - 1] == 0
    alpha = root(log_p)
    for k in rng.sample(range(n), min(n, 6)):
        want = sum(wires[2 * i][k] * wires[2 * i + 1][k] for i in range(npairs)) % P128
        assert horner(g, pow(alpha, k, P128)) == want
    z = rng.randrange(P128)
    polys = [interpolate(w, log_p) for w in wires]
    want = sum(horner(polys[2 * i], z) * horner(polys[2 * i + 1], z) for i in range(npairs)) % P128
    assert horner(g, z) == want


@pytest.mark.parametrize("log_p", [1, 2, 6, 8, 10])
def test_python_transforms_against_horner(log_p):
    """The Python fast transforms every element of the device test's outputs is compared with (math_vectors.py):
    the forward transform, the odd-point values and the gadget polynomial, against Horner's rule at a few points."""
    rng = random.Random(400 + log_p)
    n = 1 << log_p
    wires = [rand_vals(rng, n) for _ in range(4)]
    coef = [interpolate(w, log_p) for w in wires]
    alpha, beta = root(log_p), root(log_p + 1)
    vals, odd = V.evaluate(coef[0], log_p), V.odd_point_values(wires[0], log_p)
    assert vals == wires[0] and len(odd) == n
    wide = V.evaluate(coef[0], log_p + 1)
    for k in [0, n - 1] + rng.sample(range(n), min(n, 6)):
        assert horner(coef[0], pow(alpha, k, P128)) == vals[k]
        assert horner(coef[0], pow(beta, 2 * k + 1, P128)) == odd[k] == wide[2 * k + 1]
    g = V.gadget_poly(wires, log_p)
    assert len(g) == 2 * n and g[2 * n - 1] == 0
    for z in [1, beta, P128 - 1] + [rng.randrange(P128) for _ in range(4)]:
        assert horner(g, z) == sum(horner(coef[2 * i], z) * horner(coef[2 * i + 1], z) for i in range(2)) % P128
