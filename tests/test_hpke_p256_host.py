"""The device code behind the P-256 HPKE kernels (janus_amd/csrc/jx_p256.h and the DHKEM(P-256, HKDF-SHA256) part
of jx_hpke_suites.h), compiled for the host (tests/csrc/hosttest_hpke_p256.cpp), against Python integers and
tests/hpke_p256_ref.py (pinned by the reference's RFC 9180 vectors, tests/test_hpke_p256_ref.py)."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import pytest

import hpke_p256_ref as R
import math_vectors as V
import hpke_suites_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
P, N = R.P, R.N


@pytest.fixture(scope="module")
def hp():
    src = os.path.join(HERE, "csrc", "hosttest_hpke_p256.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_hpke_p256.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_field.h", "jx_sha256.h", "jx_sha_aes.h", "jx_hpke.h",
                                                                         "jx_sha512.h", "jx_chapoly.h", "jx_hpke_suites.h",
                                                                         "jx_p256.h")]
    hdrs.append(os.path.join(HERE, "csrc", "jx_testops.h"))
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.hp_fe_op.argtypes = [ctypes.c_int, vp, vp, vp]
    L.hp_point_valid.argtypes = [vp]
    L.hp_scalar_mul.argtypes = [vp, vp, vp]
    L.hp_keypair.argtypes = [vp, vp]
    L.hp_context.argtypes = [u32, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.hp_key_supported.argtypes = [u32, u32, u32]
    return L


def _b(v: int) -> bytes:
    return v.to_bytes(32, "big")


def _op(hp, op: int, a: int, b: int = 0) -> int:
    out = ctypes.create_string_buffer(32)
    assert hp.hp_fe_op(op, _b(a), _b(b), out) == 1
    return int.from_bytes(out.raw, "big")


_operands = V.p256_operands


def test_field_mul_sq_against_python_integers(hp):
    edge, rand = _operands()
    for a in edge:
        assert _op(hp, 1, a) == a * a % P, hex(a)
        for b in edge:
            assert _op(hp, 0, a, b) == a * b % P, (hex(a), hex(b))
    for a in rand:
        assert _op(hp, 1, a) == a * a % P
        for b in rand[:8] + edge[:7]:
            assert _op(hp, 0, a, b) == a * b % P


def test_field_add_sub_against_python_integers(hp):
    edge, rand = _operands()
    for a in edge + rand[:10]:
        for b in edge + rand[10:20]:
            assert _op(hp, 3, a, b) == (a + b) % P, (hex(a), hex(b))
            assert _op(hp, 4, a, b) == (a - b) % P, (hex(a), hex(b))


def test_field_invert(hp):
    edge, rand = _operands()
    assert _op(hp, 2, 0) == 0
    for a in edge[1:] + rand:
        if a:
            inv = _op(hp, 2, a)
            assert inv == pow(a, -1, P) and inv * a % P == 1, hex(a)


def test_field_refuses_unreduced_operands(hp):
    out = ctypes.create_string_buffer(32)
    for v in (P, P + 1, 2**256 - 1):
        assert hp.hp_fe_op(0, _b(v), _b(1), out) == 0
        assert hp.hp_fe_op(0, _b(1), _b(v), out) == 0


_points = V.p256_points


def test_scalar_mul_exceptional_and_random_scalars(hp):
    """sk * P at the scalars where an incomplete ladder goes wrong (leading zero bits, 1, 2, n - 1, n - 2, the two
    halves of n, single bits) and at random ones, on G, -G and random points."""
    sks = V.p256_scalars()
    assert len(sks) == 29
    out = ctypes.create_string_buffer(64)
    for pt in _points():
        for k in sks:
            assert hp.hp_scalar_mul(_b(k), R.encode(pt), out) == 1, hex(k)
            want = R.mul(k, pt)
            assert out.raw == _b(want[0]) + _b(want[1]), (hex(k), pt)
    # sk = n gives the point at infinity (create_key refuses such a key; the ladder reports it)
    assert hp.hp_scalar_mul(_b(N), R.encode(R.G), out) == 0


def test_point_validation(hp):
    for pt in _points():
        e = R.encode(pt)
        assert hp.hp_point_valid(e) == 1
        for bit in (0, 7, 100, 255):  # y with one bit flipped
            bad = bytearray(e)
            bad[64 - bit // 8] ^= 1 << (bit % 8)
            assert hp.hp_point_valid(bytes(bad)) == 0
        for tag in (0x00, 0x02, 0x03):
            assert hp.hp_point_valid(bytes([tag]) + e[1:]) == 0
    assert hp.hp_point_valid(b"\x04" + _b(P) + _b(R.GY)) == 0  # x = p
    assert hp.hp_point_valid(b"\x04" + _b(R.GX) + _b(P)) == 0  # y = p
    # x = p is 0 mod p and (0, sqrt(b)) is a point: the unreduced spelling must still be refused
    z = R.lift_x(0)
    assert z is not None and hp.hp_point_valid(R.encode(z)) == 1
    assert hp.hp_point_valid(b"\x04" + _b(P) + _b(z[1])) == 0
    # points of y^2 = x^3 - 3x + b' (the invalid-curve attack): same x^3 - 3x term, another constant
    found = 0
    for bp in (R.B + 1, R.B - 1, 7):
        x = 2
        while R.lift_x(x, bp) is None:
            x += 1
        q = R.lift_x(x, bp)
        assert R.on_curve(q, bp) and not R.on_curve(q)
        assert hp.hp_point_valid(R.encode(q)) == 0
        found += 1
    assert found == 3


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_context_all_suites(hp, kdf, aead):
    """The host-side key_schedule_context under KEM 0x0010 plus the per-lane context builder (validation, DHKEM
    decap with its 158-byte expand message, the suite's key schedule) against the Python reference, with info on
    both sides of the hashes' padding boundaries."""
    rnd = random.Random(1000 * kdf + aead)
    key, nonce, ksc = (ctypes.create_string_buffer(n) for n in (32, 12, 129))
    ksc_len = ctypes.c_uint32()
    for info_len in (0, 20, 111, 112, 200):
        sk, info = _b(rnd.randrange(1, N)), rnd.randbytes(info_len)
        pk = R.public_key(sk)
        ss, enc = R.encap(_b(rnd.randrange(1, N)), pk)
        assert hp.hp_context(kdf, aead, sk, pk, info, info_len, enc, key, nonce, ksc, ctypes.byref(ksc_len)) == 1
        want_key, want_nonce = R.key_schedule(kdf, aead, ss, info)
        assert ksc_len.value == 1 + 2 * S.nh(kdf)
        assert ksc.raw[:ksc_len.value] == R.key_schedule_context(kdf, aead, info)
        assert nonce.raw == want_nonce
        assert key.raw == want_key + bytes(32 - len(want_key))
    bad = bytearray(enc)
    bad[64] ^= 1
    assert hp.hp_context(kdf, aead, sk, pk, info, info_len, bytes(bad), key, nonce, ksc, ctypes.byref(ksc_len)) == 0


def test_keypair_check(hp):
    rnd = random.Random(7)
    k = rnd.randrange(1, N)
    pk = R.mul(k, R.G)
    assert hp.hp_keypair(_b(k), R.encode(pk)) == 0
    assert hp.hp_keypair(_b(1), R.encode(R.G)) == 0 and hp.hp_keypair(_b(N - 1), R.encode(R.neg(R.G))) == 0
    for sk, p in ((0, pk), (N, pk), (N + 1, R.G), (2**256 - 1, pk), (k, R.neg(pk)), (k, R.G), (k + 1, pk)):
        assert hp.hp_keypair(_b(sk), R.encode(p)) == 1
    off = bytearray(R.encode(pk))
    off[33] ^= 1
    assert hp.hp_keypair(_b(k), bytes(off)) == 1


def test_key_ids(hp):
    for kem in (0x10, 0x20):
        for kdf, aead in S.SUITES:
            assert hp.hp_key_supported(kem, kdf, aead) == 1
    for kem, kdf, aead in ((0x11, 1, 1), (0x12, 1, 1), (0x21, 1, 1), (0x10, 0, 1), (0x10, 4, 1), (0x10, 1, 0), (0x10, 1, 4)):
        assert hp.hp_key_supported(kem, kdf, aead) == 0


def test_create_key_checks_ids_and_keypair_without_a_device():
    """jx_hpke_create_key checks the ids (JX_HPKE_E_UNSUPPORTED) and then the keypair (JX_HPKE_E_INVALID, with a
    reason) before it looks for a device, on any machine."""
    from janus_amd import hpke
    L = hpke._declare(hpke._lib.load())
    rnd = random.Random(11)
    k = rnd.randrange(1, N)
    pk = R.encode(R.mul(k, R.G))

    def create(kem, kdf, aead, sk: bytes, pub: bytes):
        h = ctypes.c_void_p()
        st = L.jx_hpke_create_key(kem, kdf, aead, sk, len(sk), pub, len(pub), None, 0, 0, ctypes.byref(h))
        assert not h.value or st == 0
        if h.value:
            L.jx_hpke_destroy(h)
        return st, L.jx_hpke_last_error(None)

    for kem, kdf, aead in ((0x11, 1, 1), (0x12, 1, 1), (0x10, 4, 1), (0x10, 1, 4), (0x10, 0, 1), (0x20, 4, 1)):
        st, why = create(kem, kdf, aead, _b(k), pk)
        assert st == hpke.E_UNSUPPORTED == -2 and b"unsupported HPKE suite" in why
    off = bytearray(pk)
    off[40] ^= 1
    for sk, pub, word in ((_b(0), pk, b"[1, n - 1]"), (_b(N), pk, b"[1, n - 1]"), (_b(k + 1), pk, b"base point"),
                          (_b(k), R.encode(R.G), b"base point"), (_b(k), bytes(off), b"not a point"),
                          (_b(k)[:31], pk, b"32 bytes"), (_b(k), pk[:64], b"65"), (_b(k), pk[1:33], b"65"),
                          (_b(k) + b"\0", pk, b"32 bytes")):
        st, why = create(0x10, 1, 1, sk, pub)
        assert st == hpke.E_INVALID == -1 and word in why, (why, word)
    st, why = create(0x20, 1, 1, bytes(32), pk)  # an X25519 key with a 65-byte public key
    assert st == hpke.E_INVALID and b"32 bytes each" in why
    # a good keypair passes both checks: what is left is the device (-6 without one, 0 with)
    st, _ = create(0x10, 3, 3, _b(k), pk)
    assert st in (0, -6)
    with pytest.raises(ValueError):
        hpke.HpkeOpener(_b(0), pk, b"", kem_id=hpke.KEM_P256_HKDF_SHA256)
    with pytest.raises(hpke.UnsupportedSuite):
        hpke.HpkeOpener(_b(k), pk, b"", kem_id=0x12)
