"""The device headers behind the HPKE suite kernels (janus_amd/csrc/jx_sha512.h, jx_chapoly.h, jx_hpke_suites.h,
AES-256 of jx_sha_aes.h), compiled for the host (tests/csrc/hosttest_hpke_suites.cpp), against hashlib, Python
integers and tests/hpke_suites_ref.py (pinned by the reference's RFC 9180 vectors)."""
from __future__ import annotations

import ctypes
import hashlib
import hmac
import os
import random
import subprocess

import pytest

import hpke_suites_ref as S
from oracle import hpke_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))
HASH = {1: hashlib.sha256, 2: hashlib.sha384, 3: hashlib.sha512}


@pytest.fixture(scope="module")
def hs():
    src = os.path.join(HERE, "csrc", "hosttest_hpke_suites.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_hpke_suites.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_field.h", "jx_sha256.h", "jx_sha_aes.h", "jx_hpke.h",
                                                                         "jx_sha512.h", "jx_chapoly.h", "jx_hpke_suites.h")]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.hs_hash.argtypes = [ctypes.c_int, vp, u32, vp]
    L.hs_hmac.argtypes = [ctypes.c_int, vp, u32, vp, u32, vp]
    L.hs_aes256.argtypes = [vp, vp, vp]
    L.hs_chacha20_block.argtypes = [vp, u32, vp, vp]
    L.hs_poly1305.argtypes = [vp, vp, u64, vp, vp]
    L.hs_chapoly_open.argtypes = [vp, vp, vp, u64, vp, u64, vp]
    L.hs_context.argtypes = [u32, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.hs_supported.argtypes = [u32, u32, u32]
    return L


LENGTHS = [0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256]


@pytest.mark.parametrize("kind", [2, 3, 1])
def test_hashes_against_hashlib(hs, kind):
    """SHA-384 / SHA-512 (and the generic path's SHA-256) at the lengths around one and two blocks and around
    the points where the padding needs another block (112 and 240 for the 128-byte block)."""
    rnd = random.Random(kind)
    out = ctypes.create_string_buffer(64)
    for n in LENGTHS + [55, 56, 63, 64, 65, 119, 120]:
        msg = rnd.randbytes(n)
        nh = hs.hs_hash(kind, msg, n, out)
        assert out.raw[:nh] == HASH[kind](msg).digest(), n


@pytest.mark.parametrize("kind", [2, 3, 1])
def test_hmac_against_hashlib(hs, kind):
    rnd = random.Random(10 + kind)
    out = ctypes.create_string_buffer(64)
    for klen in (0, 32, 48, 64):
        for n in (0, 1, 23, 111, 112, 119, 120, 128, 129, 159, 200):
            key, msg = rnd.randbytes(klen), rnd.randbytes(n)
            nh = hs.hs_hmac(kind, key, klen, msg, n, out)
            assert out.raw[:nh] == hmac.new(key, msg, HASH[kind]).digest(), (klen, n)


def test_aes256(hs):
    out = ctypes.create_string_buffer(16)
    hs.hs_aes256(bytes(range(32)), bytes.fromhex("00112233445566778899aabbccddeeff"), out)
    assert out.raw.hex() == "8ea2b7ca516745bfeafc49904b496089"  # FIPS 197 Appendix C.3
    rnd = random.Random(256)
    for _ in range(20):
        key, blk = rnd.randbytes(32), rnd.randbytes(16)
        hs.hs_aes256(key, blk, out)
        assert out.raw == S.aes_encrypt_block(S.aes256_expand(key), blk)


def test_chacha20_block(hs):
    rnd = random.Random(20)
    out = ctypes.create_string_buffer(64)
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    hs.hs_chacha20_block(key, 1, nonce, out)  # RFC 8439 §2.3.2
    assert out.raw.hex().startswith("10f1e7e4d13b5915500fdd1fa32071c4")
    for _ in range(5):
        key, nonce = rnd.randbytes(32), rnd.randbytes(12)
        for counter in (0, 1, 2**32 - 1):
            hs.hs_chacha20_block(key, counter, nonce, out)
            assert out.raw == S.chacha20_block(key, counter, nonce), counter


def _poly(hs, key: bytes, msg: bytes):
    tag = ctypes.create_string_buffer(16)
    h = (ctypes.c_uint32 * 5)()
    hs.hs_poly1305(key, msg, len(msg), tag, h)
    assert all(x < 2**26 for x in h)
    return tag.raw, sum(x << (26 * i) for i, x in enumerate(h))


def test_poly1305_random(hs):
    rnd = random.Random(1305)
    for i in range(2000):
        key = rnd.randbytes(32)
        msg = rnd.randbytes(rnd.choice([0, 1, 15, 16, 17, 31, 32, 33, 64, 100, rnd.randrange(300)]))
        if i % 4 == 0:  # dense limbs: carries everywhere
            msg = bytes(rnd.choice([0xFF, 0xFF, 0xFE, rnd.randrange(256)]) for _ in msg)
        tag, _ = _poly(hs, key, msg)
        assert tag == S.poly1305(key, msg), (key.hex(), msg.hex())


def test_poly1305_edges(hs):
    rmax = S.R_CLAMP.to_bytes(16, "little")  # every bit the clamp permits
    rnd = random.Random(5)
    for n in (0, 1, 15, 16, 17):
        for r in (rmax, rnd.randbytes(16), (1).to_bytes(16, "little")):
            for s in (bytes(16), b"\xff" * 16, rnd.randbytes(16)):
                for msg in (b"\xff" * n, rnd.randbytes(n)):
                    assert _poly(hs, r + s, msg)[0] == S.poly1305(r + s, msg), (n, r.hex())
    for nblk in (1, 2, 3, 8, 40):  # every block 0xFF under the largest r
        for s in (bytes(16), b"\xff" * 16):
            msg = b"\xff" * (16 * nblk)
            assert _poly(hs, rmax + s, msg)[0] == S.poly1305(rmax + s, msg)
    # the accumulator in [p, 2^130) before the final reduction: with r = 1 the accumulator is the plain sum of the
    # blocks (each with its 2^128 bit), so ff..ff then 2^128 - 4 + k give 2^130 - 5 + k, k = 0..3, which the
    # partial reduction leaves as it is; the tag must come from k, not from p + k
    one = (1).to_bytes(16, "little")
    for k in range(4):
        msg = b"\xff" * 16 + (2**128 - 4 + k).to_bytes(16, "little")
        for s in (bytes(16), rnd.randbytes(16), b"\xff" * 16):
            tag, h_pre = _poly(hs, one + s, msg)
            assert S.P1305 <= h_pre < 2**130, hex(h_pre)
            assert tag == S.poly1305(one + s, msg) == ((k + int.from_bytes(s, "little")) % 2**128).to_bytes(16, "little")
    # and just below p: not reduced
    msg = b"\xff" * 16 + (2**128 - 5).to_bytes(16, "little")
    tag, h_pre = _poly(hs, one + bytes(16), msg)
    assert h_pre == S.P1305 - 1 and tag == S.poly1305(one + bytes(16), msg)


def test_chapoly_open_against_reference(hs):
    rnd = random.Random(8439)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200):
        for alen in (0, 1, 16, 17, 92):
            key, nonce, aad, pt = rnd.randbytes(32), rnd.randbytes(12), rnd.randbytes(alen), rnd.randbytes(n)
            ct = S.chapoly_seal(key, nonce, aad, pt)
            out = ctypes.create_string_buffer(max(n, 1))
            assert hs.hs_chapoly_open(key, nonce, aad, alen, ct, len(ct), out) == 1
            assert out.raw[:n] == pt
            bad = bytearray(ct)
            bad[rnd.randrange(len(bad))] ^= 1 << rnd.randrange(8)
            assert hs.hs_chapoly_open(key, nonce, aad, alen, bytes(bad), len(ct), out) == 0
            if alen:
                assert hs.hs_chapoly_open(key, nonce, aad[:-1] + bytes([aad[-1] ^ 1]), alen, ct, len(ct), out) == 0


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_context_builder_all_suites(hs, kdf, aead):
    """The host-side key_schedule_context plus the per-lane context builder (DHKEM decap, the suite's key
    schedule) against the Python reference, with info on both sides of the hashes' padding boundaries."""
    rnd = random.Random(1000 * kdf + aead)
    key, nonce, ksc = (ctypes.create_string_buffer(n) for n in (32, 12, 129))
    ksc_len = ctypes.c_uint32()
    for info_len in (0, 20, 111, 112, 200):
        sk, info, ske = rnd.randbytes(32), rnd.randbytes(info_len), rnd.randbytes(32)
        pk = H.x25519_base(sk)
        ss, enc = H.encap(ske, pk)
        nz = hs.hs_context(kdf, aead, sk, pk, info, info_len, enc, key, nonce, ksc, ctypes.byref(ksc_len))
        want_key, want_nonce = S.key_schedule(kdf, aead, ss, info)
        assert nz == 1 and ksc_len.value == 1 + 2 * S.nh(kdf)
        assert ksc.raw[:ksc_len.value] == S.key_schedule_context(kdf, aead, info)
        assert nonce.raw == want_nonce
        assert key.raw == want_key + bytes(32 - len(want_key))
    # an encapsulated key of a low-order point: the DH output is all zero
    assert hs.hs_context(kdf, aead, sk, pk, info, info_len, bytes(32), key, nonce, ksc, ctypes.byref(ksc_len)) == 0


def test_supported_ids(hs):
    for kdf, aead in S.SUITES:
        assert hs.hs_supported(0x20, kdf, aead) == 1
    for kem, kdf, aead in ((0x10, 1, 1), (0x21, 1, 1), (0x20, 0, 1), (0x20, 4, 1), (0x20, 1, 0), (0x20, 1, 4),
                           (0x20, 1, 0xFFFF)):
        assert hs.hs_supported(kem, kdf, aead) == 0


def test_create_suite_refuses_unsupported_ids_without_a_device():
    """jx_hpke_create_suite checks the ids before it looks for a device: KEM 0x0010 (P-256), KDF 4 and AEAD 4 are
    JX_HPKE_E_UNSUPPORTED with a reason, on any machine."""
    from janus_amd import hpke
    L = hpke._declare(hpke._lib.load())
    key = (ctypes.c_uint8 * 32)()
    for kem, kdf, aead in ((0x10, 1, 1), (0x20, 4, 1), (0x20, 1, 4)):
        h = ctypes.c_void_p()
        st = L.jx_hpke_create_suite(kem, kdf, aead, key, key, None, 0, 0, ctypes.byref(h))
        assert st == hpke.E_UNSUPPORTED == -2 and not h.value
        assert b"unsupported HPKE suite" in L.jx_hpke_last_error(None)
        with pytest.raises(hpke.UnsupportedSuite):
            hpke.HpkeOpener(bytes(32), bytes(32), b"", kem_id=kem, kdf_id=kdf, aead_id=aead)
