"""The serial seal bodies behind the HPKE seal kernels (janus_amd/csrc/jx_hpke_seal.h), compiled for the host
(tests/csrc/hosttest_hpke_seal.cpp), against tests/hpke_suites_ref.py and oracle/hpke_oracle.py: encapsulation, the
key schedule, the one-message-per-lane AEAD seals of the three AEADs, and the ChaCha20-Poly1305 split of a long
message over the 64 lanes of a wave."""
from __future__ import annotations

import ctypes
import json
import os
import random
import subprocess

import pytest

import hpke_suites_ref as S
from oracle import hpke_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))
SHORT_LENGTHS = [0, 1, 15, 16, 17, 54, 255]
AAD_LENGTHS = [0, 1, 16, 60, 92]
SKE_A11 = bytes.fromhex("52c4a758a802cd8b936eceea314432798d5baf2d7e9235dc084ab1b9cfa2f736")  # RFC 9180 A.1.1 skEm


@pytest.fixture(scope="module")
def hq():
    src = os.path.join(HERE, "csrc", "hosttest_hpke_seal.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_hpke_seal.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in (
        "jx_field.h", "jx_sha256.h", "jx_sha_aes.h", "jx_hpke.h", "jx_sha512.h", "jx_chapoly.h", "jx_hpke_suites.h",
        "jx_ghash_lanes.h", "jx_chapoly_lanes.h", "jx_keyreg.h", "jx_hpke_seal.h")]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.hq_context.argtypes = [u32, u32, vp, vp, vp, u32, vp, vp, vp]
    L.hq_aead_seal.argtypes = [u32, vp, vp, vp, u64, vp, u64, vp]
    L.hq_aead_seal.restype = None
    L.hq_seal.argtypes = [u32, u32, vp, vp, vp, u32, vp, u64, vp, u64, vp, vp]
    L.hq_chapoly_lanes_seal.argtypes = [vp, vp, vp, u64, vp, u64, vp]
    L.hq_chapoly_lanes_seal.restype = None
    return L


def _seal(hq, kdf, aead, ske, pk, info, aad, pt):
    enc, ct = ctypes.create_string_buffer(32), ctypes.create_string_buffer(len(pt) + 16)
    ok = hq.hq_seal(kdf, aead, ske, pk, info, len(info), aad, len(aad), pt, len(pt), enc, ct)
    return ok, enc.raw, ct.raw


def test_rfc9180_a11(hq):
    """The device code on the CPU gives the vector's enc and first ciphertext from the vector's skEm."""
    v = next(x for x in json.load(open(os.path.join(HERE, "golden", "hpke_rfc9180.json")))["vectors"]
             if (x["kem_id"], x["kdf_id"], x["aead_id"], x["mode"]) == (0x20, 1, 1, 0))
    pk, info, enc = (bytes.fromhex(v[k]) for k in ("pkRm", "info", "enc"))
    e0 = v["encryptions"][0]
    assert H.x25519_base(SKE_A11) == enc
    ok, got_enc, got_ct = _seal(hq, 1, 1, SKE_A11, pk, info, bytes.fromhex(e0["aad"]), bytes.fromhex(e0["pt"]))
    assert ok == 1 and got_enc == enc and got_ct == bytes.fromhex(e0["ct"])


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_encap_and_key_schedule(hq, kdf, aead):
    rnd = random.Random(100 * kdf + aead)
    enc, key, nonce = (ctypes.create_string_buffer(n) for n in (32, 32, 12))
    cases = [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(3)]
    cases += [(bytes(32), rnd.randbytes(32)), (b"\xff" * 32, rnd.randbytes(32))]  # clamping
    sk = rnd.randbytes(32)
    cases.append((rnd.randbytes(32), sk[:31] + bytes([sk[31] | 0x80])))  # a recipient key with bit 255 set
    for ske, seed in cases:
        pk = H.x25519_base(seed) if seed[31] < 0x80 else seed
        info = rnd.randbytes(rnd.choice([0, 20, 111, 200]))
        assert hq.hq_context(kdf, aead, ske, pk, info, len(info), enc, key, nonce) == 1
        ss, want_enc = H.encap(ske, pk)
        want_key, want_nonce = S.key_schedule(kdf, aead, ss, info)
        assert enc.raw == want_enc and nonce.raw == want_nonce
        assert key.raw == want_key + bytes(32 - len(want_key))
    # a recipient key of low order: the DH output is all zero
    assert hq.hq_context(kdf, aead, rnd.randbytes(32), bytes(32), b"", 0, enc, key, nonce) == 0


@pytest.mark.parametrize("aead", [1, 2, 3])
def test_short_aead_seal(hq, aead):
    rnd = random.Random(aead)
    for n in SHORT_LENGTHS + [63, 64, 65, 129]:
        for alen in AAD_LENGTHS:
            key = rnd.randbytes(S.NK[aead])
            nonce, aad, pt = rnd.randbytes(12), rnd.randbytes(alen), rnd.randbytes(n)
            ct = ctypes.create_string_buffer(n + 16)
            hq.hq_aead_seal(aead, key + bytes(32 - len(key)), nonce, aad, alen, pt, n, ct)
            assert ct.raw == S.aead_seal(aead, key, nonce, aad, pt), (n, alen)


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_whole_seal_all_suites(hq, kdf, aead):
    rnd = random.Random(7 * kdf + aead)
    pk = H.x25519_base(rnd.randbytes(32))
    for n in (0, 17, 54):
        ske, info, aad, pt = rnd.randbytes(32), rnd.randbytes(20), rnd.randbytes(92), rnd.randbytes(n)
        ok, enc, ct = _seal(hq, kdf, aead, ske, pk, info, aad, pt)
        assert (ok, (enc, ct)) == (1, S.seal_base(kdf, aead, pk, info, aad, pt, ske))


def test_chapoly_lanes_split(hq):
    """Lane j owns ChaCha20 blocks j, j + 64, ... and their four Poly1305 blocks each: one ChaCha20 block per lane
    is 4096 bytes; 16,384 is a second group for every lane; the length block is a group's last piece (4095) or a group
    of its own (4096)."""
    rnd = random.Random(64)
    for n in (0, 1, 15, 16, 17, 48, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4112, 16383, 16384, 16401):
        for alen in (0, 1, 16, 60, 92, 1025):
            key, nonce, aad, pt = rnd.randbytes(32), rnd.randbytes(12), rnd.randbytes(alen), rnd.randbytes(n)
            ct = ctypes.create_string_buffer(n + 16)
            hq.hq_chapoly_lanes_seal(key, nonce, aad, alen, pt, n, ct)
            want = S.chapoly_seal(key, nonce, aad, pt) if n <= 4112 else None
            if want is None:  # the Python ChaCha20 is slow: the serial device code, itself checked above, stands in
                ser = ctypes.create_string_buffer(n + 16)
                hq.hq_aead_seal(3, key, nonce, aad, alen, pt, n, ser)
                want = ser.raw
            assert ct.raw == want, (n, alen)
