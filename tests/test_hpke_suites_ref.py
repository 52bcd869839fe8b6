"""Pins tests/hpke_suites_ref.py (the checker of the suite kernels) by the RFC 9180 vectors the reference ships
for the X25519 suites (tests/golden/hpke_rfc9180_suites.json, from core/src/test-vectors.json): HKDF-SHA256 and
HKDF-SHA512, each with AES-128-GCM, AES-256-GCM and ChaCha20Poly1305. HKDF-SHA384 has no vector offline."""
from __future__ import annotations

import json
import os
import random
import shutil
import subprocess

import pytest

import hpke_suites_ref as S
from oracle import hpke_oracle as H

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hpke_rfc9180_suites.json")
VECTORS = json.load(open(GOLDEN))["vectors"]


def test_fixture_holds_the_six_x25519_suites():
    assert sorted((v["kdf_id"], v["aead_id"]) for v in VECTORS) == [(1, 1), (1, 2), (1, 3), (3, 1), (3, 2), (3, 3)]
    assert all(v["kem_id"] == 0x20 and v["mode"] == 0 for v in VECTORS)


@pytest.mark.parametrize("v", VECTORS, ids=lambda v: f"kdf{v['kdf_id']}-aead{v['aead_id']}")
def test_rfc9180_vector(v):
    kdf, aead = v["kdf_id"], v["aead_id"]
    sk, pk, enc, info = (bytes.fromhex(v[k]) for k in ("skRm", "pkRm", "enc", "info"))
    e = v["encryptions"][0]
    aad, ct, pt = (bytes.fromhex(e[k]) for k in ("aad", "ct", "pt"))
    assert len(info) == 20 and len(aad) == 7 and len(pt) == 29
    assert H.x25519_base(sk) == pk
    ss = H.decap(enc, sk, pk)
    key, nonce = S.key_schedule(kdf, aead, ss, info)
    assert nonce.hex() == v["base_nonce"] == e["nonce"] and len(key) == S.NK[aead]
    assert S.aead_seal(aead, key, nonce, aad, pt) == ct
    assert S.open_base(kdf, aead, sk, pk, info, enc, aad, ct) == pt
    # the suite id binds: no other suite opens it
    for other in S.SUITES:
        if other != (kdf, aead):
            assert S.open_base(*other, sk, pk, info, enc, aad, ct) is None


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_seal_open_round_trip(kdf, aead):
    rnd = random.Random(100 * kdf + aead)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    for n in (0, 1, 16, 65, 200):
        info, aad, pt = rnd.randbytes(n % 40), rnd.randbytes(n % 19), rnd.randbytes(n)
        enc, ct = S.seal_base(kdf, aead, pk, info, aad, pt, rnd.randbytes(32))
        assert len(ct) == n + 16
        assert S.open_base(kdf, aead, sk, pk, info, enc, aad, ct) == pt
        bad = bytearray(ct)
        bad[rnd.randrange(len(bad))] ^= 0x10
        assert S.open_base(kdf, aead, sk, pk, info, enc, aad, bytes(bad)) is None
        assert S.open_base(kdf, aead, sk, pk, info, enc, aad + b"x", ct) is None
    assert len(S.key_schedule_context(kdf, aead, b"info")) == 1 + 2 * S.nh(kdf)


def test_default_suite_equals_the_oracle():
    rnd = random.Random(5)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    info, aad, pt, ske = H.dap_info(), rnd.randbytes(92), rnd.randbytes(70), rnd.randbytes(32)
    assert S.seal_base(1, 1, pk, info, aad, pt, ske) == H.seal_base(pk, info, aad, pt, ske)


def test_rfc8439_poly1305_and_aead_vectors():
    # RFC 8439 §2.5.2
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert S.poly1305(key, b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"
    # RFC 8439 §2.8.2
    key = bytes(range(0x80, 0xA0))
    nonce = bytes.fromhex("070000004041424344454647")
    aad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
          b"sunscreen would be it.")
    out = S.chapoly_seal(key, nonce, aad, pt)
    assert out[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert out[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert S.chapoly_open(key, nonce, aad, out) == pt


def test_fips197_aes256_vector():
    # FIPS 197 Appendix C.3
    key = bytes(range(32))
    ct = S.aes_encrypt_block(S.aes256_expand(key), bytes.fromhex("00112233445566778899aabbccddeeff"))
    assert ct.hex() == "8ea2b7ca516745bfeafc49904b496089"


def _openssl(args: list[str], data: bytes) -> bytes:
    return subprocess.run(["openssl"] + args, input=data, capture_output=True, check=True).stdout


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl binary on this machine")
def test_multiblock_keystreams_against_openssl():
    """200 bytes (more than three ChaCha20 blocks, more than twelve AES blocks) of keystream against the openssl
    binary: enc -chacha20 takes a 16-byte iv = little-endian 32-bit counter || 12-byte nonce."""
    rnd = random.Random(8439)
    key, nonce = rnd.randbytes(32), rnd.randbytes(12)
    zeros = bytes(200)
    try:
        got = _openssl(["enc", "-chacha20", "-K", key.hex(), "-iv", ((1).to_bytes(4, "little") + nonce).hex()], zeros)
    except subprocess.CalledProcessError:
        pytest.skip("this openssl has no chacha20")
    assert got == S.chacha20_xor(key, 1, nonce, zeros)
    icb = nonce + (2).to_bytes(4, "big")
    got = _openssl(["enc", "-aes-256-ctr", "-K", key.hex(), "-iv", icb.hex()], zeros)
    assert got == S.aes_ctr(S.aes256_expand(key), icb, zeros)
