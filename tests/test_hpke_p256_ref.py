"""Pins tests/hpke_p256_ref.py (the checker of the P-256 kernels) by the RFC 9180 vectors the reference ships
for DHKEM(P-256, HKDF-SHA256) (tests/golden/hpke_rfc9180_p256.json, from core/src/test-vectors.json): HKDF-SHA256
and HKDF-SHA512, each with AES-128-GCM, AES-256-GCM and ChaCha20Poly1305."""
from __future__ import annotations

import json
import os
import random

import pytest

import hpke_p256_ref as R
import hpke_suites_ref as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hpke_rfc9180_p256.json")
VECTORS = json.load(open(GOLDEN))["vectors"]


def test_fixture_holds_the_six_p256_suites():
    assert sorted((v["kdf_id"], v["aead_id"]) for v in VECTORS) == [(1, 1), (1, 2), (1, 3), (3, 1), (3, 2), (3, 3)]
    assert all(v["kem_id"] == 0x10 and v["mode"] == 0 for v in VECTORS)


def test_curve_constants():
    assert R.on_curve(R.G) and R.mul(R.N, R.G) is None and R.mul(R.N - 1, R.G) == R.neg(R.G)
    assert R.add(R.G, R.G) == R.mul(2, R.G) and R.add(R.G, R.neg(R.G)) is None
    assert R.P % 4 == 3


@pytest.mark.parametrize("v", VECTORS, ids=lambda v: f"kdf{v['kdf_id']}-aead{v['aead_id']}")
def test_rfc9180_vector(v):
    kdf, aead = v["kdf_id"], v["aead_id"]
    sk, pk, enc, info = (bytes.fromhex(v[k]) for k in ("skRm", "pkRm", "enc", "info"))
    e = v["encryptions"][0]
    aad, ct, pt = (bytes.fromhex(e[k]) for k in ("aad", "ct", "pt"))
    assert len(sk) == 32 and len(pk) == 65 and len(enc) == 65
    assert R.public_key(sk) == pk
    ss = R.decap(enc, sk, pk)
    key, nonce = R.key_schedule(kdf, aead, ss, info)
    assert nonce.hex() == v["base_nonce"] == e["nonce"] and len(key) == S.NK[aead]
    assert S.aead_seal(aead, key, nonce, aad, pt) == ct
    assert R.open_base(kdf, aead, sk, pk, info, enc, aad, ct) == pt
    for other in S.SUITES:  # the suite id binds: no other suite opens it
        if other != (kdf, aead):
            assert R.open_base(*other, sk, pk, info, enc, aad, ct) is None


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_seal_open_round_trip(kdf, aead):
    rnd = random.Random(100 * kdf + aead)
    sk = rnd.randrange(1, R.N).to_bytes(32, "big")
    pk = R.public_key(sk)
    for n in (0, 1, 65):
        info, aad, pt = rnd.randbytes(n % 40), rnd.randbytes(n % 19), rnd.randbytes(n)
        enc, ct = R.seal_base(kdf, aead, pk, info, aad, pt, rnd.randrange(1, R.N).to_bytes(32, "big"))
        assert len(enc) == 65 and len(ct) == n + 16
        assert R.open_base(kdf, aead, sk, pk, info, enc, aad, ct) == pt
        bad = bytearray(ct)
        bad[rnd.randrange(len(bad))] ^= 0x10
        assert R.open_base(kdf, aead, sk, pk, info, enc, aad, bytes(bad)) is None
        assert R.open_base(kdf, aead, sk, pk, info, enc, aad + b"x", ct) is None
        off = bytearray(enc)
        off[40] ^= 1  # y with one bit flipped: not on the curve
        assert R.decode(bytes(off)) is None and R.open_base(kdf, aead, sk, pk, info, bytes(off), aad, ct) is None
        assert R.open_base(kdf, aead, sk, pk, info, enc[:64], aad, ct) is None
    assert len(R.key_schedule_context(kdf, aead, b"info")) == 1 + 2 * S.nh(kdf)
