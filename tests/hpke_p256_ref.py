"""TEST INFRASTRUCTURE ONLY (a helper module, not a test) — pure-Python RFC 9180 base mode under
DHKEM(P-256, HKDF-SHA256) (KEM 0x0010) with the KDFs and AEADs of tests/hpke_suites_ref.py, from which the AEADs
and the HKDF pieces are imported. The curve arithmetic is affine on Python integers (pow(x, -1, p)), nothing
shared with the engine's projective Montgomery-form code. tests/test_hpke_p256_ref.py pins it by the six P-256
vectors the reference ships (tests/golden/hpke_rfc9180_p256.json: KDF 1 and 3, each with AEAD 1, 2 and 3).
"""
from __future__ import annotations

import hpke_suites_ref as S

KEM_P256 = 0x0010
P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
GX = 0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296
GY = 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5
G = (GX, GY)
KEM_SUITE = b"KEM" + KEM_P256.to_bytes(2, "big")


def on_curve(pt, b: int = B) -> bool:
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x - 3 * x + b)) % P == 0


def add(p1, p2):
    """Affine addition; None is the point at infinity."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k: int, pt):
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def neg(pt):
    return pt[0], (-pt[1]) % P


def encode(pt) -> bytes:
    """SerializePublicKey: the uncompressed SEC 1 encoding, 65 bytes."""
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def decode(enc: bytes):
    """DeserializePublicKey with the validation RFC 9180 §7.1.4 asks for; None when it fails."""
    if len(enc) != 65 or enc[0] != 4:
        return None
    pt = int.from_bytes(enc[1:33], "big"), int.from_bytes(enc[33:], "big")
    return pt if on_curve(pt) else None


def public_key(sk: bytes) -> bytes:
    return encode(mul(int.from_bytes(sk, "big"), G))


def lift_x(x: int, b: int = B):
    """A point with this x on y^2 = x^3 - 3x + b, or None (p = 3 mod 4)."""
    rhs = (x * x * x - 3 * x + b) % P
    y = pow(rhs, (P + 1) // 4, P)
    return (x, y) if y * y % P == rhs else None


def _extract_and_expand(dh: bytes, kem_context: bytes) -> bytes:
    eae_prk = S._extract(S.KDF_SHA256, b"", b"HPKE-v1" + KEM_SUITE + b"eae_prk" + dh)
    return S._expand(S.KDF_SHA256, eae_prk,
                     (32).to_bytes(2, "big") + b"HPKE-v1" + KEM_SUITE + b"shared_secret" + kem_context, 32)


def decap(enc: bytes, sk: bytes, pk: bytes) -> bytes | None:
    pt = decode(enc)
    if pt is None:
        return None
    dh = mul(int.from_bytes(sk, "big"), pt)
    if dh is None:
        return None
    return _extract_and_expand(dh[0].to_bytes(32, "big"), enc + pk)


def encap(ske: bytes, pk: bytes) -> tuple[bytes, bytes]:
    """Deterministic Encap with the ephemeral secret ske. Returns (shared_secret, enc)."""
    k = int.from_bytes(ske, "big")
    assert 0 < k < N
    enc = encode(mul(k, G))
    dh = mul(k, decode(pk))
    return _extract_and_expand(dh[0].to_bytes(32, "big"), enc + pk), enc


def suite_id(kdf: int, aead: int) -> bytes:
    return b"HPKE" + KEM_P256.to_bytes(2, "big") + kdf.to_bytes(2, "big") + aead.to_bytes(2, "big")


def key_schedule_context(kdf: int, aead: int, info: bytes) -> bytes:
    sid = suite_id(kdf, aead)
    return (b"\x00" + S._extract(kdf, b"", b"HPKE-v1" + sid + b"psk_id_hash") +
            S._extract(kdf, b"", b"HPKE-v1" + sid + b"info_hash" + info))


def key_schedule(kdf: int, aead: int, shared_secret: bytes, info: bytes) -> tuple[bytes, bytes]:
    """mode_base: (key, base_nonce)."""
    sid = suite_id(kdf, aead)
    ksc = key_schedule_context(kdf, aead, info)
    secret = S._extract(kdf, shared_secret, b"HPKE-v1" + sid + b"secret")

    def labeled_expand(label: bytes, n: int) -> bytes:
        return S._expand(kdf, secret, n.to_bytes(2, "big") + b"HPKE-v1" + sid + label + ksc, n)

    return labeled_expand(b"key", S.NK[aead]), labeled_expand(b"base_nonce", S.NN)


def open_base(kdf: int, aead: int, sk: bytes, pk: bytes, info: bytes, enc: bytes, aad: bytes, ct: bytes) -> bytes | None:
    ss = decap(enc, sk, pk)
    if ss is None:
        return None
    key, nonce = key_schedule(kdf, aead, ss, info)
    return S.aead_open(aead, key, nonce, aad, ct)


def seal_base(kdf: int, aead: int, pk: bytes, info: bytes, aad: bytes, pt: bytes, ske: bytes) -> tuple[bytes, bytes]:
    """Deterministic seal with the given ephemeral secret key (tests only). Returns (enc, ct)."""
    ss, enc = encap(ske, pk)
    key, nonce = key_schedule(kdf, aead, ss, info)
    return enc, S.aead_seal(aead, key, nonce, aad, pt)
