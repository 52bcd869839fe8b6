"""The lane-indexed Poly1305 and the ChaCha20 lane -> block map behind the wave-per-report ChaCha20Poly1305 open
(janus_amd/csrc/jx_chapoly_lanes.h), compiled for the host (tests/csrc/hosttest_chapoly_lanes.cpp) with the 64 lanes
as a loop, against tests/hpke_suites_ref.py (poly1305, _chapoly_tag, chacha20_xor, chapoly_open), which the
reference's RFC 9180 ChaCha vectors pin (tests/test_hpke_suites_ref.py)."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import pytest

import hpke_suites_ref as S
import math_vectors as V

HERE = os.path.dirname(os.path.abspath(__file__))
P = S.P1305
RMAX = S.R_CLAMP.to_bytes(16, "little")  # every bit the clamp permits
ONE = (1).to_bytes(16, "little")


@pytest.fixture(scope="module")
def cl():
    src = os.path.join(HERE, "csrc", "hosttest_chapoly_lanes.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_chapoly_lanes.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_field.h", "jx_sha256.h", "jx_sha_aes.h", "jx_hpke.h",
                                                                         "jx_ghash_lanes.h", "jx_chapoly.h",
                                                                         "jx_chapoly_lanes.h")]
    hdrs.append(os.path.join(HERE, "csrc", "jx_testops.h"))
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.cl_mul.argtypes = [vp, vp, vp]
    L.cl_tag_lanes.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp, vp]
    L.cl_chacha_lanes.argtypes = [vp, vp, vp, u64, vp]
    L.cl_open_lanes.argtypes = [vp, vp, vp, u64, vp, u64, u32, vp]
    return L


def _mac_input(aad: bytes, ct: bytes) -> bytes:
    return S._pad16(aad) + S._pad16(ct) + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def _tag(cl, key: bytes, aad: bytes, ct: bytes, rot: int = 0, exps=None):
    """(tag, the limb-wise sum of the 64 lane terms as an integer). The 32-bit limb sums must not have wrapped."""
    out = ctypes.create_string_buffer(16)
    limbs = (ctypes.c_uint32 * 5)()
    assert cl.cl_tag_lanes(key, aad, len(aad), ct, len(ct), rot, out, exps, limbs) == 1, "a limb sum of the combine wrapped"
    assert all(v <= 2**32 - 64 for v in limbs)
    return out.raw, sum(v << (26 * i) for i, v in enumerate(limbs))


def _limbs(x: int):
    return (ctypes.c_uint32 * 5)(*[(x >> (26 * i)) & (2**26 - 1) for i in range(5)])


def test_product_ranges(cl):
    """pl_mul over the ranges it documents: accumulator limbs < 2^27, multiplier limbs < 2^26 + 2^25. The value is
    the product mod p, and what comes back is carried (limb 1 < 2^26 + 2^10, the others < 2^26)."""
    cases = V.pl_mul_cases()
    assert len(cases) == 329
    out = (ctypes.c_uint32 * 5)()
    for h, m in cases:
        cl.cl_mul((ctypes.c_uint32 * 5)(*h), (ctypes.c_uint32 * 5)(*m), out)
        val = lambda a: sum(v << (26 * i) for i, v in enumerate(a))  # noqa: E731
        assert val(out) % P == val(h) * val(m) % P, (h, m)
        assert out[1] < 2**26 + 2**10 and all(out[i] < 2**26 for i in (0, 2, 3, 4)), list(out)


TOTALS = [1, 2, 63, 64, 65, 127, 128, 129, 200]  # MAC blocks, the length block included
TAILS = [1, 15, 16]


@pytest.mark.parametrize("total", TOTALS)
def test_lane_split_tag_equals_the_reference(cl, total):
    """The tag of the 64 emulated lanes equals poly1305 over the AEAD's MAC input, for every AAD / ciphertext split of
    every total at and around one, two and three strides, with a last ciphertext block of 1, 15 and 16 bytes (and a
    partial last AAD block for odd AAD block counts); the lane the combine starts from does not matter; the exponent
    each lane used is total - (its last block's index)."""
    rnd = random.Random(total)
    exps = (ctypes.c_uint32 * 64)()
    seen = 0
    for na in range(total):
        nc = total - 1 - na
        for tail in TAILS if nc else [16]:
            alen = 16 * na - (3 if na % 2 else 0)
            clen = 16 * nc - (16 - tail) if nc else 0
            key, aad, ct = rnd.randbytes(32), rnd.randbytes(alen), rnd.randbytes(clen)
            want = S.poly1305(key, _mac_input(aad, ct))
            for rot in ((0, 37) if na in (0, 6) else (0,)):
                assert _tag(cl, key, aad, ct, rot, exps)[0] == want, (na, nc, tail, rot)
            for j in range(64):
                own = list(range(j, total, 64))
                assert exps[j] == (total - own[-1] if own else 0), (total, j)
            seen += 1
    assert seen >= 1


def test_tag_equals_chapoly_tag_under_a_real_key(cl):
    """The same through the AEAD's own key derivation: _chapoly_tag(key, nonce, aad, ct) with the one-time key from
    keystream block 0."""
    rnd = random.Random(8439)
    for alen, clen in ((0, 0), (92, 3207), (1027, 1), (12, 114)):
        key, nonce, aad, ct = rnd.randbytes(32), rnd.randbytes(12), rnd.randbytes(alen), rnd.randbytes(clen)
        otk = S.chacha20_block(key, 0, nonce)[:32]
        assert _tag(cl, otk, aad, ct)[0] == S._chapoly_tag(key, nonce, aad, ct)


def test_key_edges(cl):
    """r at the clamp maximum, 0 and 1, s zero and all ones, on random and on all-0xFF messages of 64, 65 and 200
    blocks (the largest limbs in the lane sums and the largest carries through the combine: _tag asserts that no
    32-bit limb sum wrapped)."""
    rnd = random.Random(5)
    for r in (RMAX, bytes(16), ONE, rnd.randbytes(16)):
        for s in (bytes(16), b"\xff" * 16):
            for nblk in (64, 65, 200):
                for na in (0, 3):
                    aad, ct = b"\xff" * (16 * na), b"\xff" * (16 * (nblk - 1 - na))
                    for rot in (0, 21):
                        assert _tag(cl, r + s, aad, ct, rot)[0] == S.poly1305(r + s, _mac_input(aad, ct)), (r.hex(), nblk)
            aad, ct = rnd.randbytes(92), rnd.randbytes(16 * 130 + 7)
            assert _tag(cl, r + s, aad, ct)[0] == S.poly1305(r + s, _mac_input(aad, ct))


def test_sum_around_p_before_the_final_reduction(cl):
    """With r = 1 every power is 1 and the accumulator is the plain sum of the blocks, each with its 2^128 bit. No
    AAD and two ciphertext blocks make three MAC blocks: x + 0 + (32 << 64) + 3 * 2^128, so x chooses the sum. At
    p - 1 nothing is reduced, at p .. 2^130 - 1 the final reduction must subtract p, and the tag comes from the
    reduced value."""
    rnd = random.Random(6)
    for target in (P - 1, P, P + 1, 2**130 - 1):
        x = target - 3 * 2**128 - (32 << 64)
        assert 0 <= x < 2**128
        ct = x.to_bytes(16, "little") + bytes(16)
        for s in (bytes(16), b"\xff" * 16, rnd.randbytes(16)):
            tag, pre = _tag(cl, ONE + s, b"", ct)
            assert pre == target, hex(pre)
            assert tag == S.poly1305(ONE + s, _mac_input(b"", ct))
            assert tag == ((target % P + int.from_bytes(s, "little")) % 2**128).to_bytes(16, "little")
    # the same sums reached through a Horner step: 66 blocks, lanes 0 and 1 hold two blocks each
    ct = b"\xff" * (16 * 65)
    for s in (bytes(16), b"\xff" * 16):
        assert _tag(cl, ONE + s, b"", ct)[0] == S.poly1305(ONE + s, _mac_input(b"", ct))


def test_every_block_counts(cl):
    """A bit flipped in any single block of a 3-stride message, the length block included, changes the tag, and the
    tag still equals the reference (a wrong stride power would skip block 64 + 5 or weigh it like another)."""
    rnd = random.Random(7)
    key, aad, ct = rnd.randbytes(32), rnd.randbytes(92), rnd.randbytes(16 * 194 - 9)
    msg = _mac_input(aad, ct)
    nblk = len(msg) // 16
    assert nblk == 6 + 194 + 1
    good = _tag(cl, key, aad, ct)[0]
    assert good == S.poly1305(key, msg)
    for blk in (0, 5, 63, 64, 64 + 5, 127, 128, nblk - 2):
        a2, c2 = bytearray(aad), bytearray(ct)
        if blk < 6:
            a2[16 * blk + 3] ^= 0x10
        else:
            c2[16 * (blk - 6) + 3] ^= 0x10
        got = _tag(cl, key, bytes(a2), bytes(c2))[0]
        assert got == S.poly1305(key, _mac_input(bytes(a2), bytes(c2))) != good, blk
    # the length block: the same padded bytes under other lengths (one AAD byte fewer, a zero byte of ciphertext less)
    aad0, ct0 = aad[:-1] + b"\0", ct[:-1] + b"\0"
    base = _tag(cl, key, aad0, ct0)[0]
    assert base == S.poly1305(key, _mac_input(aad0, ct0))
    for a2, c2 in ((aad0[:-1], ct0), (aad0, ct0[:-1])):
        assert S._pad16(a2) + S._pad16(c2) == S._pad16(aad0) + S._pad16(ct0)
        got = _tag(cl, key, a2, c2)[0]
        assert got == S.poly1305(key, _mac_input(a2, c2)) != base


def test_the_aad_ciphertext_boundary_counts(cl):
    """The same bytes split at another place (one block moved from the AAD to the ciphertext) give another tag."""
    rnd = random.Random(9)
    key, data = rnd.randbytes(32), rnd.randbytes(16 * 70)
    tags = set()
    for na in (0, 1, 6, 64, 69, 70):
        aad, ct = data[:16 * na], data[16 * na:]
        t = _tag(cl, key, aad, ct)[0]
        assert t == S.poly1305(key, _mac_input(aad, ct))
        tags.add(t)
    assert len(tags) == 6


CLENS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 4160, 8191, 8192, 8193, 8263]  # one block per lane: a stride is 4096


@pytest.mark.parametrize("clen", CLENS)
def test_chacha_block_map(cl, clen):
    """The emulated wave's plaintext equals chacha20_xor from counter 1: up to one, two and three strides of 64
    blocks, a block more than one stride, and a 7-byte tail. Nothing is written past the plaintext's end."""
    rnd = random.Random(clen)
    key, nonce, ct = rnd.randbytes(32), rnd.randbytes(12), rnd.randbytes(clen)
    out = ctypes.create_string_buffer(b"\xa5" * (clen + 32), clen + 32)
    cl.cl_chacha_lanes(key, nonce, ct, clen, out)
    assert out.raw[:clen] == S.chacha20_xor(key, 1, nonce, ct)
    assert out.raw[clen:] == b"\xa5" * 32


def test_whole_emulated_open(cl):
    """Key derivation, tag, and decryption only under a good tag, as chapoly_wave_open orders them: what
    S.chapoly_open returns, for opens and for tampered inputs (whose plaintext region stays untouched)."""
    rnd = random.Random(11)
    for n, alen in ((0, 0), (1, 92), (64, 0), (1025, 16), (4097, 92), (8263, 1027)):
        key, nonce, aad, pt = rnd.randbytes(32), rnd.randbytes(12), rnd.randbytes(alen), rnd.randbytes(n)
        ct = S.chapoly_seal(key, nonce, aad, pt)
        out = ctypes.create_string_buffer(b"\xa5" * (n + 1), n + 1)
        for rot in (0, 50):
            assert cl.cl_open_lanes(key, nonce, aad, alen, ct, len(ct), rot, out) == 1
            assert out.raw[:n] == pt == S.chapoly_open(key, nonce, aad, ct) and out.raw[n:] == b"\xa5"
        flips = {0, n // 2, max(n - 1, 0), n, n + 15} | ({16 * 64 + 5} if n > 1100 else set()) | ({4096 + 9} if n > 4200 else set())
        for f in sorted(flips):
            bad = bytearray(ct)
            bad[f] ^= 1 << rnd.randrange(8)
            out = ctypes.create_string_buffer(b"\xa5" * (n + 1), n + 1)
            assert S.chapoly_open(key, nonce, aad, bytes(bad)) is None
            assert cl.cl_open_lanes(key, nonce, aad, alen, bytes(bad), len(ct), 0, out) == 0
            assert out.raw == b"\xa5" * (n + 1)
        if alen:
            bad_aad = aad[:-1] + bytes([aad[-1] ^ 0x80])
            assert cl.cl_open_lanes(key, nonce, bad_aad, alen, ct, len(ct), 0, out) == 0
            assert S.chapoly_open(key, nonce, bad_aad, ct) is None
        assert cl.cl_open_lanes(rnd.randbytes(32), nonce, aad, alen, ct, len(ct), 0, out) == 0


def test_stand_alone_program_builds_and_passes(tmp_path):
    """The same source as a program with its own main (the form that is run under -fsanitize=address,undefined):
    it replays a fixed subset of the cases above against the serial code of jx_chapoly.h and two constants of
    S.chapoly_seal, checked here against the reference again."""
    aad = bytes((7 * i + 1) & 255 for i in range(92))
    pt = bytes((31 * i + 5) & 255 for i in range(8263))
    sealed = S.chapoly_seal(bytes(range(32)), bytes(range(12)), aad, pt)
    src = open(os.path.join(HERE, "csrc", "hosttest_chapoly_lanes.cpp")).read()
    assert ", ".join("0x%02x" % b for b in sealed[-8:]) in src and ", ".join("0x%02x" % b for b in sealed[:8]) in src
    exe = str(tmp_path / "hosttest_chapoly_lanes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DJX_HOSTTEST_MAIN", "-o", exe, os.path.join(HERE, "csrc", "hosttest_chapoly_lanes.cpp")],
                   check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("all ok"), p.stdout
