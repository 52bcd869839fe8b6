"""The device arithmetic headers (janus_amd/csrc/jx_field.h, jx_keccak.h, jx_sha256.h),
compiled for the host, against Python integers / hashlib / the oracle's Keccak."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import math_vectors as V
from math_vectors import M64, P64, P128, P25519, R, _model_take
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ht():
    src = os.path.join(HERE, "csrc", "hosttest.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_field.h", "jx_keccak.h", "jx_sha256.h",
                                                                         "jx_hpke.h", "jx_sha_aes.h", "jx_sample.h",
                                                                         "jx_flags.h")]
    hdrs.append(os.path.join(HERE, "csrc", "jx_testops.h"))
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.ht_f128.argtypes = [ctypes.c_int, vp, vp, vp]
    L.ht_reduce192.argtypes = [vp, vp]
    L.ht_reduce192_small.argtypes = [vp, vp]
    L.ht_wide_dot.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    L.ht_wacc_reduce.argtypes = [vp, vp]
    L.ht_x25519.argtypes = [vp, vp, vp]
    L.ht_fe.argtypes = [ctypes.c_int, vp, vp, vp]
    L.ht_aes128.argtypes = [vp, vp, vp]
    L.ht_ghash_mul.argtypes = [vp, vp, vp]
    L.ht_hmac32.argtypes = [vp, vp, ctypes.c_int, vp]
    L.ht_mont_lazy.argtypes = [vp, vp, vp]
    L.ht_f64.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    L.ht_f64.restype = ctypes.c_uint64
    L.ht_keccak_p12.argtypes = [vp]
    L.ht_sha256_16.argtypes = [vp, vp]
    L.ht_xof_block.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp, ctypes.c_int, vp]
    L.ht_aes128_t.argtypes = [ctypes.c_int, vp, vp, vp]
    L.ht_be_word_shift16.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.ht_be_word_shift16.restype = ctypes.c_uint32
    L.ht_wacc64_dot.argtypes = [vp, vp, ctypes.c_int]
    L.ht_wacc64_dot.restype = ctypes.c_uint64
    L.ht_reduce192_p64.argtypes = [vp]
    L.ht_reduce192_p64.restype = ctypes.c_uint64
    L.ht_ge_p128.argtypes = [vp]
    L.ht_ge_exact.argtypes = [vp]
    L.ht_ge_p64.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.ht_ge_screen_max.argtypes = [vp, ctypes.c_int]
    L.ht_ge_screen_max.restype = ctypes.c_uint32
    L.ht_sample64.argtypes = [ctypes.c_int, vp, vp]
    L.ht_sample2_f128.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, vp, vp]
    L.ht_bx_sample128.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, vp]
    L.ht_bx_sample128.restype = ctypes.c_uint32
    L.ht_xof_stream128.argtypes = [vp, ctypes.c_uint32, vp]
    L.ht_xof_stream128.restype = ctypes.c_uint32
    return L


def _b(x, n=16):
    return ctypes.create_string_buffer(x.to_bytes(n, "little"), n)


def f128(L, op, a, b=None):
    out = ctypes.create_string_buffer(16)
    L.ht_f128(op, _b(a), _b(b) if b is not None else None, out)
    return int.from_bytes(out.raw, "little")


def test_field128_add_sub(ht):
    vals = V.field128_add_sub_values()
    for a in vals[:60]:
        for b in vals[:60]:
            assert f128(ht, 0, a, b) == (a + b) % P128
            assert f128(ht, 1, a, b) == (a - b) % P128


def test_field128_montgomery(ht):
    rinv = pow(R, P128 - 2, P128)
    vals = V.field128_mont_values()
    for a in vals[:90]:
        for b in vals[:90]:
            assert f128(ht, 2, a, b) == a * b * rinv % P128
    for a in vals:
        assert f128(ht, 3, a) == a * R % P128
        assert f128(ht, 4, a) == a * rinv % P128


def test_field128_mont_lazy_bound(ht):
    rinv = pow(R, P128 - 2, P128)
    for a, b in V.mont_lazy_cases():
        out = (ctypes.c_uint64 * 3)()
        ht.ht_mont_lazy(_b(a), _b(b), out)
        v = out[0] + (out[1] << 64) + (out[2] << 128)
        assert v < 2 * P128 and v % P128 == a * b * rinv % P128


def test_reduce192(ht):
    for v in V.reduce192_cases():
        w = (ctypes.c_uint64 * 3)(v & (2**64 - 1), (v >> 64) & (2**64 - 1), v >> 128)
        out = ctypes.create_string_buffer(16)
        ht.ht_reduce192(w, out)
        assert int.from_bytes(out.raw, "little") == v % P128, hex(v)


def test_reduce192_small(ht):
    """The branch-free reduction of the output-share truncation (top word < 2^32)."""
    for v in V.reduce192_small_cases():
        w = (ctypes.c_uint64 * 3)(v & (2**64 - 1), (v >> 64) & (2**64 - 1), v >> 128)
        out = ctypes.create_string_buffer(16)
        ht.ht_reduce192_small(w, out)
        assert int.from_bytes(out.raw, "little") == v % P128, hex(v)


def test_field64(ht):
    vals = V.field64_values()
    for a in vals[:70]:
        for b in vals[:70]:
            assert ht.ht_f64(0, a, b) == (a + b) % P64
            assert ht.ht_f64(1, a, b) == (a - b) % P64
            assert ht.ht_f64(2, a, b) == a * b % P64


def test_keccak_p12_matches_oracle(ht):
    rnd = random.Random(6)
    for _ in range(10):
        st = [rnd.getrandbits(64) for _ in range(25)]
        arr = (ctypes.c_uint64 * 25)(*st)
        ht.ht_keccak_p12(arr)
        assert list(arr) == O.keccak_p1600(st, 12)


def test_sha256_16(ht):
    for _ in range(20):
        rid = os.urandom(16)
        out = ctypes.create_string_buffer(32)
        ht.ht_sha256_16(rid, out)
        assert out.raw == hashlib.sha256(rid).digest()


@pytest.mark.parametrize("usage,binder", [(1, b"\x01"), (2, b"\x01\x01"), (5, b"\x01" + bytes(range(16))),
                                          (6, bytes(range(32))), (3, b"\x01")])
def test_xof_block_builder(ht, usage, binder):
    """blk_xof_prefix + pad == the oracle's XofTurboShake128 message framing."""
    seed = os.urandom(16)
    for algo in (0, 2, 0xFFFF1003):
        w = (ctypes.c_uint32 * 42)()
        ht.ht_xof_block(algo, usage, seed, binder, len(binder), w)
        dst = bytes([8, 0]) + algo.to_bytes(4, "big") + usage.to_bytes(2, "big")
        msg = bytes([8]) + dst + seed + binder
        blk = bytearray(msg) + b"\x01" + bytes(168 - len(msg) - 1)
        blk[-1] ^= 0x80
        assert b"".join(x.to_bytes(4, "little") for x in w) == bytes(blk)


def test_wacc_reduce_columns(ht):
    """wacc_reduce's straight-line fold on raw column sums: every column up to 2^63 (the kernels' bound:
    <= 5 * 512 limb products < 2^52 per column between normalisations), zeros, and random mixes."""
    for cols in V.wacc_reduce_cases():
        out = ctypes.create_string_buffer(16)
        ht.ht_wacc_reduce((ctypes.c_uint64 * 9)(*cols), out)
        assert int.from_bytes(out.raw, "little") == sum(c << (26 * s) for s, c in enumerate(cols)) % P128, cols


@pytest.mark.parametrize("n,norm", [(1, 0), (91, 0), (700, 0), (2000, 512), (5000, 512)])
def test_wide_dot_accumulator(ht, n, norm):
    """The FLP wire sums: sum x_k c_k mod p with 26-bit limbs and deferred reduction,
    including worst-case operands (p - 1) at the term counts the kernel allows."""
    for xs, cs in V.wide_dot_operands(n):
        xb = b"".join(x.to_bytes(16, "little") for x in xs)
        cb = b"".join(c.to_bytes(16, "little") for c in cs)
        out = ctypes.create_string_buffer(16)
        ht.ht_wide_dot(xb, cb, n, norm, out)
        assert int.from_bytes(out.raw, "little") == sum(x * c for x, c in zip(xs, cs)) % P128


# ---------------------------------------------------------------------------- HPKE primitives (jx_hpke.h)
def _buf32(x: int) -> bytes:
    return x.to_bytes(32, "little")


def test_fe25519_ops(ht):
    from oracle import hpke_oracle as H  # noqa: F401
    vals = V.fe25519_values()
    out = ctypes.create_string_buffer(32)
    for a in vals:
        for b in vals[:12]:
            for op, want in ((0, a * b), (2, a - b)):
                ht.ht_fe(op, _buf32(a), _buf32(b), out)
                assert int.from_bytes(out.raw, "little") == want % P25519, (op, a, b)
        ht.ht_fe(1, _buf32(a), _buf32(0), out)
        assert int.from_bytes(out.raw, "little") == a * a % P25519
        ht.ht_fe(4, _buf32(a), _buf32(0), out)
        assert int.from_bytes(out.raw, "little") == a * 121665 % P25519
        if a:
            ht.ht_fe(3, _buf32(a), _buf32(0), out)
            assert int.from_bytes(out.raw, "little") == pow(a, P25519 - 2, P25519)


def test_fe25519_reduction_bounds(ht):
    """The product reduction on the loosest inputs the ladder makes (every limb up to 2^28 - 1): the value is the
    product mod p, and the output limbs stay within what fe_sub's 2p needs (limb 0 <= 2^27 - 38, limbs 1..8 <=
    2^27 - 2, limb 9 <= 2^22 - 2) and small enough that a sum or difference of two stays under 2^28."""
    L = ctypes.c_uint32 * 10
    ht.ht_fe_limbs.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    cases = V.fe25519_loose_limb_cases()

    def val(v):
        return sum(x << (26 * i) for i, x in enumerate(v))

    for i, a in enumerate(cases):
        b = cases[(7 * i + 3) % len(cases)]
        for op in (0, 1, 4):
            out = L()
            ht.ht_fe_limbs(op, L(*a), L(*b), out)
            want = val(a) * (val(b) if op == 0 else val(a) if op == 1 else 121665) % P25519
            assert val(out) % P25519 == want, (op, a, b)
            assert out[0] <= (1 << 27) - 38 and all(x <= (1 << 27) - 2 for x in out[1:9]) and out[9] <= (1 << 22) - 2
            assert max(out) < (1 << 26) + (1 << 17), list(out)


def test_x25519_vs_oracle(ht):
    from oracle import hpke_oracle as H
    out = ctypes.create_string_buffer(32)
    for k, u in V.x25519_cases():
        ht.ht_x25519(k, u, out)
        assert out.raw == H.x25519(k, u)


def test_aes_ghash_hmac_vs_oracle(ht):
    import hashlib
    import hmac as hm

    from oracle import hpke_oracle as H
    rnd = random.Random(3)
    out = ctypes.create_string_buffer(32)
    for _ in range(20):
        key, blk = rnd.randbytes(16), rnd.randbytes(16)
        ht.ht_aes128(key, blk, out)
        assert out.raw[:16] == H.aes128_encrypt_block(H.aes128_expand(key), blk)
        x, h = rnd.randbytes(16), rnd.randbytes(16)
        ht.ht_ghash_mul(x, h, out)
        want = H._ghash_mul(int.from_bytes(x, "big"), int.from_bytes(h, "big")).to_bytes(16, "big")
        assert out.raw[:16] == want
    for n in (0, 1, 23, 51, 55, 56, 63, 64, 92, 95, 119):
        key, msg = rnd.randbytes(32), rnd.randbytes(n)
        ht.ht_hmac32(key, msg, n, out)
        assert out.raw == hm.new(key, msg, hashlib.sha256).digest(), n


# ---- XofHmacSha256Aes128 / Field64 multiproof building blocks (jx_sha_aes.h, jx_field.h)

def test_aes128_ttable_fips197(ht):
    """T-table AES (both key-schedule forms) against the FIPS 197 Appendix C.1 vector and the oracle."""
    from oracle import oracle as O
    key, pt = bytes.fromhex("000102030405060708090a0b0c0d0e0f"), bytes.fromhex("00112233445566778899aabbccddeeff")
    rnd = random.Random(9)
    cases = [(key, pt, bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a"))]
    for _ in range(20):
        k, m = rnd.randbytes(16), rnd.randbytes(16)
        cases.append((k, m, O.aes128_encrypt(k, m)))
    for k, m, want in cases:
        for otf in (0, 1):
            out = ctypes.create_string_buffer(16)
            ht.ht_aes128_t(otf, k, m, out)
            assert out.raw == want, (otf, k.hex())


def test_be_word_shift16(ht):
    rnd = random.Random(3)
    for _ in range(100):
        lo, hi = rnd.getrandbits(32), rnd.getrandbits(32)
        b = lo.to_bytes(4, "little") + hi.to_bytes(4, "little")
        assert ht.ht_be_word_shift16(lo, hi) == int.from_bytes(b[2:6], "big")


@pytest.mark.parametrize("n", [1, 91, 1023, 1024, 1025, 3000])
def test_wacc64_dot(ht, n):
    xs, cs = V.wacc64_dot_operands(n)
    ax = (ctypes.c_uint64 * n)(*xs)
    ac = (ctypes.c_uint64 * n)(*cs)
    assert ht.ht_wacc64_dot(ax, ac, n) == sum(x * c for x, c in zip(xs, cs)) % P64


def test_reduce192_p64(ht):
    for w in V.reduce192_p64_cases():
        a = (ctypes.c_uint64 * 3)(*w)
        assert ht.ht_reduce192_p64(a) == (w[0] + (w[1] << 64) + (w[2] << 128)) % P64


# ---------------------------------------------------------------------------- ">= p" and rejection sampling
# (jx_field.h ge_p128 / ge_p64, jx_sample.h): the decode bounds and the skip branches that a real stream
# reaches once in 2^32 (Field64) or 2^59 (Field128) elements, on hand-built values and Keccak states.

@pytest.mark.parametrize("fn", ["ht_ge_p128", "ht_ge_exact"])
def test_ge_p128_exact(ht, fn):
    """ge_p128 (f128, the samplers and the verifier decode) and ge_exact (uint4, the leader's decode of its
    explicit input share) against Python integers."""
    for v in V.ge_p128_values():
        assert getattr(ht, fn)(_b(v)) == int(v >= P128), hex(v)


def test_ge_p64_exact(ht):
    for v in V.ge_p64_values():
        assert ht.ht_ge_p64(v & 0xFFFFFFFF, v >> 32) == int(v >= P64), hex(v)


def test_ge_screen_is_a_superset_and_survives_the_running_max(ht):
    """ge_screen == 0xFFFFFFFF for every v >= p128 (it may also fire just below p), and the per-block running
    max still says so with any number of smaller elements before and after."""
    ge, windows, quiet = V.ge_screen_cases()
    assert len(ge) >= 400 and len(windows) == 120
    for v in ge:
        assert ht.ht_ge_screen_max(_b(v), 1) == 0xFFFFFFFF, hex(v)
    for v in V.GE_SCREEN_QUIET:  # far below p: quiet
        assert ht.ht_ge_screen_max(_b(v), 1) != 0xFFFFFFFF, hex(v)
    for elems in windows:
        buf = ctypes.create_string_buffer(b"".join(e.to_bytes(16, "little") for e in elems), 128)
        assert ht.ht_ge_screen_max(buf, 8) == 0xFFFFFFFF
    quiet = ctypes.create_string_buffer(b"".join(e.to_bytes(16, "little") for e in quiet), 128)
    assert ht.ht_ge_screen_max(quiet, 8) != 0xFFFFFFFF


def _u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


@pytest.mark.parametrize("n", [1, 5])
def test_sample64_skips_rejected_chunks(ht, n):
    cases = V.sample64_cases(n)
    assert len(cases) == 30
    permuted = 0
    for rej, st in cases[:-1]:
        want, st_after, _ = _model_take(st, 8, n, P64, whole_chunks=21)
        buf, out = _u64s(st), (ctypes.c_uint64 * 5)()
        ht.ht_sample64(n, buf, out)
        assert list(out)[:n] == want, (n, rej)
        assert list(buf) == st_after, (n, rej)
        permuted += st_after != st
    assert permuted >= 2
    # the largest element is taken, not skipped
    st = cases[-1][1]
    assert st[0] == P64 - 1
    buf, out = _u64s(st), (ctypes.c_uint64 * 5)()
    ht.ht_sample64(n, buf, out)
    assert out[0] == P64 - 1


@pytest.mark.parametrize("cnt", [1, 2])
def test_sample2_f128_fast_flags_and_slow_skips(ht, cnt):
    FLAG_SLOW, other = 4, 16
    cases = V.sample2_cases(cnt)
    assert len(cases) == 40
    for rej, st in cases:
        chunks = [st[2 * k] | (st[2 * k + 1] << 64) for k in range(10)]
        # fast: the first cnt chunks as they are, FLAG_SLOW exactly when one of them is >= p
        buf, out, flags = _u64s(st), ctypes.create_string_buffer(32), ctypes.c_uint32(other)
        ht.ht_sample2_f128(buf, cnt, 0, out, ctypes.byref(flags))
        got = [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(2)]
        assert got[:cnt] == chunks[:cnt]
        assert flags.value == other | (FLAG_SLOW if any(c >= P128 for c in chunks[:cnt]) else 0), (rej, cnt)
        assert list(buf) == st
        # slow: the first cnt accepted chunks
        want, st_after, _ = _model_take(st, 16, cnt, P128, whole_chunks=10)
        buf, out, flags = _u64s(st), ctypes.create_string_buffer(32), ctypes.c_uint32(other)
        ht.ht_sample2_f128(buf, cnt, 1, out, ctypes.byref(flags))
        got = [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(2)]
        assert got[:cnt] == want, (rej, cnt)
        assert flags.value == other and list(buf) == st_after


def test_bx_sample128_rejection_before_a_block_boundary(ht):
    """The slow path's byte stream: a rejected element (or two in a row) whose successor straddles the
    168-byte block boundary, at several alignments of the stream. Rejections are placed in the first block
    only: what the permutation leaves in the next block cannot be chosen, so the straddling element itself
    and those after it are always below p."""
    cases = V.bx_sample_cases()
    assert len(cases) == 36
    # (first byte, elements to take, indices of the rejected elements, the state): elements are 16 bytes from byte
    # pos0; the element at index e covers bytes pos0 + 16 e ..
    for pos0, nelem, rej_at, st in cases[:-1]:
        want, st_after, pos_after = _model_take(st, 16, nelem, P128, pos=pos0)
        buf, out = _u64s(st), ctypes.create_string_buffer(16 * nelem)
        pos = ht.ht_bx_sample128(buf, pos0, nelem, out)
        got = [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(nelem)]
        assert got == want, (pos0, rej_at)
        assert pos == pos_after and list(buf) == st_after
    # no rejection at all: the eleventh element is the straddling one (bytes 160..167 and 0..7 of the next block)
    st = cases[-1][3]
    assert st[20] == M64
    want, st_after, pos_after = _model_take(st, 16, 12, P128)
    buf, out = _u64s(st), ctypes.create_string_buffer(16 * 12)
    assert ht.ht_bx_sample128(buf, 0, 12, out) == pos_after
    assert [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(12)] == want


def test_keccak_p1600_inverse_round_trip():
    """math_vectors.keccak_p1600_inverse, which builds the xof_stream128 states, against the oracle's permutation,
    in both directions."""
    rnd = random.Random(1600)
    states = [[0] * 25, [M64] * 25] + [[rnd.getrandbits(64) for _ in range(25)] for _ in range(20)]
    for st in states:
        assert V.keccak_p1600_inverse(O.keccak_p1600(st, 12), 12) == st
        assert O.keccak_p1600(V.keccak_p1600_inverse(st, 12), 12) == st
    st = states[2]  # two blocks back, as the states of the second block pair are built; other round counts
    back2 = V.keccak_p1600_inverse(V.keccak_p1600_inverse(st, 12), 12)
    assert back2 != st and O.keccak_p1600(O.keccak_p1600(back2, 12), 12) == st
    for rounds in (1, 2, 24):
        assert V.keccak_p1600_inverse(O.keccak_p1600(st, rounds), rounds) == st


def test_xof_stream128_rejects_at_every_position(ht):
    """xof_stream128 (jx_sample.h), the sampler of Prio3.shard's Field128 streams, on states built backwards through
    the permutation so that a rejected encoding sits at a chosen chunk of the first, second or third block:
    emit is called for k = 0 .. n - 1 once each and in order, with the byte-stream model's values."""
    cases = V.xof_stream_cases()
    assert len(cases) == 55 and max(n for _, n, _ in cases) <= 48
    for label, n, st in cases:
        want, _, _ = _model_take(st, 16, n, P128)
        buf, out = _u64s(st), ctypes.create_string_buffer(b"\xa5" * (16 * 49), 16 * 49)
        calls = ht.ht_xof_stream128(buf, n, out)
        assert calls == n, (label, hex(calls))
        assert [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(n)] == want, label
        assert out.raw[16 * n:] == b"\xa5" * (16 * (49 - n)), label
        assert list(buf) == st  # the operation works on a copy
