"""Operand tables and case generators of the arithmetic tests, one set for both builds of the device headers
(janus_amd/csrc/jx_*.h): the g++ host libraries (test_device_math_host.py, test_coef_limbs_host.py,
test_hpke_p256_host.py, test_chapoly_lanes_host.py) and the gfx950 harness (test_gpu_device_math.py). A plain
module: every generator seeds its own random.Random, so each call returns the same cases."""
from __future__ import annotations

import random

from oracle import oracle as O

P128 = 2**128 - 28 * 2**64 + 1
P64 = 2**64 - 2**32 + 1
R = 2**128
P25519 = 2**255 - 19
P1305 = 2**130 - 5

# ---------------------------------------------------------------------------- Field128 / Field64 operands
EDGE = [0, 1, 2, P128 - 1, P128 - 2, 2**127, 2**64, 2**64 - 1, 28 * 2**64 - 1, P128 // 2,
        # all-ones 32-bit limbs: every column sum and REDC add carries (mont128's carry chains)
        0xFFFFFFFFFFFFFFE3FFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFE3FFFFFFFF00000000, 2**96 - 1, 2**32 - 1,
        0xFFFFFFFF00000000FFFFFFFF, 0xFFFFFFFFFFFFFFE300000000FFFFFFFF]

EDGE64 = [0, 1, P64 - 1, P64 - 2, 2**32, 2**32 - 1, 2**63]

M64 = 2**64 - 1
HI128 = 0xFFFFFFFFFFFFFFE4  # high half of p128 (its low half is 1)
BOUND128 = [P128 - 1, P128, P128 + 1, (HI128 << 64) | 2**32, (HI128 + 1) << 64, ((HI128 - 1) << 64) | M64,
            2**128 - 1, HI128 << 64, (HI128 << 64) | 2, (HI128 << 64) | 2**63, 0, 1, 2**64, 2**127,
            ((HI128 - 1) << 64) | 1, (0xFFFFFFFF << 96) | 1, (0xFFFFFFFFFFFFFFFF << 64)]
BOUND64 = [P64 - 1, P64, P64 + 1, 0xFFFFFFFF80000000, 0xFFFFFFFEFFFFFFFF, M64, 0xFFFFFFFF00000000, 0xFFFFFFFF00010000,
           0xFFFFFFFE00000001, 0, 1, 2**32, 2**63]
GE64 = [P64, M64, 0xFFFFFFFF80000000, P64 + 1, 0xFFFFFFFF00010000]
GE128 = [P128, P128 + 1, 2**128 - 1, (HI128 << 64) | 2**32, (HI128 + 1) << 64]


def field128_add_sub_values():
    rnd = random.Random(1)
    return EDGE + [rnd.randrange(P128) for _ in range(200)]


def field128_mont_values():
    rnd = random.Random(2)
    return EDGE + [rnd.randrange(P128) for _ in range(300)]


def mont_lazy_cases():
    rnd = random.Random(3)
    return [(rnd.choice(EDGE + [rnd.randrange(P128)]), rnd.randrange(P128)) for _ in range(500)]


def reduce192_cases():
    rnd = random.Random(4)
    return [0, 1, P128, 2**192 - 1, 2**128, 2**128 - 1, 64 * 2 * P128] + [rnd.randrange(2**192) for _ in range(500)]


def reduce192_small_cases():
    rnd = random.Random(14)
    cases = [0, 1, P128 - 1, P128, 2**128 - 1, 2**128, 2**160 - 1, 2**128 + 2**64 - 1, (2**32 - 1) << 128,
             ((2**32 - 1) << 128) + 2**128 - 1, ((2**32 - 1) << 128) | 1, P128 * 255, 2**136 - 1]
    cases += [rnd.randrange(2**(128 + rnd.randrange(0, 33))) for _ in range(3000)]
    # tops whose fold carries: w1 close to 2^64
    cases += [(rnd.randrange(1, 2**32) << 128) | ((2**64 - rnd.randrange(1, 2**40)) << 64) | rnd.randrange(2**64)
              for _ in range(500)]
    return cases


def field64_values():
    rnd = random.Random(5)
    return EDGE64 + [rnd.randrange(P64) for _ in range(300)]


def wacc_reduce_cases():
    """Raw column sums for wacc_reduce: every column up to 2^63 - 1, zeros, and random mixes."""
    rnd = random.Random(11)
    cases = [[0] * 9, [2**63 - 1] * 9, [2**26 - 1] * 8 + [2**63 - 1], [0] * 8 + [2**63 - 1], [1] + [0] * 8,
             [2**63 - 1] + [0] * 8, [0, 0, 0, 0, 0, 2**63 - 1, 0, 0, 0]]
    cases += [[rnd.randrange(2**63) for _ in range(9)] for _ in range(300)]
    cases += [[rnd.choice([0, 2**26 - 1, 2**63 - 1, rnd.randrange(2**63)]) for _ in range(9)] for _ in range(300)]
    return cases


def wide_dot_operands(n):
    """Three (xs, cs) draws for the n-term wide dot product: all p - 1, then two mixed draws."""
    rnd = random.Random(n)
    out = []
    for trial in range(3):
        if trial == 0:
            xs = [P128 - 1] * n
            cs = [P128 - 1] * n
        else:
            xs = [rnd.randrange(P128) for _ in range(n)]
            cs = [rnd.choice([rnd.randrange(P128), P128 - 1, 2**128 - 2**100]) % P128 for _ in range(n)]
        out.append((xs, cs))
    return out


def wacc64_dot_operands(n):
    rnd = random.Random(n)
    xs = [rnd.choice(EDGE64) if rnd.random() < 0.3 else rnd.randrange(P64) for _ in range(n)]
    cs = [rnd.choice(EDGE64) if rnd.random() < 0.3 else rnd.randrange(P64) for _ in range(n)]
    if n == 1024:  # worst case for the column bound
        xs, cs = [P64 - 1] * n, [P64 - 1] * n
    return xs, cs


def reduce192_p64_cases():
    rnd = random.Random(5)
    cases = []
    for _ in range(200):
        w = [rnd.getrandbits(64) for _ in range(3)]
        if rnd.random() < 0.2:
            w = [2**64 - 1] * 3
        cases.append(w)
    return cases


def ge_p128_values():
    rnd = random.Random(41)
    vals = BOUND128 + [rnd.randrange(2**128) for _ in range(300)]
    vals += [(HI128 << 64) | rnd.randrange(2**64) for _ in range(50)]            # only the low half decides
    vals += [(rnd.randrange(HI128 - 3, 2**64) << 64) | rnd.randrange(4) for _ in range(100)]
    return vals


def ge_p64_values():
    rnd = random.Random(42)
    vals = BOUND64 + [rnd.randrange(2**64) for _ in range(300)]
    vals += [(0xFFFFFFFF << 32) | rnd.randrange(2**32) for _ in range(50)]
    vals += [(0xFFFFFFFF << 32) | (1 << k) for k in range(32)]                   # any one low bit decides
    vals += [(rnd.randrange(2**32 - 4, 2**32) << 32) | rnd.randrange(3) for _ in range(100)]
    return vals


GE_SCREEN_QUIET = [0, 1, 2**64, 2**127, (0xFFFFFFFF << 96) - 1, (0xFFFFFFFE << 96) | (2**96 - 1)]  # far below p


def ge_screen_cases():
    """(values >= p128 on which ge_screen must fire, 8-element windows with one of them at place 0, 3 or 7 among
    smaller elements, one window of small elements only)."""
    rnd = random.Random(43)
    ge = [v for v in BOUND128 if v >= P128] + [rnd.randrange(P128, 2**128) for _ in range(300)]
    ge += [(hi << 64) | lo for hi in range(HI128, 2**64) for lo in (0, 1, 2, 2**32, M64) if (hi << 64) | lo >= P128]
    windows = []
    for v in ge[:40]:
        for k in (0, 3, 7):
            elems = [rnd.randrange(2**126) for _ in range(8)]
            elems[k] = v
            windows.append(elems)
    quiet = [rnd.randrange(2**126) for _ in range(8)]
    return ge, windows, quiet


# ---------------------------------------------------------------------------- the sampler model
def _state(rnd, field_bytes):
    """25 random lanes whose rate part holds no encoding >= p (so every rejection is one the test placed)."""
    st = [rnd.randrange(2**64) for _ in range(25)]
    for i in range(21):
        if field_bytes == 8 and st[i] >> 32 == 0xFFFFFFFF:
            st[i] &= 2**63 - 1
        if field_bytes == 16 and i % 2 == 1:
            st[i] &= 2**63 - 1
    return st


def _model_take(st, nbytes, count, p, pos=0, whole_chunks=0):
    """Rejection sampling over the sponge's byte stream from byte `pos` of the block in st (168-byte rate,
    Keccak-p[1600,12] between blocks), by the oracle's permutation. whole_chunks > 0: only that many
    aligned chunks of each block are looked at (the kernels' register-resident samplers). Returns
    (samples, final state, final position)."""
    out, st = [], list(st)
    while True:
        blk = b"".join(x.to_bytes(8, "little") for x in st[:21])
        limit = whole_chunks * nbytes if whole_chunks else 168
        while pos + nbytes <= limit and len(out) < count:
            x = int.from_bytes(blk[pos:pos + nbytes], "little")
            pos += nbytes
            if x < p:
                out.append(x)
        if len(out) >= count:
            return out, st, pos
        assert whole_chunks or pos + nbytes > 168
        carry = blk[pos:168] if not whole_chunks else b""
        st = O.keccak_p1600(st, 12)
        pos = 0
        if carry:  # an element straddling two blocks
            blk = b"".join(x.to_bytes(8, "little") for x in st[:21])
            need = nbytes - len(carry)
            x = int.from_bytes(carry + blk[:need], "little")
            pos = need
            if x < p:
                out.append(x)
                if len(out) >= count:
                    return out, st, pos


def _set128(st, chunk, v):
    st[2 * chunk], st[2 * chunk + 1] = v & M64, v >> 64


def sample64_reject_positions(n):
    """Which of a block's 21 chunks hold a rejected encoding, case by case, for sample64<n>."""
    cases = [[k] for k in range(21)]                                    # one rejection at every position
    cases += [[0, 1], [0, 1, 2, 3], [3, 4, 5, 9], [19, 20], list(range(0, 17)), list(range(1, 21)),
              list(range(21 - n + 1)),                                  # fewer than n left: the next block is needed
              list(range(21))]                                          # none left
    return cases


SAMPLE2_REJECTS = ([], [0], [1], [0, 1], [2], [0, 2], [1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 7, 8])

# (first byte, elements to take, indices of the rejected elements); the successor of the last rejected
# element covers bytes 160..175, 152..167 + 0..7 of the next block, ... according to the alignment
BX_CASES = [(0, 12, [9]), (0, 12, [8, 9]), (8, 12, [0, 9]), (144, 3, [0]), (4, 12, [3]), (4, 12, [9]), (12, 12, [8])]


def bx_state(rnd, pos0, rej_at, g):
    """A Keccak state whose first block, read as 16-byte elements from byte pos0, holds g (>= p) at the
    elements rej_at and values below p elsewhere."""
    st = _state(rnd, 8)
    blk = bytearray(b"".join(x.to_bytes(8, "little") for x in st[:21]))
    for e in range((168 - pos0) // 16):  # keep the unplaced first-block elements below p
        blk[pos0 + 16 * e + 15] &= 0x7F
    for e in rej_at:
        assert pos0 + 16 * e + 16 <= 168
        blk[pos0 + 16 * e:pos0 + 16 * e + 16] = g.to_bytes(16, "little")
    st[:21] = [int.from_bytes(blk[8 * i:8 * i + 8], "little") for i in range(21)]
    return st


def sample64_cases(n):
    """(rejected chunk positions, state) per case for sample64<n>, then one state whose first element is p - 1
    (positions None): the largest element is taken, not skipped."""
    rnd = random.Random(50 + n)
    out = []
    for ci, rej in enumerate(sample64_reject_positions(n)):
        st = _state(rnd, 8)
        for j, k in enumerate(rej):
            st[k] = GE64[(ci + j) % len(GE64)]
        out.append((rej, st))
    st = _state(rnd, 8)
    st[0] = P64 - 1
    out.append((None, st))
    return out


def sample2_cases(cnt):
    """(rejected chunk positions, state) per case for sample2_f128 with `cnt` samples."""
    rnd = random.Random(60 + cnt)
    out = []
    for rej in SAMPLE2_REJECTS:
        for gi, g in enumerate(GE128):
            st = _state(rnd, 16)
            for j, k in enumerate(rej):
                _set128(st, k, GE128[(gi + j) % len(GE128)])
            if not rej:
                _set128(st, 0, P128 - 1)  # the largest element: taken, no flag
                _set128(st, 1, ((HI128 - 1) << 64) | M64)
            out.append((rej, st))
    return out


def bx_sample_cases():
    """(first byte, elements to take, rejected elements, state) per case for bx_sample128; the last case has no
    rejection at all: its eleventh element is the straddling one (bytes 160..167 and 0..7 of the next block)."""
    rnd = random.Random(70)
    out = []
    for pos0, nelem, rej_at in BX_CASES:
        for g in GE128:
            out.append((pos0, nelem, rej_at, bx_state(rnd, pos0, rej_at, g)))
    st = _state(rnd, 8)
    st[20] = M64
    out.append((0, 12, [], st))
    return out


# ---------------------------------------------------------------------------- 26-bit coefficient limbs
def coef_limb_values():
    rnd = random.Random(26)
    m26 = 2**26 - 1
    one_limb = [m26 << (26 * i) for i in range(4)] + [(2**24 - 1) << 104]
    return [0, 1, P128 - 1, 2**128 - 1] + one_limb + [rnd.randrange(2**128) for _ in range(1500)] + \
        [rnd.randrange(P128) for _ in range(1500)]


def coef_mac_operands(n):
    """40 (xs, cs, ds) draws of n calls of one slot: the first all-ones, the next seven from the edge values."""
    vals = coef_limb_values()
    rnd = random.Random(28 + n)
    out = []
    for rep in range(40):
        pool = vals[:9] if rep < 8 else vals
        xs, cs, ds = ([rnd.choice(pool) for _ in range(n)] for _ in range(3))
        if rep == 0:
            xs = cs = ds = [2**128 - 1] * n  # every limb product maximal: 5 * 512 * (2^26 - 1)^2 < 2^64
        out.append((xs, cs, ds))
    return out


# ---------------------------------------------------------------------------- X25519
def fe25519_values():
    rnd = random.Random(5)
    return [0, 1, 2, 19, P25519 - 1, P25519 - 19, 2**254, 2**255 - 20] + [rnd.randrange(P25519) for _ in range(40)]


def fe25519_loose_limb_cases():
    """Raw limbs as loose as the ladder makes them: every limb up to 2^28 - 1."""
    rnd = random.Random(25519)
    top = (1 << 28) - 1
    cases = [[top] * 10, [0] * 10, [1] + [0] * 9] + [[rnd.randrange(1 << 28) for _ in range(10)] for _ in range(300)]
    cases += [[rnd.choice([0, top, 1 << 26, (1 << 26) - 1, 1 << 27]) for _ in range(10)] for _ in range(100)]
    return cases


X25519_RFC7748 = (bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"),
                  bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c"))


def x25519_cases():
    rnd = random.Random(11)
    cases = [X25519_RFC7748]
    cases += [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(6)]
    cases += [(rnd.randbytes(32), (9).to_bytes(32, "little")), (rnd.randbytes(32), bytes(32)),
              (rnd.randbytes(32), b"\xff" * 32)]
    return cases


# ---------------------------------------------------------------------------- P-256
def p256_operands():
    import hpke_p256_ref as PR
    P = PR.P
    rnd = random.Random(256)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    for k in (31, 32, 33, 63, 64, 95, 96, 97, 128, 191, 192, 193, 223, 224, 225, 255):
        edge += [2**k - 1, 2**k, 2**k + 1]
    edge += [2**256 - 2**224, 2**224 - 1, 0xFFFFFFFF << 224, P - 2**32, P - 2**96, (1 << 255) + (1 << 32) - 1]
    return [v % P for v in edge], [rnd.randrange(P) for _ in range(40)]


def p256_points():
    import hpke_p256_ref as PR
    rnd = random.Random(2561)
    return [PR.G, PR.neg(PR.G)] + [PR.mul(rnd.randrange(1, PR.N), PR.G) for _ in range(3)]


def p256_scalars():
    """The scalars where an incomplete ladder goes wrong (leading zero bits, 1, 2, n - 1, n - 2, the two halves of
    n, single bits) and random ones."""
    import hpke_p256_ref as PR
    N = PR.N
    rnd = random.Random(2562)
    return [1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, 2**128, 2**255] + [rnd.randrange(1, N) for _ in range(20)]


# ---------------------------------------------------------------------------- Poly1305 lanes
PL_HI_H, PL_HI_M = 2**27 - 1, 2**26 + 2**25 - 1  # the largest accumulator and multiplier limbs pl_mul accepts


def pl_mul_cases():
    rnd = random.Random(1305)
    hi_h, hi_m = PL_HI_H, PL_HI_M
    cases = [([hi_h] * 5, [hi_m] * 5), ([hi_h] * 5, [0] * 5), ([0] * 5, [hi_m] * 5), ([hi_h] * 5, [1, 0, 0, 0, 0])]
    cases += [([rnd.randrange(hi_h + 1) for _ in range(5)], [rnd.randrange(hi_m + 1) for _ in range(5)]) for _ in range(300)]
    cases += [([hi_h if i == k else 0 for i in range(5)], [hi_m if i == j else 0 for i in range(5)])
              for k in range(5) for j in range(5)]
    return cases
