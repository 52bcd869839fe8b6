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


# ---------------------------------------------------------------------------- Keccak-p[1600] backwards
def _keccak_round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
            if r & 2:
                rc |= 1 << ((1 << j) - 1)
        out.append(rc)
    return out


def _keccak_rho_offsets():
    r, (x, y) = [0] * 25, (1, 0)
    for t in range(24):
        r[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


_KRC, _KRHO = _keccak_round_constants(), _keccak_rho_offsets()


def _theta_parity_map(c):
    """theta on the column parities (320 bits, column x at bits 64 x ..): C'[x] = C[x] ^ C[x-1] ^ rotl(C[x+1], 1)."""
    cs = [(c >> (64 * x)) & M64 for x in range(5)]
    rot1 = lambda v: ((v << 1) | (v >> 63)) & M64  # noqa: E731
    return sum((cs[x] ^ cs[(x - 1) % 5] ^ rot1(cs[(x + 1) % 5])) << (64 * x) for x in range(5))


def _theta_parity_inverse():
    """The inverse of _theta_parity_map as 320 columns (the image of every unit vector), by Gauss-Jordan over GF(2)."""
    n = 320
    cols = [_theta_parity_map(1 << j) for j in range(n)]
    rows = [(1 << (n + i)) | sum(((cols[j] >> i) & 1) << j for j in range(n)) for i in range(n)]  # [M | I]
    for j in range(n):
        piv = next(i for i in range(j, n) if (rows[i] >> j) & 1)
        rows[j], rows[piv] = rows[piv], rows[j]
        for i in range(n):
            if i != j and (rows[i] >> j) & 1:
                rows[i] ^= rows[j]
    inv_rows = [r >> n for r in rows]
    return [sum(((inv_rows[i] >> j) & 1) << i for i in range(n)) for j in range(n)]


_THETA_INV = []


def keccak_p1600_inverse(state, rounds):
    """The inverse of Keccak-p[1600, rounds] (the last `rounds` rounds of Keccak-f, FIPS 202 §3.3) on 25 lanes,
    lane (x, y) at index x + 5 y: per round iota, chi, pi, rho and theta undone in that order."""
    if not _THETA_INV:
        _THETA_INV.extend(_theta_parity_inverse())
    a = list(state)
    for ir in reversed(range(24 - rounds, 24)):
        a[0] ^= _KRC[ir]
        b = list(a)
        for y in range(5):  # chi^-1: a_x = b_x ^ ~b_(x+1) & (b_(x+2) ^ ~b_(x+3) & b_(x+4))
            r = b[5 * y:5 * y + 5]
            for x in range(5):
                a[x + 5 * y] = r[x] ^ (~r[(x + 1) % 5] & M64 & (r[(x + 2) % 5] ^ (~r[(x + 3) % 5] & M64 & r[(x + 4) % 5])))
        b = list(a)
        for x in range(5):  # pi and rho: B[y, 2x + 3y] = rotl(A[x, y], rho[x, y])
            for y in range(5):
                v, s = b[y + 5 * ((2 * x + 3 * y) % 5)], _KRHO[x + 5 * y]
                a[x + 5 * y] = ((v >> s) | (v << (64 - s))) & M64 if s else v
        cp = 0
        for x in range(5):
            cp |= (a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20]) << (64 * x)
        c, j = 0, 0
        while cp:  # the parities before theta
            if cp & 1:
                c ^= _THETA_INV[j]
            cp >>= 1
            j += 1
        cs = [(c >> (64 * x)) & M64 for x in range(5)]
        for x in range(5):
            v = cs[(x + 1) % 5]
            d = cs[(x - 1) % 5] ^ (((v << 1) | (v >> 63)) & M64)
            for y in range(5):
                a[x + 5 * y] ^= d
    return a


# ---------------------------------------------------------------------------- xof_stream128
def stream_chunks(st, count):
    """The first `count` 16-byte chunks of the byte stream whose first block is in st (rejected ones included)."""
    out, buf, st = [], b"", list(st)
    while len(out) < count:
        buf += b"".join(x.to_bytes(8, "little") for x in st[:21])
        while len(buf) >= 16 and len(out) < count:
            out.append(int.from_bytes(buf[:16], "little"))
            buf = buf[16:]
        st = O.keccak_p1600(st, 12)
    return out


def xof_stream_state(rnd, n, placed):
    """A state from which xof_stream128 of n elements meets exactly the chunks of `placed` ({stream position: value}
    with position 21 pair + c) as placed, every value >= p rejected, and no other rejection. The chunks of one
    case lie in one block: c < 10 in block 2 pair, c > 10 in block 2 pair + 1 (with c = 10, the straddling chunk,
    whose high half is that block's lane 0 and whose low half is whatever the block before holds, so its value
    must be given as None and it is rejected). That block is filled in and the state permuted backwards to the
    stream's first block; the blocks this leaves uncontrolled are checked to hold no encoding >= p."""
    blocks = {2 * (q // 21) + (q % 21 >= 10) for q in placed} or {0}
    assert len(blocks) == 1, "the placed chunks must lie in one block"
    blk = blocks.pop()
    st = [rnd.randrange(2**64) for _ in range(25)]
    for i in range(21):
        st[i] &= 2**63 - 1  # nothing >= p at either alignment
    for q, v in placed.items():
        c = q % 21
        if c < 10:
            st[2 * c], st[2 * c + 1] = v & M64, v >> 64
        elif c == 10:
            assert v is None
            st[0] = M64
        else:
            st[2 * (c - 11) + 1], st[2 * (c - 11) + 2] = v & M64, v >> 64
    for _ in range(blk):
        st = keccak_p1600_inverse(st, 12)
    rejected = sorted(q for q, v in placed.items() if v is None or v >= P128)
    chunks = stream_chunks(st, n + len(rejected) + 1)
    assert [q for q, v in enumerate(chunks[:n + len(rejected)]) if v >= P128] == rejected, (n, placed)
    for q, v in placed.items():
        assert q >= len(chunks) or (chunks[q] == v if v is not None else chunks[q] >> 64 == M64)
    return st


def xof_stream_cases():
    """(label, n, state) per case for xof_stream128, n <= 48. The reference is _model_take(state, 16, n, P128)."""
    rnd = random.Random(80)
    g = lambda i: GE128[i % len(GE128)]  # noqa: E731
    val = lambda q, i: None if q % 21 == 10 else g(i)  # noqa: E731
    cases = [(f"no rejection, n={n}", n, {}) for n in (1, 9, 10, 11, 20, 21, 22, 31, 32, 42, 43)]
    cases += [(f"rejection at {q}", 22, {q: val(q, q)}) for q in range(21)]       # every position of the first pair
    cases += [(f"rejection at {q} in the second pair", 40, {q: val(q, q)}) for q in (21 + 3, 21 + 10, 21 + 13)]
    # neighbours rejected together on either side of the first permutation. Position 9 lies in the block before
    # the permutation and 10, 11 in the one after it: values >= p on both sides of one permutation would take a
    # search of about 2^59 states, so 9 goes with 8 and 10 with 11.
    cases += [("rejections at 8 and 9", 22, {8: g(1), 9: g(2)}), ("rejections at 10 and 11", 22, {10: None, 11: g(3)}),
              ("rejections at 10, 11 and 12", 22, {10: None, 11: g(4), 12: g(0)}),
              ("rejections at 19 and 20", 22, {19: g(1), 20: g(2)})]
    # the last chunk needed is rejected, so that one more permutation is required
    cases += [("rejection in the last chunk needed, n=10", 10, {9: g(0)}),
              ("rejection in the last chunk needed, n=11", 11, {10: None}),
              ("rejection in the last chunk needed, n=21", 21, {20: g(1)})]
    for i in range(len(GE128)):  # every rejected encoding, before and after the permutation
        cases += [(f"GE128[{i}] at 3", 12, {3: g(i)}), (f"GE128[{i}] at 14", 22, {14: g(i)})]
    cases += [("p - 1 is taken at 0", 1, {0: P128 - 1}), ("p - 1 is taken at 9", 10, {9: P128 - 1}),
              ("p - 1 is taken at 12 and 20", 21, {12: P128 - 1, 20: P128 - 1})]
    return [(label, n, xof_stream_state(rnd, n, placed)) for label, n, placed in cases]


# ---------------------------------------------------------------------------- the prover's transforms (jx_ntt.h)
GEN128 = pow(7, (P128 - 1) >> 66, P128)  # order 2^66


def root(log_order):
    return pow(GEN128, 1 << (66 - log_order), P128)


def rev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def dft(x, w):
    n = len(x)
    return [sum(x[j] * pow(w, j * m, P128) for j in range(n)) % P128 for m in range(n)]


def horner(coef, x):
    r = 0
    for c in reversed(coef):
        r = (r * x + c) % P128
    return r


def rand_vals(rng, n):
    edge = [0, 1, P128 - 1]
    return [rng.choice(edge) if rng.random() < 0.1 else rng.randrange(P128) for _ in range(n)]


def interpolate(vals, log_p):
    """Coefficients of the polynomial of degree < P with w(alpha^k) = vals[k], by the fast transform in Python."""
    n = 1 << log_p
    a = list(vals)
    winv = pow(root(log_p), P128 - 2, P128) if log_p else 1
    ln = n
    while ln >= 2:
        half, wl = ln // 2, pow(winv, n // ln, P128)
        for s in range(0, n, ln):
            ww = 1
            for k in range(half):
                u, v = a[s + k], a[s + k + half]
                a[s + k] = (u + v) % P128
                a[s + k + half] = (u - v) * ww % P128
                ww = ww * wl % P128
        ln //= 2
    ninv = pow(n, P128 - 2, P128)
    return [a[rev(j, log_p)] * ninv % P128 for j in range(n)]


def evaluate(coef, log_n):
    """The values at root(log_n)^m, m < 2^log_n, of the polynomial with the coefficients coef (at most 2^log_n):
    the forward fast transform, by the even / odd split."""
    def split(a, w):
        if len(a) == 1:
            return a
        e, o = split(a[0::2], w * w % P128), split(a[1::2], w * w % P128)
        half, out, t = len(a) // 2, [0] * len(a), 1
        for k in range(half):
            v = t * o[k] % P128
            out[k], out[k + half] = (e[k] + v) % P128, (e[k] - v) % P128
            t = t * w % P128
        return out
    n = 1 << log_n
    return split(list(coef) + [0] * (n - len(coef)), root(log_n))


def odd_point_values(vals, log_p):
    """w(beta^(2k+1)), k < P, of the wire polynomial with w(alpha^k) = vals[k] (beta^2 = alpha): ntt_odd_points."""
    return evaluate(interpolate(vals, log_p), log_p + 1)[1::2]


def gadget_poly(wires, log_p):
    """The 2P coefficients of sum_i wire_2i wire_2i+1 of the interpolated wires, through the size-2P transform."""
    vals = [evaluate(interpolate(w, log_p), log_p + 1) for w in wires]
    prod = [sum(vals[2 * i][m] * vals[2 * i + 1][m] for i in range(len(wires) // 2)) % P128 for m in range(2 << log_p)]
    return interpolate(prod, log_p + 1)


def ntt_wave_cases():
    """(log_p, npairs, wires) for the 64-lane transforms: every size 2..1024 with one pair, and with three pairs
    up to P = 256 (the prove kernel's four-wave size), the wire values random with 0, 1 and p - 1 mixed in."""
    out = []
    for log_p in range(1, 11):
        for npairs in (1, 3):
            if npairs == 3 and log_p > 8:
                continue
            rng = random.Random(900 + 10 * log_p + npairs)
            out.append((log_p, npairs, [rand_vals(rng, 1 << log_p) for _ in range(2 * npairs)]))
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
