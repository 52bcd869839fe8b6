"""The device arithmetic headers (janus_amd/csrc/jx_*.h) run ON the GPU, one case per lane, against Python integers,
hashlib / hmac, the oracle and the Python HPKE references, at the edges the host tests use (math_vectors.py).

Why: the g++ host tests prove the portable fallbacks of the headers. Under __HIP_DEVICE_COMPILE__ the same
functions use other instructions (mac_c: a v_mad_u64_u32 whose carry-out is an SGPR-pair lane mask feeding a
v_addc_co_u32; adc32 / sbb32: __builtin_addc / __builtin_subc; xor3 / maj3: v_bitop3; alignbit; wacc_mac's asm
barrier), and the whole-kernel GPU tests feed them pseudo-random operands only. Here every launch shuffles edge and
random cases together with a fixed seed, so that the lanes of one wave carry differently, and has a case count that
is no multiple of 64, so that the last wave runs partly masked. The prover's transforms (jx_ntt.h) exchange data
between the lanes of a wave through LDS, which no host build can show: they run in the harness's second launch
shape, one wave per case, with every output element compared.

The limit of this file: the harness kernels (tests/csrc/devtest.hip) are not the product kernels, so register
allocation and instruction scheduling differ. What is identical is every __forceinline__ body of the headers and
every device-only instruction choice in them.

Every expectation is exact equality with a value computed here in Python, never with the host build or another
device run. One launch per operation and test: measured on an MI355X the whole file takes under 2 s, the slowest
tests (the first, which initialises the device, and the P-256 ladders: 147 cases in one launch) 0.4 s each."""
from __future__ import annotations

import ctypes
import hashlib
import hmac
import os
import random
import shutil

import pytest

import hpke_p256_ref as PR
import hpke_suites_ref as S
import math_vectors as V
from math_vectors import EDGE, P64, P128, P25519, R
from oracle import hpke_oracle as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

M26 = 2**26 - 1
RINV = pow(R, P128 - 2, P128)


class DevTest:
    """libjx_devtest.so: dt_run(op, records) -> records. After one failed launch nothing more is launched."""

    def __init__(self, lib):
        self.lib = lib
        self.failed = None
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        lib.dt_run.argtypes = [ctypes.c_char_p, u32, vp, u32, vp, u32, vp, u32]
        lib.dt_sizes.argtypes = [ctypes.c_char_p, vp, vp]
        lib.dt_source_hash.restype = ctypes.c_char_p
        lib.dt_ntt_table.argtypes = [u32, vp]

    def run(self, op: str, records, aux: bytes = b""):
        """records: one bytes object per case. Returns the output record of every case, in the order given. The
        cases run in a shuffled order; a count that is a multiple of 64 gets the first case once more."""
        if self.failed:
            raise RuntimeError(f"no launch after a failed one: {self.failed}")
        insz, outsz = ctypes.c_uint32(), ctypes.c_uint32()
        assert self.lib.dt_sizes(op.encode(), ctypes.byref(insz), ctypes.byref(outsz)) == 0, op
        records = list(records)
        assert records and all(len(r) == insz.value for r in records), (op, insz.value, len(records[0]))
        order = list(range(len(records)))
        if len(order) % 64 == 0:
            order.append(0)
        random.Random(0xD7).shuffle(order)
        n = len(order)
        assert n % 64 != 0
        inbuf = b"".join(records[i] for i in order)
        out = ctypes.create_string_buffer(n * outsz.value)
        rc = self.lib.dt_run(op.encode(), n, inbuf, insz.value, out, outsz.value, aux if aux else None, len(aux))
        if rc != 0:
            self.failed = f"dt_run({op}) returned {rc}"
            raise RuntimeError(self.failed)
        res = [None] * len(records)
        for slot, i in enumerate(order):
            res[i] = out.raw[slot * outsz.value:(slot + 1) * outsz.value]
        return res


@pytest.fixture(scope="module")
def dev():
    from janus_amd import build as jb
    want = jb.devtest_source_hash()
    if jb.devtest_built_hash() != want:  # stale by content (file times do not survive a copy between machines)
        if not (os.path.exists(jb.hipcc_path()) or shutil.which(jb.hipcc_path())):
            pytest.fail(f"{jb.DEVTEST_OUT} is missing or stale and there is no hipcc to rebuild it")
        jb.build_devtest()
    lib = ctypes.CDLL(jb.DEVTEST_OUT)
    d = DevTest(lib)
    assert lib.dt_source_hash().decode() == want
    return d


def le(x: int, n: int = 16) -> bytes:
    return x.to_bytes(n, "little")


def u32s(*v) -> bytes:
    return b"".join(x.to_bytes(4, "little") for x in v)


def u64s(*v) -> bytes:
    return b"".join(x.to_bytes(8, "little") for x in v)


def li(b: bytes) -> int:
    return int.from_bytes(b, "little")


def words(b: bytes, size: int):
    return [li(b[i:i + size]) for i in range(0, len(b), size)]


# ---------------------------------------------------------------------------- Field128
def test_field128_basic_operations(dev):
    """add128, sub128, neg128, mont128, to_mont128, from_mont128: EDGE x EDGE plus the host test's 90 x 90."""
    vals = V.field128_mont_values()
    pairs = [(a, b) for a in EDGE for b in EDGE] + [(a, b) for a in vals[:90] for b in vals[:90]]
    asv = V.field128_add_sub_values()
    pairs_as = pairs + [(a, b) for a in asv[:60] for b in asv[:60]]
    cases = [(0, a, b, (a + b) % P128) for a, b in pairs_as] + [(1, a, b, (a - b) % P128) for a, b in pairs_as]
    cases += [(2, a, b, a * b * RINV % P128) for a, b in pairs]
    cases += [(3, a, 0, a * R % P128) for a in vals] + [(4, a, 0, a * RINV % P128) for a in vals]
    cases += [(5, a, 0, -a % P128) for a in vals]
    got = dev.run("f128", [u32s(op, 0) + le(a) + le(b) for op, a, b, _ in cases])
    bad = [(op, hex(a), hex(b)) for (op, a, b, want), g in zip(cases, got) if li(g) != want]
    names = ["add128", "sub128", "mont128", "to_mont128", "from_mont128", "neg128"]
    assert not bad, ({names[op]: sum(b[0] == op for b in bad) for op in range(6) if any(b[0] == op for b in bad)}, bad[:8])


def test_field128_reductions(dev):
    """mont128_lazy (value and the < 2p bound), reduce192, reduce192_small (the tops whose fold carries included)."""
    lazy = V.mont_lazy_cases() + [(a, b) for a in EDGE for b in EDGE]
    got = dev.run("mont_lazy", [le(a) + le(b) for a, b in lazy])
    for (a, b), g in zip(lazy, got):
        lo, hi, top = words(g, 8)
        v = lo + (hi << 64) + (top << 128)
        assert v < 2 * P128 and v % P128 == a * b * RINV % P128, (hex(a), hex(b))
    cases = [(0, v) for v in V.reduce192_cases()] + [(1, v) for v in V.reduce192_small_cases()]
    assert all(v < 2**160 for form, v in cases if form == 1)
    got = dev.run("red192", [u32s(form, 0) + le(v, 24) for form, v in cases])
    bad = [(form, hex(v)) for (form, v), g in zip(cases, got) if li(g) != v % P128]
    assert not bad, (len(bad), bad[:8])


def test_field128_ge_p_predicates(dev):
    """ge_p128, ge_exact, and ge_screen with its running max."""
    vals = V.ge_p128_values()
    cases = [(form, v) for form in (0, 1) for v in vals]
    got = dev.run("ge128", [u32s(form, 0) + le(v) for form, v in cases])
    bad = [(form, hex(v)) for (form, v), g in zip(cases, got) if li(g) != int(v >= P128)]
    assert not bad, bad[:8]
    ge, windows, quiet = V.ge_screen_cases()
    elems, recs, fires = [], [], []
    for group, must_fire in ([[v] for v in ge], True), ([[v] for v in V.GE_SCREEN_QUIET], False), (windows, True), \
            ([quiet], False):
        for g in group:
            recs.append(u32s(len(elems), len(g)))
            fires.append((must_fire, g))
            elems += g
    got = dev.run("ge_screen", recs, b"".join(le(e) for e in elems))
    for (must_fire, g), r in zip(fires, got):
        # the screen of one element is word3 & (word2 | 0x1F); the kernels keep its maximum
        model = max((e >> 96) & (((e >> 64) & 0xFFFFFFFF) | 0x1F) for e in g)
        assert li(r) == model and (li(r) == 0xFFFFFFFF) == must_fire, [hex(e) for e in g]


def test_truncation_chains(dev):
    """trunc_add and acc_reduce: sum_j x_j << j over bits in {1, 8, 31, 32, 63} elements drawn from EDGE."""
    rnd = random.Random(17)
    chains = []
    for bits in (1, 8, 31, 32, 63):
        chains += [[e] * bits for e in EDGE]                                    # every element the same edge
        chains += [[rnd.choice(EDGE) for _ in range(bits)] for _ in range(24)]
        chains += [[rnd.choice(EDGE + [rnd.randrange(P128)]) for _ in range(bits)] for _ in range(8)]
    elems, recs = [], []
    for ch in chains:
        recs.append(u32s(len(ch), len(elems)))
        elems += ch
    got = dev.run("trunc", recs, b"".join(le(e) for e in elems))
    for ch, g in zip(chains, got):
        assert li(g) == sum(x << j for j, x in enumerate(ch)) % P128, (len(ch), [hex(x) for x in ch[:4]])


def test_k1_truncation_word_columns(dev):
    """K1's TruncW columns (truncw_mac, truncw_value, shl32_mod) in emit_meas's order: bits in {1, 31, 32} and the
    WIDE path at bits in {33, 64} (the fold at j = 32 and the lo + shl32_mod(high) finish), elements from EDGE,
    the all-ones element included."""
    rnd = random.Random(18)
    ones = 0xFFFFFFFFFFFFFFE3FFFFFFFFFFFFFFFF
    assert ones in EDGE
    chains = []
    for bits in (1, 31, 32, 33, 64):
        chains += [[e] * bits for e in EDGE]
        chains += [[rnd.choice(EDGE) for _ in range(bits)] for _ in range(24)]
        chains += [[rnd.choice([ones, P128 - 1, rnd.randrange(P128)]) for _ in range(bits)] for _ in range(8)]
    elems, recs = [], []
    for ch in chains:
        recs.append(u32s(len(ch), len(elems)))
        elems += ch
    got = dev.run("truncw", recs, b"".join(le(e) for e in elems))
    for ch, g in zip(chains, got):
        assert li(g) == sum(x << j for j, x in enumerate(ch)) % P128, (len(ch), [hex(x) for x in ch[:4]])


# ---------------------------------------------------------------------------- 26-bit limbs
def limbs26(a):
    return [(a >> (26 * i)) & M26 for i in range(4)] + [a >> 104]


def test_limbs26_pack_unpack(dev):
    vals = V.coef_limb_values()
    rnd = random.Random(27)
    pairs = [(c, vals[(i * 7 + 3) % len(vals)] if i % 3 else rnd.choice(vals[:9])) for i, c in enumerate(vals)]
    got = dev.run("cd26", [le(c) + le(d) for c, d in pairs])
    for (c, d), g in zip(pairs, got):
        w = words(g, 4)
        assert w[0:5] == limbs26(c) and w[5:10] == limbs26(d), hex(c)
        # the staged layout: row A = c's limbs 0-3, row B = d's limbs 0-3, half-row C = the two top limbs
        assert w[10:20] == limbs26(c)[:4] + limbs26(d)[:4] + [limbs26(c)[4], limbs26(d)[4]], hex(c)
        assert w[20:25] == limbs26(c) and w[25:30] == limbs26(d), hex(c)


def test_wacc_reduce_and_normalize_columns(dev):
    """wacc_reduce and wacc_normalize on raw column sums, every column up to 2^63 - 1."""
    cols = V.wacc_reduce_cases()
    cases = [(form, c) for form in (0, 1) for c in cols]
    got = dev.run("wacc_cols", [u32s(form, 0) + u64s(*c) for form, c in cases])
    for (form, c), g in zip(cases, got):
        if form == 0:
            assert li(g[:16]) == sum(v << (26 * s) for s, v in enumerate(c)) % P128, c
        else:
            want = list(c)
            for s in range(8):
                want[s + 1] = (want[s + 1] + (want[s] >> 26)) % 2**64
                want[s] &= M26
            assert words(g, 8) == want, c


def test_wide_dot_products(dev):
    """wacc_mac / wacc_normalize / wacc_reduce over n terms: n in {1, 91, 700, 2000 normalised every 512}, all
    operands p - 1 and the mixed draws."""
    elems, recs, wants = [], [], []
    for n, norm in ((1, 0), (91, 0), (700, 0), (2000, 512)):
        for xs, cs in V.wide_dot_operands(n):
            recs.append(u32s(len(elems), len(elems) + n, n, norm))
            elems += xs + cs
            wants.append(sum(x * c for x, c in zip(xs, cs)) % P128)
    got = dev.run("wide_dot", recs, b"".join(le(e) for e in elems))
    assert [li(g) for g in got] == wants


def test_packed_coefficient_mac(dev):
    """The ring's (c_k, d_k) accumulation of hosttest_coef_limbs.cpp: the nine raw columns from the staged words
    and from to_limbs26, against Python's limb products."""
    elems, recs, wants = [], [], []
    for n in (1, 5, 512):
        for xs, cs, ds in V.coef_mac_operands(n):
            want_e, want_o = [0] * 9, [0] * 9
            for x, c, d in zip(xs, cs, ds):
                xl, cl, dl = limbs26(x), limbs26(c), limbs26(d)
                for i in range(5):
                    for j in range(5):
                        want_e[i + j] += xl[i] * dl[j]
                        want_o[i + j] += xl[i] * cl[j]
            assert max(want_e + want_o) < 2**64
            base = len(elems)
            elems += xs + cs + ds
            for packed in (0, 1):
                recs.append(u32s(base, base + n, base + 2 * n, n, packed, 0))
                wants.append(want_e + want_o)
    got = dev.run("cl_mac", recs, b"".join(le(e) for e in elems))
    assert [words(g, 8) for g in got] == wants


# ---------------------------------------------------------------------------- Field64
def test_field64(dev):
    """add64, sub64, mul64 on edges x edges and the host test's 70 x 70; reduce192_p64 (all-ones words included);
    ge_p64."""
    vals = V.field64_values()
    cases = []
    for a in vals[:70]:
        for b in vals[:70]:
            cases += [(0, a, b, (a + b) % P64), (1, a, b, (a - b) % P64), (2, a, b, a * b % P64)]
    got = dev.run("f64", [u32s(op, 0) + u64s(a, b) for op, a, b, _ in cases])
    bad = [(op, hex(a), hex(b)) for (op, a, b, want), g in zip(cases, got) if li(g) != want]
    assert not bad, bad[:8]
    ws = V.reduce192_p64_cases() + [[2**64 - 1] * 3, [0, 0, 2**64 - 1], [P64, P64, P64], [P64 - 1] * 3]
    got = dev.run("red192_p64", [u64s(*w) for w in ws])
    assert [li(g) for g in got] == [(w[0] + (w[1] << 64) + (w[2] << 128)) % P64 for w in ws]
    gv = V.ge_p64_values()
    got = dev.run("ge64", [u32s(v & 0xFFFFFFFF, v >> 32) for v in gv])
    assert [li(g) for g in got] == [int(v >= P64) for v in gv]


def test_wacc64_dot_products(dev):
    """The Field64 column accumulator, n = 1024 all p - 1 (the column bound) and past the 1024-term fold."""
    elems, recs, wants = [], [], []
    for n in (1, 91, 1023, 1024, 1025, 3000):
        xs, cs = V.wacc64_dot_operands(n)
        recs.append(u32s(len(elems), len(elems) + n, n, 0))
        elems += xs + cs
        wants.append(sum(x * c for x, c in zip(xs, cs)) % P64)
    got = dev.run("wacc64_dot", recs, u64s(*elems))
    assert [li(g) for g in got] == wants


# ---------------------------------------------------------------------------- samplers
def test_samplers(dev):
    """sample64<1>, sample64<5>, sample2_f128 fast / slow and bx_sample128 across a block boundary, on the host
    test's hand-built Keccak states: the samples, the final state and the position."""
    recs, wants = [], []
    for n in (1, 5):
        for rej, st in V.sample64_cases(n):
            want, st_after, _ = V._model_take(st, 8, n, P64, whole_chunks=21)
            recs.append(u32s(n, 0) + u64s(*st))
            wants.append((st_after, want))
    got = dev.run("sample64", recs)
    for (st_after, want), g in zip(wants, got):
        w = words(g, 8)
        assert w[:25] == st_after and w[25:25 + len(want)] == want
    assert sum(li(r[8:208]) != li(g[:200]) for r, g in zip(recs, got)) >= 4  # some cases needed the next block

    FLAG_SLOW, other = 4, 16
    recs, wants = [], []
    for cnt in (1, 2):
        for rej, st in V.sample2_cases(cnt):
            chunks = [st[2 * k] | (st[2 * k + 1] << 64) for k in range(10)]
            recs.append(u32s(cnt, 0, other, 0) + u64s(*st))  # fast: the chunks as they are, FLAG_SLOW if one is >= p
            wants.append((st, chunks[:cnt], other | (FLAG_SLOW if any(c >= P128 for c in chunks[:cnt]) else 0)))
            want, st_after, _ = V._model_take(st, 16, cnt, P128, whole_chunks=10)
            recs.append(u32s(cnt, 1, other, 0) + u64s(*st))  # slow: the first cnt accepted chunks
            wants.append((st_after, want, other))
    got = dev.run("sample2", recs)
    for (st_after, want, flags), g in zip(wants, got):
        assert words(g[:200], 8) == st_after and words(g[200:232], 16)[:len(want)] == want and li(g[232:236]) == flags

    recs, wants = [], []
    for pos0, nelem, rej_at, st in V.bx_sample_cases():
        recs.append(u32s(pos0, nelem) + u64s(*st))
        wants.append(V._model_take(st, 16, nelem, P128, pos=pos0))
    got = dev.run("bx_sample", recs)
    for (want, st_after, pos_after), g in zip(wants, got):
        assert words(g[:200], 8) == st_after and li(g[200:204]) == pos_after
        assert words(g[208:], 16)[:len(want)] == want


def test_xof_stream128(dev):
    """xof_stream128, the sampler of Prio3.shard's Field128 streams, on the host test's states (built backwards
    through the permutation: a rejected encoding at every chunk of the first block pair, in the second pair, in the
    last chunk needed): emit is called for k = 0 .. n - 1 once each, in order, with the byte-stream model's values."""
    cases = V.xof_stream_cases()
    got = dev.run("xof_stream", [u32s(n, 0) + u64s(*st) for _, n, st in cases])
    for (label, n, st), g in zip(cases, got):
        want, _, _ = V._model_take(st, 16, n, P128)
        assert li(g[:4]) == n, (label, hex(li(g[:4])))
        assert words(g[8:8 + 16 * n], 16) == want, label
        assert g[8 + 16 * n:] == b"\xa5" * (16 * (48 - n)), label


# ---------------------------------------------------------------------------- the prover's transforms, 64 lanes
def _ntt_aux(dev, cases):
    """aux for the wave-per-case transforms: the table of every size once, then every case's wires, pair by pair.
    Returns (aux, {log_p: table offset}, [data offset per case]), offsets in elements."""
    aux, tab_off, data_off = b"", {}, []
    for log_p in sorted({c[0] for c in cases}):
        buf = ctypes.create_string_buffer(16 * (3 * (1 << log_p) + 1))
        assert dev.lib.dt_ntt_table(log_p, buf) == 0
        tab_off[log_p] = len(aux) // 16
        aux += buf.raw
    for _, _, wires in cases:
        data_off.append(len(aux) // 16)
        aux += b"".join(le(v) for w in wires for v in w)
    return aux, tab_off, data_off


def test_ntt_odd_points_across_a_wave(dev):
    """ntt_odd_points with nl = 64 and the prove kernel's wave_sync, one wave per case over LDS, P = 2 .. 1024:
    EVERY odd-point value against the Python fast transform (test_ntt_host.py pins that against Horner's rule). A
    misplaced sync() corrupts a few elements only, so nothing is sampled."""
    cases = [(log_p, 1, wires[:1]) for log_p, npairs, wires in V.ntt_wave_cases() if npairs == 1]
    assert [c[0] for c in cases] == list(range(1, 11))
    aux, tab_off, data_off = _ntt_aux(dev, cases)
    got = dev.run("ntt_odd", [u32s(log_p, 1, tab_off[log_p], off) for (log_p, _, _), off in zip(cases, data_off)], aux)
    for (log_p, _, wires), g in zip(cases, got):
        n = 1 << log_p
        want = V.odd_point_values(wires[0], log_p)
        bad = [k for k, (a, b) in enumerate(zip(words(g[:16 * n], 16), want)) if a != b]
        assert not bad, (log_p, len(bad), bad[:8])
        assert g[16 * n:] == b"\xa5" * (len(g) - 16 * n)


def test_ntt_gadget_polynomial_across_a_wave(dev):
    """The prove kernel's accumulation over 1 and 3 wire pairs (LDS laid out A, B, E, O) and ntt_gpoly_finish with
    64 lanes, P = 2 .. 1024 (three pairs up to 256): ALL 2P coefficients against the product of the interpolated
    wires through the Python transform of size 2P; the top coefficient is zero."""
    cases = V.ntt_wave_cases()
    assert {(c[0], c[1]) for c in cases} >= {(10, 1), (8, 3), (6, 1), (6, 3), (1, 1), (1, 3)}
    aux, tab_off, data_off = _ntt_aux(dev, cases)
    recs = [u32s(log_p, npairs, tab_off[log_p], off) for (log_p, npairs, _), off in zip(cases, data_off)]
    got = dev.run("ntt_gpoly", recs, aux)
    for (log_p, npairs, wires), g in zip(cases, got):
        n = 1 << log_p
        want = V.gadget_poly(wires, log_p)
        assert want[2 * n - 1] == 0
        bad = [j for j, (a, b) in enumerate(zip(words(g[:32 * n], 16), want)) if a != b]
        assert not bad, (log_p, npairs, len(bad), bad[:8])
        assert g[32 * n:] == b"\xa5" * (len(g) - 32 * n)


# ---------------------------------------------------------------------------- bit operations and hashes
def test_bitop3_builtins(dev):
    """xor3 and maj3 (v_bitop3_b32 with tables 0x96 and 0xE8): 0, all-ones and random words."""
    rnd = random.Random(96)
    ones = 0xFFFFFFFF
    cases = [(a, b, c) for a in (0, ones) for b in (0, ones) for c in (0, ones)]
    cases += [(rnd.getrandbits(32), rnd.getrandbits(32), rnd.getrandbits(32)) for _ in range(500)]
    cases += [(rnd.choice((0, ones, rnd.getrandbits(32))), rnd.choice((0, ones)), rnd.getrandbits(32)) for _ in range(100)]
    got = dev.run("bitop", [u32s(a, b, c, 0) for a, b, c in cases])
    for (a, b, c), g in zip(cases, got):
        assert words(g, 4) == [a ^ b ^ c, (a & b) | (a & c) | (b & c)], (hex(a), hex(b), hex(c))


def test_keccak_p12(dev):
    rnd = random.Random(6)
    states = [[rnd.getrandbits(64) for _ in range(25)] for _ in range(70)] + [[0] * 25, [2**64 - 1] * 25]
    got = dev.run("keccak", [u64s(*st) for st in states])
    assert [words(g, 8) for g in got] == [O.keccak_p1600(st, 12) for st in states]


def test_sha256_hmac_sha512(dev):
    """SHA-256 and HMAC-SHA256 at the host test's lengths on both sides of the padding boundaries, SHA-512 and
    HMAC-SHA512 at the same around the 128-byte block, sha256_16."""
    rnd = random.Random(256512)
    aux, recs, wants = bytearray(), [], []

    def add(kind, data, ln, want):
        recs.append(u32s(kind, len(aux), ln, 0))
        aux.extend(data)
        wants.append(want + bytes(64 - len(want)))

    for n in (0, 1, 55, 56, 63, 64, 119, 120, 200):
        for msg in (rnd.randbytes(n), b"\xff" * n):
            add(0, msg, n, hashlib.sha256(msg).digest())
    for n in (0, 1, 111, 112, 127, 128, 239, 240, 255, 256, 300):
        for msg in (rnd.randbytes(n), b"\xff" * n):
            add(1, msg, n, hashlib.sha512(msg).digest())
    for n in (0, 1, 23, 51, 55, 56, 63, 64, 92, 95, 119):
        for key in (rnd.randbytes(32), b"\xff" * 32, bytes(32)):
            msg = rnd.randbytes(n)
            add(2, key + msg, n, hmac.new(key, msg, hashlib.sha256).digest())
    for n in (0, 111, 112, 127, 128, 239, 240):
        key, msg = rnd.randbytes(32), rnd.randbytes(n)
        add(4, key + msg, n, hmac.new(key, msg, hashlib.sha512).digest())
    for _ in range(20):
        rid = rnd.randbytes(16)
        add(3, rid, 16, hashlib.sha256(rid).digest())
    got = dev.run("hash", recs, bytes(aux))
    bad = [(li(r[:4]), li(r[8:12])) for r, g, w in zip(recs, got, wants) if g != w]
    assert not bad, bad


def test_be_word_shift16(dev):
    rnd = random.Random(3)
    cases = [(rnd.getrandbits(32), rnd.getrandbits(32)) for _ in range(100)] + [(0, 0), (2**32 - 1, 0), (0, 2**32 - 1)]
    got = dev.run("shift16", [u32s(lo, hi) for lo, hi in cases])
    for (lo, hi), g in zip(cases, got):
        assert li(g) == int.from_bytes((le(lo, 4) + le(hi, 4))[2:6], "big")


# ---------------------------------------------------------------------------- X25519
def test_fe25519_operations(dev):
    """fe_mul, fe_sq, fe_sub, fe_invert, fe_mul_small on canonical edges; fe_mul / fe_sq / fe_mul_small on raw
    limbs up to 2^28 - 1 with the output limb bounds the host test asserts."""
    vals = V.fe25519_values()
    cases = []
    for a in vals:
        cases += [(0, a, b, a * b % P25519) for b in vals[:12]] + [(2, a, b, (a - b) % P25519) for b in vals[:12]]
        cases += [(1, a, 0, a * a % P25519), (4, a, 0, a * 121665 % P25519)]
        if a:
            cases.append((3, a, 0, pow(a, P25519 - 2, P25519)))
    got = dev.run("fe", [u32s(op, 0) + le(a, 32) + le(b, 32) for op, a, b, _ in cases])
    bad = [(op, hex(a), hex(b)) for (op, a, b, want), g in zip(cases, got) if li(g) != want]
    assert not bad, bad[:8]

    loose = V.fe25519_loose_limb_cases()

    def val(v):
        return sum(x << (26 * i) for i, x in enumerate(v))

    cases = [(op, a, loose[(7 * i + 3) % len(loose)]) for i, a in enumerate(loose) for op in (0, 1, 4)]
    got = dev.run("fe_limbs", [u32s(op, 0) + u32s(*a) + u32s(*b) for op, a, b in cases])
    for (op, a, b), g in zip(cases, got):
        out = words(g, 4)
        want = val(a) * (val(b) if op == 0 else val(a) if op == 1 else 121665) % P25519
        assert val(out) % P25519 == want, (op, a, b)
        assert out[0] <= (1 << 27) - 38 and all(x <= (1 << 27) - 2 for x in out[1:9]) and out[9] <= (1 << 22) - 2
        assert max(out) < (1 << 26) + (1 << 17), out


def test_x25519_ladder(dev):
    """The ladder on the RFC 7748 vector, u in {0, 1, 9, p - 1, p, p + 1, 2^255 - 1} and random pairs; the
    low-order inputs give the all-zero result."""
    rnd = random.Random(7748)
    cases = V.x25519_cases()
    special = [0, 1, 9, P25519 - 1, P25519, P25519 + 1, 2**255 - 1]
    for u in special:
        cases += [(rnd.randbytes(32), le(u, 32)) for _ in range(4)]
    cases += [(b"\xff" * 32, le(u, 32)) for u in special] + [(bytes(32), le(u, 32)) for u in special]
    cases += [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(250)]
    got = dev.run("x25519", [k + u for k, u in cases])
    assert got[0] == bytes.fromhex("c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")
    for (k, u), g in zip(cases, got):
        assert g == H.x25519(k, u), (k.hex(), u.hex())
        if li(u) % 2**255 % P25519 in (0, 1, P25519 - 1):
            assert g == bytes(32)


# ---------------------------------------------------------------------------- P-256
def be(v: int) -> bytes:
    return v.to_bytes(32, "big")


def test_p256_field(dev):
    """p256_mul, sq, add, sub, invert on p256_operands(); operands >= p are refused."""
    P = PR.P
    edge, rand = V.p256_operands()
    cases = []
    for a in edge:
        cases.append((1, a, 0, a * a % P))
        cases += [(0, a, b, a * b % P) for b in edge]
    for a in rand:
        cases.append((1, a, 0, a * a % P))
        cases += [(0, a, b, a * b % P) for b in rand[:8] + edge[:7]]
    for a in edge + rand[:10]:
        for b in edge + rand[10:20]:
            cases += [(3, a, b, (a + b) % P), (4, a, b, (a - b) % P)]
    cases += [(2, 0, 0, 0)] + [(2, a, 0, pow(a, -1, P)) for a in edge[1:] + rand if a]
    n_good = len(cases)
    for v in (P, P + 1, 2**256 - 1):
        cases += [(0, v, 1, None), (0, 1, v, None), (3, v, v, None)]
    got = dev.run("p256_fe", [u32s(op, 0) + be(a) + be(b) for op, a, b, _ in cases])
    for i, ((op, a, b, want), g) in enumerate(zip(cases, got)):
        if i < n_good:
            assert li(g[:4]) == 1 and int.from_bytes(g[8:], "big") == want, (op, hex(a), hex(b))
        else:
            assert li(g[:4]) == 0, (hex(a), hex(b))


def test_p256_point_validation(dev):
    P = PR.P
    cases = []
    for pt in V.p256_points():
        e = PR.encode(pt)
        cases.append((e, 1))
        for bit in (0, 7, 100, 255):  # y with one bit flipped
            bad = bytearray(e)
            bad[64 - bit // 8] ^= 1 << (bit % 8)
            cases.append((bytes(bad), 0))
        cases += [(bytes([tag]) + e[1:], 0) for tag in (0x00, 0x02, 0x03)]
    cases += [(b"\x04" + be(P) + be(PR.GY), 0), (b"\x04" + be(PR.GX) + be(P), 0)]  # x = p, y = p
    z = PR.lift_x(0)  # x = p is 0 mod p and (0, sqrt(b)) is a point: the unreduced spelling is refused
    cases += [(PR.encode(z), 1), (b"\x04" + be(P) + be(z[1]), 0)]
    for bp in (PR.B + 1, PR.B - 1, 7):  # points of y^2 = x^3 - 3x + b' (the invalid-curve attack)
        x = 2
        while PR.lift_x(x, bp) is None:
            x += 1
        q = PR.lift_x(x, bp)
        assert PR.on_curve(q, bp) and not PR.on_curve(q)
        cases.append((PR.encode(q), 0))
    got = dev.run("p256_valid", [e + bytes(7) for e, _ in cases])
    assert [li(g) for g in got] == [v for _, v in cases]


def test_p256_scalar_ladder(dev):
    """sk * P (the _xy and _x forms agreeing) at the exceptional and random scalars on G, -G and random points, in
    one launch; sk = n reports infinity."""
    cases = [(k, pt) for pt in V.p256_points() for k in V.p256_scalars()]
    n_good = len(cases)
    cases += [(PR.N, PR.G), (PR.N, V.p256_points()[3])]
    got = dev.run("p256_mul", [be(k) + PR.encode(pt) + bytes(7) for k, pt in cases])
    for i, ((k, pt), g) in enumerate(zip(cases, got)):
        if i < n_good:
            want = PR.mul(k, pt)
            assert li(g[:4]) == 1 and g[8:] == be(want[0]) + be(want[1]), (hex(k), pt)
        else:
            assert li(g[:4]) == 0


# ---------------------------------------------------------------------------- Poly1305, GHASH, AES
def test_poly1305(dev):
    """pl_mul at the loose and fully carried limb extremes of its header; the serial poly1305 of jx_chapoly.h on
    all-0xFF and random messages under r at the clamp maximum, 0, 1 and random, s zero and all ones."""
    cases = V.pl_mul_cases()
    carried = 2**26 + 2**10 - 1
    cases += [([carried] * 5, [carried] * 5), ([M26] * 5, [M26] * 5), ([V.PL_HI_H] * 5, [carried] * 5)]
    got = dev.run("pl_mul", [u32s(*h) + u32s(*m) for h, m in cases])

    def val(a):
        return sum(v << (26 * i) for i, v in enumerate(a))

    for (h, m), g in zip(cases, got):
        out = words(g, 4)
        assert val(out) % V.P1305 == val(h) * val(m) % V.P1305, (h, m)
        assert out[1] < 2**26 + 2**10 and all(out[i] < 2**26 for i in (0, 2, 3, 4)), out

    rnd = random.Random(1305)
    rmax, one = S.R_CLAMP.to_bytes(16, "little"), (1).to_bytes(16, "little")
    aux, recs, wants = bytearray(), [], []
    for r in (rmax, bytes(16), one, b"\xff" * 16, rnd.randbytes(16), rnd.randbytes(16)):
        for s in (bytes(16), b"\xff" * 16):
            msgs = [b"\xff" * n for n in (0, 1, 15, 16, 17, 32, 64, 16 * 20, 16 * 20 + 7)]
            msgs += [rnd.randbytes(n) for n in (1, 16, 33, 100, 255)]
            for msg in msgs:
                recs.append(r + s + u32s(len(aux), len(msg)))
                aux.extend(msg)
                wants.append(S.poly1305(r + s, msg))
    got = dev.run("poly1305", recs, bytes(aux))
    assert got == wants


def test_ghash_products(dev):
    """ghash_mul and the 4-bit-table product against the oracle's GF(2^128) multiply."""
    rnd = random.Random(128)
    edge = [bytes(16), b"\xff" * 16, b"\x80" + bytes(15), bytes(15) + b"\x01", b"\xe1" + bytes(15)]
    pairs = [(x, h) for x in edge for h in edge] + [(rnd.randbytes(16), rnd.randbytes(16)) for _ in range(150)]
    pairs += [(rnd.choice(edge), rnd.randbytes(16)) for _ in range(20)] + [(rnd.randbytes(16), rnd.choice(edge)) for _ in range(20)]
    cases = [(form, x, h) for form in (0, 1) for x, h in pairs]
    got = dev.run("ghash", [u32s(form, 0) + x + h for form, x, h in cases])
    for (form, x, h), g in zip(cases, got):
        assert g == H._ghash_mul(int.from_bytes(x, "big"), int.from_bytes(h, "big")).to_bytes(16, "big"), (form, x.hex())


def test_aes128_ttable(dev):
    """The T-table AES in both key-schedule forms on the FIPS 197 Appendix C.1 vector and random blocks."""
    key, pt = bytes.fromhex("000102030405060708090a0b0c0d0e0f"), bytes.fromhex("00112233445566778899aabbccddeeff")
    rnd = random.Random(9)
    cases = [(key, pt, bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a"))]
    for _ in range(40):
        k, m = rnd.randbytes(16), rnd.randbytes(16)
        cases.append((k, m, O.aes128_encrypt(k, m)))
    cases += [(k, m, O.aes128_encrypt(k, m)) for k in (bytes(16), b"\xff" * 16) for m in (bytes(16), b"\xff" * 16)]
    full = [(otf, k, m, want) for otf in (0, 1) for k, m, want in cases]
    got = dev.run("aes_t", [u32s(otf, 0) + k + m for otf, k, m, _ in full])
    assert got == [want for _, _, _, want in full]
