"""The Prio3 instances the device prover (janus_amd/csrc/jx_shard.hip) is swept over, the geometry of
its kernels at an instance, worked out from janus_amd.vdaf.Prio3 alone, and the ledger: the conditions the matrix
has to meet so that every transform size, wave layout, absorb tail and stream exit runs (test_shard_shapes.py
asserts it on the CPU; test_gpu_shard.py runs the matrix on the device). A plain module: no GPU, no library."""
from __future__ import annotations

from dataclasses import dataclass

from janus_amd.vdaf import PRIO3_HISTOGRAM, PRIO3_SUM, PRIO3_SUMVEC, Prio3

LDS_BYTES = 64 * 1024  # what a workgroup of shard_prove_kernel may hold (SHARD_WG_LDS)

SUM_BITS = list(range(1, 22)) + [31, 32, 33, 63, 64]
SUMVEC_SHAPES = [(1, 1, 1), (2, 5, 3), (1, 3, 8), (1, 32, 8), (3, 7, 5), (1, 42, 6), (1, 40, 21), (2, 130, 7),
                 (4, 63, 5), (1, 150, 6), (1, 255, 1), (1, 1530, 6), (1, 300, 1), (1, 900, 3), (1, 1022, 2),
                 (1, 600, 1), (1, 2046, 2), (8, 1000, 88)]
HISTOGRAM_SHAPES = [(n, 1) for n in range(1, 22)] + [(3, 2), (50, 7), (64, 9), (256, 16), (600, 5), (271, 3), (355, 5)]

INSTANCES = [Prio3.sum(b) for b in SUM_BITS] + [Prio3.sum_vec(*s) for s in SUMVEC_SHAPES] + \
    [Prio3.histogram(*s) for s in HISTOGRAM_SHAPES]

W2_P512 = Prio3.sum_vec(1, 900, 3)    # two waves forced by LDS, three slots: the waves' trip counts differ
W4_P256 = Prio3.sum_vec(1, 1530, 6)   # four waves holding the whole 64 KiB


def shape_id(v: Prio3) -> str:
    if v.algo_id == PRIO3_SUM:
        return f"sum{v.bits}"
    if v.algo_id == PRIO3_SUMVEC:
        return f"sumvec{v.bits}x{v.length}c{v.chunk_length}"
    assert v.algo_id == PRIO3_HISTOGRAM
    return f"hist{v.length}c{v.chunk_length}"


@dataclass(frozen=True)
class Geometry:
    two_wire: bool       # SumVec and Histogram (ParallelSum of Mul); Sum has the one wire of Range2
    P: int               # transform size
    calls: int           # gadget calls: points 1..calls of a wire are live, the rest up to P - 1 zero
    chunk: int           # wire pairs (1 for Sum)
    W: int               # waves of a prove workgroup
    chunk_mod_W: int     # != 0: the waves walk different numbers of slots
    padded: int          # slots of the last call past the measurement
    meas_mod_21: int     # decides where shard_absorb_kernel's padding byte lands
    absorb_blocks: int   # (42 + 16 meas_len) // 168
    streams: tuple       # the lengths xof_stream128 is asked for: measurement share, prove randomness, proof share


def geometry(v: Prio3) -> Geometry:
    two_wire = v.algo_id != PRIO3_SUM
    chunk = v.chunk_length if two_wire else 1
    W = max(1, min(4, LDS_BYTES // (64 * v.P), chunk)) if two_wire else 1
    proof_len = v.arity + 2 * v.P - 1
    assert proof_len == v.proof_len
    return Geometry(two_wire, v.P, v.calls, chunk, W, chunk % W, v.calls * chunk - v.meas_len if two_wire else 0,
                    v.meas_len % 21, (42 + 16 * v.meas_len) // 168, (v.meas_len, v.arity, proof_len))


def unmet(instances) -> list:
    """The ledger's conditions that `instances` does not meet, as sentences; empty when the matrix is complete."""
    gs = [(v, geometry(v)) for v in instances]
    two = [g for _, g in gs if g.two_wire]
    one = [g for _, g in gs if not g.two_wire]
    miss = []

    def need(ok, what):
        if not ok:
            miss.append(what)

    # 1. transform sizes
    for lg in range(1, 11):
        need(any(g.P == 1 << lg for g in two), f"two-wire P = {1 << lg}")
    for lg in range(1, 8):
        need(any(g.P == 1 << lg for g in one), f"one-wire P = {1 << lg}")
    for bits in (8, 16, 32, 64):
        need(any(v.algo_id == PRIO3_SUM and v.bits == bits for v, _ in gs), f"Prio3Sum bits = {bits}")
    # 2. wave layouts
    for W, rem in ((1, 0), (2, 0), (2, 1), (3, 0), (4, 0), (4, 1), (4, 2), (4, 3)):
        need(any((g.W, g.chunk_mod_W) == (W, rem) for g in two), f"W = {W} with chunk % W = {rem}")
    need(any(g.W == 2 and g.P == 512 and g.chunk >= 3 for g in two), "W = 2 at P = 512 with chunk >= 3")
    need(any(g.W == 4 and g.P == 256 for g in two), "W = 4 at P = 256")
    # 3. the zero tail of a wire
    need(any(g.calls == g.P - 1 and 4 <= g.P <= 16 for g in two), "calls = P - 1 at some 4 <= P <= 16")
    for P in (256, 512, 1024):
        need(any(g.calls == g.P - 1 and g.P == P for g in two), f"calls = P - 1 at P = {P}")
    need(any(g.calls == g.P // 2 and g.P >= 4 for g in two), "calls = P / 2 at some P >= 4")
    # 4. the last call
    need(any(g.padded > 0 for g in two), "a last call with padded slots")
    need(any(g.padded == 0 for g in two), "a last call without padded slots")
    need(any(g.chunk > g.streams[0] for g in two), "a chunk longer than the measurement")
    # 5. the absorb kernel's tail (every instance here has joint randomness)
    jr = [g for v, g in gs if v.joint_rand_len]
    for res in range(21):
        need(any(g.meas_mod_21 == res for g in jr), f"meas_len mod 21 = {res}")
    for res in (8, 18):
        need(any(g.meas_mod_21 == res and g.absorb_blocks >= 3 for g in jr),
             f"meas_len mod 21 = {res} with at least three absorb blocks")
    # 6. the exits of xof_stream128
    for si, name in enumerate(("measurement share", "prove randomness", "proof share")):
        for res in (0, 10, 11):
            need(any(g.streams[si] % 21 == res for g in two), f"{name} stream of length = {res} mod 21")
        need(any(g.streams[si] < 10 for g in two), f"{name} stream shorter than 10")
    return miss
