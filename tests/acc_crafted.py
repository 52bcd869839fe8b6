"""Crafted output shares for the accumulation kernels (shared helper).

Every other test accumulates what an honest prepare produced: random field elements. Here a test chooses
every output-share element. The leader's output share is its explicit measurement share, and the leader
accepts a report whenever the prep message equals its own corrected joint-randomness seed (the proof plays
no part on the leader), which the C oracle's prep_init returns as its fourth value. So, for instances whose
truncation is the identity (Count, Histogram, SumVec of 1-bit entries):
  * the wanted canonical elements are the measurement part of the leader input share, the proof part is any
    canonical elements, the blind and the public share are any bytes;
  * leader_initialized_batch, then leader_continued_batch with the oracle's seeds (nothing for Count, which
    has no joint randomness), leaves exactly those elements as the batch's output shares.
craft() builds such reports and asserts, per report, that the oracle agrees (rc 0, output share == the
crafted row); model() is the reference aggregate in Python integers with hashlib's SHA-256, sharing no code
with the engine or the C oracle. tests/test_acc_crafted.py keeps both honest on the CPU;
tests/test_gpu_accumulate_edges.py runs every accumulate path of the engine on them.
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass

import numpy as np

from janus_amd.vdaf import Prio3
from math_vectors import EDGE, EDGE64, P64, P128
from oracle import oracle as O

# name -> the instance; out_len 5 is no multiple of the 4 waves of a workgroup, 257 + 1 crosses a 256-thread
# workgroup of the combine kernels, 6000 lowers accumulate_many's segments per pass below SEG_MAX
INSTANCES = {
    "count": Prio3.count,
    "hist5": lambda: Prio3.histogram(5, 2),
    "mp5": lambda: Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 1, 5, 2),
    "hist257": lambda: Prio3.histogram(257, 16),
    "hist6000": lambda: Prio3.histogram(6000, 78),
}

REJECT_INIT, REJECT_FINISH = 1, 4  # the leader's verdicts: prepare_init failure, prepare_next failure


class Instance:
    def __init__(self, name: str):
        v = self.vdaf = INSTANCES[name]()
        self.name = name
        self.orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)
        self.fb = v.field_bytes
        self.p = P64 if self.fb == 8 else P128
        self.out_len = v.output_len
        self.vk = bytes(range(90, 90 + v.verify_key_len))
        self.joint_rand = v.joint_rand_len > 0
        assert v.meas_len == v.output_len, "the truncation must be the identity"

    def encode(self, row) -> bytes:
        return b"".join(int(x).to_bytes(self.fb, "little") for x in row)


@functools.lru_cache(maxsize=None)
def instance(name: str) -> Instance:
    return Instance(name)


# -------------------------------------------------------------------- value patterns over (report r, element j)


def _edges(inst):
    return [x for x in (EDGE64 if inst.fb == 8 else EDGE) if x < inst.p]


def pattern_names(inst: Instance) -> tuple:
    return ("all_max", "cancel", "edge_cycle", "random") + (("carry64",) if inst.fb == 16 else ())


def pattern(inst: Instance, name: str, n: int, seed: int = 0) -> list:
    """n rows of out_len canonical elements (Python ints).
    all_max: every element p - 1; cancel: p - 1 and 1 alternating by report (an even selection sums to a multiple
    of p); edge_cycle: the canonical EDGE / EDGE64 entries by (r + j); random: uniform below p; carry64 (Field128):
    2^64 - 1 and 2^64 in neighbouring reports (the low word carries on every second add)."""
    p, m = inst.p, inst.out_len
    if name == "all_max":
        return [[p - 1] * m for _ in range(n)]
    if name == "cancel":
        return [[p - 1 if r % 2 == 0 else 1] * m for r in range(n)]
    if name == "edge_cycle":
        e = _edges(inst)
        return [[e[(r + j) % len(e)] for j in range(m)] for r in range(n)]
    if name == "random":
        rng = np.random.default_rng([seed, n, m])
        raw = rng.integers(0, 256, size=(n, m, inst.fb), dtype=np.uint8)
        return [[int.from_bytes(raw[r, j].tobytes(), "little") % p for j in range(m)] for r in range(n)]
    if name == "carry64":
        assert inst.fb == 16
        return [[2**64 - 1 if (r + j) % 2 == 0 else 2**64 for j in range(m)] for r in range(n)]
    raise KeyError(name)


# -------------------------------------------------------------------- crafted reports


@dataclass
class Crafted:
    inst: Instance
    elems: list               # n rows of out_len ints: the output share of every accepted report
    nonces: np.ndarray        # uint8[n, 16]
    ps: np.ndarray            # uint8[n, public share]
    lis: np.ndarray           # uint8[n, leader input share]
    msgs: np.ndarray | None   # uint8[n, seed]: the prep messages to finish with; None for Count
    verdicts: np.ndarray      # uint8[n]: the designed leader verdict after finish (0, 1 or 4)
    outs: np.ndarray          # uint8[n, out_len * field bytes]: elems, encoded

    @property
    def n(self):
        return len(self.elems)

    @property
    def accepted(self):
        return self.verdicts == 0

    def out_bytes(self, r) -> bytes:
        return self.outs[r].tobytes()

    def take(self, idx) -> "Crafted":
        """The reports idx (a slice or an index array), in that order."""
        idx = np.arange(self.n)[idx]
        return Crafted(self.inst, [self.elems[i] for i in idx], self.nonces[idx], self.ps[idx], self.lis[idx],
                       None if self.msgs is None else self.msgs[idx], self.verdicts[idx], self.outs[idx])


def craft(inst: Instance, elems, seed: int, reject_init=(), reject_finish=()) -> Crafted:
    """Reports whose leader output shares are the rows of elems (n x out_len ints below p).
    reject_init: rows whose first element is sent as p (not canonical: verdict 1 at init); reject_finish: rows with
    one bit of the prep message flipped (verdict 4 at finish; instances with joint randomness only). Asserts, per
    report, the oracle's outcome: rc 0 and the crafted row, or the rejection."""
    v, fb, p = inst.vdaf, inst.fb, inst.p
    n = len(elems)
    rng = np.random.default_rng([seed, n, 0xACC])
    S = v.seed_size
    nproof = v.num_proofs * v.proof_len
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    ps = rng.integers(0, 256, size=(n, v.public_share_len), dtype=np.uint8)
    proofs = rng.integers(0, 256, size=(n, nproof, fb), dtype=np.uint8)
    proofs[:, :, fb - 1] &= 0x7F  # below 2^(8 fb - 1) < p: canonical
    blinds = rng.integers(0, 256, size=(n, S if inst.joint_rand else 0), dtype=np.uint8)
    reject_init, reject_finish = set(reject_init), set(reject_finish)
    assert not reject_finish or inst.joint_rand, "Count has no prep message to damage"
    assert not (reject_init & reject_finish)
    lis = np.zeros((n, v.leader_input_share_len), np.uint8)
    msgs = np.zeros((n, S), np.uint8) if inst.joint_rand else None
    verdicts = np.zeros(n, np.uint8)
    outs = np.zeros((n, inst.out_len * fb), np.uint8)
    for r in range(n):
        row = list(elems[r])
        assert len(row) == inst.out_len and all(0 <= x < p for x in row)
        outs[r] = np.frombuffer(inst.encode(row), np.uint8)
        sent = [p] + row[1:] if r in reject_init else row
        share = inst.encode(sent) + proofs[r].tobytes() + blinds[r].tobytes()
        lis[r] = np.frombuffer(share, np.uint8)
        rc, _, out, corr = inst.orc.prep_init(inst.vk, 0, nonces[r].tobytes(), ps[r].tobytes(), share)
        if r in reject_init:
            assert rc != 0, (inst.name, r, "an element of p must fail the leader's decode")
            verdicts[r] = REJECT_INIT
            continue
        assert rc == 0 and out == outs[r].tobytes(), (inst.name, r)
        if msgs is not None:
            msgs[r] = np.frombuffer(corr[:S], np.uint8)
            if r in reject_finish:
                msgs[r, int(rng.integers(0, S))] ^= 1 << int(rng.integers(0, 8))
                verdicts[r] = REJECT_FINISH
    return Crafted(inst, [list(map(int, row)) for row in elems], nonces, ps, lis, msgs, verdicts, outs)


def spread_rejects(inst: Instance, n: int):
    """Rejected rows for n reports: rows 5, 28, 51, ... at init and rows 16, 39, 62, ... at finish (at init too for
    Count). The period of 23 walks the rejections through every lane of the 64-report blocks, and any slice of 23
    rows holds one of each kind."""
    init = [r for r in range(n) if r % 23 == 5 or (r % 23 == 16 and not inst.joint_rand)]
    fin = [r for r in range(n) if r % 23 == 16 and inst.joint_rand]
    return init, fin


POOL_N = 6144


@functools.lru_cache(maxsize=None)
def pool(name: str, pat: str, n: int = POOL_N) -> Crafted:
    """n crafted reports of one instance and pattern with spread_rejects' rejections, built once per process;
    tests take slices of it as their batches."""
    inst = instance(name)
    init, fin = spread_rejects(inst, n)
    seed = sum(map(ord, name + pat))
    return craft(inst, pattern(inst, pat, n, seed), seed, init, fin)


# -------------------------------------------------------------------- the reference


def model(p: int, fb: int, elems, nonces, selected, prev=None):
    """(aggregate bytes, count, checksum) after merging the rows `selected` (indices, repeats allowed, or a boolean
    array) of elems / nonces into prev (default: the empty aggregation). Python integers and hashlib only."""
    sel = np.asarray(selected)
    idx = np.nonzero(sel)[0] if sel.dtype == bool else sel.astype(np.int64)
    m = len(elems[0]) if len(elems) else (len(prev[0]) // fb if prev else 0)
    if prev is None:
        total, count, cs = [0] * m, 0, 0
    else:
        total = [int.from_bytes(prev[0][fb * j:fb * j + fb], "little") for j in range(m)]
        count, cs = prev[1], int.from_bytes(prev[2], "big")
    for r in idx:
        row = elems[int(r)]
        for j in range(m):
            total[j] += row[j]
        count += 1
        cs ^= int.from_bytes(hashlib.sha256(bytes(nonces[int(r)])).digest(), "big")
    return b"".join((x % p).to_bytes(fb, "little") for x in total), count, cs.to_bytes(32, "big")


def empty(inst: Instance):
    return bytes(inst.out_len * inst.fb), 0, bytes(32)
