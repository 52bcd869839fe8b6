"""Reports from a cheating client, wire-level edits and per-element decide sweeps (shared helper).

Everything the suite rejected before this module was an honest client's report with a damaged
leader prep share. Here the inputs are
  * cheats: a proof that is perfectly consistent with an invalid measurement (a "bit" of 2, a
    Histogram with two buckets set, ...), sharded by oracle/pyref.py's shard_encoded;
  * wire edits: one flipped bit in a helper input share seed, the public share, the leader blind or a
    leader share element, after which the leader prepares from what it received;
  * decide sweeps: one honest report whose leader prep share has exactly one verifier element
    replaced by x + 1 (re-encoded canonically), once per element of every proof, and one copy per
    byte of the joint-randomness part with that byte's low bit flipped;
  * order cases: two defects at once, to pin which verdict wins.
Leader prep shares always come from the C oracle's prep_init, and expected results from its
helper_prep_batch. tests/test_oracle_dishonest.py proves on the CPU that every case has the
designed verdict in both restatements, so the GPU tests of tests/test_gpu_dishonest.py cannot pass
emptily. Sets are built once per instance and shared by both modules.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from janus_amd.vdaf import Prio3
from oracle import oracle as O
from oracle import pyref

P128 = 2**128 - 28 * 2**64 + 1

# name -> (pyref kind, bits, length, chunk, proofs); the smallest instances that reach every decide
# kernel and every group layout of the FLP kernels
INSTANCES = {
    "count": ("count", 0, 0, 0, 1),
    "sum1": ("sum", 1, 0, 0, 1),
    "sum3": ("sum", 3, 0, 0, 1),
    "sum8": ("sum", 8, 0, 0, 1),
    "sumvec_1x4_1": ("sumvec", 1, 4, 1, 1),
    "sumvec_2x5_2": ("sumvec", 2, 5, 2, 1),
    "sumvec_2x5_3": ("sumvec", 2, 5, 3, 1),
    "sumvec_1x20_9": ("sumvec", 1, 20, 9, 1),
    "histogram_4_1": ("histogram", 0, 4, 1, 1),
    "histogram_5_3": ("histogram", 0, 5, 3, 1),
    "histogram_19_9": ("histogram", 0, 19, 9, 1),
    "mp2_2x5_3": ("sumvec_f64_multiproof", 2, 5, 3, 2),
    "mp3_1x7_3": ("sumvec_f64_multiproof", 1, 7, 3, 3),
    "mp8_2x33_4": ("sumvec_f64_multiproof", 2, 33, 4, 8),
    "fp16_len4": ("fixedpoint", 16, 4, 0, 1),
    "fp32_len3": ("fixedpoint", 32, 3, 0, 1),
}
BOTH_ROLES = ("sumvec_2x5_3", "histogram_5_3", "mp3_1x7_3")


class Instance:
    def __init__(self, name: str):
        kind, bits, length, chunk, proofs = INSTANCES[name]
        self.name, self.kind = name, kind
        if kind == "count":
            self.vdaf, self.py = Prio3.count(), pyref.Prio3("count")
        elif kind == "sum":
            self.vdaf, self.py = Prio3.sum(bits), pyref.Prio3("sum", bits=bits)
        elif kind == "sumvec":
            self.vdaf = Prio3.sum_vec(bits, length, chunk)
            self.py = pyref.Prio3("sumvec", bits=bits, length=length, chunk=chunk)
        elif kind == "histogram":
            self.vdaf = Prio3.histogram(length, chunk)
            self.py = pyref.Prio3("histogram", length=length, chunk=chunk)
        elif kind == "sumvec_f64_multiproof":
            self.vdaf = Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(proofs, bits, length, chunk)
            self.py = pyref.Prio3(kind, proofs=proofs, bits=bits, length=length, chunk=chunk)
        else:
            self.vdaf = Prio3.fixedpoint_boundedl2_vec_sum(bits, length)
            self.py = pyref.Prio3("fixedpoint", bits=bits, length=length)
        v = self.vdaf
        self.orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)
        self.p = self.py.F.p
        self.fb = v.field_bytes
        self.vk = bytes(range(60, 60 + v.verify_key_len))
        self.seed = sum(map(ord, name)) * 101 + 7
        # one pyref prep_init per distinct report, however many leader prep shares are tried on it
        self.py.prep_init = functools.lru_cache(maxsize=None)(self.py.prep_init)

    # ---------------------------------------------------------------- measurements
    def honest_measurement(self, rng):
        v = self.vdaf
        if self.kind == "count":
            return int(rng.integers(0, 2))
        if self.kind == "sum":
            return int(rng.integers(0, 1 << v.bits))
        if self.kind == "histogram":
            return int(rng.integers(0, v.length))
        if self.kind == "fixedpoint":  # squared norm well below 1
            lim = (1 << (v.bits - 1)) // (2 * v.length)
            return [int(x) & ((1 << v.bits) - 1) for x in rng.integers(-lim, lim, size=v.length)]
        return [int(x) for x in rng.integers(0, 1 << v.bits, size=v.length)]

    def encode(self, m):
        return self.py.valid.encode(m)

    def truncate(self, elems):
        return self.py.valid.truncate(elems)


@dataclass
class Row:
    """One report of a batch: its wire bytes, the leader prep share the helper receives, and what
    the case was designed to give."""
    label: str            # "" for an honest report
    nonce: bytes
    ps: bytes
    lis: bytes
    his: bytes
    lps: bytes
    expect: int | None    # the designed helper verdict (None: any rejection)
    rc: int = 0           # the oracle's leader prep_init status
    truth: list | None = None      # honest reports: the truncated measurement
    leader_side: bool = False      # wire edits of the leader input share or the public share


@dataclass
class Batch:
    inst: Instance
    rows: list
    nonces: np.ndarray = field(init=False)
    ps: np.ndarray = field(init=False)
    lis: np.ndarray = field(init=False)
    his: np.ndarray = field(init=False)
    lps: np.ndarray = field(init=False)
    want: dict = field(init=False)     # the C oracle's helper_prep_batch on this batch

    def __post_init__(self):
        n = len(self.rows)

        def cat(attr):
            w = len(getattr(self.rows[0], attr))
            if w == 0:
                return np.zeros((n, 0), np.uint8)
            return np.frombuffer(b"".join(getattr(r, attr) for r in self.rows), np.uint8).reshape(n, w).copy()
        self.nonces, self.ps, self.lis, self.his, self.lps = (cat(a) for a in ("nonce", "ps", "lis", "his", "lps"))
        i = self.inst
        self.want = i.orc.helper_prep_batch(i.vk, self.nonces, self.ps, self.his, self.lps, nthreads=4,
                                            want_out_shares=True)

    @property
    def n(self):
        return len(self.rows)

    @property
    def labels(self):
        return [r.label for r in self.rows]

    @property
    def bad(self):
        return [k for k, r in enumerate(self.rows) if r.label]

    def expected(self):
        """The designed verdicts; None where the design only says 'rejected'."""
        return [r.expect for r in self.rows]

    def describe(self, k):
        return f"{self.inst.name} lane {k}: {self.rows[k].label or 'honest'}"


# -------------------------------------------------------------------- building blocks


def _rand_bytes(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _leader_prep(inst: Instance, nonce, ps, lis):
    rc, share, _, _ = inst.orc.prep_init(inst.vk, 0, nonce, ps, lis)
    return rc, share


def honest_row(inst: Instance, rng) -> Row:
    m = inst.honest_measurement(rng)
    nonce, rand = _rand_bytes(rng, 16), _rand_bytes(rng, inst.orc.sizes.client_rand)
    ps, lis, his = inst.orc.shard(m, nonce, rand)
    rc, lps = _leader_prep(inst, nonce, ps, lis)
    return Row("", nonce, ps, lis, his, lps, 0, rc, truth=inst.truncate(inst.encode(m)))


def cheat_row(inst: Instance, label: str, elems, rng) -> Row:
    """A consistent proof of the (invalid) encoded measurement `elems`."""
    nonce, rand = _rand_bytes(rng, 16), _rand_bytes(rng, inst.orc.sizes.client_rand)
    ps, lis, his = inst.py.shard_encoded(elems, nonce, rand)
    rc, lps = _leader_prep(inst, nonce, ps, lis)
    return Row(label, nonce, ps, lis, his, lps, 3, rc)


def cheat_measurements(inst: Instance, rng) -> list:
    """(label, encoded measurement) of every cheat kind of the instance."""
    v, p = inst.vdaf, inst.p
    out = []
    if inst.kind == "count":
        return [("count element 2", [2]), ("count element p-1", [p - 1]), ("count element (p+1)/2", [(p + 1) // 2])]
    if inst.kind in ("sum", "sumvec", "sumvec_f64_multiproof"):
        n = v.meas_len
        pos = [0, n - 1] if inst.kind == "sum" else [0, v.chunk_length - 1, v.chunk_length, n - 1]
        pos = sorted({q for q in pos if 0 <= q < n})
        for q in pos:
            for val, what in ((2, "2"), (p - 1, "p-1")):
                e = inst.encode(inst.honest_measurement(rng))
                e[q] = val
                out.append((f"element {q} = {what}", e))
        if len(pos) >= 2:
            e = inst.encode(inst.honest_measurement(rng))
            e[pos[0]], e[pos[-1]] = 2, p - 1
            out.append((f"elements {pos[0]} = 2 and {pos[-1]} = p-1", e))
        return out
    if inst.kind == "histogram":
        n = v.length
        zero = [0] * n
        two = [1] + [0] * (n - 2) + [1]
        swap = [2] + [0] * (n - 2) + [p - 1]
        one2 = [0] * n
        one2[n // 2] = 2
        return [("all zero (sum fails)", zero), ("two ones (range passes, sum fails)", two),
                ("2 and p-1 (sum passes, range fails)", swap), (f"entry {n // 2} = 2 alone", one2)]
    # fixedpoint: entries' bits || claimed norm's bits
    nb, E = v.bits, v.length
    base = inst.encode(inst.honest_measurement(rng))
    e = list(base)
    e[nb + 3] = 2
    out.append(("entry bit = 2", e))
    e = list(base)
    e[nb * E + 5] = 2
    out.append(("claimed-norm bit = 2", e))
    e = list(base)
    e[nb * E] ^= 1
    out.append(("honest bits, claimed norm != computed norm (range passes)", e))
    # the same value spelled with a 2: bits (0, 1) at (j, j+1) become (2, 0); only the range check fails
    for lo, hi, what in ((0, nb * E, "entry"), (nb * E, len(base), "claimed-norm")):
        width = nb if what == "entry" else hi - lo
        for j in range(lo, hi - 1):
            if base[j] == 0 and base[j + 1] == 1 and (j - lo) % width != width - 1:
                e = list(base)
                e[j], e[j + 1] = 2, 0
                out.append((f"{what} bits (0,1) spelled (2,0): norm passes, range fails", e))
                break
    return out


def cheat_rows(inst: Instance, rng) -> list:
    kinds = cheat_measurements(inst, rng)
    rows = [cheat_row(inst, label, e, rng) for label, e in kinds]
    k = 0
    while len(rows) < 4:  # the layout has four fixed lanes to fill: the same kinds with fresh randomness
        label, e = kinds[k % len(kinds)]
        rows.append(cheat_row(inst, label + " (again)", e, rng))
        k += 1
    return rows


def _flip_element_below_p(buf: bytearray, off: int, fb: int, p: int):
    x = int.from_bytes(buf[off:off + fb], "little")
    for bit in range(8 * fb):
        if (x ^ (1 << bit)) < p:
            buf[off:off + fb] = (x ^ (1 << bit)).to_bytes(fb, "little")
            return
    raise AssertionError("no bit keeps the element below p")


def wire_rows(inst: Instance, rng) -> list:
    """One honest report per kind, one bit flipped on the wire; the leader prepares afterwards."""
    v, S, fb = inst.vdaf, inst.vdaf.seed_size, inst.fb
    jr = v.joint_rand_len > 0
    kinds = [("helper measurement seed", "his", 0), ("helper proof seed", "his", S)]
    if jr:
        kinds += [("helper blind", "his", 2 * S), ("public share, leader half", "ps", 0),
                  ("public share, helper half", "ps", S), ("leader blind", "lis", v.leader_input_share_len - S)]
    kinds += [("leader measurement element", "lis-elem", (v.meas_len // 2) * fb),
              ("last leader proof element", "lis-elem", (v.meas_len + v.num_proofs * v.proof_len - 1) * fb)]
    rows = []
    for label, where, off in kinds:
        r = honest_row(inst, rng)
        ps, lis, his = bytearray(r.ps), bytearray(r.lis), bytearray(r.his)
        if where == "lis-elem":
            _flip_element_below_p(lis, off, fb, inst.p)
        else:
            {"his": his, "ps": ps, "lis": lis}[where][off + int(rng.integers(0, S))] ^= 1 << int(rng.integers(0, 8))
        ps, lis, his = bytes(ps), bytes(lis), bytes(his)
        rc, lps = _leader_prep(inst, r.nonce, ps, lis)
        rows.append(Row("wire: " + label, r.nonce, ps, lis, his, lps, None, rc,
                        leader_side=where in ("ps", "lis", "lis-elem")))
    return rows


def _with_lps(r: Row, label: str, lps: bytes, expect: int) -> Row:
    return Row(label, r.nonce, r.ps, r.lis, r.his, lps, expect, r.rc)


def _plus_one(lps: bytes, k: int, fb: int, p: int) -> bytes:
    x = int.from_bytes(lps[k * fb:(k + 1) * fb], "little")
    return lps[:k * fb] + ((x + 1) % p).to_bytes(fb, "little") + lps[(k + 1) * fb:]


def sweep_rows(inst: Instance, r: Row) -> list:
    """Every verifier element of every proof + 1 (-> 3), every part byte's low bit flipped (-> 4)."""
    v, fb, p = inst.vdaf, inst.fb, inst.p
    VL = v.verifier_len
    rows = []
    for k in range(VL * v.num_proofs):
        rows.append(_with_lps(r, f"sweep: proof {k // VL} element {k % VL} + 1", _plus_one(r.lps, k, fb, p), 3))
    if v.joint_rand_len:
        base = VL * v.num_proofs * fb
        for b in range(v.seed_size):
            t = bytearray(r.lps)
            t[base + b] ^= 1
            rows.append(_with_lps(r, f"sweep: joint-rand part byte {b} low bit", bytes(t), 4))
    return rows


def order_rows(inst: Instance, r: Row) -> list:
    """Two defects at once: decode failure (2) before decide (3) before the joint-rand check (4)."""
    v, fb, p = inst.vdaf, inst.fb, inst.p
    nel = v.verifier_len * v.num_proofs
    v1 = _plus_one(r.lps, 0, fb, p)                       # proof 0's v
    ge = lambda b: b[:(nel - 1) * fb] + b"\xff" * fb + b[nel * fb:]  # noqa: E731  last element of the last proof >= p
    rows = [_with_lps(r, f"order: proof {v.num_proofs - 1} element {v.verifier_len - 1} >= p with v + 1", ge(v1), 2)]
    if v.joint_rand_len:
        part = lambda b: b[:-1] + bytes([b[-1] ^ 0x80])  # noqa: E731
        rows += [_with_lps(r, "order: v + 1 with a flipped part", part(v1), 3),
                 _with_lps(r, "order: element >= p with a flipped part", part(ge(r.lps)), 2),
                 _with_lps(r, "order: flipped part alone", part(r.lps), 4)]
    return rows


def layout(inst: Instance, bad: list, honest) -> Batch:
    """Honest reports between the bad ones; a bad one at lane 0, 63, 64 and the last lane of a partial
    final block. `honest()` gives the next honest row."""
    assert len(bad) >= 4
    n = max(2 * len(bad) + 2, 70)
    if n % 64 == 0:
        n += 2
    slots = [0, 63, 64, n - 1] + [k for k in range(2, n - 1, 2) if k != 64]
    rows = [None] * n
    for k, r in zip(slots, bad):
        rows[k] = r
    rows = [r if r is not None else honest() for r in rows]
    assert n > 64 and n % 64 and all(rows[k].label for k in (0, 63, 64, n - 1))
    return Batch(inst, rows)


# Built once per instance and process, on first use; both test modules share them.


@functools.lru_cache(maxsize=None)
def instance(name: str) -> Instance:
    return Instance(name)


@functools.lru_cache(maxsize=None)
def cheat_batch(name: str) -> Batch:
    """The cheats between distinct honest reports (the only set that runs pyref's prover)."""
    inst = instance(name)
    rng = np.random.default_rng(inst.seed)
    return layout(inst, cheat_rows(inst, rng), lambda: honest_row(inst, rng))


@functools.lru_cache(maxsize=None)
def wire_batch(name: str) -> Batch:
    """The wire edits between distinct honest reports."""
    inst = instance(name)
    rng = np.random.default_rng(inst.seed + 1)
    return layout(inst, wire_rows(inst, rng), lambda: honest_row(inst, rng))


@functools.lru_cache(maxsize=None)
def sweep_batch(name: str) -> Batch:
    """Sweep and order cases of one honest report, its unmodified copies between them."""
    inst = instance(name)
    target = honest_row(inst, np.random.default_rng(inst.seed + 2))
    return layout(inst, sweep_rows(inst, target) + order_rows(inst, target), lambda: target)


def counts(name: str) -> dict:
    sw = sweep_batch(name).labels
    return {"cheat": len(cheat_batch(name).bad), "wire": len(wire_batch(name).bad),
            "sweep": sum(s.startswith("sweep:") for s in sw), "order": sum(s.startswith("order:") for s in sw)}
