"""GPU: the accumulation kernels (K4) on crafted output shares, every path and branch, against Python integers.

K4 is the one stage whose wrong result lands in a batch aggregation silently: no verdict depends on it. Every other
test feeds it honest, random output shares. Here every output-share element is chosen (tests/acc_crafted.py: the
leader's output share is its explicit measurement share, and the leader accepts on the oracle's own corrected seed):
columns of p - 1, columns that sum to an exact multiple of p, the arithmetic edge values, carries out of the low and
the middle accumulator word on every add, and an existing aggregate of p - n under all of them.

Every case sets up through prepared(): leader init and finish on the engine, the verdicts asserted to be the designed
ones and the output shares asserted to be the crafted rows byte for byte, so a later failure is the accumulate's.
It then accumulates by the path under test and compares aggregate_share() of every aggregation touched with
acc_crafted.model(), exactly. Every batch holds rejected rows of both kinds, every aggregation is accumulated into at
least twice, and accept masks hold bytes from {0, 1, 2, 255}: include/jx_prio3.h takes a report when
accept_mask[i] != 0, and so does the model.

Case -> kernel and branch:
  1 test_one_kernel_path      accumulate_small_kernel (debug 8 = 0), n around the 64-report block and at ACC_SMALL
  2 test_chunked_path         select / accumulate / reduce_partials, debug 2 splitting 17, 24 and 25 blocks into the
                              unrolled 4-block loop plus every remainder, and into chunks past the last block
  3 test_deferred_path,       accumulate_multi_kernel: a wave with one batch and with two, ACC_MULTI_MAX and a second
    test_deferred_report_budget  launch; flushed by the 64th deferral, by the report budget, by debug 9, by the read
  4 test_segmented_path       seg_* kernels, host and device forms: item lengths L - 1, L, L + 1, 2 L + 1, one long
                              item per segment (the unrolled gather loop), unnamed and out-of-range table entries
  5 test_more_than_seg_max    the second and third pass of accumulate_many (s0 > 0)
  6 test_lowered_ns_max       the pass size lowered below SEG_MAX by the partials budget
  7 test_combine_*            combine_kernel / record_combine_kernel: sums of exactly p, out_len + 1 across a workgroup
"""
from __future__ import annotations

import numpy as np
import pytest

import acc_crafted as A
from janus_amd import distributed as D
from janus_amd._lib import EngineError
from janus_amd.engine import HelperEngine

pytestmark = pytest.mark.gpu

MASK_BYTES = np.array([0, 1, 2, 255], np.uint8)
SEG_MAX, ACC_SMALL, ACC_MULTI_MAX = 4096, 1024, 64  # jx_kernels.h


def prepared(eng, c) -> int:
    """Leader init and finish of the crafted batch c on the engine; returns the batch id, ready to accumulate."""
    init = eng.leader_initialized_batch(c.nonces, c.ps, c.lis)
    np.testing.assert_array_equal(init.verdicts, (c.verdicts == A.REJECT_INIT).astype(np.uint8))
    fin = eng.leader_continued_batch(c.msgs, want_out_shares=True, init=init)
    np.testing.assert_array_equal(fin.verdicts, c.verdicts)
    ok = c.accepted
    np.testing.assert_array_equal(fin.out_shares[ok], c.outs[ok])
    return fin.batch_id


class Ledger:
    """What every aggregation must hold, by acc_crafted.model()."""

    def __init__(self, inst):
        self.inst, self.state = inst, {}

    def add(self, agg_id, c, sel):
        i = self.inst
        self.state[int(agg_id)] = A.model(i.p, i.fb, c.elems, c.nonces, sel, prev=self.state.get(int(agg_id)))

    def add_by_index(self, c, sel, dense, table):
        """Rows sel of c into table[dense[r]]; indices at and past len(table) are skipped."""
        groups = {}
        for r in np.nonzero(sel)[0]:
            if dense[r] < len(table):
                groups.setdefault(int(table[dense[r]]), []).append(int(r))
        for agg_id, rows in groups.items():
            self.add(agg_id, c, np.array(rows, np.int64))
        return set(groups)

    def check(self, eng, ids=None, what=""):
        for agg_id in (self.state if ids is None else ids):
            want = self.state.get(int(agg_id), A.empty(self.inst))
            assert eng.aggregate_share(int(agg_id)) == want, (self.inst.name, what, int(agg_id))


def engine(inst):
    return HelperEngine(inst.vdaf, inst.vk)


def distinct_ids(rng, k):
    """k distinct arbitrary u32 batch-aggregation ids (not 0), in random order."""
    ids = np.unique(rng.integers(1, 1 << 32, size=2 * k + 8, dtype=np.uint64))
    assert len(ids) >= k
    return rng.permutation(ids)[:k].astype(np.uint32)


def random_mask(rng, n):
    m = rng.choice(MASK_BYTES, size=n)
    if n >= 4:  # every byte value present
        m[rng.choice(n, size=4, replace=False)] = MASK_BYTES
    return m


# ---------------------------------------------------------------------------- 1: the one-kernel path


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024])
@pytest.mark.parametrize("name", ["count", "hist5", "mp5"])
def test_one_kernel_path(name, n):
    """accumulate_small_kernel: three batches per aggregation (the second and third meet an existing aggregate; the
    third starts with a rejected row) with no mask, with a random mask, and with an all-zero mask on the last two,
    which leaves aggregate, count and checksum as they were."""
    inst = A.instance(name)
    rng = np.random.default_rng(n)
    with engine(inst) as eng:
        eng.debug(8, 0)
        led = Ledger(inst)
        agg_id = 1000
        for pat in A.pattern_names(inst):
            pool = A.pool(name, pat)
            for mode in ("none", "random", "zero"):
                agg_id += 1
                for k, off in enumerate((7, 2900, 1201)):
                    c = pool.take(slice(off, off + n))
                    mask = None
                    if mode == "random":
                        mask = random_mask(rng, n)
                    elif mode == "zero" and k > 0:
                        mask = np.zeros(n, np.uint8)
                    bid = prepared(eng, c)
                    eng.accumulate(n, mask, np.full(n, agg_id, np.uint32), batch_id=bid)
                    led.add(agg_id, c, c.accepted if mask is None else c.accepted & (mask != 0))
                    led.check(eng, [agg_id], (pat, mode, k))
        # all_max without a mask: the existing aggregate was p - (the reports so far)
        assert led.state[1001][0] == (-led.state[1001][1] % inst.p).to_bytes(inst.fb, "little") * inst.out_len


# ---------------------------------------------------------------------------- 2: the chunked path


@pytest.mark.parametrize("name,chunks", [(nm, c) for nm in ("count", "hist5") for c in (0, 1, 5, 7, 16, 4096)] +
                         [("mp5", 7)])
def test_chunked_path(name, chunks):
    """select + accumulate + reduce_partials at 1025, 1536 and 1537 reports (17, 24 and 25 blocks of 64) with the
    report chunks set by debug option 2 (0: the engine's default). 24 blocks split as 24 (c = 1), 5+5+5+5+4 (5),
    six fours and an empty chunk (7), twos (16) and ones with thousands of empty chunks (4096); 17 and 25 blocks
    leave remainders of 1, 2 and 3 after the unrolled loop."""
    inst = A.instance(name)
    rng = np.random.default_rng(chunks)
    with engine(inst) as eng:
        if chunks:
            eng.debug(2, chunks)
        led = Ledger(inst)
        agg_id = 2000
        for pat in A.pattern_names(inst):
            pool = A.pool(name, pat)
            for n in (1025, 1536, 1537):
                for masked in (False, True):
                    agg_id += 1
                    for k, off in enumerate((7, 2900)):
                        c = pool.take(slice(off, off + n))
                        mask = random_mask(rng, n) if masked else None
                        bid = prepared(eng, c)
                        eng.accumulate(n, mask, np.full(n, agg_id, np.uint32), batch_id=bid)
                        led.add(agg_id, c, c.accepted if mask is None else c.accepted & (mask != 0))
                    led.check(eng, [agg_id], (pat, n, masked))


# ---------------------------------------------------------------------------- 3: the deferred path

DEFER_SIZES = (1, 63, 64, 65, 100, 1024)


def _deferred_round(eng, led, pool, nb, ids, rnd, sizes=DEFER_SIZES):
    for k in range(nb):
        n = sizes[k % len(sizes)]
        off = (k * 131 + rnd * 977) % (pool.n - 1024)
        c = pool.take(slice(off, off + n))
        bid = prepared(eng, c)
        agg_id = ids[k % len(ids)]
        eng.accumulate(n, None, np.full(n, agg_id, np.uint32), batch_id=bid)
        led.add(agg_id, c, c.accepted)


@pytest.mark.parametrize("spread", [1, 3])
@pytest.mark.parametrize("nb", [1, 4, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["count", "hist5", "mp5"])
def test_deferred_path(name, nb, spread):
    """accumulate_multi_kernel: nb deferred batches of 1 to 1,024 reports into one aggregation or spread over three,
    twice. nb = 4 and 5: a wave with one batch, a wave with two; 64: ACC_MULTI_MAX in one launch, flushed by the 64th
    deferral; 65 and 130: a second launch. Between the rounds the waiting batches are flushed by debug option 9 (even
    nb) or by the read; the second round meets the first's aggregate and is flushed by the read."""
    inst = A.instance(name)
    pats = A.pattern_names(inst) if nb <= 5 else ("all_max", "random")
    with engine(inst) as eng:
        led = Ledger(inst)
        for q, pat in enumerate(pats):
            pool = A.pool(name, pat)
            ids = [3000 + 10 * q + t for t in range(spread)]
            _deferred_round(eng, led, pool, nb, ids, 0)
            if nb % 2 == 0:
                eng.debug(9, 0)
            else:
                led.check(eng, ids, (pat, "first round"))
            _deferred_round(eng, led, pool, nb, ids, 1)
            led.check(eng, ids, (pat, "second round"))


@pytest.mark.parametrize("name", ["count", "hist5"])
def test_deferred_report_budget(name):
    """17 deferred batches of 1,024 reports: the 16th reaches the queue's report budget (16,384) and flushes, the
    17th waits for the read; a second round flushes at its 15th batch."""
    inst = A.instance(name)
    with engine(inst) as eng:
        led = Ledger(inst)
        for q, pat in enumerate(("all_max", "edge_cycle")):
            pool = A.pool(name, pat)
            for rnd in (0, 1):
                _deferred_round(eng, led, pool, 17, [3500 + q], rnd, sizes=(1024,))
                led.check(eng, [3500 + q], (pat, rnd))


# ---------------------------------------------------------------------------- 4: the segmented path


def seg_items_len(inst, n, chunks):
    """jx_engine_acc.cpp seg_items_len: reports per work item."""
    nch = chunks or min(4096, max(16, -(-16384 // inst.out_len)))
    return max(64, -(-(-(-n // nch)) // 64) * 64)


def seg_batch(pool, sizes, rng, shuffle, masked, first=0, stray=()):
    """A batch whose segment s (dense index first + s) holds exactly sizes[s] selected reports, plus rejected rows
    (mask set) and, with a mask, accepted rows with mask byte 0; one accepted row per index of `stray`; contiguous
    by segment, or shuffled. Returns (batch, dense index, mask or None)."""
    acc, rej = np.nonzero(pool.accepted)[0], np.nonzero(~pool.accepted)[0]
    a0 = int(rng.integers(0, len(acc) - sum(sizes) - 4 * len(sizes) - len(stray)))
    r0 = int(rng.integers(0, len(rej) - 3 * len(sizes)))
    rows, dense, mask = [], [], []
    for s, z in enumerate(sizes):
        take = [(acc[a0 + k], MASK_BYTES[1 + (k + s) % 3]) for k in range(z)]
        a0 += z
        take += [(rej[r0 + k], 1) for k in range(1 + s % 2)]
        r0 += 1 + s % 2
        if masked:
            take += [(acc[a0 + k], 0) for k in range(1 + s % 3)]
            a0 += 1 + s % 3
        take = [take[i] for i in rng.permutation(len(take))]
        rows += [t[0] for t in take]
        mask += [t[1] for t in take]
        dense += [first + s] * len(take)
    for k, d in enumerate(stray):
        rows.append(acc[a0 + k])
        mask.append(255)
        dense.append(d)
    order = rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
    rows, mask = (np.array(x)[order] for x in (rows, mask))
    dense = np.array(dense, np.uint32)[order]
    return pool.take(rows), dense, mask.astype(np.uint8) if masked else None


# variant -> (debug option 2 value or 0, the work-item length L it gives, selected reports per segment). The item
# length follows from the batch size (all rows, rejected ones too), so with three chunks a batch holds up to 3 L rows:
# L - 1 and L, L + 1, and 2 L + 1 come in three batches, each filled up to between 2.4 L and 3 L rows.
SEG_VARIANTS = {
    "default-L64": (0, 64, [1, 63, 64, 65, 129, 255, 256, 257, 449, 1, 320]),
    "one-item": (1, None, [1, 63, 64, 65, 255, 256, 257, 449, 1, 320, 0, 513]),
    "three-chunks-L320": (3, 320, [319, 320, 1, 63, 100]),
    "three-chunks-L320-over": (3, 320, [321, 320, 65, 100]),
    "three-chunks-L320-long": (3, 320, [641, 1, 100, 63]),
}


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("variant", list(SEG_VARIANTS))
@pytest.mark.parametrize("name", ["count", "hist5", "mp5"])
def test_segmented_path(name, variant, form):
    """seg_count / plan / scatter / accumulate / checksum / reduce with the selected reports per segment given
    exactly, three batches into the same aggregations: contiguous by segment, shuffled, and shuffled without a mask.
    With the default chunking the work items hold L = 64 sorted positions (segments of L - 1, L, L + 1 and 2 L + 1
    among the sizes); with debug 2 = 1 every segment is one long item, so segments of 255 to 513 run
    seg_accumulate_kernel's unrolled four-gather loop and its tail; with debug 2 = 3 the items hold L = 320
    positions. Device form: table entries that no report names stay zero with count 0, and indices at and past the
    table length are skipped."""
    import torch

    inst = A.instance(name)
    chunks, L, sizes = SEG_VARIANTS[variant]
    rng = np.random.default_rng(len(variant))
    dev = torch.device("cuda", 0)
    with engine(inst) as eng:
        if chunks:
            eng.debug(2, chunks)
        led = Ledger(inst)
        for pat in A.pattern_names(inst):
            pool = A.pool(name, pat)
            # arbitrary u32 ids; the device table begins and ends with an entry that no report names
            table = [int(x) for x in distinct_ids(rng, len(sizes) + 2)]
            first = 0 if form == "host" else 1
            stray = [] if form == "host" else [len(table), len(table) + 1, 2**31 - 1, 2**31, 2**32 - 1,
                                               len(table) + SEG_MAX]
            for rnd, (shuffle, masked) in enumerate(((False, True), (True, True), (True, False))):
                c, dense, mask = seg_batch(pool, sizes, rng, shuffle, masked, first, stray)
                n = c.n
                if L is None:
                    assert seg_items_len(inst, n, chunks) >= max(sizes)
                else:
                    assert seg_items_len(inst, n, chunks) == L, (n, L)
                sel = c.accepted if mask is None else c.accepted & (mask != 0)
                assert [int((sel & (dense == first + s)).sum()) for s in range(len(sizes))] == sizes
                bid = prepared(eng, c)
                if form == "host":
                    eng.accumulate(n, mask, np.array(table, np.uint32)[dense], batch_id=bid)
                else:
                    d_seg = torch.from_numpy(dense.view(np.int32).copy()).to(dev)
                    d_mask = torch.from_numpy(mask.copy()).to(dev) if masked else None
                    torch.cuda.synchronize()
                    eng.accumulate_device(bid, n, d_mask.data_ptr() if masked else None, d_seg.data_ptr(), table)
                    eng.sync()
                touched = led.add_by_index(c, sel, dense, table)
                assert touched == {t for t, z in zip(table[first:], sizes) if z}
                led.check(eng, table, (pat, variant, rnd))
            if form == "device":
                assert table[0] not in led.state and table[-1] not in led.state  # check() compared them with empty


# ---------------------------------------------------------------------------- 5, 6: several passes of accumulate_many


def _many_segments(inst, pools, table_len, n, pass_len, big, rng):
    """n reports per batch over a table of table_len ids, two batches: most reports land on random entries of a
    random two thirds of the table (the rest stay empty), reports of every pass interleaved; the entries `big` get
    a few hundred reports each. Every used aggregation and the empty ones next to each pass boundary are compared."""
    import torch

    dev = torch.device("cuda", 0)
    table = distinct_ids(rng, table_len)
    usable = np.nonzero(rng.random(table_len) < 0.66)[0]
    boundaries = [b for b in range(pass_len, table_len, pass_len)]
    near = sorted({k for b in boundaries + [0, table_len] for k in range(b - 3, b + 3) if 0 <= k < table_len})
    with engine(inst) as eng:
        led = Ledger(inst)
        used = set()
        for rnd, pool in enumerate(pools):
            c = pool.take(slice(rnd * (pool.n - n), rnd * (pool.n - n) + n))
            dense = usable[rng.integers(0, len(usable), size=n)].astype(np.uint32)
            mask = random_mask(rng, n)
            mask[rng.random(n) < 0.6] = 255  # most reports accepted
            order = rng.permutation(np.nonzero(c.accepted)[0])
            per = max(4, n // 25)
            for k, b in enumerate(big):  # accepted rows; all but the last are surely selected
                rows = order[k * per:(k + 1) * per]
                dense[rows] = b
                mask[rows[:-1]] = 2
            stray = order[len(big) * per:len(big) * per + 5]
            dense[stray] = [table_len, table_len + 1, 2**31, 2**32 - 1, table_len + pass_len]
            mask[stray] = 1
            sel = c.accepted & (mask != 0)
            bid = prepared(eng, c)
            d_seg = torch.from_numpy(dense.view(np.int32).copy()).to(dev)
            d_mask = torch.from_numpy(mask.copy()).to(dev)
            torch.cuda.synchronize()
            eng.accumulate_device(bid, n, d_mask.data_ptr(), d_seg.data_ptr(), table)
            eng.sync()
            used |= led.add_by_index(c, sel, dense, table)
        passes = {int(np.nonzero(table == t)[0][0]) // pass_len for t in used}
        assert passes == set(range(-(-table_len // pass_len))), "every pass has reports"
        for b in big:
            assert led.state[int(table[b])][1] >= 2 * (max(4, n // 25) - 1)
        led.check(eng, sorted(used), "used")
        empties = [int(table[k]) for k in near if int(table[k]) not in used]
        assert empties, "some aggregations next to a pass boundary stay empty"
        led.check(eng, empties, "empty")
        return len(used)


@pytest.mark.parametrize("table_len", [4097, 8197])
@pytest.mark.parametrize("name", ["count", "hist5"])
def test_more_than_seg_max(name, table_len):
    """More than SEG_MAX (4,096) table entries: accumulate_many runs a second (4,097: one entry long) and a third
    pass with s0 > 0, where seg[r] - s0 wraps for the earlier passes' reports, the counts are zeroed again and the
    pointer tables are offset. Larger segments sit on both sides of each pass boundary."""
    inst = A.instance(name)
    rng = np.random.default_rng(table_len)
    big = [0, SEG_MAX - 1, SEG_MAX, table_len - 1] + ([2 * SEG_MAX - 1, 2 * SEG_MAX] if table_len > 2 * SEG_MAX else [])
    pools = [A.pool(name, "all_max"), A.pool(name, "edge_cycle")]
    nused = _many_segments(inst, pools, table_len, 5000, SEG_MAX, big, rng)
    assert nused > 1500


def test_lowered_ns_max():
    """Histogram(6000, 78): the per-item partials (out_len x 24 bytes) bound a pass to 3,726 segments, below SEG_MAX,
    so a table of 4,000 ids takes passes of 3,726 and 274."""
    inst = A.instance("hist6000")
    n, table_len = 96, 4000
    L = seg_items_len(inst, n, 0)
    ns_max = (512 << 20) // (inst.out_len * 24) - -(-n // L)
    assert (L, ns_max) == (64, 3726)
    rng = np.random.default_rng(6000)
    pools = []
    for pat in ("all_max", "edge_cycle"):
        init, fin = A.spread_rejects(inst, 2 * n)
        pools.append(A.craft(inst, A.pattern(inst, pat, 2 * n), 6, init, fin))
    _many_segments(inst, pools, table_len, n, ns_max, [ns_max - 1, ns_max, table_len - 1], rng)


# ---------------------------------------------------------------------------- 7: the combine kernels

COMBINE_PARTS = ("p-1 and 1", "p-1", "edge_cycle", "random")


def _parts(inst, kind, nparts, rng):
    p, m = inst.p, inst.out_len
    if kind == "p-1 and 1":  # two parts sum to exactly p
        return [[p - 1 if q % 2 == 0 else 1] * m for q in range(nparts)]
    if kind == "p-1":
        return [[p - 1] * m for _ in range(nparts)]
    return A.pattern(inst, kind, nparts, seed=nparts) if kind == "random" else \
        [row[::-1] for row in A.pattern(inst, kind, nparts)]


@pytest.mark.parametrize("name", ["count", "hist5", "hist257"])
def test_combine_kernels(name):
    """combine_device and combine_records_device over 1, 2, 3 and 8 parts of p - 1 and 1 (sums of exactly p),
    of p - 1 alone (p - 1 eight times), of the edge values and of random elements, with counts around 2^32. For
    Histogram(257) out_len + 1 = 258 threads cross the 256-thread workgroup: the second workgroup writes the last
    element and the count / checksum tail."""
    import torch

    inst = A.instance(name)
    p, fb, m = inst.p, inst.fb, inst.out_len
    rng = np.random.default_rng(m)
    counts = [2**32 - 1, 1, 2**32, 2**31, 0, 2**32 + 1, 2**33 - 1, 7]
    with engine(inst) as eng:
        rb = eng.record_bytes()
        assert rb == m * fb + 40
        for kind in COMBINE_PARTS:
            for nparts in (1, 2, 3, 8):
                rows = _parts(inst, kind, nparts, rng)
                ids = rng.integers(0, 256, size=(nparts, 16), dtype=np.uint8)
                want = A.model(p, fb, rows, ids, np.ones(nparts, bool))
                shares = np.stack([np.frombuffer(inst.encode(r), np.uint8) for r in rows])
                d_parts = torch.from_numpy(shares.copy()).cuda()
                d_out = torch.full((m * fb,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                eng.combine_device(d_parts.data_ptr(), nparts, d_out.data_ptr())
                eng.sync()
                assert d_out.cpu().numpy().tobytes() == want[0], (kind, nparts)
                assert want[0] == D.merge_aggregate_shares([s.tobytes() for s in shares], fb)
                # records: the same shares with counts around 2^32 and arbitrary checksums
                cs = rng.integers(0, 256, size=(nparts, 32), dtype=np.uint8)
                recs = np.stack([D.pack_record(shares[q].tobytes(), counts[q], cs[q].tobytes()) for q in range(nparts)])
                d_recs = torch.from_numpy(recs.copy()).cuda()
                d_rout = torch.full((rb,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                eng.combine_records_device(d_recs.data_ptr(), nparts, d_rout.data_ptr())
                eng.sync()
                got = D.unpack_record(d_rout.cpu().numpy(), fb)
                xor = np.bitwise_xor.reduce(cs, axis=0).tobytes()
                assert got == (want[0], sum(counts[:nparts]), xor), (kind, nparts)
                assert got == D.merge_records(recs, fb)


@pytest.mark.parametrize("name", ["count", "hist5", "hist257"])
def test_combine_refuses_non_canonical_last_element(name):
    """An element of p at the last element of the last part (the existing test damages the first element of the
    second part) is refused by both device merges on the next sync, like the host merge; p - 1 there is not."""
    import torch

    inst = A.instance(name)
    p, fb, m = inst.p, inst.fb, inst.out_len
    with engine(inst) as eng:
        rb = eng.record_bytes()
        for nparts in (1, 3):
            for bad in (False, True):
                rows = [[p - 1] * m for _ in range(nparts)]
                shares = np.stack([np.frombuffer(inst.encode(r), np.uint8) for r in rows]).copy()
                if bad:
                    shares[-1, -fb:] = np.frombuffer(p.to_bytes(fb, "little"), np.uint8)
                recs = np.stack([D.pack_record(s.tobytes(), 1, bytes(32)) for s in shares])
                d_parts, d_recs = torch.from_numpy(shares).cuda(), torch.from_numpy(recs.copy()).cuda()
                d_out = torch.zeros(rb, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                for call, arg in ((eng.combine_device, d_parts), (eng.combine_records_device, d_recs)):
                    call(arg.data_ptr(), nparts, d_out.data_ptr())
                    if bad:
                        with pytest.raises(EngineError, match="non-canonical"):
                            eng.sync()
                    eng.sync()  # the flag is cleared once reported
                if bad:
                    with pytest.raises(ValueError, match="not canonical"):
                        D.merge_records(recs, fb)
                else:
                    assert D.merge_records(recs, fb)[0] == ((nparts * (p - 1)) % p).to_bytes(fb, "little") * m
