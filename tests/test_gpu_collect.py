"""GPU: collection at all three roles. jx_collect_seal[_device] (merge the shard records of many collection jobs,
check them, seal the shares to the collector) and jx_collect_open[_device] (open both shares, unshard) on synthetic
records of random canonical elements, against Python integers and oracle/hpke_oracle.py byte for byte; then the loop
closed: shard -> prepare -> accumulate through BatchAggregationWriter -> leader_collect -> handle_aggregate_share ->
Collection -> Collector.unshard. Nothing has a tolerance."""
from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

from janus_amd import hpke
from janus_amd.engine import (COLLECT_BAD_RECORD, COLLECT_BATCH_MISMATCH, COLLECT_INVALID_BATCH_SIZE, COLLECT_OK,
                              COLLECT_SEAL_FAILED, HelperEngine)
from janus_amd.messages import AggregateShareAad, BatchSelector, Interval
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H

pytestmark = pytest.mark.gpu

P64, P128 = 2**64 - 2**32 + 1, 2**128 - 28 * 2**64 + 1
TASK = bytes(range(50, 82))
INFO_L = hpke.application_info(hpke.LABEL_AGGREGATE_SHARE, hpke.ROLE_LEADER, hpke.ROLE_COLLECTOR)
INFO_H = hpke.application_info(hpke.LABEL_AGGREGATE_SHARE, hpke.ROLE_HELPER, hpke.ROLE_COLLECTOR)
SK = random.Random(77).randbytes(32)
PK = H.x25519_base(SK)
E_INVALID = -1

INSTANCES = {
    "count": Prio3.count(),                                   # Field64, OUT = 1
    "sumvec_1_5_3": Prio3.sum_vec(1, 5, 3),                   # Field128, OUT = 5: less than a wave
    "sumvec_1_257_16": Prio3.sum_vec(1, 257, 16),             # OUT = 257: one past a 256-lane tile
    "multiproof_2_1_7_3": Prio3.sum_vec_field64_multiproof_hmacsha256_aes128(2, 1, 7, 3),  # Field64, OUT = 7
    "histogram_3_2": Prio3.histogram(3, 2),
}


@pytest.fixture(params=list(INSTANCES), scope="module")
def v(request):
    return INSTANCES[request.param]


def modulus(v):
    return P64 if v.field_bytes == 8 else P128


def engine(v):
    return HelperEngine(v, bytes(v.verify_key_len))


class Records:
    """nrec synthetic batch-aggregation rows: random canonical elements, a count, a checksum; and their bytes."""

    def __init__(self, v, seed, nrec, counts=None):
        rng = random.Random(seed)
        self.v, self.p, self.fb = v, modulus(v), v.field_bytes
        self.elems = [[rng.randrange(self.p) for _ in range(v.output_len)] for _ in range(nrec)]
        self.counts = list(counts) if counts is not None else [rng.randrange(1, 50) for _ in range(nrec)]
        self.checksums = [rng.randbytes(32) for _ in range(nrec)]

    def row(self, r) -> bytes:
        return (b"".join(e.to_bytes(self.fb, "little") for e in self.elems[r]) + self.counts[r].to_bytes(8, "little") +
                self.checksums[r])

    def bytes(self) -> bytes:
        return b"".join(self.row(r) for r in range(len(self.elems)))

    def merge(self, job):
        """(share bytes, count, checksum) of a job, with Python integers."""
        total = [sum(self.elems[r][i] for r in job) % self.p for i in range(self.v.output_len)]
        cs = bytes(32)
        for r in job:
            cs = bytes(a ^ b for a, b in zip(cs, self.checksums[r]))
        return b"".join(t.to_bytes(self.fb, "little") for t in total), sum(self.counts[r] for r in job), cs


def aad_of(j: int) -> bytes:
    sel = BatchSelector.time_interval(Interval(3600 * j, 3600 * (1 + j % 3)))
    return AggregateShareAad(TASK, b"" if j % 2 else b"\x07" * j, sel).encode()


def dev_u8(*shape):
    import torch
    return torch.full(shape, 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))


def to_dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to(torch.device("cuda", 0))


class DevOut:
    """The outputs of jx_collect_seal_device, pre-filled with 0xA5."""

    def __init__(self, njobs, pt):
        self.status, self.counts, self.checksums = dev_u8(njobs), dev_u8(njobs, 8), dev_u8(njobs, 32)
        self.encs, self.cts, self.shares = dev_u8(njobs, 32), dev_u8(njobs, pt + 16), dev_u8(njobs, pt)

    def ptrs(self):
        return [t.data_ptr() for t in (self.status, self.counts, self.checksums, self.encs, self.cts, self.shares)]

    def host(self):
        return [t.cpu().numpy() for t in (self.status, self.counts, self.checksums, self.encs, self.cts, self.shares)]

    def untouched(self):
        return all((a == 0xA5).all() for a in self.host())


# ----------------------------------------------------------------------------- 1. merge and seal


def test_merge_and_seal(v):
    """One call with jobs of 33, 3, 1 and 2 records (two share record 12; the job order is not the record order):
    count, checksum and status are Python's, enc and ciphertext are seal_base's byte for byte and open_base gives the
    Python sum back; the device form, queued behind a sleeping producer on torch's stream, gives the same bytes."""
    import torch

    recs = Records(v, 1000 + v.output_len, 40)
    jobs = [list(range(39, 6, -1)), [12, 0, 5], [7], [3, 12]]
    assert [len(j) for j in jobs] == [33, 3, 1, 2]
    aads = [aad_of(j) for j in range(len(jobs))]
    skes = [random.Random(5 + j).randbytes(32) for j in range(len(jobs))]
    want = [recs.merge(j) for j in jobs]
    expect = [(c, cs) for _, c, cs in want]
    pt = v.output_len * v.field_bytes
    with engine(v) as eng, hpke.HpkeSealer(PK, INFO_H) as sender:
        assert eng.record_bytes() == pt + 40
        got = eng.collect_seal(recs.bytes(), jobs, aads, b"".join(skes), sender, 1, 0, expect=expect, want_shares=True)
        # the device form: the records and the keys arrive on torch's stream behind a sleeping kernel
        h_rec = torch.from_numpy(np.frombuffer(recs.bytes(), np.uint8).copy()).pin_memory()
        h_sk = torch.from_numpy(np.frombuffer(b"".join(skes), np.uint8).copy()).pin_memory()
        d_rec, d_sk = dev_u8(h_rec.numel()), dev_u8(h_sk.numel())
        out = DevOut(len(jobs), pt)
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)
        d_rec.copy_(h_rec, non_blocking=True)
        d_sk.copy_(h_sk, non_blocking=True)
        eng.collect_seal_device(d_rec.data_ptr(), 40, jobs, aads, d_sk.data_ptr(), sender, 1, 0, *out.ptrs(), expect=expect)
        st, cnt, cs, encs, cts, shares = out.host()
    assert list(got.status) == [COLLECT_OK] * len(jobs)
    for j, (share, count, checksum) in enumerate(want):
        assert int(got.counts[j]) == count and got.checksums[j].tobytes() == checksum
        assert got.shares[j].tobytes() == share
        enc, ct = H.seal_base(PK, INFO_H, aads[j], share, skes[j])
        assert got.encs[j].tobytes() == enc and got.cts[j].tobytes() == ct
        assert H.open_base(SK, PK, INFO_H, got.encs[j].tobytes(), aads[j], got.cts[j].tobytes()) == share
    np.testing.assert_array_equal(st, got.status)
    np.testing.assert_array_equal(cnt.view(np.uint64).reshape(-1), got.counts)
    for a, b in ((cs, got.checksums), (encs, got.encs), (cts, got.cts), (shares, got.shares)):
        np.testing.assert_array_equal(a, b)


# ----------------------------------------------------------------------------- 2. every status in one call


def test_every_status_in_one_call(v):
    """min 10, max 20: an empty job, counts of 9, 10, 20 and 21, a count and a checksum that differ from the
    expectation, an element equal to p at the first element of a job's first record and at the last element of a job's
    last record (one of them with a count below the minimum as well: the record comes first). The jobs that pass are
    sealed as if alone; every refused job's enc, ciphertext and share are zeros in buffers that held 0xA5. Then the
    same call under an all-zero collector key: what passed is SEAL_FAILED, what was refused keeps its status."""
    lo, hi = 10, 20
    #           0   1   2   3   4   5   6   7  8  9  10  11 12
    counts = [9, 10, 20, 21, 15, 15, 15, 3, 4, 5, 12, 2, 0]
    recs = Records(v, 2000 + v.output_len, len(counts), counts)
    p, last = recs.p, v.output_len - 1
    recs.elems[6][0] = p          # job 7: the first element of its first record
    recs.elems[9][last] = p       # job 8: the last element of its last record
    recs.elems[11][last] = p      # job 10: a bad record and a count below the minimum
    jobs = [[], [0], [1], [2], [3], [4], [5], [6, 10], [7, 8, 9], [10], [11], [12, 10]]
    merged = [recs.merge(j) for j in jobs]
    expect = [(c, cs) for _, c, cs in merged]
    expect[5] = (16, expect[5][1])
    cs6 = expect[6][1]
    expect[6] = (15, cs6[:31] + bytes([cs6[31] ^ 0x10]))
    want = [COLLECT_INVALID_BATCH_SIZE, COLLECT_INVALID_BATCH_SIZE, COLLECT_OK, COLLECT_OK, COLLECT_INVALID_BATCH_SIZE,
            COLLECT_BATCH_MISMATCH, COLLECT_BATCH_MISMATCH, COLLECT_BAD_RECORD, COLLECT_BAD_RECORD, COLLECT_OK,
            COLLECT_BAD_RECORD, COLLECT_OK]
    n = len(jobs)
    aads = [aad_of(j) for j in range(n)]
    skes = [random.Random(40 + j).randbytes(32) for j in range(n)]
    pt = v.output_len * v.field_bytes
    d_rec, d_sk = to_dev(recs.bytes()), to_dev(b"".join(skes))
    with engine(v) as eng, hpke.HpkeSealer(PK, INFO_H) as sender, hpke.HpkeSealer(bytes(32), INFO_H) as zero_key:
        out, out0 = DevOut(n, pt), DevOut(n, pt)
        eng.collect_seal_device(d_rec.data_ptr(), len(counts), jobs, aads, d_sk.data_ptr(), sender, lo, hi, *out.ptrs(),
                                expect=expect)
        eng.collect_seal_device(d_rec.data_ptr(), len(counts), jobs, aads, d_sk.data_ptr(), zero_key, lo, hi, *out0.ptrs(),
                                expect=expect)
        st, cnt, cs, encs, cts, shares = out.host()
        st0, cnt0, cs0, encs0, cts0, shares0 = out0.host()
        host = eng.collect_seal(recs.bytes(), jobs, aads, b"".join(skes), sender, lo, hi, expect=expect, want_shares=True)
        leader = eng.collect_seal(recs.bytes(), jobs, aads, b"".join(skes), sender, lo, hi, want_shares=True)
    assert list(st) == want
    for j in range(n):
        share, count, checksum = merged[j]
        assert int(cnt[j].view(np.uint64)[0]) == count and cs[j].tobytes() == checksum
        if want[j] == COLLECT_OK:
            enc, ct = H.seal_base(PK, INFO_H, aads[j], share, skes[j])
            assert encs[j].tobytes() == enc and cts[j].tobytes() == ct and shares[j].tobytes() == share
        else:
            assert not encs[j].any() and not cts[j].any() and not shares[j].any()
    # an all-zero collector key: X25519 gives zero, no seal comes about
    assert list(st0) == [COLLECT_SEAL_FAILED if w == COLLECT_OK else w for w in want]
    assert not encs0.any() and not cts0.any() and not shares0.any()
    np.testing.assert_array_equal(cnt0, cnt)
    np.testing.assert_array_equal(cs0, cs)
    # the host form gives the same; without expectations (the leader) the two mismatches pass
    np.testing.assert_array_equal(host.status, st)
    for a, b in ((host.encs, encs), (host.cts, cts), (host.shares, shares), (host.checksums, cs)):
        np.testing.assert_array_equal(a, b)
    assert list(leader.status) == [COLLECT_OK if w == COLLECT_BATCH_MISMATCH else w for w in want]
    for j in (5, 6):
        enc, ct = H.seal_base(PK, INFO_H, aads[j], merged[j][0], skes[j])
        assert leader.encs[j].tobytes() == enc and leader.cts[j].tobytes() == ct


# ----------------------------------------------------------------------------- 3. whole-call refusals


def test_whole_call_refusals_write_nothing():
    """Decreasing offsets, an index past the records, a record named twice by one job, a recipient context where a
    sender context belongs: JX_E_INVALID before anything is queued, and the outputs still hold 0xA5. njobs = 0 is
    JX_OK and writes nothing either."""
    v = INSTANCES["sumvec_1_5_3"]
    recs = Records(v, 3000, 6)
    pt = v.output_len * v.field_bytes
    d_rec, d_sk = to_dev(recs.bytes()), to_dev(bytes(range(96)))
    aad = np.frombuffer(b"".join(aad_of(j) for j in range(3)), np.uint8).copy()
    aoff = np.zeros(4, np.uint64)
    aoff[1:] = np.cumsum([len(aad_of(j)) for j in range(3)])
    u64p, u32p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p

    def call(eng, ctx, njobs, off, idx, out, aoffs=aoff):
        off, idx = np.asarray(off, np.uint64), np.asarray(idx, np.uint32)
        return eng._L.jx_collect_seal_device(eng.handle, njobs, d_rec.data_ptr(), 6, off.ctypes.data_as(u64p),
                                             idx.ctypes.data_as(u32p), None, None, 1, 0, aad.ctypes.data_as(vp),
                                             aoffs.ctypes.data_as(u64p), d_sk.data_ptr(), ctx.handle, *out.ptrs())

    with engine(v) as eng, hpke.HpkeSealer(PK, INFO_H) as sender, hpke.HpkeOpener(SK, PK, INFO_H) as opener:
        out = DevOut(3, pt)
        assert call(eng, sender, 3, [0, 3, 2, 4], [0, 1, 2, 3], out) == E_INVALID       # decreasing record offsets
        assert call(eng, sender, 3, [0, 1, 2, 3], [0, 1, 2], out, aoff[[0, 2, 1, 3]].copy()) == E_INVALID  # aad offsets
        assert call(eng, sender, 3, [0, 1, 3, 4], [0, 1, 6, 3], out) == E_INVALID       # index == nrecords
        assert call(eng, sender, 3, [0, 1, 4, 5], [0, 1, 2, 1, 3], out) == E_INVALID    # record 1 twice in job 1
        assert call(eng, opener, 3, [0, 1, 2, 3], [0, 1, 2], out) == E_INVALID          # not a sender context
        assert call(eng, sender, 0, [0], [0], out) == 0
        eng.sync()
        assert out.untouched()
        # the same record in two jobs is no refusal, and the call goes through once it is well formed
        assert call(eng, sender, 3, [0, 1, 3, 4], [0, 1, 2, 1], out) == 0
        eng.sync()
        assert list(out.host()[0]) == [0, 0, 0]


# ----------------------------------------------------------------------------- 4. open and unshard


def py_unshard(v, shares, count):
    if v.algo_id == INSTANCES["multiproof_2_1_7_3"].algo_id:  # Prio3.unshard does not cover it: Python integers
        p = modulus(v)
        vals = [[int.from_bytes(s[8 * i:8 * i + 8], "little") for i in range(v.output_len)] for s in shares]
        return [sum(col) % p for col in zip(*vals)]
    return v.unshard(shares, count)


def row_result(v, row: bytes):
    fb = v.field_bytes
    vals = [int.from_bytes(row[fb * i:fb * i + fb], "little") for i in range(v.output_len)]
    return vals[0] if v.output_len == 1 and v.algo_id in (0, 1) else vals


def open_cases(v, seed, suite=(1, 1)):
    """12 collections whose shares the test seals with HpkeSealer; (leader shares, helper shares, aads, the aads to
    open with, want status, plaintext pairs)."""
    rng = random.Random(seed)
    p, fb, out_len = modulus(v), v.field_bytes, v.output_len
    n = 12
    share = lambda: [rng.randrange(p) for _ in range(out_len)]  # noqa: E731
    enc_share = lambda s: b"".join(e.to_bytes(fb, "little") for e in s)  # noqa: E731
    pl, ph = [share() for _ in range(n)], [share() for _ in range(n)]
    pl[7][out_len - 1] = p   # the leader's share: an element equal to p at its last position
    ph[8][out_len - 1] = p   # the helper's
    ptl, pth = [enc_share(s) for s in pl], [enc_share(s) for s in ph]
    ptl[9] = ptl[9][:-fb]    # one element short
    pth[10] = pth[10][:-fb]
    aads = [aad_of(j) for j in range(n)]
    kdf, aead = suite
    with hpke.HpkeSealer(PK, INFO_L, kdf_id=kdf, aead_id=aead) as sl, hpke.HpkeSealer(PK, INFO_H, kdf_id=kdf, aead_id=aead) as sh:
        ls = sl.seal_long_batch([rng.randbytes(32) for _ in range(n)], ptl, aads)
        hs = sh.seal_long_batch([rng.randbytes(32) for _ in range(n)], pth, aads)
    flip = lambda s, bit: (s[0], s[1][:bit // 8] + bytes([s[1][bit // 8] ^ (1 << (bit % 8))]) + s[1][bit // 8 + 1:])  # noqa: E731
    ls[3] = flip(ls[3], 8 * (len(ls[3][1]) - 1) + 7)  # the last bit of the tag
    hs[4] = flip(hs[4], 0)                           # the first bit of the ciphertext
    open_aads = list(aads)
    open_aads[5] = aads[5][:-1] + bytes([aads[5][-1] ^ 1])
    ls[6], hs[6] = hs[6], ls[6]                      # swapped between the roles: the info differs, neither opens
    want = [0, 0, 0, 1, 2, 1, 1, 3, 4, 3, 4, 0]
    return ls, hs, open_aads, want, list(zip(ptl, pth))


def check_open(v, got_rows, got_status, want, pts):
    assert list(got_status) == want
    for i, st in enumerate(want):
        if st == 0:
            assert row_result(v, got_rows[i].tobytes()) == py_unshard(v, list(pts[i]), 1)
        else:
            assert not got_rows[i].any()


def test_open_and_unshard(v):
    """The collector: 12 collections in one call, sealed by the test. The rows of those that open equal Prio3.unshard
    of the plaintexts; a flipped bit in either share, the wrong aad, shares swapped between the roles, an element equal
    to p at a share's last position and a share one element short each get their status and a zero row. The device
    form gives the same in buffers that held 0xA5."""
    ls, hs, aads, want, pts = open_cases(v, 4000 + v.output_len)
    n, pt = len(want), v.output_len * v.field_bytes
    with engine(v) as eng, hpke.HpkeOpener(SK, PK, INFO_L) as ol, hpke.HpkeOpener(SK, PK, INFO_H) as oh:
        got = eng.collect_open(ol, oh, ls, hs, aads)
        d_le, d_lc = to_dev(b"".join(e for e, _ in ls)), to_dev(b"".join(c for _, c in ls))
        d_he, d_hc = to_dev(b"".join(e for e, _ in hs)), to_dev(b"".join(c for _, c in hs))
        d_out, d_st = dev_u8(n, pt), dev_u8(n)
        lo = np.concatenate([[0], np.cumsum([len(c) for _, c in ls])]).astype(np.uint64)
        ho = np.concatenate([[0], np.cumsum([len(c) for _, c in hs])]).astype(np.uint64)
        eng.collect_open_device(ol, oh, n, d_le.data_ptr(), d_lc.data_ptr(), lo, d_he.data_ptr(), d_hc.data_ptr(), ho, aads,
                                d_out.data_ptr(), d_st.data_ptr())
        rows, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        with hpke.HpkeSealer(PK, INFO_L) as wrong_kind:
            with pytest.raises(Exception):
                eng.collect_open(wrong_kind, oh, ls, hs, aads)
    check_open(v, got.aggregates, got.status, want, pts)
    check_open(v, rows, st, want, pts)


# ----------------------------------------------------------------------------- 5. another suite


def test_non_default_suite():
    """Tests 1 and 4 at OUT = 5 under X25519 / HKDF-SHA512 / ChaCha20Poly1305. The Python oracle covers the default
    suite only: here the sealed shares go through the existing opener and must give the Python sums back."""
    v = INSTANCES["sumvec_1_5_3"]
    kdf, aead = hpke.KDF_HKDF_SHA512, hpke.AEAD_CHACHA20_POLY1305
    recs = Records(v, 5000, 40)
    jobs = [list(range(39, 6, -1)), [12, 0, 5], [7], [3, 12]]
    aads = [aad_of(j) for j in range(len(jobs))]
    skes = [random.Random(60 + j).randbytes(32) for j in range(len(jobs))]
    want = [recs.merge(j) for j in jobs]
    ls, hs, open_aads, want_open, pts = open_cases(v, 5001, (kdf, aead))
    with engine(v) as eng, hpke.HpkeSealer(PK, INFO_L, kdf_id=kdf, aead_id=aead) as sender, \
            hpke.HpkeOpener(SK, PK, INFO_L, kdf_id=kdf, aead_id=aead) as ol, \
            hpke.HpkeOpener(SK, PK, INFO_H, kdf_id=kdf, aead_id=aead) as oh:
        assert sender.suite == (hpke.KEM_X25519_HKDF_SHA256, kdf, aead)
        got = eng.collect_seal(recs.bytes(), jobs, aads, b"".join(skes), sender, 1, 0, want_shares=True)
        opened = ol.open_long_batch([e.tobytes() for e in got.encs], [c.tobytes() for c in got.cts], aads)
        res = eng.collect_open(ol, oh, ls, hs, open_aads)
    assert list(got.status) == [COLLECT_OK] * len(jobs)
    for j, (share, count, checksum) in enumerate(want):
        assert opened[j] == share == got.shares[j].tobytes()
        assert int(got.counts[j]) == count and got.checksums[j].tobytes() == checksum
    check_open(v, res.aggregates, res.status, want_open, pts)


# ----------------------------------------------------------------------------- 6. the loop closed


def test_the_loop_closed():
    """sum_vec(2, 5, 3), 130 reports in two time buckets, two engines whose writers have three shard ords: shard ->
    leader init -> helper init -> leader finish, each job written through its BatchAggregationWriter; then
    leader_collect -> handle_aggregate_share -> the Collection body -> Collector.unshard gives the column sums."""
    from janus_amd.aggregator import (BatchMismatch, CollectTask, LeaderReport, handle_aggregate_init,
                                      handle_aggregate_share, leader_aggregate_init, leader_collect,
                                      leader_finish_collection, leader_process_helper_response)
    from janus_amd.batch_aggregation import AGGREGATING, COLLECTED, SCRUBBED, BatchAggregationWriter
    from janus_amd.collector import Collector
    from janus_amd.messages import (AggregateShare, AggregateShareReq, Collection, HpkeCiphertext, PartialBatchSelector,
                                    ReportMetadata)

    v = Prio3.sum_vec(2, 5, 3)
    n, precision = 130, 3600
    t0 = 1_700_000_000 // precision * precision
    times = [t0 + 100 + 50 * i for i in range(n)]
    assert {t // precision for t in times} == {t0 // precision, t0 // precision + 1}
    segs = [t // precision for t in times]
    rng = np.random.default_rng(6)
    meas = rng.integers(0, 4, size=(n, 5), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    task = CollectTask(TASK, precision, min_batch_size=100, max_batch_size=0, report_expiry_age=86400, collector_config_id=9)
    iv = Interval(t0, 2 * precision)
    sel = BatchSelector.time_interval(iv)
    vk = bytes(range(16))
    ske_l, ske_h = bytes(range(1, 33)), bytes(range(2, 34))
    with HelperEngine(v, vk) as leader, HelperEngine(v, vk) as helper, hpke.HpkeSealer(PK, INFO_L) as seal_l, \
            hpke.HpkeSealer(PK, INFO_H) as seal_h, Collector(v, TASK, (SK, PK)) as collector:
        lw = BatchAggregationWriter(field_bytes=v.field_bytes, shard_count=3, seed=1)
        hw = BatchAggregationWriter(field_bytes=v.field_bytes, shard_count=3, seed=2)
        sh = leader.shard_batch(meas, nonces, rng.integers(0, 256, size=(n, v.client_rand_len), dtype=np.uint8))
        assert not sh.status.any()
        for lo, hi in ((0, 50), (50, 100), (100, 130)):  # three aggregation jobs: rows at several shard ords
            reports = [LeaderReport(ReportMetadata(nonces[i].tobytes(), times[i]), sh.public_shares[i].tobytes(),
                                    sh.leader_input_shares[i].tobytes(), HpkeCiphertext(0, b"", b"")) for i in range(lo, hi)]
            step = leader_aggregate_init(leader, reports, segs[lo:hi], writer=lw)
            his = [sh.helper_input_shares[lo + i].tobytes() for i in step.stepped]
            out_h = handle_aggregate_init(helper, step.prepare_inits, his, [segs[lo + i] for i in step.stepped], writer=hw)
            out_l = leader_process_helper_response(leader, step, out_h.responses, segs[lo:hi], writer=lw)
            assert out_h.finished.all() and out_l.finished.all()
        assert all(r.state == AGGREGATING for r in hw.datastore.rows.values())

        lc = leader_collect(leader, lw, task, iv, b"", seal_l, ske_l)
        req = AggregateShareReq.decode(lc.request_body, 1)
        assert req.report_count == n and req.batch_selector == sel
        cache: dict = {}
        now = t0 + 3 * precision
        # a request whose count is off by one: BatchMismatch with both sides, and nothing is consumed
        off_by_one = AggregateShareReq(sel, b"", n + 1, req.checksum).encode()
        with pytest.raises(BatchMismatch) as mm:
            handle_aggregate_share(helper, hw, task, off_by_one, seal_h, ske_h, now, cache)
        assert (mm.value.own_report_count, mm.value.peer_report_count) == (n, n + 1)
        assert mm.value.own_checksum == mm.value.peer_checksum == req.checksum
        assert not cache and all(r.state == AGGREGATING for r in hw.datastore.rows.values())
        # the request itself, its transaction retried once: the same bytes as one attempt writes
        body = handle_aggregate_share(helper, hw, task, lc.request_body, seal_h, ske_h, now, cache, inject_tx_failures=1)
        assert hw.datastore.attempts >= 2
        coll_body = leader_finish_collection(lc, body)
        res = collector.unshard(coll_body, sel, b"")
        coll = Collection.decode(coll_body, 1)
        # served again from the cache: the same plaintext, and under the same ephemeral key the same bytes
        (job,) = cache.values()
        again = handle_aggregate_share(helper, hw, task, lc.request_body, seal_h, ske_h, now, cache)
        (job2,) = cache.values()
        with pytest.raises(BatchMismatch):
            handle_aggregate_share(helper, hw, task, off_by_one, seal_h, ske_h, now, cache)
        late = hw.write_job(helper, 0, 0, None, None, [], [(segs[0], times[0])], initial_write=True, terminal=True)
        helper_rows, leader_rows = dict(hw.datastore.rows), dict(lw.datastore.rows)
    sums = [int(meas[:, j].astype(object).sum()) for j in range(5)]
    assert res.aggregate_result == sums and res.report_count == n
    assert coll.report_count == n and coll.partial_batch_selector == PartialBatchSelector.time_interval()
    want_iv = Interval(min(times) // precision * precision, 0)
    want_iv = Interval(want_iv.start, -(-(max(times) + 1 - want_iv.start) // precision) * precision)
    assert coll.interval == want_iv == Interval(t0, 2 * precision) == res.interval
    assert coll.leader_encrypted_agg_share.config_id == coll.helper_encrypted_agg_share.config_id == 9
    assert again == body and job2 == job and job.report_count == n
    ct = AggregateShare.decode(body).encrypted_aggregate_share
    aad = AggregateShareAad(TASK, b"", sel).encode()
    assert H.open_base(SK, PK, INFO_H, ct.encapsulated_key, aad, ct.payload) == job.aggregate_share
    lct = coll.leader_encrypted_agg_share
    assert H.open_base(SK, PK, INFO_L, lct.encapsulated_key, aad, lct.payload) == lc.aggregate_share
    assert v.unshard([lc.aggregate_share, job.aggregate_share], n) == sums
    # every (bucket, ord) row exists now: scrubbed at the helper (no share left), collected at the leader
    keys = {(s, o) for s in set(segs) for o in range(3)}
    assert set(helper_rows) == set(leader_rows) == keys
    assert all(r.state == SCRUBBED and r.aggregate_share is None for r in helper_rows.values())
    assert all(r.state == COLLECTED for r in leader_rows.values())
    assert late == {segs[0]}  # a later job into the batch: its reports fail with BatchCollected
