"""The lane-indexed GHASH behind the wave-per-report HPKE open (janus_amd/csrc/jx_ghash_lanes.h), compiled for the
host (tests/csrc/hosttest_hpke_long.cpp) with the 64 lanes as a loop, against oracle/hpke_oracle.py; the T-table
AES of both key lengths against tests/hpke_suites_ref.py. Also the host side of the leader's upload path: the
Report codec against the reference's vectors (tests/golden/hpke_report_kat.json: the hpke prefix keeps it out of
test_gpu_parity's glob of Prio3 fixtures) and aggregator.handle_upload's checks that need no device, with a stub
engine."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import pytest

import hpke_suites_ref as S
from oracle import hpke_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hl():
    src = os.path.join(HERE, "csrc", "hosttest_hpke_long.cpp")
    so = os.path.join(HERE, "csrc", "libjx_hosttest_hpke_long.so")
    hdrs = [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_field.h", "jx_sha256.h", "jx_sha_aes.h", "jx_hpke.h",
                                                                         "jx_ghash_lanes.h")]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs + [src]):
        tmp = f"{so}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.hl_ghash_mul.argtypes = [vp, vp, vp]
    L.hl_ghash_mul_tab4.argtypes = [vp, vp, vp]
    L.hl_ghash_lanes.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp]
    L.hl_aes_t.argtypes = [vp, u32, vp, vp]
    return L


def _b(x: int) -> bytes:
    return x.to_bytes(16, "big")


def test_table_product_equals_the_bit_loop(hl):
    """ghash_mul_tab4 (the fixed-multiplier product of the Horner step) against ghash_mul and the oracle's
    _ghash_mul: random operands, every single-bit operand on either side (each nibble position and each of the 16
    reductions of the shift by x^4), zero and all ones."""
    rnd = random.Random(4)
    out, ref = ctypes.create_string_buffer(16), ctypes.create_string_buffer(16)
    single = [1 << i for i in range(128)]
    cases = [(rnd.getrandbits(128), rnd.getrandbits(128)) for _ in range(300)]
    h0 = rnd.getrandbits(128)
    cases += [(x, h0) for x in single] + [(h0, x) for x in single]
    cases += [(x, y) for x in (single[0], single[3], single[4], single[127]) for y in single[::9]]
    cases += [(0, h0), (h0, 0), (2**128 - 1, h0), (h0, 2**128 - 1), (2**128 - 1, 2**128 - 1)]
    # a low nibble of every value, so that every reduction constant of the shift occurs with a known operand
    cases += [(2**128 - 1, 1 << k) for k in range(8)] + [(n, h0 | 0xF) for n in range(16)]
    for x, h in cases:
        hl.hl_ghash_mul_tab4(_b(x), _b(h), out)
        hl.hl_ghash_mul(_b(x), _b(h), ref)
        assert out.raw == ref.raw == _b(H._ghash_mul(x, h)), (hex(x), hex(h))


TOTALS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
TAILS = [1, 15, 16]


@pytest.mark.parametrize("total", TOTALS)
def test_lane_split_ghash_equals_the_oracle(hl, total):
    """The combined tag input of the 64 emulated lanes equals _ghash, for every AAD / ciphertext split of every total
    at and around one, two and three strides, with a last ciphertext block of 1, 15 and 16 bytes (and a partial last
    AAD block for odd AAD block counts); the order in which the lanes are combined does not matter."""
    rnd = random.Random(total)
    out = ctypes.create_string_buffer(16)
    exps = (ctypes.c_uint32 * 64)()
    seen = 0
    for na in range(total + 1):
        nc = total - na
        for tail in TAILS if nc else [16]:
            alen = 16 * na - (3 if na % 2 else 0)
            clen = 16 * nc - (16 - tail) if nc else 0
            h, aad, ct = rnd.getrandbits(128), rnd.randbytes(alen), rnd.randbytes(clen)
            want = _b(H._ghash(h, aad, ct))
            for rot in ((0, 37) if na in (0, 6) else (0,)):
                hl.hl_ghash_lanes(_b(h), aad, alen, ct, clen, rot, out, exps)
                assert out.raw == want, (na, nc, tail, rot)
            # the exponents: lane j's last block is k_j, its power total - k_j, whichever lane holds the tail
            for j in range(64):
                own = list(range(j, total, 64))
                assert exps[j] == (total - own[-1] if own else 0), (total, j)
            seen += 1
    assert seen >= 1


def test_lane_split_ghash_sees_every_block(hl):
    """A bit flipped in any single block of a 3-stride message changes the result (a wrong stride power would skip
    block 64 + 5 or weigh it like another)."""
    rnd = random.Random(7)
    h, aad, ct = rnd.getrandbits(128), rnd.randbytes(92), rnd.randbytes(16 * 194 - 9)
    out = ctypes.create_string_buffer(16)
    hl.hl_ghash_lanes(_b(h), aad, len(aad), ct, len(ct), 0, out, None)
    good = out.raw
    assert good == _b(H._ghash(h, aad, ct))
    for blk in (0, 5, 63, 64, 64 + 5, 127, 128, 193):
        bad = bytearray(ct)
        bad[16 * blk + 3] ^= 0x10
        hl.hl_ghash_lanes(_b(h), aad, len(aad), bytes(bad), len(ct), 0, out, None)
        assert out.raw == _b(H._ghash(h, aad, bytes(bad))) != good, blk


def test_aes_t_table_both_key_lengths(hl):
    out = ctypes.create_string_buffer(16)
    hl.hl_aes_t(bytes(range(32)), 32, bytes.fromhex("00112233445566778899aabbccddeeff"), out)
    assert out.raw.hex() == "8ea2b7ca516745bfeafc49904b496089"  # FIPS 197 Appendix C.3
    hl.hl_aes_t(bytes(range(16)), 16, bytes.fromhex("00112233445566778899aabbccddeeff"), out)
    assert out.raw.hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"  # FIPS 197 Appendix C.1
    rnd = random.Random(197)
    for _ in range(20):
        for n in (16, 32):
            key, blk = rnd.randbytes(n), rnd.randbytes(16)
            hl.hl_aes_t(key, n, blk, out)
            assert out.raw == S.aes_encrypt_block(S.aes_expand(key), blk)


# ---------------------------------------------------------------------------- the Report codec, handle_upload's host checks


def test_report_codec_known_answers():
    """Report (messages/src/lib.rs:1353-1432) against the reference's roundtrip_report vectors."""
    import json

    from janus_amd.messages import CodecError, HpkeCiphertext, Report, ReportMetadata

    vectors = json.load(open(os.path.join(HERE, "golden", "hpke_report_kat.json")))["vectors"]
    assert len(vectors) == 2
    for v in vectors:
        enc = bytes.fromhex("".join(v["encoded"]))
        ct = {k: HpkeCiphertext(v[k]["config_id"], bytes.fromhex(v[k]["encapsulated_key"]), bytes.fromhex(v[k]["payload"]))
              for k in ("leader", "helper")}
        rep = Report(ReportMetadata(bytes.fromhex(v["report_id"]), v["time"]), bytes.fromhex(v["public_share"]),
                     ct["leader"], ct["helper"])
        assert rep.encode() == enc
        assert Report.decode(enc) == rep
        with pytest.raises(CodecError):
            Report.decode(enc + b"\0")
        with pytest.raises(CodecError):
            Report.decode(enc[:-1])


class _StubEngine:
    """Stands in for HelperEngine: records what handle_upload sends to the device and accepts it all."""

    class vdaf:  # noqa: N801
        public_share_len = 4

    def __init__(self):
        self.calls = []

    def leader_upload_open(self, ids, times, ps, task_id, keypairs, key_index, encs, payloads, lis_stride=0):
        from janus_amd.engine import UploadOpen
        import numpy as np

        self.calls.append((bytes(ids), list(times), bytes(ps), task_id, list(keypairs), key_index.tolist(), encs, payloads))
        n = len(payloads)
        return UploadOpen(np.zeros(n, np.uint8), [b""] * n, "rows", 64)


def test_handle_upload_time_checks_need_no_engine():
    """The three time rejections of handle_upload_generic (aggregator.rs:1544-1573), in its order and with its
    comparisons (strictly after), and the public share's length, are made on the host: such reports never reach the
    engine, the others do, in order, with the keypairs of their config id."""
    from janus_amd.aggregator import (ReportRejection, ReportRejectionReason, StoredReport, UploadTask, handle_upload)
    from janus_amd.messages import HpkeCiphertext, Report, ReportMetadata

    now, skew, expiration, expiry_age = 1_000_000, 60, 1_000_030, 5000
    task_key, global_key = object(), object()
    task = UploadTask(b"T" * 32, {7: task_key}, skew, expiration, expiry_age)

    def rep(i, t, ps=b"3210", cfg=7):
        return Report(ReportMetadata(bytes([i]) * 16, t), ps, HpkeCiphertext(cfg, b"e" * 32, b"leader%d" % i),
                      HpkeCiphertext(1, b"h" * 32, b"helper"))

    R = ReportRejectionReason
    cases = [
        (rep(0, now + skew), R.TaskExpired),        # at the deadline: not too early, but past the task's end
        (rep(1, now + skew + 1), R.TooEarly),       # too early wins over expired task
        (rep(2, expiration), None),                 # at the task's end: accepted
        (rep(3, expiration + 1), R.TaskExpired),
        (rep(4, now - expiry_age), None),           # now == time + age: not expired
        (rep(5, now - expiry_age - 1), R.Expired),
        (rep(6, now, ps=b"321"), R.DecodeFailure),  # public share of another length
        (rep(7, now, cfg=9), None),                 # a config id only the global keys hold
        (rep(8, now, cfg=11), None),                # unknown everywhere: the engine reports it (KEY_NONE)
    ]
    eng = _StubEngine()
    reports = [c[0] for c in cases]
    out = handle_upload(eng, task, [r.encode() if i % 2 else r for i, r in enumerate(reports)], now,
                        global_keypairs={7: global_key, 9: global_key})
    for i, (r, want) in enumerate(cases):
        got = out.results[i]
        if want is None:
            assert isinstance(got, StoredReport) and got.metadata == r.metadata, i
            assert got.helper_encrypted_input_share == r.helper_encrypted_input_share
        else:
            assert got == ReportRejection(task.task_id, r.metadata.report_id, r.metadata.time, want), i
    assert out.counters == {"upload_decode_failure": 1}
    (ids, times, ps, task_id, keypairs, key_index, encs, payloads), = eng.calls
    sent = [2, 4, 7, 8]
    assert ids == b"".join(reports[i].metadata.report_id for i in sent) and times == [reports[i].metadata.time for i in sent]
    assert payloads == [b"leader%d" % i for i in sent] and ps == b"3210" * 4 and task_id == task.task_id
    assert keypairs == [task_key, global_key]
    assert key_index == [[0, 1], [0, 1], [1, 0xFF], [0xFF, 0xFF]]
    assert [out.results[i].row for i in sent] == [0, 1, 2, 3]
    # no report left for the device: the engine is not called
    eng2 = _StubEngine()
    out2 = handle_upload(eng2, task, [rep(1, now + skew + 1)], now)
    assert eng2.calls == [] and out2.rows is None and out2.results[0].reason == R.TooEarly
