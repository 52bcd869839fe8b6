"""GPU: HPKE seal (jx_hpke_seal_batch / jx_hpke_seal_long_batch, janus_amd/csrc/jx_hpke_seal.hip) under the nine
X25519 suites, byte for byte against tests/hpke_suites_ref.py (pinned by the reference's RFC 9180 vectors) with the
ephemeral keys given: the RFC 9180 A.1.1 vector from its skEm, every suite in the short and the long form, the edge
cases of the keys, the round trip through the existing opens, a low-order recipient key, and what the calls refuse."""
from __future__ import annotations

import ctypes
import json
import os
import random

import numpy as np
import pytest

import hpke_suites_ref as S
from janus_amd import hpke
from janus_amd.engine import HelperEngine
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpke_rfc9180.json")
INFO = H.dap_info()
SKE_A11 = bytes.fromhex("52c4a758a802cd8b936eceea314432798d5baf2d7e9235dc084ab1b9cfa2f736")  # RFC 9180 A.1.1 skEm
SHORT_LENS = [1, 0, 15, 16, 17, 54, 255]
LONG_LENS = [1, 0, 1023, 1024, 1025]           # one AES block per lane, +- 1
CHACHA_LENS = [4095, 4096, 4097]               # one ChaCha20 block per lane, +- 1
AAD_LENS = [0, 1, 16, 60, 92]
LIS_SUMVEC = Prio3.sum_vec(8, 1000, 88).leader_input_share_len
N = 65


def _raw_seal(ctx, call, sks, pts, aads, start=1):
    """The C call itself, with the plaintexts packed from byte `start` on (so they begin at odd offsets wherever the
    lengths before them allow): (status, encs, cts, ok)."""
    L = hpke._declare(hpke._lib.load())
    n = len(sks)
    po = np.zeros(n + 1, np.uint64)
    ao = np.zeros(n + 1, np.uint64)
    po[0], ao[0] = start, start
    po[1:] = start + np.cumsum([len(p) for p in pts])
    ao[1:] = start + np.cumsum([len(a) for a in aads])
    sk = np.frombuffer(b"".join(sks) or b"\0", np.uint8).copy()
    pt = np.frombuffer(b"\xee" * start + b"".join(pts) + b"\0", np.uint8).copy()
    ad = np.frombuffer(b"\xee" * start + b"".join(aads) + b"\0", np.uint8).copy()
    encs = np.full(32 * max(n, 1), 0xA5, np.uint8)
    cts = np.full(int(po[-1]) + 16 * n + 1, 0xA5, np.uint8)
    ok = np.full(max(n, 1), 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = getattr(L, call)(ctx.handle, n, p(sk), p(pt), p(po), p(ad), p(ao), p(encs), p(cts), p(ok))
    out = [(encs[32 * i:32 * i + 32].tobytes(), cts[int(po[i]) + 16 * i:int(po[i + 1]) + 16 * (i + 1)].tobytes())
           for i in range(n)]
    return st, out, ok[:n]


def test_rfc9180_a11():
    v = json.load(open(GOLDEN))["vectors"][0]
    pk, info, enc = (bytes.fromhex(v[k]) for k in ("pkRm", "info", "enc"))
    e0 = v["encryptions"][0]
    assert H.x25519_base(SKE_A11) == enc  # the key is the vector's skEm
    aad, pt = bytes.fromhex(e0["aad"]), bytes.fromhex(e0["pt"])
    assert S.seal_base(1, 1, pk, info, aad, pt, SKE_A11) == (enc, bytes.fromhex(e0["ct"]))
    with hpke.HpkeSealer(pk, info) as s:
        assert s.suite == (hpke.KEM_X25519_HKDF_SHA256, 1, 1) and s.enc_len == 32
        assert s.seal_batch([SKE_A11], [pt], [aad]) == [(enc, bytes.fromhex(e0["ct"]))]
        assert s.seal_long_batch([SKE_A11], [pt], [aad]) == [(enc, bytes.fromhex(e0["ct"]))]


def _cases(rnd, lens, n=N):
    sks = [rnd.randbytes(32) for _ in range(n)]
    assert len(set(sks)) == n  # all-distinct ephemeral keys
    pts = [rnd.randbytes(lens[i % len(lens)]) for i in range(n)]
    aads = [rnd.randbytes(AAD_LENS[(i // 2) % len(AAD_LENS)]) for i in range(n)]
    return sks, pts, aads


@pytest.mark.parametrize("kdf,aead", S.SUITES)
def test_every_suite(kdf, aead):
    """n = 1, 64 and 65 (a wave of lane pairs holds 32 seals: two waves, and one seal more), short and long form."""
    rnd = random.Random(5000 + 10 * kdf + aead)
    pk = H.x25519_base(rnd.randbytes(32))
    long_lens = LONG_LENS + (CHACHA_LENS if aead == 3 else [])
    with hpke.HpkeSealer(pk, INFO, kdf_id=kdf, aead_id=aead) as s:
        for call, lens in (("jx_hpke_seal_batch", SHORT_LENS), ("jx_hpke_seal_long_batch", long_lens)):
            sks, pts, aads = _cases(rnd, lens)
            if call.endswith("long_batch") and kdf == 1:  # a leader's share of the headline instance
                pts[3] = rnd.randbytes(6 + LIS_SUMVEC)
            want = [S.seal_base(kdf, aead, pk, INFO, aads[i], pts[i], sks[i]) for i in range(N)]
            for n in (1, 64, 65):
                st, got, ok = _raw_seal(s, call, sks[:n], pts[:n], aads[:n])
                assert st == 0 and ok.tolist() == [1] * n, (call, n)
                bad = [i for i in range(n) if got[i] != want[i]]
                assert not bad, f"{call} ({kdf}, {aead}) n={n}: seals {bad[:8]} differ (lengths {[len(pts[i]) for i in bad[:8]]})"


def test_key_edge_cases():
    rnd = random.Random(77)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    hi = rnd.randbytes(31) + bytes([0x80 | rnd.randrange(128)])  # a recipient key with bit 255 set
    for pkr in (pk, hi):
        with hpke.HpkeSealer(pkr, INFO, kdf_id=2, aead_id=3) as s:
            same = rnd.randbytes(32)
            sks = [bytes(32), b"\xff" * 32] + [same] * 64  # clamping; then the same key in every lane
            pts = [rnd.randbytes(54) for _ in sks]
            aads = [rnd.randbytes(92) for _ in sks]
            want = [S.seal_base(2, 3, pkr, INFO, aads[i], pts[i], sks[i]) for i in range(len(sks))]
            assert len({w[0] for w in want[2:]}) == 1
            for call in ("jx_hpke_seal_batch", "jx_hpke_seal_long_batch"):
                st, got, ok = _raw_seal(s, call, sks, pts, aads)
                assert st == 0 and ok.all() and got == want, call


@pytest.mark.parametrize("kdf,aead", [(1, 1), (3, 2), (2, 3)])
def test_round_trip_through_the_opens(kdf, aead):
    """A recipient context seals too, and the existing opens open what the device sealed."""
    rnd = random.Random(31 + aead)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    sks, pts, aads = _cases(rnd, [0, 1, 54, 255, 1025, 4097], n=40)
    with hpke.HpkeOpener(sk, pk, INFO, kdf_id=kdf, aead_id=aead) as op, \
            hpke.HpkeSealer(pk, INFO, kdf_id=kdf, aead_id=aead) as s:
        short, long = s.seal_batch(sks, pts, aads), op.seal_long_batch(sks, pts, aads)
        assert short == long and None not in short
        encs, cts = [e for e, _ in short], [c for _, c in short]
        assert op.open_batch(encs, cts, aads) == pts
        assert op.open_long_batch(encs, cts, aads) == pts


def test_zero_dh():
    rnd = random.Random(0)
    with hpke.HpkeSealer(bytes(32), INFO, kdf_id=1, aead_id=3) as s:
        sks, pts, aads = _cases(rnd, [0, 54, 1025], n=33)
        for call in ("jx_hpke_seal_batch", "jx_hpke_seal_long_batch"):
            st, got, ok = _raw_seal(s, call, sks, pts, aads)
            assert st == 0 and not ok.any()
            assert all(e == bytes(32) and c == bytes(len(c)) for e, c in got), call
        assert s.seal_batch(sks[:2], pts[:2], aads[:2]) == [None, None]


def test_device_forms():
    """jx_hpke_seal_batch_device / _long_batch_device, everything in HBM (the offsets too), give the host forms' bytes;
    a seal whose offsets decrease fails alone (ok = 0), since no host code sees them."""
    import torch

    rnd = random.Random(12)
    pk = H.x25519_base(rnd.randbytes(32))
    sks, pts, aads = _cases(rnd, [54, 0, 17, 1025, 4097], n=N)
    dev = torch.device("cuda", 0)
    po = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    ao = np.concatenate([[0], np.cumsum([len(a) for a in aads])]).astype(np.int64)
    to_dev = lambda b: torch.from_numpy(np.frombuffer(b + b"\0", np.uint8).copy()).to(dev)  # noqa: E731
    d_sk, d_pt, d_ad = to_dev(b"".join(sks)), to_dev(b"".join(pts)), to_dev(b"".join(aads))
    d_po, d_ao = torch.from_numpy(po).to(dev), torch.from_numpy(ao).to(dev)
    with hpke.HpkeSealer(pk, INFO, kdf_id=3, aead_id=3) as s:
        want = s.seal_batch(sks, pts, aads)
        for long in (False, True):
            d_enc = torch.full((32 * N,), 0xA5, dtype=torch.uint8, device=dev)
            d_ct = torch.full((int(po[-1]) + 16 * N,), 0xA5, dtype=torch.uint8, device=dev)
            d_ok = torch.full((N,), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.seal_batch_device(N, d_sk.data_ptr(), d_pt.data_ptr(), d_po.data_ptr(), d_ad.data_ptr(), d_ao.data_ptr(),
                                d_enc.data_ptr(), d_ct.data_ptr(), d_ok.data_ptr(), long=long)
            torch.cuda.ExternalStream(s.stream).synchronize()
            enc, ct, ok = d_enc.cpu().numpy(), d_ct.cpu().numpy(), d_ok.cpu().numpy()
            got = [(enc[32 * i:32 * i + 32].tobytes(), ct[int(po[i]) + 16 * i:int(po[i + 1]) + 16 * (i + 1)].tobytes())
                   for i in range(N)]
            assert ok.all() and got == want, long
        bad = po.copy()
        bad[2] = bad[1] - 1  # seal 1 ends before it begins; seal 2 is longer for it, and still a seal
        d_bad = torch.from_numpy(bad).to(dev)
        d_ok = torch.full((3,), 0xA5, dtype=torch.uint8, device=dev)
        d_enc = torch.zeros(96, dtype=torch.uint8, device=dev)
        d_ct = torch.zeros(int(po[3]) + 48, dtype=torch.uint8, device=dev)
        for long in (False, True):
            s.seal_batch_device(3, d_sk.data_ptr(), d_pt.data_ptr(), d_bad.data_ptr(), d_ad.data_ptr(), d_ao.data_ptr(),
                                d_enc.data_ptr(), d_ct.data_ptr(), d_ok.data_ptr(), long=long)
            torch.cuda.ExternalStream(s.stream).synchronize()
            assert d_ok.cpu().numpy().tolist() == [1, 0, 1], long


def test_refusals():
    L = hpke._declare(hpke._lib.load())
    rnd = random.Random(1)
    h = ctypes.c_void_p()
    pk65 = (ctypes.c_uint8 * 65)()
    assert L.jx_hpke_create_sender(0x10, 1, 1, pk65, 65, None, 0, 0, ctypes.byref(h)) == hpke.E_UNSUPPORTED == -2
    assert not h.value and b"P-256" in L.jx_hpke_last_error(None)
    with pytest.raises(hpke.UnsupportedSuite):
        hpke.HpkeSealer(bytes(65), INFO, kem_id=hpke.KEM_P256_HKDF_SHA256)
    with pytest.raises(hpke.UnsupportedSuite):
        hpke.HpkeSealer(bytes(32), INFO, kdf_id=4)
    sk = rnd.randbytes(32)
    pk = H.x25519_base(sk)
    v = Prio3.count()
    with hpke.HpkeSealer(pk, INFO) as s, hpke.HpkeOpener(sk, pk, INFO) as op, HelperEngine(v, bytes(16)) as eng:
        enc, ct = s.seal_batch([rnd.randbytes(32)], [b"x" * 54], [b"aad"])[0]
        # a sender context opens nothing: refused before anything is queued, in the stand-alone opens and in prepare
        co, ao = np.array([0, len(ct)], np.uint64), np.array([0, 3], np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        bufs = [np.frombuffer(x, np.uint8).copy() for x in (enc, ct, b"aad")]
        out, ok = np.zeros(64, np.uint8), np.zeros(1, np.uint8)
        for name in ("jx_hpke_open_batch", "jx_hpke_open_long_batch"):
            st = getattr(L, name)(s.handle, 1, p(bufs[0]), p(bufs[1]), p(co), p(bufs[2]), p(ao), p(out), p(ok))
            assert st == hpke.E_INVALID and b"sender" in L.jx_hpke_last_error(None), name
        with pytest.raises(Exception, match="sender context"):
            eng.helper_initialized_encrypted_batch(np.zeros((1, 16), np.uint8), [1], b"", bytes(32), [s], [[0, 0xFF]], [enc],
                                                   [ct], np.zeros((1, v.prep_share_len), np.uint8))
        # both are usable afterwards
        assert op.open_batch([enc], [ct], [b"aad"]) == [b"x" * 54]
        assert eng.shard_batch([1], bytes(16), bytes(eng.client_rand_bytes())).status.tolist() == [0]
        # decreasing offsets; n == 0
        sks = np.zeros(64, np.uint8)
        enc2, ct2, ok2 = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(2, np.uint8)
        for po, ao2 in (([0, 8, 4], [0, 0, 0]), ([0, 4, 8], [2, 1, 1])):
            for name in ("jx_hpke_seal_batch", "jx_hpke_seal_long_batch"):
                st = getattr(L, name)(s.handle, 2, p(sks), p(out), p(np.array(po, np.uint64)), p(out),
                                      p(np.array(ao2, np.uint64)), p(enc2), p(ct2), p(ok2))
                assert st == hpke.E_INVALID, (name, po)
        for name in ("jx_hpke_seal_batch", "jx_hpke_seal_long_batch", "jx_hpke_seal_batch_device",
                     "jx_hpke_seal_long_batch_device"):
            assert getattr(L, name)(s.handle, 0, None, None, None, None, None, None, None, None) == 0, name
        assert s.seal_batch([], [], []) == []
