"""GPU: the wave-per-report HPKE open of long payloads (jx_hpke_open_long_batch[_device], jx_hpke_long.hip) against
the three Python references that seal (oracle/hpke_oracle.py for the default suite, tests/hpke_suites_ref.py for the
other X25519 suites, tests/hpke_p256_ref.py for the P-256 KEM) and against the per-lane open on the same inputs.

Each suite's batch is sealed once and shared by the tests that need it (a Python AES-GCM seal of 3 KB takes a
quarter of a second). The batch holds every plaintext length of LENS (0..200 AES blocks: 63, 64, 65, 128, 129 and
200 blocks with full and partial tails, that is one, two, three and four 64-block strides of the lanes) and every
associated-data length of AAD_LENS; payloads and associated data are packed back to back, so most start at odd
byte offsets."""
from __future__ import annotations

import ctypes
import functools
import random

import numpy as np
import pytest

import hpke_p256_ref as R
import hpke_suites_ref as S
from janus_amd import hpke
from oracle import hpke_oracle as H

pytestmark = pytest.mark.gpu

INFO = H.dap_info(recipient=hpke.ROLE_LEADER)
X25519, P256 = hpke.KEM_X25519_HKDF_SHA256, hpke.KEM_P256_HKDF_SHA256
LENS = [0, 1, 15, 16, 17, 1007, 1008, 1023, 1024, 1025, 1040, 2037, 2048, 2064, 3207]
AAD_LENS = [0, 1, 16, 92, 1027]
BIG = LENS.index(3207)  # the 3-stride payload: 201 blocks, the last one of 7 bytes

SUITES = [(X25519, 1, 1), (X25519, 1, 2), (X25519, 1, 3), (X25519, 2, 1), (X25519, 3, 2), (P256, 1, 1)]


@functools.lru_cache(maxsize=None)
def _sealed(kem: int, kdf: int, aead: int):
    """(sk, pk, encs, cts, aads, pts) of one batch; report i has LENS[i] plaintext bytes and AAD_LENS[(i + 4) % 5]
    of associated data (the 3-stride payload gets the DAP-shaped 92 bytes)."""
    rnd = random.Random(1000 * kem + 10 * kdf + aead)
    if kem == P256:
        sk = rnd.randrange(1, R.N).to_bytes(32, "big")
        pk = R.public_key(sk)
    else:
        sk = rnd.randbytes(32)
        pk = H.x25519_base(sk)
    encs, cts, aads, pts = [], [], [], []
    for i, n in enumerate(LENS):
        aad, pt = rnd.randbytes(AAD_LENS[(i + 4) % 5]), rnd.randbytes(n)
        if kem == P256:
            enc, ct = R.seal_base(kdf, aead, pk, INFO, aad, pt, rnd.randrange(1, R.N).to_bytes(32, "big"))
        elif (kdf, aead) == (1, 1):
            enc, ct = H.seal_base(pk, INFO, aad, pt, rnd.randbytes(32))
        else:
            enc, ct = S.seal_base(kdf, aead, pk, INFO, aad, pt, rnd.randbytes(32))
        encs.append(enc)
        cts.append(ct)
        aads.append(aad)
        pts.append(pt)
    assert len(aads[BIG]) == 92 and {len(a) for a in aads} == set(AAD_LENS)
    return sk, pk, encs, cts, aads, pts


def _opener(kem, kdf, aead):
    sk, pk = _sealed(kem, kdf, aead)[:2]
    return hpke.HpkeOpener(sk, pk, INFO, kem_id=kem, kdf_id=kdf, aead_id=aead)


def _ref_open(kem, kdf, aead, enc, aad, ct):
    sk, pk = _sealed(kem, kdf, aead)[:2]
    if kem == P256:
        return R.open_base(kdf, aead, sk, pk, INFO, enc, aad, ct)
    if (kdf, aead) == (1, 1):
        return H.open_base(sk, pk, INFO, enc, aad, ct)
    return S.open_base(kdf, aead, sk, pk, INFO, enc, aad, ct)


@pytest.mark.parametrize("kem,kdf,aead", SUITES)
def test_long_open_vs_references(kem, kdf, aead):
    """Every plaintext and ok equals the reference's (which sealed them, and whose own open agrees), and the per-lane
    jx_hpke_open_batch gives the same on the same inputs."""
    _, _, encs, cts, aads, pts = _sealed(kem, kdf, aead)
    assert _ref_open(kem, kdf, aead, encs[5], aads[5], cts[5]) == pts[5]
    with _opener(kem, kdf, aead) as op:
        got = op.open_long_batch(encs, cts, aads)
        old = op.open_batch(encs, cts, aads)
    assert [None if g is None else len(g) for g in got] == LENS
    assert got == pts
    assert old == got


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    out = bytearray(b)
    out[byte] ^= 1 << bit
    return bytes(out)


@pytest.mark.parametrize("aead", [1, 2, 3])
def test_tampered_reports_fail_alone(aead):
    """One flipped bit in the first ciphertext block, in blocks lane 63 owns (GHASH block 63 is ciphertext block 57
    after the 6 blocks of associated data; CTR block 63), in block 64 + 5 of the 3-stride payload (which a wrong
    stride power would skip), in the last partial block, in the tag, in the associated data: ok = 0 for that
    report, and the untouched reports between them still open to the reference's plaintexts."""
    _, _, encs, cts, aads, pts = _sealed(X25519, 1, aead)
    enc, ct, aad, pt = encs[BIG], cts[BIG], aads[BIG], pts[BIG]
    assert len(ct) == 3207 + 16
    bad = [
        (_flip(ct, 3), aad),  # first block
        (_flip(ct, 16 * 57 + 9, 7), aad),  # lane 63's first GHASH block
        (_flip(ct, 16 * 63), aad),  # lane 63's first counter block
        (_flip(ct, 16 * 127 + 15, 3), aad),  # lane 63, second stride
        (_flip(ct, 16 * (64 + 5) + 1, 5), aad),  # second stride, lane 5 by counter, lane 11 by GHASH block
        (_flip(ct, 16 * (64 + 5 - 6) + 1, 5), aad),  # GHASH block 64 + 5
        (_flip(ct, 16 * 200 + 6, 1), aad),  # the last byte of the partial block
        (_flip(ct, 3207, 0), aad),  # tag, first byte
        (_flip(ct, 3207 + 15, 7), aad),  # tag, last bit
        (ct, _flip(aad, 40, 2)),  # associated data
        (ct, _flip(aad, 91, 0)),  # its partial last block
    ]
    e2, c2, a2, want = [], [], [], []
    for k, (c, a) in enumerate(bad):
        g = (7 * k) % len(LENS)  # an untouched report before each tampered one
        e2 += [encs[g], enc]
        c2 += [cts[g], c]
        a2 += [aads[g], a]
        want += [pts[g], None]
        if k in (0, 7, 9):  # (the reference agrees; one open of each kind keeps the test quick)
            assert _ref_open(X25519, 1, aead, enc, a, c) is None
    e2.append(enc), c2.append(ct), a2.append(aad), want.append(pt)
    with _opener(X25519, 1, aead) as op:
        got = op.open_long_batch(e2, c2, a2)
        old = op.open_batch(e2, c2, a2)
    assert got == want
    assert old == want


def test_kem_failures_and_short_rows():
    """What fails before the AEAD: an all-zero DH output, a P-256 encapsulated key off the curve. The other reports
    of the batch open."""
    _, _, encs, cts, aads, pts = _sealed(X25519, 1, 1)
    with _opener(X25519, 1, 1) as op:
        got = op.open_long_batch([encs[3], bytes(32), encs[9]], [cts[3], cts[9], cts[9]], [aads[3], aads[9], aads[9]])
    assert got == [pts[3], None, pts[9]]
    _, _, encs, cts, aads, pts = _sealed(P256, 1, 1)
    off = _flip(encs[9], 20, 3)
    assert R.decode(off) is None
    with _opener(P256, 1, 1) as op:
        got = op.open_long_batch([encs[3], off, encs[9]], [cts[3], cts[9], cts[9]], [aads[3], aads[9], aads[9]])
    assert got == [pts[3], None, pts[9]]


def test_device_buffers_and_every_byte_offset():
    """jx_hpke_open_long_batch_device on the caller's device buffers, with the one payload at each of the 16 byte
    offsets of its 16-byte line (and the plaintexts landing at every offset too): the same bytes as the host call,
    and nothing written outside a report's plaintext range."""
    import torch

    _, _, encs, cts, aads, pts = _sealed(X25519, 1, 2)
    i = LENS.index(1025)
    n = 16
    # 1025 + 16 = 1041 = 65 * 16 + 1 bytes each: report k of the back-to-back packing starts at offset k mod 16
    ct_buf = b"".join([cts[i]] * n)
    co = np.arange(n + 1, dtype=np.uint64) * len(cts[i])
    assert sorted(int(c) % 16 for c in co[:-1]) == list(range(16))
    aad_buf = b"".join([aads[i]] * n) or b"\0"
    ao = np.arange(n + 1, dtype=np.uint64) * len(aads[i])
    dev = torch.device("cuda")
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    d_enc, d_ct, d_aad = t(b"".join([encs[i]] * n)), t(ct_buf), t(aad_buf)
    d_co, d_ao = torch.from_numpy(co.astype(np.int64)).to(dev), torch.from_numpy(ao.astype(np.int64)).to(dev)
    d_pt = torch.full((n * 1025 + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    with _opener(X25519, 1, 2) as op:
        L = op._L
        st = L.jx_hpke_open_long_batch_device(op.handle, n, d_enc.data_ptr(), d_ct.data_ptr(), d_co.data_ptr(),
                                              d_aad.data_ptr(), d_ao.data_ptr(), d_pt.data_ptr(), d_ok.data_ptr())
        assert st == 0, L.jx_hpke_last_error(op.handle)
        torch.cuda.synchronize()
        pt, ok = d_pt.cpu().numpy(), d_ok.cpu().numpy()
    assert ok[:n].tolist() == [1] * n and ok[n:].tolist() == [7] * 64
    assert pt[:n * 1025].tobytes() == pts[i] * n
    assert pt[n * 1025:].tolist() == [0xA5] * 64


def test_refusals_before_any_launch():
    """A ciphertext of 2^32 bytes or more, one shorter than a tag, and missing pointers are JX_HPKE_E_INVALID; the
    offsets alone decide, no buffer is read."""
    with _opener(X25519, 1, 1) as op:
        L = op._L
        one = np.zeros(64, np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        ao = np.zeros(2, np.uint64)
        for end in (2**32 + 16, 2**32, 15):
            co = np.array([0, end], np.uint64)
            st = L.jx_hpke_open_long_batch(op.handle, 1, p(one), p(one), p(co), p(one), p(ao), p(one), p(one))
            assert st == hpke.E_INVALID, end
        assert b"2^32" in L.jx_hpke_last_error(op.handle) or b"16 bytes" in L.jx_hpke_last_error(op.handle)
        assert L.jx_hpke_open_long_batch(op.handle, 1, None, p(one), p(co), p(one), p(ao), p(one), p(one)) == hpke.E_INVALID
        assert L.jx_hpke_open_long_batch(op.handle, 0, None, None, None, None, None, None, None) == 0
