"""GPU: the wave-per-report open under ChaCha20Poly1305 (chapoly_wave_open of jx_hpke_long.hip, jx_chapoly_lanes.h)
through jx_hpke_open_long_batch[_device] and the leader's upload path, against the Python references that seal
(tests/hpke_suites_ref.py, tests/hpke_p256_ref.py) and against the per-lane open on the same inputs.

These are parity tests: the entry points and results are those of the serial code this replaces. They reach what the
batches of test_gpu_hpke_long.py (at most 3,207 bytes) do not: a second and third ChaCha20 stride (a stride is 64
lanes x 64 bytes = 4,096 bytes) next to the second Poly1305 stride (64 blocks = 1,024 bytes). Each suite's batch is
sealed once and shared (the Python ChaCha20 of 8 KB is the cost)."""
from __future__ import annotations

import functools
import random
import struct

import numpy as np
import pytest

import hpke_p256_ref as R
import hpke_suites_ref as S
from janus_amd import hpke
from janus_amd.engine import HelperEngine
from janus_amd.messages import Extension
from janus_amd.vdaf import Prio3
from oracle import hpke_oracle as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INFO = H.dap_info(recipient=hpke.ROLE_LEADER)
X25519, P256 = hpke.KEM_X25519_HKDF_SHA256, hpke.KEM_P256_HKDF_SHA256
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1007, 1008, 1024, 2048, 4095, 4096, 4097, 8192, 8263]
AAD_LENS = [0, 1, 16, 92, 1027]
BIG = LENS.index(8263)  # three ChaCha strides (130 blocks, the last one of 7 bytes), nine Poly1305 strides
SUITES = [(X25519, 1, 3), (X25519, 3, 3), (P256, 1, 3)]


class Key:
    """A recipient keypair of one suite, with the reference's seal and open."""

    def __init__(self, rnd, kem=X25519, kdf=1, aead=3):
        self.kem, self.kdf, self.aead = kem, kdf, aead
        if kem == P256:
            self.sk = rnd.randrange(1, R.N).to_bytes(32, "big")
            self.pk = R.public_key(self.sk)
        else:
            self.sk = rnd.randbytes(32)
            self.pk = H.x25519_base(self.sk)

    def opener(self):
        return hpke.HpkeOpener(self.sk, self.pk, INFO, kem_id=self.kem, kdf_id=self.kdf, aead_id=self.aead)

    def seal(self, rnd, aad, pt):
        if self.kem == P256:
            return R.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, rnd.randrange(1, R.N).to_bytes(32, "big"))
        return S.seal_base(self.kdf, self.aead, self.pk, INFO, aad, pt, rnd.randbytes(32))

    def open(self, enc, aad, ct):
        if self.kem == P256:
            return R.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 65 else None
        return S.open_base(self.kdf, self.aead, self.sk, self.pk, INFO, enc, aad, ct) if len(enc) == 32 else None


@functools.lru_cache(maxsize=None)
def _sealed(kem: int, kdf: int, aead: int):
    """(key, encs, cts, aads, pts) of one batch; report i has LENS[i] plaintext bytes and AAD_LENS[(i + 2) % 5] of
    associated data (the 3-stride payload gets the DAP-shaped 92 bytes)."""
    rnd = random.Random(1000 * kem + 10 * kdf + aead)
    key = Key(rnd, kem, kdf, aead)
    encs, cts, aads, pts = [], [], [], []
    for i, n in enumerate(LENS):
        aad, pt = rnd.randbytes(AAD_LENS[(i + 2) % 5]), rnd.randbytes(n)
        enc, ct = key.seal(rnd, aad, pt)
        encs.append(enc), cts.append(ct), aads.append(aad), pts.append(pt)
    assert len(aads[BIG]) == 92 and {len(a) for a in aads} == set(AAD_LENS)
    return key, encs, cts, aads, pts


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    out = bytearray(b)
    out[byte] ^= 1 << bit
    return bytes(out)


@pytest.mark.parametrize("kem,kdf,aead", SUITES)
def test_long_open_vs_references(kem, kdf, aead):
    """Every plaintext equals the one the reference sealed (whose own open agrees), and the per-lane
    jx_hpke_open_batch gives the same on the same inputs. Payloads and associated data are packed back to back, so
    most start at odd byte offsets."""
    key, encs, cts, aads, pts = _sealed(kem, kdf, aead)
    assert key.open(encs[BIG], aads[BIG], cts[BIG]) == pts[BIG]
    assert any(sum(len(c) for c in cts[:i]) % 2 for i in range(len(cts)))
    with key.opener() as op:
        got = op.open_long_batch(encs, cts, aads)
        old = op.open_batch(encs, cts, aads)
    assert [None if g is None else len(g) for g in got] == LENS
    assert got == pts
    assert old == got


def test_tampered_reports_fail_alone():
    """One flipped bit in ciphertext byte 0, in Poly1305 block 64 (the second MAC stride: 6 blocks of associated
    data, so ciphertext block 58), past byte 4,096 (the second ChaCha20 stride), in the last ciphertext byte, in the
    tag, in the associated data and in the encapsulated key: ok = 0 for that report, and the untouched reports
    between them (its neighbours in the workgroup of four) still open to the reference's plaintexts."""
    key, encs, cts, aads, pts = _sealed(X25519, 1, 3)
    enc, ct, aad, pt = encs[BIG], cts[BIG], aads[BIG], pts[BIG]
    assert len(ct) == 8263 + 16 and len(aad) == 92
    bad = [
        (enc, _flip(ct, 0, 6), aad),  # ciphertext byte 0
        (enc, _flip(ct, 16 * 58 + 9, 7), aad),  # Poly1305 block 64: lane 0's second block
        (enc, _flip(ct, 4096 + 64 * 5 + 33, 2), aad),  # ChaCha20 block 64 + 5: lane 5's second block
        (enc, _flip(ct, 8192 + 3, 1), aad),  # the third ChaCha20 stride
        (enc, _flip(ct, 8262, 4), aad),  # the last ciphertext byte
        (enc, _flip(ct, 8263, 0), aad),  # tag, first byte
        (enc, _flip(ct, 8263 + 15, 7), aad),  # tag, last bit
        (enc, ct, _flip(aad, 40, 2)),  # associated data
        (enc, ct, _flip(aad, 91, 0)),  # its partial last block
        (_flip(enc, 7, 3), ct, aad),  # the encapsulated key
    ]
    e2, c2, a2, want = [], [], [], []
    for k, (e, c, a) in enumerate(bad):
        g = (7 * k) % len(LENS)  # an untouched report before each tampered one
        e2 += [encs[g], e]
        c2 += [cts[g], c]
        a2 += [aads[g], a]
        want += [pts[g], None]
        if k in (1, 2, 7, 9):  # (the reference agrees; a few opens keep the test quick)
            assert key.open(e, a, c) is None
    e2.append(enc), c2.append(ct), a2.append(aad), want.append(pt)
    with key.opener() as op:
        got = op.open_long_batch(e2, c2, a2)
        old = op.open_batch(e2, c2, a2)
    assert got == want
    assert old == want


@pytest.mark.parametrize("n_pt", [65, 4097])
def test_device_buffers_and_every_byte_offset(n_pt):
    """jx_hpke_open_long_batch_device on the caller's device buffers, with one payload at each of the 16 byte offsets
    of its 16-byte line (and the plaintexts landing at every offset too), at a length of two ChaCha20 blocks and at
    one of two strides, each with a one-byte tail: the same bytes as the reference's, nothing written outside a
    report's plaintext range, and nothing written for a report whose tag fails."""
    import torch

    key, encs, cts, aads, pts = _sealed(X25519, 1, 3)
    i = LENS.index(n_pt)
    n = 16
    # n_pt + 16 = 16 k + 1 bytes each: report k of the back-to-back packing starts at offset k mod 16
    assert (n_pt + 16) % 16 == 1
    bad = _flip(cts[i], n_pt - 1, 5)  # the 17th report, at offset 0 again: its last ciphertext byte is tampered
    ct_buf = b"".join([cts[i]] * n) + bad
    co = np.arange(n + 2, dtype=np.uint64) * len(cts[i])
    assert sorted(int(c) % 16 for c in co[:n]) == list(range(16))
    aad_buf = b"".join([aads[i]] * (n + 1)) or b"\0"
    ao = np.arange(n + 2, dtype=np.uint64) * len(aads[i])
    dev = torch.device("cuda")
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    d_enc, d_ct, d_aad = t(b"".join([encs[i]] * (n + 1))), t(ct_buf), t(aad_buf)
    d_co, d_ao = torch.from_numpy(co.astype(np.int64)).to(dev), torch.from_numpy(ao.astype(np.int64)).to(dev)
    d_pt = torch.full(((n + 1) * n_pt + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n + 1 + 64,), 7, dtype=torch.uint8, device=dev)
    with key.opener() as op:
        L = op._L
        st = L.jx_hpke_open_long_batch_device(op.handle, n + 1, d_enc.data_ptr(), d_ct.data_ptr(), d_co.data_ptr(),
                                              d_aad.data_ptr(), d_ao.data_ptr(), d_pt.data_ptr(), d_ok.data_ptr())
        assert st == 0, L.jx_hpke_last_error(op.handle)
        torch.cuda.synchronize()
        pt, ok = d_pt.cpu().numpy(), d_ok.cpu().numpy()
    assert ok[:n + 1].tolist() == [1] * n + [0] and ok[n + 1:].tolist() == [7] * 64
    assert pt[:n * n_pt].tobytes() == pts[i] * n
    assert pt[n * n_pt:].tolist() == [0xA5] * (n_pt + 64)


# ---------------------------------------------------------------------------- the upload path

TASK = bytes(range(32))
P128 = 2**128 - 28 * 2**64 + 1
OK, DECRYPT, PLAINTEXT, INPUT_SHARE, UNKNOWN = 0, 1, 2, 6, 7
VDAF = Prio3.histogram(512, 23)  # leader input share of 9,952 bytes: past two ChaCha20 strides (8,256 with the framing)

_rk = random.Random(303)
CHACHA_TASK = Key(_rk, aead=3)                # config id 1, the task's
AES_GLOBAL = Key(_rk, aead=2)                 # config id 1, the global fallback of the same id
AES_TASK = Key(_rk, aead=2)                   # config id 2, the task's
CHACHA_GLOBAL = Key(_rk, kdf=3, aead=3)       # config id 2, the global fallback of the same id
CHACHA_P256 = Key(_rk, kem=P256, aead=3)      # config id 3, global only
STRANGER = Key(_rk, aead=3)                   # nobody's key
KEYS = [CHACHA_TASK, AES_GLOBAL, AES_TASK, CHACHA_GLOBAL, CHACHA_P256]
TASK_KEYS = {1: CHACHA_TASK, 2: AES_TASK}
GLOBAL_KEYS = {1: AES_GLOBAL, 2: CHACHA_GLOBAL, 3: CHACHA_P256}
EXT1 = Extension(0x0000, b"hello").encode()


def _plaintext(exts: bytes, payload: bytes) -> bytes:
    return struct.pack(">H", len(exts)) + exts + struct.pack(">I", len(payload)) + payload


def _set_elem(lis: bytes, idx: int, value: int) -> bytes:
    return lis[:16 * idx] + value.to_bytes(16, "little") + lis[16 * (idx + 1):]


def _cases():
    """(kind, sealing key, config id, plaintext builder)"""
    last = VDAF.meas_len + VDAF.num_proofs * VDAF.proof_len - 1
    good = lambda lis: _plaintext(b"", lis)  # noqa: E731
    return [
        ("chacha_first", CHACHA_TASK, 1, lambda lis: _plaintext(EXT1, lis)),
        ("aes_fallback", AES_GLOBAL, 1, good),        # the ChaCha task key fails, the AES-256-GCM global one opens
        ("chacha_fallback", CHACHA_GLOBAL, 2, good),  # the reverse: the AES task key fails, the ChaCha global one opens
        ("aes_first", AES_TASK, 2, good),             # the AES task key opens: no ChaCha trial in that wave
        ("chacha_p256", CHACHA_P256, 3, good),        # a ChaCha P-256 key only the global keys hold
        ("stranger", STRANGER, 1, good),              # both trials fail
        ("p_proof_last", CHACHA_TASK, 1, lambda lis: _plaintext(b"", _set_elem(lis, last, P128))),
        ("pm1_proof_last", CHACHA_TASK, 1, lambda lis: _plaintext(b"", _set_elem(lis, last, P128 - 1))),
        ("tamper_stride2", CHACHA_TASK, 1, good),     # a flipped bit past byte 4,096
        ("unknown_config", CHACHA_TASK, 9, good),
    ]


@functools.lru_cache(maxsize=None)
def _upload_reports():
    """(kinds, report ids, times, public shares, config ids, encs, payloads, verify key)"""
    orc = O.Prio3Oracle(VDAF.algo_id, VDAF.bits, VDAF.length, VDAF.chunk_length, VDAF.num_proofs)
    rnd = random.Random("upload-chapoly")
    out = []
    for i, (kind, key, cfg, build) in enumerate(_cases()):
        rid = rnd.randbytes(16)
        ps, lis, _ = orc.shard(rnd.randrange(VDAF.length), rid, rnd.randbytes(orc.sizes.client_rand))
        assert len(lis) == VDAF.leader_input_share_len > 8256
        t = 1_700_000_000 + i
        enc, ct = key.seal(rnd, hpke.input_share_aad(TASK, rid, t, ps), build(lis))
        if kind == "tamper_stride2":
            ct = _flip(ct, 4096 + 64 * 9 + 17, 3)
        out.append((kind, rid, t, ps, cfg, enc, ct))
    return out


def _ref_upload(rid, t, ps, cfg, enc, ct):
    """handle_upload_generic after its time checks, restated: (status, extension bytes, payload)."""
    keys = [k for k in (TASK_KEYS.get(cfg), GLOBAL_KEYS.get(cfg)) if k is not None]
    if not keys:
        return UNKNOWN, b"", None
    aad = hpke.input_share_aad(TASK, rid, t, ps)
    pt = None
    for k in keys:
        pt = k.open(enc, aad, ct)
        if pt is not None:
            break
    if pt is None:
        return DECRYPT, b"", None
    # PlaintextInputShare::get_decoded
    if len(pt) < 2 or 2 + int.from_bytes(pt[:2], "big") > len(pt):
        return PLAINTEXT, b"", None
    end = 2 + int.from_bytes(pt[:2], "big")
    i = 2
    while i < end:
        if i + 4 > end or int.from_bytes(pt[i:i + 2], "big") not in (0x0000, 0xFF00):
            return PLAINTEXT, b"", None
        i += 4 + int.from_bytes(pt[i + 2:i + 4], "big")
        if i > end:
            return PLAINTEXT, b"", None
    if end + 4 > len(pt) or end + 4 + int.from_bytes(pt[end:end + 4], "big") != len(pt):
        return PLAINTEXT, b"", None
    payload = pt[end + 4:]
    # A::InputShare::get_decoded_with_param(&(&vdaf, 0), payload)
    ne = VDAF.meas_len + VDAF.num_proofs * VDAF.proof_len
    if len(payload) != VDAF.leader_input_share_len or any(
            int.from_bytes(payload[16 * k:16 * (k + 1)], "little") >= P128 for k in range(ne)):
        return INPUT_SHARE, b"", None
    return OK, pt[2:end], payload


def test_upload_open_mixed_aeads_vs_restated_loop():
    """The leader's upload path on shares of 9,952 bytes whose two trials name different AEADs: a ChaCha task key with
    an AES-256-GCM global fallback of the same config id, the reverse, a ChaCha P-256 global-only key and a
    stranger's key, in one launch (so in the same workgroups). Status, row and extension list of every report equal
    the restated loop's; a rejected report's row is zero. An element equal to p at the last proof element is refused
    (p - 1 is not), and so is a flipped bit in the second ChaCha20 stride."""
    reports = _upload_reports()
    kinds = [r[0] for r in reports]
    want = [_ref_upload(*r[1:]) for r in reports]
    by_kind = dict(zip(kinds, want))
    assert by_kind["chacha_first"][:2] == (OK, EXT1)
    assert {by_kind[k][0] for k in ("aes_fallback", "chacha_fallback", "aes_first", "chacha_p256", "pm1_proof_last")} == {OK}
    assert by_kind["stranger"][0] == by_kind["tamper_stride2"][0] == DECRYPT
    assert by_kind["p_proof_last"][0] == INPUT_SHARE and by_kind["unknown_config"][0] == UNKNOWN
    idx = {id(k): i for i, k in enumerate(KEYS)}
    ki = []
    for r in reports:
        ks = [k for k in (TASK_KEYS.get(r[4]), GLOBAL_KEYS.get(r[4])) if k is not None]
        ki.append([idx[id(ks[0])] if ks else 0xFF, idx[id(ks[1])] if len(ks) > 1 else 0xFF])
    n, lis = len(reports), VDAF.leader_input_share_len
    openers = [k.opener() for k in KEYS]
    try:
        with HelperEngine(VDAF, bytes(VDAF.verify_key_len)) as eng:
            got = eng.leader_upload_open(
                np.frombuffer(b"".join(r[1] for r in reports), np.uint8).reshape(n, 16), [r[2] for r in reports],
                np.frombuffer(b"".join(r[3] for r in reports), np.uint8), TASK, openers, np.array(ki, np.uint8),
                [r[5] for r in reports], [r[6] for r in reports])
            rows = got.rows.cpu().numpy()
    finally:
        for o in openers:
            o.close()
    assert got.status.tolist() == [w[0] for w in want], kinds
    assert got.extensions == [w[1] for w in want]
    assert rows.shape == (n, lis)
    for i, (st, _, payload) in enumerate(want):
        assert rows[i].tobytes() == (payload if st == OK else bytes(lis)), kinds[i]
