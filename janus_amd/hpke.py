"""Batched HPKE open, and seal, of report shares on the GPU (wrapper of include/jx_hpke.h).

Mirror of janus_core::hpke::open (core/src/hpke.rs:200-230) as the helper calls it once per
report in its aggregate-init loop (aggregator/src/aggregator.rs:1772-1832): RFC 9180 base
mode with DHKEM(X25519, HKDF-SHA256) or DHKEM(P-256, HKDF-SHA256) and the KDF and AEAD of the keypair's HpkeConfig
(messages/src/lib.rs:768-846): HKDF-SHA256 / -SHA384 / -SHA512 with AES-128-GCM / AES-256-GCM /
ChaCha20Poly1305, by default X25519 / HKDF-SHA256 / AES-128-GCM: the 18 suites the reference opens. Application info HpkeApplicationInfo::new(&Label::InputShare,
&Role::Client, &Role::Helper) (core/src/hpke.rs:69-84), associated data the encoded InputShareAad
(messages/src/lib.rs:1854-1858). Here the whole request's ciphertexts are opened in one launch. There
is no CPU fallback: any other id is refused when the opener is created (UnsupportedSuite). HpkeSealer is the client's
side, janus_core::hpke::seal (core/src/hpke.rs:167): a context with the recipient's public key alone, which seals
under the nine X25519 suites (sealing under the P-256 KEM is out of scope: UnsupportedSuite) with ephemeral keys the
caller supplies. A P-256 keypair is a
32-byte private key (big-endian) with a 65-byte public key (the uncompressed SEC 1 point); its encapsulated keys
are 65 bytes.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import EngineError

# Role (messages/src/lib.rs:512-517) and Label (core/src/hpke.rs:56-66)
ROLE_COLLECTOR, ROLE_CLIENT, ROLE_LEADER, ROLE_HELPER = 0, 1, 2, 3
LABEL_INPUT_SHARE = b"dap-09 input share"
LABEL_AGGREGATE_SHARE = b"dap-09 aggregate share"

# HpkeKemId, HpkeKdfId, HpkeAeadId (messages/src/lib.rs:768-846): the ids the engine opens
KEM_X25519_HKDF_SHA256 = 0x0020
KEM_P256_HKDF_SHA256 = 0x0010
KDF_HKDF_SHA256, KDF_HKDF_SHA384, KDF_HKDF_SHA512 = 0x0001, 0x0002, 0x0003
AEAD_AES_128_GCM, AEAD_AES_256_GCM, AEAD_CHACHA20_POLY1305 = 0x0001, 0x0002, 0x0003
E_UNSUPPORTED = -2  # JX_HPKE_E_UNSUPPORTED
E_INVALID = -1  # JX_HPKE_E_INVALID

EXPORTED_SYMBOLS = ("jx_hpke_create", "jx_hpke_create_suite", "jx_hpke_create_key", "jx_hpke_create_sender",
                    "jx_hpke_seal_batch", "jx_hpke_seal_batch_device", "jx_hpke_seal_long_batch",
                    "jx_hpke_seal_long_batch_device", "jx_hpke_suite", "jx_hpke_enc_len",
                    "jx_hpke_stream", "jx_hpke_destroy",
                    "jx_hpke_open_batch", "jx_hpke_open_batch_device", "jx_hpke_open_long_batch",
                    "jx_hpke_open_long_batch_device", "jx_hpke_last_error")


class UnsupportedSuite(EngineError):
    """A KEM, KDF or AEAD id the engine does not open (include/jx_hpke.h: JX_HPKE_E_UNSUPPORTED)."""


def application_info(label: bytes = LABEL_INPUT_SHARE, sender: int = ROLE_CLIENT, recipient: int = ROLE_HELPER) -> bytes:
    """HpkeApplicationInfo::new (core/src/hpke.rs:74-84)."""
    return label + bytes([sender, recipient])


def input_share_aad(task_id: bytes, report_id: bytes, time: int, public_share: bytes) -> bytes:
    """InputShareAad encoding: task_id || ReportMetadata(id, time) || u32-prefixed public share
    (messages/src/lib.rs:1854-1858)."""
    if len(task_id) != 32 or len(report_id) != 16:
        raise ValueError("task id is 32 bytes, report id 16")
    return task_id + report_id + time.to_bytes(8, "big") + len(public_share).to_bytes(4, "big") + public_share


def _declare(L):
    if getattr(L, "_jx_hpke_declared", False):
        return L
    vp, u64, i32, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32
    L.jx_hpke_create.restype = i32
    L.jx_hpke_create.argtypes = [vp, vp, vp, u32, i32, ctypes.POINTER(vp)]
    L.jx_hpke_create_suite.restype = i32
    L.jx_hpke_create_suite.argtypes = [u32, u32, u32, vp, vp, vp, u32, i32, ctypes.POINTER(vp)]
    L.jx_hpke_create_key.restype = i32
    L.jx_hpke_create_key.argtypes = [u32, u32, u32, vp, u32, vp, u32, vp, u32, i32, ctypes.POINTER(vp)]
    L.jx_hpke_enc_len.restype = i32
    L.jx_hpke_enc_len.argtypes = [vp]
    L.jx_hpke_suite.restype = i32
    L.jx_hpke_suite.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.jx_hpke_stream.restype = i32
    L.jx_hpke_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.jx_hpke_destroy.restype = None
    L.jx_hpke_destroy.argtypes = [vp]
    L.jx_hpke_open_batch.restype = i32
    L.jx_hpke_open_batch.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.jx_hpke_open_batch_device.restype = i32
    L.jx_hpke_open_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    for name in ("jx_hpke_open_long_batch", "jx_hpke_open_long_batch_device"):
        f = getattr(L, name)  # a library without them is an error here, not a fall-back to the per-lane open
        f.restype = i32
        f.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.jx_hpke_create_sender.restype = i32
    L.jx_hpke_create_sender.argtypes = [u32, u32, u32, vp, u32, vp, u32, i32, ctypes.POINTER(vp)]
    for name in ("jx_hpke_seal_batch", "jx_hpke_seal_batch_device", "jx_hpke_seal_long_batch",
                 "jx_hpke_seal_long_batch_device"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.jx_hpke_last_error.restype = ctypes.c_char_p
    L.jx_hpke_last_error.argtypes = [vp]
    L._jx_hpke_declared = True
    return L


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


class _HpkeContext:
    """What a recipient context and a sender context share: the handle, its suite and stream, and seal."""

    def _adopt(self, h):
        self._h = h
        self._enc_len = int(self._L.jx_hpke_enc_len(h))
        kem, kdf, aead = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._L.jx_hpke_suite(h, ctypes.byref(kem), ctypes.byref(kdf), ctypes.byref(aead))
        self._suite = (kem.value, kdf.value, aead.value)

    @property
    def suite(self) -> tuple[int, int, int]:
        """(kem_id, kdf_id, aead_id) of the context, as jx_hpke_suite reports it."""
        return self._suite

    @property
    def enc_len(self) -> int:
        """The length of an encapsulated key under the context's KEM (jx_hpke_enc_len): 32 or 65."""
        return self._enc_len

    @property
    def handle(self):
        """The jx_hpke context (for jx_helper_prep_encrypted_batch, jx_client_seal_*)."""
        return self._h

    @property
    def stream(self) -> int:
        """The context's hipStream_t (jx_hpke_stream), on which the device-buffer calls run."""
        s = ctypes.c_void_p()
        st = self._L.jx_hpke_stream(self._h, ctypes.byref(s))
        if st != 0:
            raise EngineError(f"jx_hpke_stream: status {st}")
        return s.value or 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.jx_hpke_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def seal_long_batch(self, ephemeral_sks: list[bytes], plaintexts: list[bytes], aads: list[bytes]):
        """seal_batch for long payloads such as leader input shares (jx_hpke_seal_long_batch): the same bytes, with
        the AEAD of each seal spread over a wave."""
        return self.seal_batch(ephemeral_sks, plaintexts, aads, _call="jx_hpke_seal_long_batch")

    def seal_batch(self, ephemeral_sks: list[bytes], plaintexts: list[bytes], aads: list[bytes],
                   _call: str = "jx_hpke_seal_batch") -> list[tuple[bytes, bytes] | None]:
        """Seal n plaintexts to the context's public key, seal i under the X25519 private key ephemeral_sks[i] (32
        bytes from the caller's CSPRNG; the engine clamps it and draws no randomness). Returns (enc, ciphertext) per
        seal; None where the DH output was all zero (a low-order recipient key)."""
        n = len(ephemeral_sks)
        if not (len(plaintexts) == len(aads) == n) or any(len(k) != 32 for k in ephemeral_sks):
            raise ValueError("one 32-byte ephemeral key, plaintext and aad per seal")
        if n == 0:
            return []
        sks = np.frombuffer(b"".join(ephemeral_sks), np.uint8).copy()
        pts = np.frombuffer(b"".join(plaintexts) or b"\0", np.uint8).copy()
        aad = np.frombuffer(b"".join(aads) or b"\0", np.uint8).copy()
        po = np.zeros(n + 1, np.uint64)
        ao = np.zeros(n + 1, np.uint64)
        po[1:] = np.cumsum([len(p) for p in plaintexts])
        ao[1:] = np.cumsum([len(a) for a in aads])
        encs = np.zeros(32 * n, np.uint8)
        cts = np.zeros(int(po[-1]) + 16 * n, np.uint8)
        ok = np.zeros(n, np.uint8)
        st = getattr(self._L, _call)(self._h, n, _p(sks), _p(pts), _p(po), _p(aad), _p(ao), _p(encs), _p(cts), _p(ok))
        if st == E_UNSUPPORTED:
            raise UnsupportedSuite(self._L.jx_hpke_last_error(self._h).decode())
        if st != 0:
            raise EngineError(f"{_call}: status {st} {self._L.jx_hpke_last_error(self._h).decode()}")
        out: list[tuple[bytes, bytes] | None] = []
        for i in range(n):
            a = int(po[i]) + 16 * i
            out.append((encs[32 * i:32 * i + 32].tobytes(), cts[a:a + len(plaintexts[i]) + 16].tobytes()) if ok[i] else None)
        return out

    def seal_batch_device(self, n: int, d_ephemeral_sks: int, d_pts: int, d_pt_offsets: int, d_aads: int,
                          d_aad_offsets: int, d_out_encs: int, d_out_cts: int, d_out_ok: int, long: bool = False):
        """jx_hpke_seal_batch_device / jx_hpke_seal_long_batch_device: everything in HBM, the offsets included;
        asynchronous on the context's stream."""
        call = "jx_hpke_seal_long_batch_device" if long else "jx_hpke_seal_batch_device"
        st = getattr(self._L, call)(self._h, n, d_ephemeral_sks, d_pts, d_pt_offsets, d_aads, d_aad_offsets, d_out_encs,
                                    d_out_cts, d_out_ok)
        if st != 0:
            raise EngineError(f"{call}: status {st} {self._L.jx_hpke_last_error(self._h).decode()}")


class HpkeSealer(_HpkeContext):
    """The client's side: one recipient PUBLIC key of one X25519 HPKE suite + application info on one GPU
    (jx_hpke_create_sender). It seals; any call that opens refuses it."""

    def __init__(self, public_key: bytes, info: bytes, device: int = 0, kem_id: int = KEM_X25519_HKDF_SHA256,
                 kdf_id: int = KDF_HKDF_SHA256, aead_id: int = AEAD_AES_128_GCM):
        self._L = _declare(_lib.load())
        h = ctypes.c_void_p()
        pk = np.frombuffer(public_key, np.uint8).copy() if public_key else np.zeros(1, np.uint8)
        inf = np.frombuffer(info, np.uint8).copy() if info else np.zeros(1, np.uint8)
        st = self._L.jx_hpke_create_sender(kem_id, kdf_id, aead_id, _p(pk), len(public_key), _p(inf), len(info), device,
                                           ctypes.byref(h))
        if st == E_UNSUPPORTED:
            raise UnsupportedSuite(self._L.jx_hpke_last_error(None).decode())
        if st == E_INVALID:
            raise ValueError(f"jx_hpke_create_sender: {self._L.jx_hpke_last_error(None).decode() or 'invalid argument'}")
        if st != 0:
            raise EngineError(f"jx_hpke_create_sender: status {st}")
        self._adopt(h)


class HpkeOpener(_HpkeContext):
    """One recipient key pair of one HPKE suite + application info on one GPU."""

    def __init__(self, private_key: bytes, public_key: bytes, info: bytes, device: int = 0,
                 kem_id: int = KEM_X25519_HKDF_SHA256, kdf_id: int = KDF_HKDF_SHA256, aead_id: int = AEAD_AES_128_GCM):
        if len(private_key) != 32 or len(public_key) not in (32, 65):
            raise ValueError("private keys are 32 bytes; public keys 32 (X25519) or 65 (P-256)")
        self._L = _declare(_lib.load())
        h = ctypes.c_void_p()
        sk = np.frombuffer(private_key, np.uint8).copy()
        pk = np.frombuffer(public_key, np.uint8).copy()
        inf = np.frombuffer(info, np.uint8).copy() if info else np.zeros(1, np.uint8)
        if len(public_key) == 32:  # the X25519 entry: any other KEM id is refused there
            call = "jx_hpke_create_suite"
            st = self._L.jx_hpke_create_suite(kem_id, kdf_id, aead_id, _p(sk), _p(pk), _p(inf), len(info), device,
                                              ctypes.byref(h))
        else:
            call = "jx_hpke_create_key"
            st = self._L.jx_hpke_create_key(kem_id, kdf_id, aead_id, _p(sk), len(sk), _p(pk), len(pk), _p(inf), len(info),
                                            device, ctypes.byref(h))
        if st == E_UNSUPPORTED:
            raise UnsupportedSuite(self._L.jx_hpke_last_error(None).decode())
        if st == E_INVALID:
            raise ValueError(f"{call}: {self._L.jx_hpke_last_error(None).decode() or 'invalid argument'}")
        if st != 0:
            raise EngineError(f"{call}: status {st}")
        self._adopt(h)

    def open_long_batch(self, encs: list[bytes], ciphertexts: list[bytes], aads: list[bytes]) -> list[bytes | None]:
        """open_batch for long payloads such as leader input shares (jx_hpke_open_long_batch): the same results,
        with the AEAD of each report spread over a wave instead of chained in one lane."""
        return self.open_batch(encs, ciphertexts, aads, _call="jx_hpke_open_long_batch")

    def open_batch(self, encs: list[bytes], ciphertexts: list[bytes], aads: list[bytes],
                   _call: str = "jx_hpke_open_batch") -> list[bytes | None]:
        """Open n HPKE ciphertexts; None where opening fails (PrepareError::HpkeDecryptError)."""
        n = len(encs)
        if not (len(ciphertexts) == len(aads) == n):
            raise ValueError("one enc, ciphertext and aad per report")
        if n == 0:
            return []
        # a malformed share fails alone (HpkeDecryptError for that report, aggregator.rs:1772-1831):
        # an encapsulated key of another length than the KEM's or a ciphertext shorter than the tag never reaches the GPU
        idx = [i for i in range(n) if len(encs[i]) == self._enc_len and len(ciphertexts[i]) >= 16]
        out: list[bytes | None] = [None] * n
        if not idx:
            return out
        enc = np.frombuffer(b"".join(encs[i] for i in idx), np.uint8).copy()
        cts = np.frombuffer(b"".join(ciphertexts[i] for i in idx) or b"\0", np.uint8).copy()
        aad = np.frombuffer(b"".join(aads[i] for i in idx) or b"\0", np.uint8).copy()
        co = np.zeros(len(idx) + 1, np.uint64)
        ao = np.zeros(len(idx) + 1, np.uint64)
        co[1:] = np.cumsum([len(ciphertexts[i]) for i in idx])
        ao[1:] = np.cumsum([len(aads[i]) for i in idx])
        pts = np.zeros(max(1, int(co[-1]) - 16 * len(idx)), np.uint8)
        ok = np.zeros(len(idx), np.uint8)
        st = getattr(self._L, _call)(self._h, len(idx), _p(enc), _p(cts), _p(co), _p(aad), _p(ao), _p(pts), _p(ok))
        if st != 0:
            raise EngineError(f"{_call}: status {st} {self._L.jx_hpke_last_error(self._h).decode()}")
        for j, i in enumerate(idx):
            if ok[j]:
                a = int(co[j]) - 16 * j
                out[i] = pts[a:a + len(ciphertexts[i]) - 16].tobytes()
        return out
