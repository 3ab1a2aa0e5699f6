"""Batch Ed25519 key derivation and signing on the GPU (hsv_signer_*, include/hsv.h).

The GPU form of the reference's ``generate_keypair`` and ``Signature::new``
(crypto/src/lib.rs:167-175, 185-191) for load generators and input synthesis:
``Signer(seeds)`` expands the seeds once into key records in HBM, and
``sign`` / ``sign_device`` produce RFC 8032 signatures bit-exact with
``verifier.sign_many``; ``sign_transactions`` / ``sign_transactions_device``
fill in ``pk || R || s`` at the end of mempool transactions, the signing mirror
of ``mempool.verify_transactions*``; ``sign_msgs`` / ``sign_msgs_device`` sign
whole messages of differing lengths, the mirror of ``verifier.verify_msgs*``.
Not constant time (table lookups are indexed by
secret digits): never use it to hold a validator's key.  There is no CPU
fallback; without a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data) if a.size else None


class Signer:
    def __init__(self, seeds):
        if isinstance(seeds, (bytes, bytearray)):
            seeds = np.frombuffer(bytes(seeds), np.uint8)
        arr = np.ascontiguousarray(seeds, np.uint8).reshape(-1, 32)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.hsv_signer_create(_ptr(arr), arr.shape[0], ctypes.byref(self._h)), "hsv_signer_create")
        self._n = arr.shape[0]

    def __len__(self) -> int:
        return self._n

    def public_keys(self) -> np.ndarray:
        """(nkeys, 32) uint8, in seed order."""
        out = np.zeros((self._n, 32), np.uint8)
        _lib.check(self._lib.hsv_signer_public_keys(self._h, _ptr(out)), "hsv_signer_public_keys")
        return out

    def sign(self, msgs, key_idx=None) -> np.ndarray:
        """msgs: (m, L) uint8, one message per item, or (L,) one shared message
        (then m = len(key_idx), or every key when key_idx is None).  key_idx:
        (m,) key per item; None: item i uses key i.  An index >= nkeys gives 64
        zero bytes.  Returns (m, 64) uint8, R || s."""
        msgs = np.ascontiguousarray(msgs, np.uint8)
        idx = None if key_idx is None else np.ascontiguousarray(key_idx, np.uint32).reshape(-1)
        if msgs.ndim == 1:
            m, length, stride = (self._n if idx is None else idx.size), msgs.size, 0
        else:
            m, length = msgs.shape
            stride = length
            if idx is not None and idx.size != m:
                raise ValueError("key_idx and msgs differ in length")
        out = np.zeros((m, 64), np.uint8)
        if m:
            _lib.check(self._lib.hsv_signer_sign(self._h, None if idx is None else _ptr(idx), _ptr(msgs), length,
                                                 stride, m, _ptr(out)), "hsv_signer_sign")
        return out

    def sign_device(self, msg, sig, key_idx=None, msg_len=None, stream=None, fault=None) -> None:
        """Device tensors, enqueued on ``stream`` (default: torch's current
        stream), no synchronisation.  msg: (m, L) uint8 rows (any row stride) or
        (L,) one shared message; sig: (m, >= 64) uint8 rows whose address and
        stride are multiples of 16 -- a (m, 64) slice of packed pk||R||s
        records works; key_idx: (m,) int32 / uint32 or None; msg_len: bytes of
        each row that are signed (default: the row length L); fault: optional
        per-call fault words (verifier.verify_device)."""
        from .verifier import _fault_ptr
        import torch
        m = sig.shape[0]
        for t in (msg, key_idx, fault):
            if t is not None and t.device != sig.device:
                raise ValueError(f"all tensors must live on {sig.device}, got {t.device}")
        if msg.dim() == 1:
            length, stride = msg.shape[0], 0
        else:
            length, stride = msg.shape[1], msg.stride(0)
        if msg_len is not None:
            length = msg_len
        with torch.cuda.device(sig.device):
            if stream is None:
                stream = torch.cuda.current_stream(sig.device).cuda_stream
            rc = self._lib.hsv_signer_sign_device(
                self._h, ctypes.c_void_p(key_idx.data_ptr()) if key_idx is not None else None,
                ctypes.c_void_p(msg.data_ptr()), length, stride, m, ctypes.c_void_p(sig.data_ptr()), sig.stride(0),
                _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_signer_sign_device")

    def sign_msgs(self, msgs, key_idx=None) -> np.ndarray:
        """Whole messages of any lengths (hsv_signer_sign_msgs), the signing
        mirror of ``verifier.verify_msgs``.  msgs: a sequence of m ``bytes``
        (some may be empty).  key_idx: (m,) key per item; None: item i uses key
        i (m <= nkeys); an index >= nkeys gives 64 zero bytes.  Returns (m, 64)
        uint8, R || s."""
        from .verifier import pack_msgs
        buf, offsets = pack_msgs(msgs)
        m = offsets.size - 1
        idx = None if key_idx is None else np.ascontiguousarray(key_idx, np.uint32).reshape(-1)
        if idx is not None and idx.size != m:
            raise ValueError("key_idx and msgs differ in length")
        out = np.zeros((m, 64), np.uint8)
        if m:
            _lib.check(self._lib.hsv_signer_sign_msgs(self._h, None if idx is None else _ptr(idx), _ptr(buf),
                                                      _ptr(offsets), 0, 0, m, _ptr(out)), "hsv_signer_sign_msgs")
        return out

    def sign_msgs_device(self, msgs, sig, offsets=None, msg_len: int = 0, msg_stride=None, key_idx=None,
                         stream=None, fault=None) -> None:
        """Device tensors, enqueued on ``stream`` (default: torch's current
        stream), no synchronisation (hsv_signer_sign_msgs_device).  msgs: the
        message bytes at any alignment (None when every message is empty);
        offsets: an int64 tensor of m + 1 byte offsets into it, or None for
        ``msg_len`` bytes per item at ``msg_stride`` (default msg_len; 0 = one
        shared message) -- the conventions of ``verifier.verify_msgs_device``.
        sig: (m, >= 64) uint8 rows whose address and stride are multiples of
        16; key_idx: (m,) int32 / uint32 or None; fault: optional per-call
        fault words (``sign_device``).  An item whose offsets decrease, or whose
        key index is out of range, gets 64 zero bytes."""
        from .verifier import _fault_ptr
        import torch
        m = sig.shape[0]
        for t in (msgs, offsets, key_idx, fault):
            if t is not None and t.device != sig.device:
                raise ValueError(f"all tensors must live on {sig.device}, got {t.device}")
        if offsets is not None and offsets.numel() != m + 1:
            raise ValueError("one message per item (m + 1 offsets)")
        if key_idx is not None and key_idx.numel() != m:
            raise ValueError("key_idx and sig differ in length")
        if msg_stride is None:
            msg_stride = msg_len
        with torch.cuda.device(sig.device):
            if stream is None:
                stream = torch.cuda.current_stream(sig.device).cuda_stream
            rc = self._lib.hsv_signer_sign_msgs_device(
                self._h, ctypes.c_void_p(key_idx.data_ptr()) if key_idx is not None else None,
                ctypes.c_void_p(msgs.data_ptr()) if msgs is not None else None,
                ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None, msg_len, msg_stride, m,
                ctypes.c_void_p(sig.data_ptr()), sig.stride(0), _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_signer_sign_msgs_device")

    def sign_transactions(self, txs, key_idx=None, offsets=None) -> np.ndarray:
        """Mempool transactions ``message || pk || R || s`` (hsv_signer_sign_transactions):
        a signed copy of ``txs``, whose last 96 bytes per transaction become pk
        and the signature over SHA-512(message)[..32] -- what
        ``mempool.verify_transactions`` accepts.  txs: (n, tx_size) uint8 of
        equal transactions, or a flat buffer with ``offsets`` (n + 1 byte
        offsets).  key_idx: (n,) key per item; None: item i uses key i; an
        index >= nkeys gives 96 zero bytes.  A transaction shorter than 96
        bytes raises."""
        out = np.array(txs, dtype=np.uint8, order="C", copy=True)
        idx = None if key_idx is None else np.ascontiguousarray(key_idx, np.uint32).reshape(-1)
        if offsets is None:
            if out.ndim != 2:
                raise ValueError("expected an (n, tx_size) array, or a flat buffer and offsets")
            n, size, offs = out.shape[0], out.shape[1], None
        else:
            offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
            out = out.reshape(-1)
            n, size = offs.size - 1, 0
            if n < 0 or (n and int(offs.max()) > out.size):
                raise ValueError("offsets do not fit the buffer")
        if idx is not None and idx.size != n:
            raise ValueError("key_idx and txs differ in length")
        if n > 0:
            _lib.check(self._lib.hsv_signer_sign_transactions(
                self._h, None if idx is None else _ptr(idx), ctypes.c_void_p(out.ctypes.data),
                None if offs is None else _ptr(offs), size, n), "hsv_signer_sign_transactions")
        return out

    def sign_transactions_device(self, txs, offsets=None, tx_size=None, key_idx=None, stream=None, fault=None) -> None:
        """In place on the device, enqueued on ``stream`` (default: torch's
        current stream), no synchronisation.  txs: uint8 tensor at any byte
        address; offsets: (n + 1,) int64 byte offsets relative to txs, or None
        with ``tx_size`` (default: the row length of a 2-D txs) for equal
        transactions; key_idx: (n,) int32 / uint32 or None; fault: optional
        per-call fault words (verifier.verify_device).  A transaction shorter
        than 96 bytes, or a decreasing pair of offsets, is left untouched."""
        from .verifier import _fault_ptr
        import torch
        for t in (offsets, key_idx, fault):
            if t is not None and t.device != txs.device:
                raise ValueError(f"all tensors must live on {txs.device}, got {t.device}")
        if offsets is not None:
            n, size = offsets.numel() - 1, 0
        else:
            if tx_size is None:
                if txs.dim() != 2 or not txs.is_contiguous():
                    raise ValueError("tx_size is needed unless txs is a contiguous (n, tx_size) tensor")
                tx_size = txs.shape[1]
            size = int(tx_size)
            n = txs.numel() // size if size else 0
        if key_idx is not None and key_idx.numel() != n:
            raise ValueError("key_idx and txs differ in length")
        with torch.cuda.device(txs.device):
            if stream is None:
                stream = torch.cuda.current_stream(txs.device).cuda_stream
            rc = self._lib.hsv_signer_sign_transactions_device(
                self._h, ctypes.c_void_p(key_idx.data_ptr()) if key_idx is not None else None,
                ctypes.c_void_p(txs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None,
                size, n, _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_signer_sign_transactions_device")

    def close(self) -> None:
        if self._h:
            self._lib.hsv_signer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
