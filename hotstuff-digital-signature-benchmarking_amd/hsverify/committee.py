"""Committee key cache over the C ABI.

A HotStuff committee's keys are fixed per epoch (reference
consensus/src/config.rs: Committee, looked up by stake(name) in
QC::verify / TC::verify, consensus/src/messages.rs:186,296).  ``Committee``
builds a 384 KiB fixed-base comb table of -A per key in HBM once; votes by
members are then verified with 64 mixed additions and no doublings.  Results
are bit-identical to the generic path (same flag byte per vote).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


class Committee:
    """``compact=True`` builds 48 KiB tables of 4-bit digits instead of the
    384 KiB ones (hsv_committee_create_ex): an eighth of the memory for 80
    instead of 64 additions per signature, and no latency form for small
    batches.  Every method answers the same bytes either way."""

    def __init__(self, public_keys, compact: bool = False):
        keys = [k.data if hasattr(k, "data") and isinstance(k.data, bytes) else bytes(k) for k in public_keys] \
            if not isinstance(public_keys, np.ndarray) else None
        arr = np.ascontiguousarray(public_keys, np.uint8).reshape(-1, 32) if keys is None else \
            np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy()
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.hsv_committee_create_ex(_ptr(arr) if arr.size else None, arr.shape[0], 4 if compact else 8,
                                                     ctypes.byref(self._h)), "hsv_committee_create_ex")
        self._n = arr.shape[0]
        self._keys = arr.copy()  # by member index (learn(skip=...) re-creates a committee from them)

    @classmethod
    def learn(cls, txs, min_count: int = 2, max_keys: int = 8192, compact: bool = False, skip=None, slots=None):
        """A committee of the frequent signers of ``txs`` (mempool.census: a
        sequence of ``bytes`` or an (n, tx_size) array; nothing is verified):
        the keys that occur at least ``min_count`` times, at most ``max_keys``
        of them in census order (most frequent first).  With ``skip`` (a
        Committee) its members are left out of the census and the result holds
        ``skip``'s keys followed by the new ones.  A committee is immutable --
        its tables are built once, at creation -- so growing one means
        creating another; ``skip`` stays valid and is the caller's to close."""
        from .mempool import census
        keys, counts, _ = census(txs, skip=skip, slots=slots)
        new = keys[counts >= min_count][:max_keys]
        if skip is not None:
            new = np.concatenate([skip._keys, new]) if new.size else skip._keys
        return cls(np.ascontiguousarray(new, np.uint8).reshape(-1, 32), compact=compact)

    @property
    def digit_bits(self) -> int:
        """8 (full tables) or 4 (compact); 0 once closed."""
        return int(self._lib.hsv_committee_digit_bits(self._h))

    @property
    def table_bytes(self) -> int:
        """Table memory held on the device: 393216 or 49152 bytes per key."""
        return int(self._lib.hsv_committee_table_bytes(self._h))

    def __len__(self) -> int:
        return self._n

    def index(self, pk) -> int:
        b = pk.data if hasattr(pk, "data") and isinstance(pk.data, bytes) else bytes(pk)
        return int(self._lib.hsv_committee_index(self._h, ctypes.c_char_p(b)))

    def verify_flags(self, key_idx, sig, msg) -> np.ndarray:
        """key_idx (m,) member indices, sig (m,64), msg (m,32) or (32,) -> flags (m,)."""
        idx = np.ascontiguousarray(key_idx, np.uint32).reshape(-1)
        sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
        msg = np.ascontiguousarray(msg, np.uint8)
        m = idx.size
        stride = 0 if (msg.ndim == 1 and msg.size == 32) else 32
        out = np.zeros(m, np.uint8)
        if m:
            _lib.check(self._lib.hsv_committee_verify(self._h, _ptr(idx), _ptr(sig), _ptr(msg), stride, m, _ptr(out)),
                       "hsv_committee_verify")
        return out

    def verify_batch(self, digest, votes):
        """crypto::Signature::verify_batch for votes by (mostly) members -> crypto.Result."""
        from .crypto import OK, CryptoError, Result
        votes = list(votes)
        packed = b"".join(pk.data + sig.flatten() for pk, sig in votes)
        d = digest.data if hasattr(digest, "data") else bytes(digest)
        rc = _lib.check(self._lib.hsv_committee_verify_batch_packed(
            self._h, ctypes.c_char_p(d), ctypes.c_char_p(packed) if packed else None, len(votes)),
            "hsv_committee_verify_batch_packed")
        return OK if rc == 1 else Result(CryptoError("signature error"))

    def verify_device(self, key_idx, sig, msg, flags, stream=None, fault=None) -> None:
        """Device tensors: key_idx (m,) int32, sig (m,64) u8, msg (m,32) or (32,), flags (m,) u8;
        fault: optional per-call fault words (verifier.verify_device)."""
        from .verifier import _fault_ptr
        import torch
        m = key_idx.shape[0]
        if stream is None:
            stream = torch.cuda.current_stream(sig.device).cuda_stream
        rc = self._lib.hsv_committee_verify_device(
            self._h, ctypes.c_void_p(key_idx.data_ptr()), ctypes.c_void_p(sig.data_ptr()), sig.stride(0),
            ctypes.c_void_p(msg.data_ptr()), 0 if msg.dim() == 1 else msg.stride(0), m,
            ctypes.c_void_p(flags.data_ptr()), _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_committee_verify_device")

    def verify_transactions(self, txs) -> np.ndarray:
        """Ragged list of mempool transactions (``message || pk || sig``, mempool.py)
        -> flag bytes, bit for bit those of mempool.verify_transactions: a
        transaction signed by a member takes the member's comb table, any other
        the generic kernels.  Raises HsvLibraryError for a transaction shorter
        than 96 bytes."""
        from .mempool import pack
        txs = list(txs)
        out = np.zeros(len(txs), np.uint8)
        if txs:
            buf, offsets = pack(txs)
            _lib.check(self._lib.hsv_committee_verify_transactions(self._h, _ptr(buf), _ptr(offsets), 0, len(txs),
                                                                   _ptr(out)), "hsv_committee_verify_transactions")
        return out

    def verify_transactions_fixed(self, txs) -> np.ndarray:
        """(n, tx_size) u8 array of equal-size transactions -> (n,) flag bytes."""
        txs = np.ascontiguousarray(txs, dtype=np.uint8)
        if txs.ndim != 2:
            raise ValueError("expected an (n, tx_size) array")
        n, size = txs.shape
        out = np.zeros(n, np.uint8)
        if n:
            _lib.check(self._lib.hsv_committee_verify_transactions(self._h, _ptr(txs), None, size, n, _ptr(out)),
                       "hsv_committee_verify_transactions")
        return out

    def verify_transactions_device(self, txs, offsets=None, tx_size: int = 0, n=None, flags=None, strict_bits=None,
                                   stream=None, fault=None) -> None:
        """Device tensors, as mempool.verify_transactions_device: txs uint8,
        offsets int64 (n + 1) or None with tx_size; flags (n,) uint8 and / or
        strict_bits (ceil(n / 32),) int32.  No synchronisation."""
        from .verifier import _fault_ptr
        import torch
        if n is None:
            n = offsets.numel() - 1 if offsets is not None else txs.numel() // tx_size
        if stream is None:
            stream = torch.cuda.current_stream(txs.device).cuda_stream
        rc = self._lib.hsv_committee_verify_transactions_device(
            self._h, ctypes.c_void_p(txs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None,
            tx_size, n, ctypes.c_void_p(flags.data_ptr()) if flags is not None else None,
            ctypes.c_void_p(strict_bits.data_ptr()) if strict_bits is not None else None, _fault_ptr(fault),
            ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_committee_verify_transactions_device")

    def verify_msgs(self, pk, sig, msgs) -> np.ndarray:
        """Whole messages of any length, as verifier.verify_msgs (pk (n,32),
        sig (n,64), ``msgs`` a sequence of n ``bytes`` or a ``(buffer,
        offsets)`` pair) -> flag bytes, bit for bit that call's: an item signed
        by a member takes the member's comb table, any other the generic
        kernels.  Decreasing offsets raise HsvLibraryError."""
        from .verifier import pack_msgs
        pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
        sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
        n = pk.shape[0]
        if sig.shape[0] != n:
            raise ValueError("pk/sig length mismatch")
        if isinstance(msgs, tuple) and len(msgs) == 2 and not isinstance(msgs[0], (bytes, bytearray, memoryview)):
            buf = np.ascontiguousarray(msgs[0], dtype=np.uint8).reshape(-1)
            offsets = np.ascontiguousarray(msgs[1], dtype=np.uint64).reshape(-1)
        else:
            buf, offsets = pack_msgs(msgs)
        if offsets.size != n + 1:
            raise ValueError("one message per item (n + 1 offsets)")
        if n and buf.size < int(offsets.max()):
            raise ValueError("offsets run past the buffer")
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _lib.check(self._lib.hsv_committee_verify_msgs(self._h, _ptr(pk), _ptr(sig), _ptr(buf) if buf.size else None,
                                                           _ptr(offsets), 0, 0, n, _ptr(out)),
                       "hsv_committee_verify_msgs")
        return out

    def verify_msgs_device(self, pk, sig, msgs, offsets=None, msg_len: int = 0, msg_stride: int | None = None,
                           flags=None, strict_bits=None, stream=None, fault=None) -> None:
        """Device tensors, as verifier.verify_msgs_device: pk (n,32) and sig
        (n,64) rows at strides that are multiples of 16, ``msgs`` at any
        alignment, ``offsets`` int64 (n + 1) or None for ``msg_len`` bytes per
        item at ``msg_stride`` (default msg_len; 0 = one shared message);
        ``flags`` (n,) uint8 and / or ``strict_bits`` (ceil(n / 32),) int32.
        No synchronisation."""
        from .verifier import _fault_ptr
        import torch
        n = pk.shape[0]
        for t in (sig, msgs, offsets, flags, strict_bits, fault):
            if t is not None and t.device != pk.device:
                raise ValueError(f"all tensors must live on {pk.device}, got {t.device}")
        if msg_stride is None:
            msg_stride = msg_len
        if stream is None:
            stream = torch.cuda.current_stream(pk.device).cuda_stream
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self._lib.hsv_committee_verify_msgs_device(
            self._h, p(pk), pk.stride(0), p(sig), sig.stride(0), p(msgs), p(offsets), msg_len, msg_stride, n,
            p(flags), p(strict_bits), _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_committee_verify_msgs_device")

    def verify_msgs_indexed(self, key_idx, sig, msgs) -> np.ndarray:
        """Whole messages by member index: key_idx (m,) member indices
        (``index`` per vote), sig (m,64), ``msgs`` a sequence of m ``bytes`` or
        a ``(buffer, offsets)`` pair -> flag bytes, bit for bit those of
        verifier.verify_msgs for (member's key, sig, message); an index >=
        len(self) gives flags 0.  Decreasing offsets raise HsvLibraryError."""
        from .verifier import pack_msgs
        idx = np.ascontiguousarray(key_idx, np.uint32).reshape(-1)
        sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
        m = idx.size
        if sig.shape[0] != m:
            raise ValueError("key_idx/sig length mismatch")
        if isinstance(msgs, tuple) and len(msgs) == 2 and not isinstance(msgs[0], (bytes, bytearray, memoryview)):
            buf = np.ascontiguousarray(msgs[0], dtype=np.uint8).reshape(-1)
            offsets = np.ascontiguousarray(msgs[1], dtype=np.uint64).reshape(-1)
        else:
            buf, offsets = pack_msgs(msgs)
        if offsets.size != m + 1:
            raise ValueError("one message per item (m + 1 offsets)")
        if m and buf.size < int(offsets.max()):
            raise ValueError("offsets run past the buffer")
        out = np.zeros(m, dtype=np.uint8)
        if m:
            _lib.check(self._lib.hsv_committee_verify_msgs_indexed(
                self._h, _ptr(idx), _ptr(sig), _ptr(buf) if buf.size else None, _ptr(offsets), 0, 0, m, _ptr(out)),
                "hsv_committee_verify_msgs_indexed")
        return out

    def verify_msgs_indexed_device(self, key_idx, sig, msgs, offsets=None, msg_len: int = 0,
                                   msg_stride: int | None = None, flags=None, stream=None, fault=None) -> None:
        """Device tensors, shaped as verify_msgs_device with key_idx (m,) int32
        in the place of pk: sig (m,64) rows at a stride that is a multiple of
        16, ``msgs`` at any alignment, ``offsets`` int64 (m + 1) or None for
        ``msg_len`` bytes per item at ``msg_stride`` (default msg_len; 0 = one
        shared message); ``flags`` (m,) uint8, required (there are no strict
        bits).  One launch at m <= 4096 on full tables.  No synchronisation."""
        from .verifier import _fault_ptr
        import torch
        m = key_idx.shape[0]
        for t in (sig, msgs, offsets, flags, fault):
            if t is not None and t.device != key_idx.device:
                raise ValueError(f"all tensors must live on {key_idx.device}, got {t.device}")
        if msg_stride is None:
            msg_stride = msg_len
        if stream is None:
            stream = torch.cuda.current_stream(key_idx.device).cuda_stream
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self._lib.hsv_committee_verify_msgs_indexed_device(
            self._h, p(key_idx), p(sig), sig.stride(0), p(msgs), p(offsets), msg_len, msg_stride, m, p(flags),
            _fault_ptr(fault), ctypes.c_void_p(stream))
        _lib.check(rc, "hsv_committee_verify_msgs_indexed_device")

    def close(self) -> None:
        if self._h:
            self._lib.hsv_committee_destroy(self._h)
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
