"""Mempool transaction-signature verification.

The reference's client transactions are ``message || pk (32 B) || sig (64 B)``
and the check it carries (commented out in the shipped code) is, per
transaction (``mempool/src/batch_maker.rs:79-85``)::

    message   = tx[..len-96]
    digest    = Digest(SHA-512(message)[..32])
    signature = Signature::from_bytes(sig[..32], sig[32..64])
    signature.verify(&digest, &PublicKey(pk)).is_ok()

``BatchMaker::run`` keeps only transactions that pass; ``Core::make_vote``
(``consensus/src/core.rs:121-131``) refuses to vote for a block whose batch
holds any transaction that fails.  Those two call shapes are
:func:`filter_transactions` and :func:`verify_batch_transactions` below, over
the GPU path (``hsv_verify_transactions*`` in ``include/hsv.h``): digests are
computed on the device by ``hsv_tx_record_kernel``, then verified by the
generic verification kernels.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Sequence

import numpy as np

from . import _lib

TX_OVERHEAD = 96  # pk (32) || signature (64) at the end of every transaction


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def make_transaction(message: bytes, pk: bytes, sig: bytes) -> bytes:
    """Client-side layout: message || pk || part1 (R) || part2 (s)."""
    if len(pk) != 32 or len(sig) != 64:
        raise ValueError("pk must be 32 bytes and sig 64 bytes")
    return bytes(message) + bytes(pk) + bytes(sig)


def pack(txs: Sequence[bytes]):
    """Ragged list of transactions -> (concatenated u8 buffer, n+1 u64 offsets)."""
    lens = np.fromiter((len(t) for t in txs), dtype=np.uint64, count=len(txs))
    offsets = np.zeros(len(txs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = np.frombuffer(b"".join(txs), dtype=np.uint8) if txs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf), offsets


def verify_transactions(txs: Sequence[bytes]) -> np.ndarray:
    """Per-transaction flag bytes (``HSV_*`` bits; STRICT_OK = the reference's
    ``verify(..).is_ok()``).  Raises HsvLibraryError for a transaction shorter
    than 96 bytes, where the reference's slice would panic."""
    n = len(txs)
    out = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return out
    buf, offsets = pack(txs)
    lib = _lib.load()
    _lib.check(lib.hsv_verify_transactions(_ptr(buf), _ptr(offsets), n, _ptr(out)), "hsv_verify_transactions")
    return out


def verify_transactions_fixed(txs: np.ndarray) -> np.ndarray:
    """(n, tx_size) u8 array of equal-size transactions -> (n,) flag bytes."""
    txs = np.ascontiguousarray(txs, dtype=np.uint8)
    if txs.ndim != 2:
        raise ValueError("expected an (n, tx_size) array")
    n, size = txs.shape
    out = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return out
    lib = _lib.load()
    _lib.check(lib.hsv_verify_transactions_fixed(_ptr(txs), size, n, _ptr(out)), "hsv_verify_transactions_fixed")
    return out


def verify_transactions_device(txs, offsets=None, tx_size: int = 0, n: int | None = None, flags=None,
                               strict_bits=None, stream=None, fault=None) -> None:
    """Enqueue verification of device-resident transactions (torch uint8 tensor
    ``txs``; ``offsets`` an int64 tensor of n+1 byte offsets, or None with
    ``tx_size`` for fixed-size transactions).  Outputs: ``flags`` (n,) uint8
    and/or ``strict_bits`` (ceil(n/32),) int32; ``fault`` optional per-call
    fault words (verifier.verify_device).  No synchronisation."""
    from .verifier import _fault_ptr
    import torch

    if n is None:
        n = offsets.numel() - 1 if offsets is not None else txs.numel() // tx_size
    if stream is None:
        stream = torch.cuda.current_stream(txs.device).cuda_stream
    lib = _lib.load()
    rc = lib.hsv_verify_transactions_device(
        ctypes.c_void_p(txs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None,
        tx_size, n, ctypes.c_void_p(flags.data_ptr()) if flags is not None else None,
        ctypes.c_void_p(strict_bits.data_ptr()) if strict_bits is not None else None, _fault_ptr(fault),
        ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_verify_transactions_device")


def filter_transactions(txs: Sequence[bytes], committee=None) -> List[bytes]:
    """``BatchMaker::run`` with the check enabled (batch_maker.rs:79-97): the
    transactions whose signature verifies, in order.  ``committee`` (a
    committee.Committee of the known clients' keys): its members' transactions
    are verified from their comb tables, with the same result."""
    flags = committee.verify_transactions(txs) if committee is not None else verify_transactions(txs)
    return [t for t, f in zip(txs, flags) if f & _lib.STRICT_OK]


def verify_batch_transactions(txs: Iterable[bytes], committee=None) -> bool:
    """``Core::make_vote`` batch re-check (core.rs:121-131): True iff every
    transaction of the batch verifies (an empty batch passes).  ``committee``
    as in :func:`filter_transactions`."""
    txs = list(txs)
    if not txs:
        return True
    flags = committee.verify_transactions(txs) if committee is not None else verify_transactions(txs)
    return bool((flags & _lib.STRICT_OK).all())


def verify_serialized_batch(buf: bytes, committee=None) -> bool:
    """``Core::make_vote``'s check from the stored bytes (core.rs:113-142): the
    bincode of ``MempoolMessage::Batch`` as read from the store, verified where
    it lies (``hsv_batch_verify_bincode``; nothing is deserialized or
    re-packed).  True iff it is a well-formed Batch and every transaction
    verifies; False for a failing transaction (one shorter than 96 bytes
    included) and for malformed bytes or a ``BatchRequest``, which make_vote
    rejects alike.  ``committee`` as in :func:`filter_transactions`."""
    from . import wire
    try:
        ok, _ = wire.batch_verify(buf, committee)
    except _lib.HsvLibraryError as e:
        if "HSV_ERR_PARSE" in str(e):
            return False
        raise
    return ok


# ---- signer census (hsv_census_*) -------------------------------------------------
# Who signs a batch, and how often: the distinct 32-byte signer keys counted on
# the GPU, for a node that wants to build the committee of its known clients
# (committee.Committee.learn) from the transactions it actually sees.

class CensusSummary(ctypes.Structure):
    """hsv_census_summary (include/hsv.h): items == counted + members +
    malformed + overflow, always."""
    _fields_ = [("items", ctypes.c_uint64), ("counted", ctypes.c_uint64), ("members", ctypes.c_uint64),
                ("malformed", ctypes.c_uint64), ("overflow", ctypes.c_uint64), ("distinct", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


def default_census_slots(n: int) -> int:
    """The next power of two >= 4 x min(n, 2^20), at least 16: load <= 1/4 if
    every item had a key of its own, up to the table's largest size."""
    slots = 16
    while slots < 4 * min(int(n), 1 << 20):
        slots <<= 1
    return slots


def _check_slots(slots: int) -> int:
    slots = int(slots)
    if slots < 16 or slots > (1 << 22) or slots & (slots - 1):
        raise ValueError("slots must be a power of two in [16, 2^22]")
    return slots


def census(txs, skip=None, slots: int | None = None):
    """The distinct signer keys of ``txs`` and how often each occurs
    (``hsv_census_transactions``; nothing is verified).  ``txs``: a sequence of
    ``bytes`` (ragged) or an ``(n, tx_size)`` uint8 array.  ``skip`` (a
    committee.Committee): its members are counted in ``members`` and not
    returned.  ``slots``: the census table's size, a power of two in
    [16, 2^22]; default :func:`default_census_slots`.  Returns ``(keys (k, 32)
    uint8, counts (k,) uint32, summary dict)``, sorted by count descending, then
    key bytes ascending.  A transaction shorter than 96 bytes is counted in
    ``malformed``."""
    if isinstance(txs, np.ndarray):
        arr = np.ascontiguousarray(txs, dtype=np.uint8)
        if arr.ndim != 2:
            raise ValueError("expected an (n, tx_size) array")
        n, size = arr.shape
        buf, offsets = arr, None
    else:
        txs = list(txs)
        n, size = len(txs), 0
        buf, offsets = pack(txs)
    slots = default_census_slots(n) if slots is None else _check_slots(slots)
    keys = np.zeros((slots, 32), np.uint8)
    counts = np.zeros(slots, np.uint32)
    summary = CensusSummary()
    lib = _lib.load()
    _lib.check(lib.hsv_census_transactions(skip._h if skip is not None else None, _ptr(buf) if buf.size else None,
                                           _ptr(offsets) if offsets is not None else None, size, n, slots, _ptr(keys),
                                           _ptr(counts), slots, ctypes.byref(summary)), "hsv_census_transactions")
    k = int(summary.distinct)
    return keys[:k].copy(), counts[:k].copy(), summary.as_dict()


def census_device(txs, offsets=None, tx_size: int = 0, n: int | None = None, skip=None, slots: int | None = None,
                  keys_out=None, counts_out=None, summary_out=None, stream=None):
    """Enqueue a census of device-resident transactions (torch uint8 tensor
    ``txs``; ``offsets`` an int64 tensor of n + 1 byte offsets, or None with
    ``tx_size``), as :func:`verify_transactions_device` addresses them.
    Outputs (allocated on ``txs``'s device when not given): ``keys_out``
    (slots, 32) uint8, ``counts_out`` (slots,) int32, ``summary_out`` (6,)
    int64 -- items, counted, members, malformed, overflow, distinct.  The first
    ``distinct`` entries are the census, in no particular order; the rest are
    0.  No synchronisation.  Returns ``(keys_out, counts_out, summary_out)``."""
    import torch

    if n is None:
        n = offsets.numel() - 1 if offsets is not None else txs.numel() // tx_size
    slots = default_census_slots(n) if slots is None else _check_slots(slots)
    dev = txs.device
    if keys_out is None:
        keys_out = torch.empty((slots, 32), dtype=torch.uint8, device=dev)
    if counts_out is None:
        counts_out = torch.empty(slots, dtype=torch.int32, device=dev)
    if summary_out is None:
        summary_out = torch.empty(6, dtype=torch.int64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()
    rc = lib.hsv_census_transactions_device(
        skip._h if skip is not None else None, ctypes.c_void_p(txs.data_ptr()),
        ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None, tx_size, n, slots,
        ctypes.c_void_p(keys_out.data_ptr()), ctypes.c_void_p(counts_out.data_ptr()),
        ctypes.c_void_p(summary_out.data_ptr()), ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_census_transactions_device")
    return keys_out, counts_out, summary_out


# ---- sealing verified transactions into batches (hsv_seal_*) ------------------------
# BatchMaker::run / seal on the device: the transactions whose signature verifies,
# cut by the greedy rule at batch_size and serialized as MempoolMessage::Batch.

SEAL_OK, SEAL_OVERFLOW = 0, 1


class SealSummary(ctypes.Structure):
    """hsv_seal_summary (include/hsv.h): items == sealed + rejected + malformed +
    held, always."""
    _fields_ = [("items", ctypes.c_uint64), ("sealed", ctypes.c_uint64), ("rejected", ctypes.c_uint64),
                ("malformed", ctypes.c_uint64), ("held", ctypes.c_uint64), ("held_first", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("n_batches", ctypes.c_uint32), ("status", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}

    @classmethod
    def from_words(cls, words) -> "SealSummary":
        """From the (8,) int64 tensor or array :func:`seal_device` fills."""
        return cls.from_buffer_copy(np.ascontiguousarray(np.asarray(words), dtype=np.int64).tobytes())


def seal_bound(total_tx_bytes: int, n: int, batch_size: int):
    """``(bytes, batches)``: an ``out_cap`` and a ``batches_cap`` that are never
    below what sealing ``n`` transactions of ``total_tx_bytes`` bytes needs
    (``hsv_seal_bound``; no GPU)."""
    b, k = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.load().hsv_seal_bound(int(total_tx_bytes), int(n), int(batch_size), ctypes.byref(b),
                                          ctypes.byref(k)), "hsv_seal_bound")
    return int(b.value), int(k.value)


def seal(txs, batch_size: int, committee=None, flush: bool = True, digests: bool = False):
    """``BatchMaker::run`` with the check enabled, and ``seal``
    (batch_maker.rs:78-131): verify ``txs`` (a sequence of ``bytes`` or an
    ``(n, tx_size)`` uint8 array), keep those that pass, cut them greedily at
    ``batch_size`` and serialize each batch (``hsv_seal_transactions``).
    ``flush``: close a last partial batch; otherwise its transactions are held
    and ``summary["held_first"]`` is the index to resubmit from.  ``committee``
    as in :func:`filter_transactions`.  Returns ``(batches, flags, summary)``,
    batches a list of ``bytes``, and with ``digests`` a fourth element, the
    (n_batches, 32) uint8 array of ``SHA-512(batch)[..32]``."""
    if isinstance(txs, np.ndarray):
        arr = np.ascontiguousarray(txs, dtype=np.uint8)
        if arr.ndim != 2:
            raise ValueError("expected an (n, tx_size) array")
        n, size = arr.shape
        buf, offsets = arr, None
        total = n * size
    else:
        txs = list(txs)
        n, size = len(txs), 0
        buf, offsets = pack(txs)
        total = int(offsets[-1])
    cap, bcap = seal_bound(total, n, batch_size)
    out = np.zeros(max(cap, 1), np.uint8)
    boff = np.zeros(bcap + 1, np.uint64)
    dig = np.zeros((max(bcap, 1), 32), np.uint8) if digests else None
    flags = np.zeros(max(n, 1), np.uint8)
    summary = SealSummary()
    lib = _lib.load()
    _lib.check(lib.hsv_seal_transactions(committee._h if committee is not None else None,
                                         _ptr(buf) if buf.size else None,
                                         _ptr(offsets) if offsets is not None else None, size, n, int(batch_size),
                                         1 if flush else 0, _ptr(out), cap, _ptr(boff), bcap,
                                         _ptr(dig) if digests else None, _ptr(flags), ctypes.byref(summary)),
               "hsv_seal_transactions")
    if summary.status != SEAL_OK:
        raise _lib.HsvLibraryError("hsv_seal_transactions: the bound was too small")
    k = int(summary.n_batches)
    batches = [out[int(boff[b]):int(boff[b + 1])].tobytes() for b in range(k)]
    res = (batches, flags[:n].copy(), summary.as_dict())
    return res + (dig[:k].copy(),) if digests else res


def seal_device(txs, offsets=None, tx_size: int = 0, n: int | None = None, flags=None, batch_size: int = 500_000,
                flush: bool = True, out=None, batch_offsets=None, digests=None, summary_out=None, stream=None):
    """Enqueue the seal of device-resident transactions (torch uint8 tensor
    ``txs``; ``offsets`` an int64 tensor of n + 1 byte offsets, or None with
    ``tx_size``), as :func:`verify_transactions_device` addresses them, with
    the ``flags`` (n,) uint8 any verify call wrote (None: keep everything).
    ``out`` (uint8) and ``batch_offsets`` (int64, batches_cap + 1 entries) are
    allocated by :func:`seal_bound` when not given (fixed size only: a ragged
    batch's byte total is on the device); ``digests``: None, or a
    (batches_cap, 32) uint8 tensor, or True to allocate one; ``summary_out``
    (8,) int64, read with :meth:`SealSummary.from_words`.  No synchronisation.
    Returns ``(out, batch_offsets, digests, summary_out)``."""
    import torch

    if n is None:
        n = offsets.numel() - 1 if offsets is not None else txs.numel() // tx_size
    dev = txs.device
    if out is None or batch_offsets is None:
        if offsets is not None:
            raise ValueError("a ragged batch needs out and batch_offsets (seal_bound of its byte total)")
        cap, bcap = seal_bound(n * tx_size, n, batch_size)
        if out is None:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        if batch_offsets is None:
            batch_offsets = torch.empty(bcap + 1, dtype=torch.int64, device=dev)
    bcap = batch_offsets.numel() - 1
    if digests is True:
        digests = torch.empty((max(bcap, 1), 32), dtype=torch.uint8, device=dev)
    if digests is not None and digests.numel() < 32 * bcap:
        raise ValueError("digests holds fewer than batches_cap entries")
    if summary_out is None:
        summary_out = torch.empty(8, dtype=torch.int64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()
    rc = lib.hsv_seal_transactions_device(
        ctypes.c_void_p(txs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()) if offsets is not None else None,
        tx_size, n, ctypes.c_void_p(flags.data_ptr()) if flags is not None else None, int(batch_size),
        1 if flush else 0, ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(batch_offsets.data_ptr()),
        bcap, ctypes.c_void_p(digests.data_ptr()) if digests is not None else None,
        ctypes.c_void_p(summary_out.data_ptr()), ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_seal_transactions_device")
    return out, batch_offsets, digests, summary_out


# ---- the benchmark's sample transactions (hsv_batch_samples_bincode*) ----------------
# What the `benchmark` block of BatchMaker::seal logs about a batch
# (batch_maker.rs:118-125, 133-153): the ids of its sample transactions (first
# byte 0, longer than 8 bytes; the id is bytes 1..9 big-endian) and its size,
# the sum of the transactions' lengths.  hsverify.benchlog formats the lines.

BATCH_OK, BATCH_TX, BATCH_PARSE, BATCH_OVERFLOW = 0, 1, 2, 3


class BatchSamples(ctypes.Structure):
    """hsv_batch_samples (include/hsv.h), 40 bytes."""
    _fields_ = [("status", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("n_tx", ctypes.c_uint64),
                ("size", ctypes.c_uint64), ("n_samples", ctypes.c_uint64), ("first_sample", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}

    @classmethod
    def from_words(cls, words) -> "BatchSamples":
        """From one (5,) int64 row of the index :func:`batches_samples_device` fills."""
        return cls.from_buffer_copy(np.ascontiguousarray(np.asarray(words), dtype=np.int64).tobytes())


def batch_samples(buf: bytes, count_only: bool = False):
    """The sample index of one serialized ``MempoolMessage::Batch`` on the host
    (``hsv_batch_samples_bincode``; no GPU).  Returns ``(summary dict, ids)``,
    ids a (n_samples,) uint64 array in transaction order, or None with
    ``count_only``.  Raises HsvLibraryError (HSV_ERR_PARSE) for malformed bytes."""
    buf = bytes(buf)
    lib = _lib.load()
    res = BatchSamples()
    _lib.check(lib.hsv_batch_samples_bincode(buf, len(buf), ctypes.byref(res), None, 0), "hsv_batch_samples_bincode")
    if count_only:
        return res.as_dict(), None
    ids = np.zeros(max(int(res.n_samples), 1), np.uint64)
    _lib.check(lib.hsv_batch_samples_bincode(buf, len(buf), ctypes.byref(res), _ptr(ids), int(res.n_samples)),
               "hsv_batch_samples_bincode")
    return res.as_dict(), ids[:int(res.n_samples)].copy()


def batches_samples_device(bufs, offsets, tx_cap: int, n_batches: int | None = None, index=None, ids=None,
                           stream=None):
    """Enqueue the sample index of device-resident serialized batches (torch
    uint8 tensor ``bufs``; ``offsets`` an int64 tensor of n_batches + 1 byte
    offsets), parsed as ``hsv_batches_verify_bincode_device`` parses them.
    ``(out, batch_offsets)`` of :func:`seal_device` can be passed whole, with
    ``tx_cap`` the seal's n: the entries past the real batch count come out as
    BATCH_PARSE with no ids.  Outputs (allocated on ``bufs``'s device when not
    given): ``index`` (n_batches, 5) int64 -- status | pad << 32, n_tx, size,
    n_samples, first_sample per batch, read with :meth:`BatchSamples.from_words`
    -- and ``ids`` int64 (the ids' bit patterns; default ``tx_cap`` entries,
    which always suffices), of which only the first total-sample-count entries
    are written.  No synchronisation.  Returns ``(index, ids)``."""
    import torch

    if n_batches is None:
        n_batches = offsets.numel() - 1
    dev = bufs.device
    if index is None:
        index = torch.empty((max(n_batches, 1), 5), dtype=torch.int64, device=dev)
    if ids is None:
        ids = torch.empty(max(int(tx_cap), 1), dtype=torch.int64, device=dev)
        ids_cap = int(tx_cap)
    else:
        ids_cap = ids.numel()
    if index.numel() < 5 * n_batches:
        raise ValueError("index holds fewer than n_batches entries")
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()
    rc = lib.hsv_batches_samples_bincode_device(
        ctypes.c_void_p(bufs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), n_batches, int(tx_cap),
        ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(ids.data_ptr()) if ids_cap else None, ids_cap,
        ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_batches_samples_bincode_device")
    return index, ids
