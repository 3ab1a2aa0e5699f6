"""Wire formats: QC / TC certificates as bincode bytes.

Encoders restate bincode 1.3's default encoding of the reference's serde
derives (little-endian fixed-width integers, u64 length prefixes; PublicKey
serialises as its base64 string, crypto/src/lib.rs:94-101):

    QC = hash (32) | round u64 | votes: u64 n, n x (PublicKey str, R (32), s (32))
                                                  consensus/src/messages.rs:162-167
    TC = round u64 | votes: u64 n, n x (PublicKey str, R, s, high_qc_round u64)
                                                  consensus/src/messages.rs:281-285

:func:`qc_verify` / :func:`tc_verify` hand the bytes to
``hsv_qc_verify_bincode`` / ``hsv_tc_verify_bincode``, which parse them in C++
and verify on the GPU (QC: ``verify_batch`` over ``qc.digest()``; TC: one
strict verification per vote over SHA-512(round_le || high_qc_round_le)[..32]).

The objects that carry them (consensus/src/messages.rs:16-24, 112-118, 222-228):

    Block   = qc | tc: Option<TC> (u8 tag 0 / 1) | author: PublicKey str |
              round u64 | payload: u64 n, n x Digest (32) | signature R, s
    Vote    = hash (32) | round u64 | author | signature
    Timeout = high_qc: QC | round u64 | author | signature

:func:`block_verify`, :func:`timeout_verify`, :func:`vote_verify` and
:func:`blocks_verify` (a chain) check every signature of the object -- the
author's (strict), the embedded QC's (batch rule, skipped for the genesis QC)
and the embedded TC's (strict) -- in ONE verification call and report the
first failing stage in the reference's order; :func:`proposal_verify` is the
same for a block given as plain data (``hsv_proposal_verify``).  The stake and
quorum checks stay with the caller.
"""
from __future__ import annotations

import base64
import ctypes
import struct
from typing import Sequence, Tuple

import numpy as np

from . import _lib


def _str(s: bytes) -> bytes:
    return struct.pack("<Q", len(s)) + s


def encode_public_key(pk: bytes) -> bytes:
    """bincode of PublicKey: its base64 (standard, padded) string."""
    return _str(base64.b64encode(bytes(pk)))


def encode_qc(block_hash: bytes, round_: int, votes: Sequence[Tuple[bytes, bytes]]) -> bytes:
    """bincode of consensus::QC{hash, round, votes: [(pk, sig R||s)]}."""
    out = [bytes(block_hash), struct.pack("<QQ", round_, len(votes))]
    for pk, sig in votes:
        out.append(encode_public_key(pk))
        out.append(bytes(sig))
    return b"".join(out)


def encode_tc(round_: int, votes: Sequence[Tuple[bytes, bytes, int]]) -> bytes:
    """bincode of consensus::TC{round, votes: [(pk, sig, high_qc_round)]}."""
    out = [struct.pack("<QQ", round_, len(votes))]
    for pk, sig, hqc in votes:
        out.append(encode_public_key(pk))
        out.append(bytes(sig))
        out.append(struct.pack("<Q", hqc))
    return b"".join(out)


def encode_block(qc: bytes, tc, author: bytes, round_: int, payload: Sequence[bytes], signature: bytes) -> bytes:
    """bincode of consensus::Block{qc, tc: Option<TC>, author, round, payload:
    Vec<Digest>, signature} (consensus/src/messages.rs:16-24).  ``qc`` and
    ``tc`` are their encodings (:func:`encode_qc`, :func:`encode_tc`); ``tc``
    None is Option::None."""
    out = [bytes(qc), b"\x00" if tc is None else b"\x01" + bytes(tc), encode_public_key(author),
           struct.pack("<QQ", round_, len(payload))]
    out += [bytes(d) for d in payload]
    out.append(bytes(signature))
    return b"".join(out)


def encode_vote(block_hash: bytes, round_: int, author: bytes, signature: bytes) -> bytes:
    """bincode of consensus::Vote{hash, round, author, signature} (messages.rs:112-118)."""
    return bytes(block_hash) + struct.pack("<Q", round_) + encode_public_key(author) + bytes(signature)


def encode_timeout(high_qc: bytes, round_: int, author: bytes, signature: bytes) -> bytes:
    """bincode of consensus::Timeout{high_qc, round, author, signature} (messages.rs:222-228)."""
    return bytes(high_qc) + struct.pack("<Q", round_) + encode_public_key(author) + bytes(signature)


def block_digest(author: bytes, round_: int, payload: Sequence[bytes], qc_hash: bytes) -> bytes:
    """Block::digest (messages.rs:80-89): what the author signs."""
    import hashlib
    return hashlib.sha512(bytes(author) + struct.pack("<Q", round_) + b"".join(bytes(d) for d in payload)
                          + bytes(qc_hash)).digest()[:32]


def vote_digest(block_hash: bytes, round_: int) -> bytes:
    """Vote::digest and QC::digest (messages.rs:149-156, 201-207)."""
    import hashlib
    return hashlib.sha512(bytes(block_hash) + struct.pack("<Q", round_)).digest()[:32]


def timeout_digest(round_: int, high_qc_round: int) -> bytes:
    """Timeout::digest and a TC vote's digest (messages.rs:268-275, 306-313)."""
    import hashlib
    return hashlib.sha512(struct.pack("<QQ", round_, high_qc_round)).digest()[:32]


# hsv_proposal_result.stage (include/hsv.h)
STAGE_OK, STAGE_AUTHOR, STAGE_QC, STAGE_TC, STAGE_PARSE = range(5)


class ProposalResult(ctypes.Structure):
    """hsv_proposal_result: the first failing stage and its lowest failing vote."""
    _fields_ = [("stage", ctypes.c_uint32), ("index", ctypes.c_uint32)]

    def as_tuple(self):
        return int(self.stage), int(self.index)


class Proposal(ctypes.Structure):
    """hsv_proposal (include/hsv.h): a Block as plain data."""
    _fields_ = [("author", ctypes.c_uint8 * 32), ("signature", ctypes.c_uint8 * 64), ("round", ctypes.c_uint64),
                ("payload", ctypes.c_void_p), ("n_payload", ctypes.c_size_t),
                ("qc_hash", ctypes.c_uint8 * 32), ("qc_round", ctypes.c_uint64),
                ("qc_votes", ctypes.c_void_p), ("n_qc", ctypes.c_size_t),
                ("has_tc", ctypes.c_int), ("tc_round", ctypes.c_uint64),
                ("tc_votes", ctypes.c_void_p), ("n_tc", ctypes.c_size_t)]


def _handle(committee):
    return None if committee is None else committee._h


def proposal_verify(author: bytes, signature: bytes, round_: int, payload: Sequence[bytes], qc_hash: bytes,
                    qc_round: int, qc_votes: Sequence[Tuple[bytes, bytes]], tc_round=None,
                    tc_votes: Sequence[Tuple[bytes, bytes, int]] = (), committee=None):
    """hsv_proposal_verify on a block given as plain data (``tc_round`` None:
    no TC) -> (ok, (stage, index), raw flags of author, QC votes, TC votes)."""
    lib = _lib.load()
    pay = np.frombuffer(b"".join(bytes(d) for d in payload), np.uint8)
    qv = np.frombuffer(b"".join(bytes(pk) + bytes(sig) for pk, sig in qc_votes), np.uint8)
    tv = np.frombuffer(b"".join(bytes(pk) + bytes(sig) + struct.pack("<Q", h) for pk, sig, h in tc_votes), np.uint8)
    p = Proposal()
    p.author[:] = bytes(author)
    p.signature[:] = bytes(signature)
    p.round, p.qc_round = round_, qc_round
    p.qc_hash[:] = bytes(qc_hash)
    p.payload, p.n_payload = (pay.ctypes.data if pay.size else None), len(payload)
    p.qc_votes, p.n_qc = (qv.ctypes.data if qv.size else None), len(qc_votes)
    p.has_tc = 0 if tc_round is None else 1
    p.tc_round = 0 if tc_round is None else tc_round
    p.tc_votes, p.n_tc = (tv.ctypes.data if tv.size else None), len(tc_votes)
    res = ProposalResult()
    flags = np.zeros(1 + len(qc_votes) + len(tc_votes), np.uint8)
    rc = _lib.check(lib.hsv_proposal_verify(_handle(committee), ctypes.byref(p), ctypes.byref(res),
                                            ctypes.c_void_p(flags.ctypes.data)), "hsv_proposal_verify")
    return rc == 1, res.as_tuple(), flags


def block_verify(buf: bytes, committee=None):
    """Block::verify's signature half in one call (``hsv_block_verify_bincode``)
    -> (ok, (stage, index), n_qc, n_tc, decoded keys (1 + n_qc + n_tc, 32): the
    author, the QC voters, the TC voters).  ``committee``: a
    :class:`hsverify.committee.Committee` (votes verified by member index) or
    None (the generic path with the automatic cache).  Raises HsvLibraryError
    on malformed bytes (HSV_ERR_PARSE) or an infrastructure error."""
    lib = _lib.load()
    res = ProposalResult()
    n_qc, n_tc = ctypes.c_size_t(0), ctypes.c_size_t(0)
    pks = np.zeros((1 + len(buf) // 115, 32), np.uint8)  # a vote is at least 116 encoded bytes
    rc = _lib.check(lib.hsv_block_verify_bincode(_handle(committee), buf, len(buf), ctypes.byref(res),
                                                 ctypes.byref(n_qc), ctypes.byref(n_tc),
                                                 ctypes.c_void_p(pks.ctypes.data)), "hsv_block_verify_bincode")
    return rc == 1, res.as_tuple(), n_qc.value, n_tc.value, pks[: 1 + n_qc.value + n_tc.value]


def timeout_verify(buf: bytes, committee=None):
    """Timeout::verify's signature half (``hsv_timeout_verify_bincode``)
    -> (ok, (stage, index), n_qc, decoded keys: the author, then the QC voters)."""
    lib = _lib.load()
    res = ProposalResult()
    n_qc = ctypes.c_size_t(0)
    pks = np.zeros((1 + len(buf) // 115, 32), np.uint8)
    rc = _lib.check(lib.hsv_timeout_verify_bincode(_handle(committee), buf, len(buf), ctypes.byref(res),
                                                   ctypes.byref(n_qc), ctypes.c_void_p(pks.ctypes.data)),
                    "hsv_timeout_verify_bincode")
    return rc == 1, res.as_tuple(), n_qc.value, pks[: 1 + n_qc.value]


def vote_verify(buf: bytes, committee=None) -> bool:
    """Vote::verify's signature half (``hsv_vote_verify_bincode``)."""
    lib = _lib.load()
    return _lib.check(lib.hsv_vote_verify_bincode(_handle(committee), buf, len(buf)), "hsv_vote_verify_bincode") == 1


def blocks_verify(blocks: Sequence[bytes], committee=None):
    """A chain of blocks in one verification call (``hsv_blocks_verify_bincode``)
    -> (number of blocks that verify, [(stage, index)] per block); a block
    that does not parse gets STAGE_PARSE."""
    lib = _lib.load()
    offsets = np.zeros(len(blocks) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    bufs = b"".join(bytes(b) for b in blocks)
    results = (ProposalResult * max(1, len(blocks)))()
    rc = _lib.check(lib.hsv_blocks_verify_bincode(_handle(committee), bufs, ctypes.c_void_p(offsets.ctypes.data),
                                                  len(blocks), ctypes.cast(results, ctypes.c_void_p)),
                    "hsv_blocks_verify_bincode")
    return rc, [results[i].as_tuple() for i in range(len(blocks))]


# ---- serialized mempool batches (mempool/src/batch_maker.rs:127-131) -------------
# hsv_batch_result.status (include/hsv.h)
BATCH_OK, BATCH_TX, BATCH_PARSE, BATCH_OVERFLOW = range(4)


class BatchResult(ctypes.Structure):
    """hsv_batch_result: the batch's verdict, its lowest failing transaction,
    its transaction count and its first index in the flags array."""
    _fields_ = [("status", ctypes.c_uint32), ("index", ctypes.c_uint32), ("n_tx", ctypes.c_uint64),
                ("first", ctypes.c_uint64)]

    def as_tuple(self):
        return int(self.status), int(self.index), int(self.n_tx), int(self.first)


def encode_batch(txs: Sequence[bytes]) -> bytes:
    """bincode of mempool::MempoolMessage::Batch(Vec<Vec<u8>>) as
    BatchMaker::seal serializes it: u32 variant tag 0 | u64 count | count x
    (u64 length, bytes)."""
    out = [struct.pack("<IQ", 0, len(txs))]
    for t in txs:
        out.append(_str(bytes(t)))
    return b"".join(out)


def encode_batch_request(digests: Sequence[bytes], requestor: bytes) -> bytes:
    """bincode of MempoolMessage::BatchRequest(Vec<Digest>, PublicKey): variant
    tag 1 -- what Core::make_vote rejects where it expects a Batch."""
    return struct.pack("<IQ", 1, len(digests)) + b"".join(bytes(d) for d in digests) + encode_public_key(requestor)


def decode_batch(buf: bytes):
    """``hsv_batch_parse_bincode`` (host only, no GPU) -> the transactions.
    Raises HsvLibraryError (HSV_ERR_PARSE) on malformed bytes."""
    lib = _lib.load()
    buf = bytes(buf)
    n = ctypes.c_size_t(0)
    _lib.check(lib.hsv_batch_parse_bincode(buf, len(buf), ctypes.byref(n), None, 0), "hsv_batch_parse_bincode")
    spans = np.zeros(2 * n.value, np.uint64)
    _lib.check(lib.hsv_batch_parse_bincode(buf, len(buf), ctypes.byref(n), ctypes.c_void_p(spans.ctypes.data),
                                           spans.size), "hsv_batch_parse_bincode")
    return [buf[int(spans[2 * i]): int(spans[2 * i + 1])] for i in range(n.value)]


def batches_verify(batches: Sequence[bytes], committee=None):
    """Serialized batches in one call (``hsv_batches_verify_bincode``) ->
    (number of batches that pass, [(status, index, n_tx, first)] per batch,
    flag bytes of all transactions in batch order).  A batch that does not
    parse gets BATCH_PARSE and leaves its neighbours alone."""
    lib = _lib.load()
    offsets = np.zeros(len(batches) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in batches], dtype=np.uint64)
    bufs = b"".join(bytes(b) for b in batches)
    flags = np.zeros(max(1, len(bufs) // 8), np.uint8)  # a transaction is at least its 8-byte length
    results = (BatchResult * max(1, len(batches)))()
    rc = _lib.check(lib.hsv_batches_verify_bincode(_handle(committee), bufs, ctypes.c_void_p(offsets.ctypes.data),
                                                   len(batches), ctypes.cast(results, ctypes.c_void_p),
                                                   ctypes.c_void_p(flags.ctypes.data), flags.size),
                    "hsv_batches_verify_bincode")
    res = [results[i].as_tuple() for i in range(len(batches))]
    total = sum(r[2] for r in res)
    return rc, res, flags[:total]


def batch_verify(buf: bytes, committee=None):
    """One serialized batch (``hsv_batch_verify_bincode``) -> (ok, (status,
    index, n_tx, first)).  Raises HsvLibraryError (HSV_ERR_PARSE) on malformed
    bytes."""
    lib = _lib.load()
    buf = bytes(buf)
    res = BatchResult()
    rc = _lib.check(lib.hsv_batch_verify_bincode(_handle(committee), buf, len(buf), ctypes.byref(res)),
                    "hsv_batch_verify_bincode")
    return rc == 1, res.as_tuple()


def batches_verify_device(bufs, offsets, n_batches: int, tx_cap: int, results, flags=None, committee=None,
                          stream=None, fault=None) -> None:
    """Enqueue ``hsv_batches_verify_bincode_device`` on device-resident bytes:
    ``bufs`` a torch uint8 tensor, ``offsets`` an int64 tensor of n_batches + 1
    byte offsets, ``results`` an int64 tensor of 3 * n_batches words (one
    hsv_batch_result each; :func:`batch_results` reads them), ``flags``
    (optional) a uint8 tensor of tx_cap bytes.  No synchronisation."""
    from .verifier import _fault_ptr
    import torch

    if stream is None:
        stream = torch.cuda.current_stream(bufs.device).cuda_stream
    lib = _lib.load()
    rc = lib.hsv_batches_verify_bincode_device(
        _handle(committee), ctypes.c_void_p(bufs.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), n_batches, tx_cap,
        ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(flags.data_ptr()) if flags is not None else None,
        _fault_ptr(fault), ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_batches_verify_bincode_device")


def batch_results(words) -> list:
    """[(status, index, n_tx, first)] from the 3 * n 64-bit words of n
    hsv_batch_result structures (a numpy array or a CPU tensor)."""
    w = np.asarray(words).astype(np.int64).view(np.uint64).reshape(-1, 3)
    return [(int(a & np.uint64(0xffffffff)), int(a >> np.uint64(32)), int(n), int(f)) for a, n, f in w]


def qc_verify(buf: bytes):
    """-> (ok: bool, decoded public keys (n, 32) u8).  Raises HsvLibraryError on
    malformed bytes (HSV_ERR_PARSE) or an infrastructure error."""
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    # keys are written only after a successful parse; size the buffer generously
    pks = np.zeros((max(1, len(buf) // 115), 32), np.uint8)
    rc = _lib.check(lib.hsv_qc_verify_bincode(buf, len(buf), ctypes.byref(n), ctypes.c_void_p(pks.ctypes.data)),
                    "hsv_qc_verify_bincode")
    return rc == 1, pks[: n.value]


def tc_verify(buf: bytes):
    """-> (ok: bool, per-vote flag bytes)."""
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    flags = np.zeros(max(1, len(buf) // 123), np.uint8)
    rc = _lib.check(lib.hsv_tc_verify_bincode(buf, len(buf), ctypes.byref(n), ctypes.c_void_p(flags.ctypes.data)),
                    "hsv_tc_verify_bincode")
    return rc == 1, flags[: n.value]
