"""The three log lines the reference's benchmark is computed from
(``benchmark/benchmark/logs.py:87, 104, 107``), formatted exactly as the Rust
``info!`` calls write their message part:

* the client, ``node/src/client.rs:124``:
  ``Sending sample transaction {counter}``
* ``BatchMaker::seal``, ``mempool/src/batch_maker.rs:144-152``:
  ``Batch {digest:?} contains sample tx {id}`` per sample and
  ``Batch {digest:?} contains {size} B`` per batch

``{digest:?}`` is ``Digest``'s ``Debug`` form, the standard base64 of its 32
bytes with padding (``crypto/src/lib.rs:34-38``).  The inputs are what
``hsverify.synth.client_bursts*``, ``mempool.seal_device`` (the digests) and
``mempool.batch_samples`` / ``batches_samples_device`` (ids and size) deliver;
the timestamp and level in front of a line are the logger's, not these
functions'.
"""
from __future__ import annotations

import base64
from typing import Iterable, List


def _digest(digest) -> str:
    raw = bytes(digest)
    if len(raw) != 32:
        raise ValueError("a digest is 32 bytes")
    return base64.b64encode(raw).decode()


def sending_sample_line(counter: int) -> str:
    return f"Sending sample transaction {int(counter) % 2**64}"


def batch_sample_lines(digest, ids: Iterable[int]) -> List[str]:
    d = _digest(digest)
    return [f"Batch {d} contains sample tx {int(i) % 2**64}" for i in ids]


def batch_size_line(digest, size: int) -> str:
    return f"Batch {_digest(digest)} contains {int(size)} B"
