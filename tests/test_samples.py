"""hsv_batches_samples_bincode_device and hsv_client_bursts_device: the benchmark's
sample transactions through the device pipeline -- the client's bursts
(node/src/client.rs:121-135), signed, verified and sealed there, and the index of
what the `benchmark` block of BatchMaker::seal logs per batch
(mempool/src/batch_maker.rs:118-125, 133-153).

No expected value comes from the calls under test: transactions are the client
loop restated in tests/test_samples_host.py, batches are wire.encode_batch over
lists built here, ids and sizes the seal filter restated there, the numbering
and the overflow rule restated in _expect below.
"""
import ctypes
import hashlib
import os
import re
import struct

import numpy as np
import pytest

from conftest import PKG
from test_samples_host import client_rs, sample, seal_filter

pytestmark = pytest.mark.gpu

FILL = 0xA5
CANARY = 0x5A5A5A5A5A5A5A5A
OK, PARSE, OVERFLOW = 0, 2, 3
TILE = int(re.search(r"kSamplesTile = (\d+)", open(os.path.join(PKG, "csrc", "hsv_samples.hpp")).read()).group(1))


def standard(i, size):
    return (bytes([1]) + struct.pack(">Q", i) + bytes(max(size - 9, 0)))[:size]


def _expect(batches, tx_cap):
    """batches: lists of transactions, or raw bytes for a malformed batch ->
    (index rows as dicts, all ids in order).  Transactions are numbered over the
    well-formed batches; a batch that does not lie below tx_cap overflows."""
    rows, ids, run = [], [], 0
    for b in batches:
        if isinstance(b, bytes):
            rows.append({"status": PARSE, "n_tx": 0, "size": 0, "n_samples": 0, "first_sample": 0})
            continue
        mine, size = seal_filter(b)
        if run > tx_cap or len(b) > tx_cap - run:
            rows.append({"status": OVERFLOW, "n_tx": len(b), "size": size, "n_samples": 0, "first_sample": None})
        else:
            rows.append({"status": OK, "n_tx": len(b), "size": size, "n_samples": len(mine), "first_sample": len(ids)})
            ids += mine
        run += len(b)
    for r in rows:  # an overflowed batch: where its ids would have begun (every batch that fits lies before it)
        if r["first_sample"] is None:
            r["first_sample"] = len(ids)
    return rows, ids


def _index(batches, tx_cap, ids_cap=None, base=3):
    """The device call on the batches laid at `base` of a filled tensor ->
    (rows, the ids array with its 4 canary words).  Checks that the input is
    only read and that the index entries past n_batches are untouched."""
    import torch
    from hsverify import mempool, wire
    dev = torch.device("cuda:0")
    encs = [b if isinstance(b, bytes) else wire.encode_batch(b) for b in batches]
    blob = np.frombuffer(b"".join(encs), np.uint8)
    host = np.full(base + blob.size + 64, FILL, np.uint8)
    host[base:base + blob.size] = blob
    offs = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.int64)
    nb = len(encs)
    ids_cap = tx_cap if ids_cap is None else ids_cap
    d_in = torch.from_numpy(host).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_index = torch.full(((nb + 1) * 5,), -1, dtype=torch.int64, device=dev)
    d_ids = torch.from_numpy(np.full(ids_cap + 4, CANARY, np.uint64).view(np.int64)).to(dev)
    mempool.batches_samples_device(d_in[base:], d_off, tx_cap, nb, index=d_index[:nb * 5], ids=d_ids[:ids_cap])
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == host).all()
    words = d_index.cpu().numpy()
    assert (words[nb * 5:] == -1).all()
    rows = [mempool.BatchSamples.from_words(words[5 * b:5 * b + 5]) for b in range(nb)]
    assert all(r.pad == 0 for r in rows)
    return [r.as_dict() for r in rows], d_ids.cpu().numpy().view(np.uint64)


def _check(batches, tx_cap, ids_cap=None):
    rows, ids = _index(batches, tx_cap, ids_cap)
    want_rows, want_ids = _expect(batches, tx_cap)
    cap = tx_cap if ids_cap is None else ids_cap
    for b, (g, w) in enumerate(zip(rows, want_rows)):
        assert g == w, b
    k = min(len(want_ids), cap)
    assert ids[:k].tolist() == want_ids[:k]
    assert (ids[k:] == CANARY).all()  # nothing between the total and ids_cap, nothing at or beyond ids_cap
    return rows, want_ids


def _six_batches():
    big = [standard(i, 12) for i in range(TILE + 44)]
    for k, i in enumerate((TILE - 1, TILE, TILE + 43)):
        big[i] = sample((1 << 63) + k, 12)
    ragged = [(bytes([0 if i % 3 == 0 else 1 + i % 2 * 254]) + struct.pack(">Q", 1000 + i) + bytes(32))[:i % 41]
              for i in range(TILE + 1)]
    bad = struct.pack("<IQ", 0, 2) + struct.pack("<Q", 9) + sample(77, 9) + struct.pack("<Q", 30) + bytes(29)
    return [big, [], [sample(5, 100)], ragged, bad, [sample(6, 9), standard(1, 9), sample(8, 64)]]


def test_one_batch_of_three():
    rows, ids = _check([[sample(0xDEADBEEF, 9), bytes(8), standard(3, 40)]], 3)
    assert rows == [{"status": OK, "n_tx": 3, "size": 57, "n_samples": 1, "first_sample": 0}] and ids == [0xDEADBEEF]


def test_six_batches_in_one_call():
    batches = _six_batches()
    total = sum(len(b) for b in batches if not isinstance(b, bytes))
    rows, ids = _check(batches, total)
    assert [r["status"] for r in rows] == [OK, OK, OK, OK, PARSE, OK]
    assert [r["n_samples"] for r in rows[:3]] == [3, 0, 1] and rows[3]["n_samples"] > 50
    assert rows[5]["first_sample"] == len(ids) - 2 and ids[-2:] == [6, 8]
    # the ragged batch starts inside a tile and has samples on both sides of the next tile edge
    first = TILE + 45
    flags = [len(t) > 8 and t[0] == 0 for t in batches[3]]
    assert first % TILE and any(flags[:2 * TILE - first]) and any(flags[2 * TILE - first:])
    _check(batches, total + 100)  # a cap with room: the padding is no transaction


def test_ids_cap_below_the_total():
    batches = _six_batches()
    total = sum(len(b) for b in batches if not isinstance(b, bytes))
    n_ids = len(_expect(batches, total)[1])
    _check(batches, total, ids_cap=n_ids - 2)
    _check(batches, total, ids_cap=0)


def test_tx_cap_inside_the_third_batch():
    batches = [[sample(1, 9), standard(1, 30), sample(2, 30), standard(2, 9), standard(3, 200)],
               [standard(4, 96), sample(3, 96), b""],
               [sample(4, 20), standard(5, 20), standard(6, 20), sample(5, 20), standard(7, 20), standard(8, 20)],
               [], [standard(9, 10), sample(6, 10)]]
    rows, ids = _check(batches, 5 + 3 + 3)
    assert [r["status"] for r in rows] == [OK, OK, OVERFLOW, OVERFLOW, OVERFLOW]
    assert ids == [1, 2, 3] and [r["n_tx"] for r in rows] == [5, 3, 6, 0, 2] and rows[2]["size"] == 120
    _check(batches, 8)   # the third batch begins at the cap
    _check(batches, 14)  # and fits exactly: only the last overflows


def test_no_batches_and_no_room():
    import torch
    from hsverify import _lib, mempool
    dev = torch.device("cuda:0")
    _check([[], [sample(1, 9)], b"\x00" * 5], 0)  # tx_cap == 0: the empty batch passes, the other overflows
    d_buf = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(4, dtype=torch.int64, device=dev)
    d_index = torch.full((10,), -1, dtype=torch.int64, device=dev)
    d_ids = torch.full((4,), -1, dtype=torch.int64, device=dev)
    mempool.batches_samples_device(d_buf, d_off, 16, 0, index=d_index, ids=d_ids)  # n_batches == 0
    torch.cuda.synchronize()
    assert (d_index.cpu().numpy() == -1).all() and (d_ids.cpu().numpy() == -1).all()
    lib = _lib.load()
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    args = lambda **kw: [kw.get("buf", p(d_buf)), kw.get("off", p(d_off)), kw.get("nb", 1), kw.get("cap", 4),
                         kw.get("index", p(d_index)), kw.get("ids", p(d_ids)), kw.get("ids_cap", 4), None]
    assert lib.hsv_batches_samples_bincode_device(*args(index=p(d_index, 4))) == -5
    assert lib.hsv_batches_samples_bincode_device(*args(ids=p(d_ids, 4))) == -5
    assert lib.hsv_batches_samples_bincode_device(*args(off=p(d_off, 4))) == -5
    assert lib.hsv_batches_samples_bincode_device(*args(index=None)) == -3
    assert lib.hsv_batches_samples_bincode_device(*args(ids=None)) == -3
    assert lib.hsv_batches_samples_bincode_device(*args(cap=1 << 32)) == -3
    assert lib.hsv_batches_samples_bincode_device(*args(ids=None, ids_cap=0)) == 0  # counting only
    torch.cuda.synchronize()
    assert mempool.BatchSamples.from_words(d_index[:5].cpu().numpy()).status == PARSE  # a zero-length batch


@pytest.mark.parametrize("tx_size", [105, 512])
@pytest.mark.parametrize("base", [0, 1, 15])
def test_client_bursts_device_equals_the_client_loop(base, tx_size):
    import torch
    from hsverify import synth
    n, burst, counter0, r0, trailer = 23, 5, 3, (1 << 64) - 3, 96
    want, _, r_next = client_rs(n, tx_size - trailer, burst, counter0, r0)
    d = torch.full((16 + n * tx_size + 32,), FILL, dtype=torch.uint8, device="cuda:0")
    assert d.data_ptr() % 16 == 0
    txs, r = synth.client_bursts_gpu(n, tx_size, burst, counter0, r0, trailer, out=d[base:base + n * tx_size])
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert r == r_next
    assert (got[:base] == FILL).all() and (got[base + n * tx_size:] == FILL).all()
    rows = got[base:base + n * tx_size].reshape(n, tx_size)
    assert [bytes(t) for t in rows[:, :tx_size - trailer]] == want
    assert (rows[:, tx_size - trailer:] == FILL).all()  # the trailers are never written
    host, r_host = synth.client_bursts(n, tx_size, burst, counter0, r0, trailer, out=np.full((n, tx_size), FILL, np.uint8))
    assert r_host == r and (host == rows).all()
    # the reference's unsigned filler, at the smallest size
    d9 = torch.full((16 + 9 * n + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    synth.client_bursts_gpu(n, 9, burst, counter0, r0, 0, out=d9[base:base + 9 * n])
    torch.cuda.synchronize()
    got = d9.cpu().numpy()
    assert got[base:base + 9 * n].tobytes() == b"".join(client_rs(n, 9, burst, counter0, r0)[0])
    assert (got[:base] == FILL).all() and (got[base + 9 * n:] == FILL).all()


def test_the_chain_from_bursts_to_the_log_lines():
    import torch
    from hsverify import benchlog, mempool, synth, wire
    from hsverify.signer import Signer
    n, size, burst, counter0, batch_size = 23, 128, 5, 3, 600
    seeds = np.random.default_rng(11).integers(0, 256, (n, 32), dtype=np.uint8)
    with Signer(seeds) as s:
        txs, _ = synth.client_bursts_gpu(n, size, burst, counter0, signer=s)
        torch.cuda.synchronize()
    msgs, sent, _ = client_rs(n, size - 96, burst, counter0, 0)
    assert sent == [3, 4, 5, 6, 7] and [i for i, m in enumerate(msgs) if m[0] == 0] == [3, 9, 10, 16, 22]
    bad = (9, 12)  # a sample and a standard transaction
    for i in bad:
        txs[i, 100] ^= 1  # a byte of s
    flags = torch.zeros(n, dtype=torch.uint8, device=txs.device)
    mempool.verify_transactions_device(txs, tx_size=size, n=n, flags=flags)
    out, boff, dig, summ = mempool.seal_device(txs, tx_size=size, n=n, flags=flags, batch_size=batch_size, digests=True)
    torch.cuda.synchronize()
    before_out, before_txs = out.clone(), txs.clone()
    bcap = boff.numel() - 1
    index, ids = mempool.batches_samples_device(out, boff, n)  # n_batches = batches_cap, no read-back
    torch.cuda.synchronize()
    assert (out == before_out).all() and (txs == before_txs).all()
    assert ((flags.cpu().numpy() & 1) == [i not in bad for i in range(n)]).all()
    # client, filter and greedy cut restated
    host = txs.cpu().numpy()
    assert [bytes(t[:32]) for t in host] == msgs
    kept = [bytes(host[i]) for i in range(n) if i not in bad]
    batches, cur, acc = [], [], 0
    for t in kept:
        cur.append(t)
        acc += len(t)
        if acc >= batch_size:
            batches.append(cur)
            cur, acc = [], 0
    if cur:
        batches.append(cur)
    assert [len(b) for b in batches] == [5, 5, 5, 5, 1] and bcap >= 5
    assert mempool.SealSummary.from_words(summ.cpu().numpy()).n_batches == 5
    rows = [mempool.BatchSamples.from_words(w).as_dict() for w in index.cpu().numpy()]
    got_ids = ids.cpu().numpy().view(np.uint64)
    at, lines = 0, []
    for b, txl in enumerate(batches):
        want_ids, want_size = seal_filter(txl)
        assert rows[b] == {"status": OK, "n_tx": len(txl), "size": want_size, "n_samples": len(want_ids),
                           "first_sample": at}, b
        assert got_ids[at:at + len(want_ids)].tolist() == want_ids
        at += len(want_ids)
        digest = hashlib.sha512(wire.encode_batch(txl)).digest()[:32]
        assert bytes(dig[b].cpu().numpy()) == digest
        lines += benchlog.batch_sample_lines(dig[b].cpu().numpy(), got_ids[rows[b]["first_sample"]:][:rows[b]["n_samples"]])
        lines.append(benchlog.batch_size_line(dig[b].cpu().numpy(), rows[b]["size"]))
    assert got_ids[:at].tolist() == [3, 5, 6, 7]  # the corrupted sample's id, 4, is absent
    assert [r["size"] for r in rows[:5]] == [640, 640, 640, 640, 128]
    for r in rows[5:]:  # the repeated end offsets: zero-length batches
        assert r == {"status": PARSE, "n_tx": 0, "size": 0, "n_samples": 0, "first_sample": 0}
    assert len(rows) == bcap
    assert len(lines) == 4 + 5 and lines[0].endswith(" contains sample tx 3") and lines[-1].endswith(" contains 128 B")
