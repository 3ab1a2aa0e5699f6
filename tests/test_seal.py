"""hsv_seal_transactions*: BatchMaker::run / seal (mempool/src/batch_maker.rs:78-131)
on the device -- keep the transactions whose flags say HSV_STRICT_OK, cut them
greedily at batch_size, lay each batch down as MempoolMessage::Batch bincode and
hash it.

No expected value comes from the library.  Expected bytes are wire.encode_batch
over a restatement of the greedy rule written here; expected digests are
hashlib.sha512(...)[:32]; expected flags are the C oracle's
(conftest.oracle_tx_flags).  The seal does not care where its flags come from,
so most cases use synthetic flag bytes and need no signatures.
"""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import PKG, oracle_tx_flags

pytestmark = pytest.mark.gpu

STRICT_OK = 1
FILL = 0xA5
TILE = int(re.search(r"kSealTile = (\d+)", open(os.path.join(PKG, "csrc", "hsv_seal.hpp")).read()).group(1))


def _greedy(lens, keep, batch_size, flush):
    """batch_maker.rs:87-105 -> (batches as lists of indices, held indices)"""
    batches, cur, size = [], [], 0
    for i, (n, k) in enumerate(zip(lens, keep)):
        if not k:
            continue
        size += n
        cur.append(i)
        if size >= batch_size:
            batches.append(cur)
            cur, size = [], 0
    if flush and cur:
        batches.append(cur)
        cur = []
    return batches, cur


def _expect(txs, keep, batch_size, flush, n_malformed=0):
    from hsverify import wire
    lens = [len(t) for t in txs]
    batches, held = _greedy(lens, keep, batch_size, flush)
    encs = [wire.encode_batch([txs[i] for i in b]) for b in batches]
    sealed = sum(len(b) for b in batches)
    summary = {"items": len(txs), "sealed": sealed, "rejected": len(txs) - sum(map(bool, keep)) - n_malformed,
               "malformed": n_malformed, "held": len(held), "held_first": held[0] if held else len(txs),
               "bytes": sum(map(len, encs)), "n_batches": len(encs), "status": 0}
    return encs, summary


def _seal(blob, n, batch_size, flush, offsets=None, tx_size=0, flags=None, in_base=3, out_base=5, out_cap=None,
          batches_cap=None, digests=True):
    """hsv_seal_transactions_device on `blob` laid at in_base of a filled tensor,
    into a filled output tensor at out_base.  Checks that the input is only
    read and that nothing is written outside [out_base, out_base + bytes), the
    batches_cap + 1 offsets and the first n_batches digests.
    -> (summary dict, out bytes [0, bytes), offsets list, digests array)"""
    import torch
    from hsverify import mempool
    dev = torch.device("cuda:0")
    blob = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob
    host = np.full(blob.size + 256, FILL, np.uint8)
    host[in_base:in_base + blob.size] = blob
    d_in = torch.from_numpy(host).to(dev)
    total = blob.size
    cap, bcap = mempool.seal_bound(total, n, batch_size)
    out_cap = cap if out_cap is None else out_cap
    batches_cap = bcap if batches_cap is None else batches_cap
    d_out = torch.full((out_base + out_cap + 64,), FILL, dtype=torch.uint8, device=dev)
    d_boff = torch.full((batches_cap + 1 + 4,), -1, dtype=torch.int64, device=dev)
    d_dig = torch.full(((batches_cap + 2) * 32 + 1,), FILL, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8 + 2,), -1, dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev) if offsets is not None else None
    d_flags = torch.from_numpy(np.asarray(flags, np.uint8)).to(dev) if flags is not None else None
    mempool.seal_device(d_in[in_base:], d_off, tx_size, n, d_flags, batch_size, flush, out=d_out[out_base:out_base + out_cap],
                        batch_offsets=d_boff[:batches_cap + 1], digests=d_dig[1:1 + 32 * batches_cap] if digests else None,
                        summary_out=d_sum[:8])
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == host).all()  # the input is only read
    if flags is not None:
        assert (d_flags.cpu().numpy() == np.asarray(flags, np.uint8)).all()
    s = mempool.SealSummary.from_words(d_sum[:8].cpu().numpy()).as_dict()
    assert (d_sum[8:].cpu().numpy() == -1).all()
    out = d_out.cpu().numpy()
    boff = d_boff.cpu().numpy()
    dig = d_dig.cpu().numpy()
    assert (boff[batches_cap + 1:] == -1).all()
    assert (out[:out_base] == FILL).all() and (out[out_base + out_cap:] == FILL).all()  # never at or beyond out_cap
    assert dig[0] == FILL and (dig[1 + 32 * batches_cap:] == FILL).all()
    assert s["items"] == s["sealed"] + s["rejected"] + s["malformed"] + s["held"]
    if s["status"] == 0:
        k, b = s["n_batches"], s["bytes"]
        assert (out[out_base + b:] == FILL).all()  # the guard fill past `bytes`
        assert boff[0] == 0 and (boff[k:batches_cap + 1] == b).all()  # entries past n_batches repeat the end
        if digests:
            assert (dig[1 + 32 * k:] == FILL).all()
        else:
            assert (dig == FILL).all()
        return s, out[out_base:out_base + b].tobytes(), boff[:k + 1].tolist(), dig[1:1 + 32 * k].reshape(k, 32)
    return s, None, None, None


def _check(got, encs, want_summary, digests=True):
    s, out, boff, dig = got
    assert s == want_summary
    assert out == b"".join(encs)
    assert boff == list(np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.int64))
    if digests:
        for b, e in enumerate(encs):
            assert dig[b].tobytes() == hashlib.sha512(e).digest()[:32], b


# ---- 1. real transactions, oracle flags ------------------------------------------------
@pytest.fixture(scope="module")
def signed(hsv, tx_golden, oracle_lib):
    """The 47 golden transactions and 37 ragged ones (test_batch_wire.py's recipe:
    lengths 0, 95, 96, 97, ..., three corrupted) with the oracle's flags."""
    from hsverify import mempool
    from test_batch_wire import _signed
    lens = [0, 95, 96, 97] + list(np.random.default_rng(3).integers(96, 700, 33))
    txs = list(tx_golden["txs"]) + _signed(lens, 11, bad=(8, 20, 36))
    assert len(txs) == 84
    buf, offsets = mempool.pack(txs)
    flags = oracle_tx_flags(oracle_lib, buf, offsets)
    assert (flags[:47] == tx_golden["flags"]).all()
    assert [i for i in range(37) if not flags[47 + i] & STRICT_OK] == [0, 1, 8, 20, 36]
    return txs, buf, offsets, flags


@pytest.mark.parametrize("flush", [0, 1])
@pytest.mark.parametrize("batch_size", [1, 97, 1000, 15000, 1 << 40])
def test_golden_and_ragged(signed, batch_size, flush):
    txs, buf, offsets, flags = signed
    keep = [bool(f & STRICT_OK) for f in flags]
    encs, want = _expect(txs, keep, batch_size, flush)
    assert want["sealed"] + want["held"] == sum(keep) and want["rejected"] == len(txs) - sum(keep)
    got = _seal(buf, len(txs), batch_size, flush, offsets=offsets, flags=flags, in_base=3, out_base=5)
    _check(got, encs, want)


def test_round_trip_through_the_batch_verifier(signed):
    """The sealed output, unchanged, is a valid (d_bufs, d_offsets) of
    hsv_batches_verify_bincode_device: every batch HSV_BATCH_OK with the sealed
    count, and hsv_batch_parse_bincode accepts each batch."""
    import torch
    from hsverify import mempool, wire
    txs, buf, offsets, flags = signed
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), buf])).to(dev)[1:]
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_flags = torch.zeros(len(txs), dtype=torch.uint8, device=dev)
    mempool.verify_transactions_device(d_in, d_off, 0, len(txs), flags=d_flags)
    cap, bcap = mempool.seal_bound(buf.size, len(txs), 1000)
    d_out = torch.full((cap + 7,), FILL, dtype=torch.uint8, device=dev)
    out, boff, _, d_sum = mempool.seal_device(d_in, d_off, 0, len(txs), d_flags, 1000, True, out=d_out[7:],
                                              batch_offsets=torch.empty(bcap + 1, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert (d_flags.cpu().numpy() == flags).all()
    s = mempool.SealSummary.from_words(d_sum.cpu().numpy())
    keep = [bool(f & STRICT_OK) for f in flags]
    encs, want = _expect(txs, keep, 1000, True)
    assert s.as_dict() == want
    k = int(s.n_batches)
    results = torch.full((3 * k,), -1, dtype=torch.int64, device=dev)
    vflags = torch.full((int(s.sealed),), 0xff, dtype=torch.uint8, device=dev)
    fault = torch.zeros(2, dtype=torch.int32, device=dev)
    wire.batches_verify_device(out, boff, k, int(s.sealed), results, flags=vflags, fault=fault)
    torch.cuda.synchronize()
    assert not fault.cpu().numpy().any()
    res = wire.batch_results(results.cpu().numpy())
    first = 0
    for b, e in enumerate(encs):
        n_tx = int.from_bytes(e[4:12], "little")
        assert res[b] == (0, 0, n_tx, first), (b, res[b])
        first += n_tx
    assert (vflags.cpu().numpy() & STRICT_OK).all()
    host, offs = out.cpu().numpy(), boff.cpu().numpy()
    kept = [t for t, f in zip(txs, keep) if f]
    back = []
    for b in range(k):
        back += wire.decode_batch(host[offs[b]:offs[b + 1]].tobytes())
    assert back == kept


@pytest.mark.parametrize("with_committee", [False, True])
def test_host_form(signed, oracle_lib, with_committee):
    """The host form equals the oracle filter plus encode_batch.  It verifies
    where hsv_verify_transactions_device does, so the 0- and 95-byte
    transactions are rejections, not argument errors."""
    from hsverify import mempool
    from hsverify.committee import Committee
    from test_batch_wire import SEEDS
    from hsverify import verifier
    txs, buf, offsets, flags = signed
    committee = None
    if with_committee:
        pk, _ = verifier.sign_many(SEEDS[:4], np.zeros((4, 32), np.uint8))
        committee = Committee(pk)
    keep = [bool(f & STRICT_OK) for f in flags]
    for batch_size, flush in ((1000, True), (15000, False)):
        encs, want = _expect(txs, keep, batch_size, flush)
        batches, got_flags, summary, dig = mempool.seal(txs, batch_size, committee=committee, flush=flush, digests=True)
        assert (got_flags == flags).all()
        assert summary == want
        assert batches == encs
        assert [d.tobytes() for d in dig] == [hashlib.sha512(e).digest()[:32] for e in encs]
    # host caps one short: the summary says what is needed, nothing is copied
    lib = hsv_lib()
    encs, want = _expect(txs, keep, 1000, True)
    for short_out, short_b in ((1, 0), (0, 1)):
        out = np.full(want["bytes"], FILL, np.uint8)
        boff = np.full(want["n_batches"] + 1, FILL, np.uint64)
        s = mempool.SealSummary()
        rc = lib.hsv_seal_transactions(committee._h if committee else None, ctypes.c_void_p(buf.ctypes.data),
                                       ctypes.c_void_p(offsets.ctypes.data), 0, len(txs), 1000, 1,
                                       ctypes.c_void_p(out.ctypes.data), want["bytes"] - short_out,
                                       ctypes.c_void_p(boff.ctypes.data), want["n_batches"] - short_b, None, None,
                                       ctypes.byref(s))
        assert rc == 0 and s.as_dict() == dict(want, status=1)
        assert (out == FILL).all() and (boff == FILL).all()


def hsv_lib():
    from hsverify import _lib
    return _lib.load()


# ---- 2. synthetic flags ------------------------------------------------------------------
def _random_case(n, lo, hi, seed, p_keep=0.8):
    rnd = np.random.default_rng(seed)
    lens = rnd.integers(lo, hi + 1, n)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    blob = rnd.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    flags = rnd.integers(0, 256, n, dtype=np.uint8)
    flags = (flags & 0xfe) | (rnd.random(n) < p_keep)
    txs = [blob[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]
    return txs, blob, offsets, flags.astype(np.uint8)


@pytest.mark.parametrize("tx_size", list(range(96, 113)))
def test_fixed_size_every_alignment(hsv, tx_size):
    """Fixed tx_size 96..112, input base offsets 0..15, output base offsets 0, 1,
    7, 15, accept-all: with the sizes, every (source, destination) misalignment
    of a transaction's bytes occurs."""
    n = 21
    blob = np.random.default_rng(tx_size).integers(0, 256, n * tx_size, dtype=np.uint8)
    txs = [blob[i * tx_size:(i + 1) * tx_size].tobytes() for i in range(n)]
    encs, want = _expect(txs, [True] * n, 5 * tx_size, True)
    assert want["n_batches"] == 5
    for in_base in range(16):
        for out_base in (0, 1, 7, 15):
            got = _seal(blob, n, 5 * tx_size, True, tx_size=tx_size, flags=np.full(n, 0xff, np.uint8),
                        in_base=in_base, out_base=out_base, digests=(in_base == out_base))
            _check(got, encs, want, digests=(in_base == out_base))


def test_empty_all_rejected_no_flags_and_malformed(hsv):
    # n == 0
    s, out, boff, dig = _seal(b"", 0, 100, True, offsets=[0])
    assert s == {"items": 0, "sealed": 0, "rejected": 0, "malformed": 0, "held": 0, "held_first": 0, "bytes": 0,
                 "n_batches": 0, "status": 0} and out == b"" and boff == [0]
    # n == 0 with room for batches: every offset is written
    s, out, boff, _ = _seal(b"", 0, 100, True, offsets=[0], batches_cap=3, out_cap=50)
    assert s["n_batches"] == 0 and boff == [0]
    txs, blob, offsets, flags = _random_case(300, 96, 130, 5)
    # all rejected
    got = _seal(blob, 300, 1000, True, offsets=offsets, flags=flags & 0xfe)
    _check(got, *_expect(txs, [False] * 300, 1000, True))
    # d_flags == NULL: every transaction is kept, whatever its length
    short, sblob, soff, _ = _random_case(300, 0, 40, 6)
    for flush in (0, 1):
        got = _seal(sblob, 300, 500, flush, offsets=soff, flags=None)
        _check(got, *_expect(short, [True] * 300, 500, flush))
    # decreasing offsets: malformed, dropped and counted, whatever the flags say
    bad = offsets.copy()
    bad_at = [7, 130, 299]
    for i in bad_at:
        bad[i + 1] = bad[i] - 1 - (i % 3)  # transaction i decreases; i + 1 is then longer than it was
    lens = np.diff(bad)
    txs2 = [blob[bad[i]:bad[i + 1]].tobytes() if lens[i] >= 0 else b"" for i in range(300)]
    keep = [bool(f & STRICT_OK) and lens[i] >= 0 for i, f in enumerate(flags)]
    encs, want = _expect(txs2, keep, 1000, False, n_malformed=3)
    want["rejected"] = 300 - sum(keep) - 3
    got = _seal(blob, 300, 1000, False, offsets=bad, flags=flags)
    _check(got, encs, want)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_scan_tile_seams(hsv, n):
    txs, blob, offsets, flags = _random_case(n, 96, 160, n)
    for batch_size, flush in ((5000, 0), (1, 1)):
        keep = [bool(f & STRICT_OK) for f in flags]
        got = _seal(blob, n, batch_size, flush, offsets=offsets, flags=flags, in_base=9, out_base=2)
        _check(got, *_expect(txs, keep, batch_size, flush))


def test_many_tiles(hsv):
    """2^17 + 5 transactions of 96..160 bytes: more than 256 scan workgroups, so
    the scan of the workgroup sums takes runs of several per lane."""
    n = (1 << 17) + 5
    txs, blob, offsets, flags = _random_case(n, 96, 160, 17)
    keep = [bool(f & STRICT_OK) for f in flags]
    encs, want = _expect(txs, keep, 5000, False)
    assert want["n_batches"] > 2000 and want["held"] > 0
    got = _seal(blob, n, 5000, False, offsets=offsets, flags=flags, in_base=1, out_base=13)
    _check(got, encs, want)


def test_overflow_reports_the_exact_need(hsv):
    txs, blob, offsets, flags = _random_case(500, 96, 160, 23)
    keep = [bool(f & STRICT_OK) for f in flags]
    encs, want = _expect(txs, keep, 3000, True)
    assert want["n_batches"] > 5
    # exactly enough: fine
    got = _seal(blob, 500, 3000, True, offsets=offsets, flags=flags, out_cap=want["bytes"],
                batches_cap=want["n_batches"])
    _check(got, encs, want)
    # one byte, one batch short: status and the exact needs; _seal checks the guards
    for out_cap, batches_cap in ((want["bytes"] - 1, want["n_batches"]), (want["bytes"], want["n_batches"] - 1),
                                 (0, 0)):
        s, out, _, _ = _seal(blob, 500, 3000, True, offsets=offsets, flags=flags, out_cap=out_cap,
                             batches_cap=batches_cap)
        assert out is None and s == dict(want, status=1)


def test_one_long_transaction_among_small_ones(hsv):
    """A 3 MiB transaction among 100 small ones: its pieces beyond the first go
    through the piece kernel."""
    rnd = np.random.default_rng(31)
    lens = [int(x) for x in rnd.integers(96, 300, 100)]
    lens.insert(41, 3 * (1 << 20) + 77)
    lens.insert(70, 16384 + 1)   # one byte into a second piece
    lens.insert(80, 16384)       # exactly one piece
    n = len(lens)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    blob = rnd.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    txs = [blob[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]
    flags = np.ones(n, np.uint8)
    flags[[3, 50]] = 0
    keep = [bool(f) for f in flags]
    encs, want = _expect(txs, keep, 4000, True)
    got = _seal(blob, n, 4000, True, offsets=offsets, flags=flags, in_base=7, out_base=10)
    _check(got, encs, want)
