"""Serialized mempool batches verified from their bincode bytes
(hsv_batch*_verify_bincode*): Core::make_vote's payload check
(consensus/src/core.rs:113-142) where the bytes lie, through a span table that
the host parser or the device parse (csrc/hsv_batchwire.hip) writes.

Expected flags come from the C oracle over the same transactions packed
contiguously (conftest.oracle_tx_flags); expected verdicts are computed here
from those flags.  No expected value comes from another call of the library.
"""
import ctypes
import hashlib
import os
import re
import struct

import numpy as np
import pytest

import ed25519_ref as o
from conftest import PKG, oracle_tx_flags

pytestmark = pytest.mark.gpu

OK, TX, PARSE, OVERFLOW = range(4)
SEEDS = np.random.default_rng(2026).integers(0, 256, (8, 32), dtype=np.uint8)
W = int(re.search(r"kScanWindow = (\d+)", open(os.path.join(PKG, "csrc", "hsv_batchscan.hpp")).read()).group(1))


def _signed(lens, seed, bad=()):
    """Transactions of the given lengths: those of >= 96 bytes signed by one of
    SEEDS over SHA-512(message)[..32] (index in `bad`: R corrupted), shorter
    ones random bytes."""
    from hsverify import verifier
    rnd = np.random.default_rng(seed)
    lens = [int(n) for n in lens]
    long_ = [i for i, n in enumerate(lens) if n >= 96]
    msgs = {i: rnd.integers(0, 256, lens[i] - 96, dtype=np.uint8).tobytes() for i in long_}
    dig = np.stack([np.frombuffer(hashlib.sha512(msgs[i]).digest()[:32], np.uint8) for i in long_]) \
        if long_ else np.zeros((0, 32), np.uint8)
    keys = rnd.integers(0, len(SEEDS), len(long_))
    pk, sig = verifier.sign_many(SEEDS[keys], dig)
    txs = [rnd.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    bad = set(bad)
    for k, i in enumerate(long_):
        s = sig[k].copy()
        if i in bad:
            s[3] ^= 0x10
        txs[i] = msgs[i] + pk[k].tobytes() + s.tobytes()
    return txs


def _want_flags(oracle_lib, txs):
    from hsverify import mempool
    if not txs:
        return np.zeros(0, np.uint8)
    buf, offsets = mempool.pack(txs)
    return oracle_tx_flags(oracle_lib, buf, offsets)


def _want_results(batches, flags, tx_cap=None):
    """[(status, index, n_tx, first)] for batches given as lists of
    transactions (None: malformed) from the oracle's flags in batch order"""
    out, first = [], 0
    for txs in batches:
        if txs is None:
            out.append((PARSE, 0, 0, first))
            continue
        n = len(txs)
        if tx_cap is not None and first + n > tx_cap:
            out.append((OVERFLOW, 0, n, first))
        else:
            failing = np.nonzero((flags[first:first + n] & o.STRICT_OK) == 0)[0]
            out.append((TX, int(failing[0]), n, first) if failing.size else (OK, 0, n, first))
        first += n
    return out


def _host(encs, committee=None, base=1):
    """hsv_batches_verify_bincode on the batches laid end to end at an odd
    address -> (rc, results, flags)"""
    from hsverify import _lib, wire
    lib = _lib.load()
    blob = b"".join(encs)
    backing = np.full(len(blob) + 64, 0xA5, np.uint8)
    assert backing.ctypes.data % 16 == 0
    backing[base:base + len(blob)] = np.frombuffer(blob, np.uint8)
    offsets = np.zeros(len(encs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in encs], dtype=np.uint64)
    res = (wire.BatchResult * len(encs))()
    flags = np.full(len(blob) // 8 + 1, 0xff, np.uint8)
    rc = _lib.check(lib.hsv_batches_verify_bincode(None if committee is None else committee._h,
                                                   ctypes.c_void_p(backing.ctypes.data + base),
                                                   ctypes.c_void_p(offsets.ctypes.data), len(encs),
                                                   ctypes.cast(res, ctypes.c_void_p), ctypes.c_void_p(flags.ctypes.data),
                                                   flags.size), "hsv_batches_verify_bincode")
    return rc, [r.as_tuple() for r in res], flags


def _device(encs, tx_cap, committee=None, base=3, fill=0xA5, with_flags=True, lengths=None):
    """hsv_batches_verify_bincode_device on the batches laid end to end at an
    odd address inside a tensor filled with `fill` -> (results, flags or None).
    lengths: the batch lengths the offsets claim (default: the true ones)."""
    import torch
    from hsverify import wire
    dev = torch.device("cuda:0")
    blob = b"".join(encs)
    host = np.full(len(blob) + 4096, fill, np.uint8)
    host[base:base + len(blob)] = np.frombuffer(blob, np.uint8)
    backing = torch.from_numpy(host).to(dev)
    offsets = np.zeros(len(encs) + 1, np.int64)
    offsets[1:] = np.cumsum([len(e) for e in encs] if lengths is None else lengths)
    d_off = torch.from_numpy(offsets).to(dev)
    results = torch.full((3 * len(encs),), -1, dtype=torch.int64, device=dev)
    flags = torch.full((max(1, tx_cap),), 0xff, dtype=torch.uint8, device=dev) if with_flags else None
    fault = torch.zeros(2, dtype=torch.int32, device=dev)
    wire.batches_verify_device(backing[base:], d_off, len(encs), tx_cap, results, flags=flags, committee=committee,
                               fault=fault)
    torch.cuda.synchronize()
    assert not fault.cpu().numpy().any()  # d_fault reads zero
    assert (backing.cpu().numpy() == host).all()  # the input is only read
    return wire.batch_results(results.cpu().numpy()), (flags.cpu().numpy()[:tx_cap] if with_flags else None)


# ---- 1. the small route, host form ------------------------------------------------------
@pytest.fixture(scope="module")
def small(hsv, tx_golden, oracle_lib):
    from hsverify import wire
    lens = [0, 95, 96, 97] + list(np.random.default_rng(3).integers(96, 700, 33))
    ragged = _signed(lens, 11, bad=(8, 20, 36))
    assert len(ragged) == 37
    batches = [tx_golden["txs"], [], None, ragged]
    encs = [wire.encode_batch(tx_golden["txs"]), wire.encode_batch([]),
            wire.encode_batch_request([bytes(32)] * 4, bytes(SEEDS[0])), wire.encode_batch(ragged)]
    flags = _want_flags(oracle_lib, tx_golden["txs"] + ragged)
    assert (flags[:47] == tx_golden["flags"]).all()
    r = flags[47:]
    # 0 and 95 bytes: flags 0; 96 (an empty message) and 97 verify; the three corrupted ones do not
    assert not r[:2].any() and [i for i in range(37) if not r[i] & o.STRICT_OK] == [0, 1, 8, 20, 36]
    return batches, encs, flags


def test_small_route_host_form(small):
    from hsverify import mempool, wire
    batches, encs, want = small
    exp = _want_results(batches, want)
    assert [e[0] for e in exp] == [TX, OK, PARSE, TX]  # the golden vectors hold rejections
    rc, res, flags = _host(encs)
    assert res == exp, (res, exp)
    assert rc == 1
    assert (flags[:want.size] == want).all(), np.nonzero(flags[:want.size] != want)[0][:8]
    assert (flags[want.size:] == 0xff).all()  # nothing past the total is written
    # each batch alone
    for enc, e in zip(encs, exp):
        if e[0] == PARSE:
            with pytest.raises(Exception, match="HSV_ERR_PARSE"):
                wire.batch_verify(enc)
            assert mempool.verify_serialized_batch(enc) is False
        else:
            ok, r = wire.batch_verify(enc)
            assert (ok, r) == (e[0] == OK, (e[0], e[1], e[2], 0))
            assert mempool.verify_serialized_batch(enc) is (e[0] == OK)
    # a batch of passing transactions only
    good = wire.encode_batch([t for t, f in zip(batches[3], want[47:]) if f & o.STRICT_OK])
    assert wire.batch_verify(good) == (True, (OK, 0, 32, 0))
    assert wire.batches_verify([good, encs[1]])[0] == 2


# ---- 2. the large route ------------------------------------------------------------------
SIZES = (5000, 1, 3256)
FIRST_BAD = (77, 0, 1234)  # the first failure of each batch


@pytest.fixture(scope="module", params=["fixed136", "ragged"])
def large(request, hsv, oracle_lib):
    from hsverify import wire
    n = sum(SIZES)
    assert n == 2 ** 13 + 65 and all(sum(SIZES[:k]) % 64 for k in (1, 2))
    rnd = np.random.default_rng(5)
    lens = [136] * n if request.param == "fixed136" else list(rnd.integers(96, 401, n))
    bad, starts = set(), np.cumsum((0,) + SIZES)
    for b, (size, fb) in enumerate(zip(SIZES, FIRST_BAD)):
        bad.add(int(starts[b]) + fb)
        later = rnd.integers(fb + 1, size, size // 100) if size > fb + 1 else []
        bad |= {int(starts[b]) + int(i) for i in later}
    txs = _signed(lens, 17, bad=bad)
    batches = [txs[starts[b]:starts[b + 1]] for b in range(3)]
    encs = [wire.encode_batch(b) for b in batches]
    want = _want_flags(oracle_lib, txs)
    assert sorted(np.nonzero((want & o.STRICT_OK) == 0)[0]) == sorted(bad)
    exp = _want_results(batches, want)
    assert exp == [(TX, fb, size, int(st)) for fb, size, st in zip(FIRST_BAD, SIZES, starts)]
    return batches, encs, want


def test_large_route_host_form(large):
    batches, encs, want = large
    rc, res, flags = _host(encs)
    assert res == _want_results(batches, want) and rc == 0
    assert (flags[:want.size] == want).all(), np.nonzero(flags[:want.size] != want)[0][:8]


# ---- 3. the device form --------------------------------------------------------------------
def _check_device(batches, encs, want, **kw):
    total = want.size
    for tx_cap in (total, total + 100, total - 1):
        res, flags = _device(encs, tx_cap, **kw)
        exp = _want_results(batches, want, tx_cap)
        assert res == exp, (tx_cap, res, exp)
        if tx_cap < total:
            assert exp[-1][0] == OVERFLOW and all(e[0] != OVERFLOW for e in exp[:-1])
        # every byte written: a batch that is not verified and the padding read 0
        full = np.zeros(tx_cap, np.uint8)
        for e in exp:
            if e[0] in (OK, TX):
                full[e[3]:e[3] + e[2]] = want[e[3]:e[3] + e[2]]
        assert (flags == full).all(), (tx_cap, np.nonzero(flags != full)[0][:8])
    res, none = _device(encs, total, with_flags=False, **kw)
    assert none is None and res == _want_results(batches, want)


def test_device_form_small(small):
    batches, encs, want = small
    _check_device(batches, encs, want)
    assert _device(encs, want.size)[0] == _host(encs)[1]


def test_device_form_large(large):
    batches, encs, want = large
    _check_device(batches, encs, want)
    assert _device(encs, want.size)[0] == _host(encs)[1]


# ---- 4. window edges ---------------------------------------------------------------------------
def _stepped_lengths(mis, windows):
    """tests/native/batchscan_host.cpp's stepped batch: with the batch at
    misalignment mis, a length prefix `split` bytes before window edge k for
    (k, split) = (1, 1) .. (7, 7), (8, 1), ...; between the edges the lengths
    step by one, so the prefixes visit every residue mod 16."""
    lens, pos, step = [], mis + 12, 0
    for k in range(1, windows + 1):
        target = k * W - ((k - 1) % 7 + 1)
        while pos + 8 + step + 8 + 120 <= target:
            lens.append(step)
            pos += 8 + step
            step = (step + 1) % 200
        lens.append(target - pos - 8)
        pos = target
    return lens + [97]


def test_window_edges_device_form(hsv, oracle_lib):
    from hsverify import wire
    base, at, batches, encs = 3, 0, [], []
    for k, windows in enumerate((8, 15, 9)):
        mis = (base + at) % 16
        lens = _stepped_lengths(mis, windows)
        prefixes = mis + 12 + np.cumsum([0] + [8 + n for n in lens[:-1]])
        assert set(prefixes % 16) == set(range(16))
        assert {W - int(p % W) for p in prefixes if W - p % W < 8} == set(range(1, 8))
        txs = _signed(lens, 40 + k, bad=(len(lens) - 1,) if k == 1 else ())
        enc = wire.encode_batch(txs)
        assert len(enc) >= 3 * W
        batches.append(txs)
        encs.append(enc)
        at += len(enc)
    want = _want_flags(oracle_lib, sum(batches, []))
    assert (want & o.STRICT_OK).any() and not (want & o.STRICT_OK).all()
    res, flags = _device(encs, want.size, base=base)
    assert res == _want_results(batches, want)
    assert (flags == want).all(), np.nonzero(flags != want)[0][:8]
    rc, hres, hflags = _host(encs, base=base)
    assert hres == res and (hflags[:want.size] == want).all()


# ---- 5. malformed batches between good ones, device form ------------------------------------------
def test_malformed_batches_leave_their_neighbours_alone(hsv, oracle_lib):
    from hsverify import wire
    a = _signed([136, 200, 96, 513], 50)
    z = _signed([300, 136, 137], 51, bad=(1,))
    mid = _signed([150, 160], 52)
    enc = wire.encode_batch(mid)
    count_too_large = enc[:4] + struct.pack("<Q", (len(enc) - 12) // 8 + 1) + enc[12:]
    # the last length runs 40 bytes into the next batch, whose bytes would make it a fine transaction
    second = 12 + 8 + 150
    into_next = enc[:second] + struct.pack("<Q", 160 + 40) + enc[second + 8:]
    in_prefix = enc[:second + 5]                      # truncated inside the second length prefix
    high_bits = enc[:second] + struct.pack("<Q", 160 | (1 << 63)) + enc[second + 8:]
    wraps = enc[:second] + struct.pack("<Q", 2 ** 64 - 8) + enc[second + 8:]  # prefix + length wraps to the prefix
    encs = [wire.encode_batch(a), count_too_large, into_next, in_prefix, high_bits, wraps, wire.encode_batch(z)]
    batches = [a, None, None, None, None, None, z]
    want = _want_flags(oracle_lib, a + z)
    exp = _want_results(batches, want)
    assert [e[0] for e in exp] == [OK, PARSE, PARSE, PARSE, PARSE, PARSE, TX] and exp[-1][1] == 1
    for fill in (0x00, 0xff, 0xA5):  # the bytes around d_bufs change no result
        res, flags = _device(encs, want.size + 5, fill=fill)
        assert res == exp, (fill, res, exp)
        assert (flags[:want.size] == want).all() and not flags[want.size:].any()
    assert _host(encs)[1] == exp
    # decreasing d_offsets: that batch alone is malformed (the claimed lengths: good, -20, +20 more, good)
    two = [wire.encode_batch(a), wire.encode_batch(z)]
    res, _ = _device([two[0], b"", b"", two[1]], want.size, lengths=[len(two[0]), -20, 20, len(two[1])])
    assert [r[0] for r in res] == [OK, PARSE, PARSE, TX]


# ---- 6. committee routes ---------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_committee_routes(small, large, compact):
    """K = 4: SEEDS[0..3] are members, SEEDS[4..7] strangers, so about half of
    the signers take the comb pass and half the generic pass."""
    from hsverify.committee import Committee
    keys = np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in SEEDS[:4]])
    with Committee(keys, compact=compact) as c:
        assert c.digit_bits == (4 if compact else 8)
        for batches, encs, want in (small, large):
            exp = _want_results(batches, want)
            rc, res, flags = _host(encs, committee=c)
            assert res == exp and rc == sum(e[0] == OK for e in exp)
            assert (flags[:want.size] == want).all(), np.nonzero(flags[:want.size] != want)[0][:8]
            res, flags = _device(encs, want.size + 3, committee=c)
            assert res == exp
            assert (flags[:want.size] == want).all() and not flags[want.size:].any()
