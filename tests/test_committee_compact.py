"""Compact committees on the GPU (hsv_committee_create_ex with 4-bit digits:
48 KiB of comb table per key instead of 384 KiB).

A compact committee must answer every call that takes a committee with the
bytes a full one answers over the same keys -- flags, strict bits, fault words
and the hit / miss split -- which are the bytes of the generic calls and of the
oracle.  The generators are those of tests/test_committee_tx.py and
tests/test_verify_msgs.py; every expectation comes from the committed golden
flags or the C oracle.  The whole module runs on libhsv_test.so, which exports
the count and injection hooks.
"""
import numpy as np
import pytest

import ed25519_ref as o
from conftest import oracle_flags, oracle_tx_flags
from test_committee_msgs import _check as _check_msgs, _hits
from test_committee_tx import SEEDS as TX_SEEDS, _check_device as _check_tx, _signed
from test_verify_msgs import oracle_msgs, ragged_batch

pytestmark = pytest.mark.gpu

FULL_BYTES, COMPACT_BYTES = 393216, 49152


@pytest.fixture(scope="module", autouse=True)
def tlib(hsv):
    from hsverify import _testing
    with _testing.test_library() as lib:
        yield lib


def _committee(keys, compact=True):
    from hsverify.committee import Committee
    return Committee(np.ascontiguousarray(keys, np.uint8).reshape(-1, 32), compact=compact)


def _device_votes(c, idx, sig, msg):
    """hsv_committee_verify_device on cuda:0, outputs pre-filled: (flags, fault words)."""
    import torch
    dev = torch.device("cuda:0")
    flags = torch.full((len(idx),), 0xff, dtype=torch.uint8, device=dev)
    fault = torch.zeros(2, dtype=torch.int32, device=dev)
    c.verify_device(torch.from_numpy(idx.astype(np.int32)).to(dev), torch.from_numpy(sig.copy()).to(dev),
                    torch.from_numpy(msg.copy()).to(dev), flags, fault=fault)
    torch.cuda.synchronize()
    return flags.cpu().numpy(), fault.cpu().tolist()


# ---- 4. the golden edge vectors by member index ------------------------------------------
def test_golden_edge_vectors_by_member_index(golden):
    n = golden["n_edge"]
    pk, sig, msg, want = (golden[k][:n] for k in ("pk", "sig", "msg", "flags"))
    keys = list(dict.fromkeys(bytes(k) for k in pk))
    kidx = {k: i for i, k in enumerate(keys)}
    assert (want & o.A_OK == 0).any() and (want & o.SMALL_A).any()      # such keys are members below
    assert (want & o.STRICT_OK).any()
    with _committee(np.frombuffer(b"".join(keys), np.uint8)) as c:
        assert c.digit_bits == 4 and c.table_bytes == len(keys) * COMPACT_BYTES and len(c) == len(keys)
        for m in (1, 63, 64, 65, 257):
            rows = np.arange(m) % n                                      # prefixes, tiled past n_edge
            idx = np.array([kidx[bytes(k)] for k in pk[rows]], np.uint32)
            exp = want[rows].copy()
            if m > 1:
                idx[m // 2] = len(keys) + (m % 3)                        # no such member: flags 0
                exp[m // 2] = 0
            got = c.verify_flags(idx, sig[rows], msg[rows])
            assert (got == exp).all(), (m, [golden["cases"][rows[i]] for i in np.nonzero(got != exp)[0][:8]])
            dgot, fault = _device_votes(c, idx, sig[rows], msg[rows])
            assert (dgot == exp).all(), (m, np.nonzero(dgot != exp)[0][:8])
            assert fault == [0, 0]


# ---- 5. build chunking ----------------------------------------------------------------
@pytest.fixture(scope="module")
def many_keys(oracle_lib):
    """1025 signed digests, one per key, every eighth corrupted, and the
    oracle's flags (computed once, read-only); smaller committees are prefixes."""
    from hsverify import synth, verifier
    n = 1025
    seeds = synth.committee_seeds(n, 11)
    msg = np.random.default_rng(12).integers(0, 256, (n, 32), dtype=np.uint8)
    pk, sig = verifier.sign_many(seeds, msg)
    bad = np.arange(n) % 8 == 3
    rows = np.nonzero(bad)[0]
    sig[rows, 33 + rows % 20] ^= 4                                       # one bit of s
    exp = oracle_flags(oracle_lib, pk, sig, msg)
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
    for a in (pk, sig, msg, exp):
        a.setflags(write=False)
    return pk, sig, msg, exp


@pytest.mark.parametrize("k", [1, 63, 65, 1025])
def test_build_runs(k, many_keys):
    """K = 1025 crosses the 1024-key build run; 63 and 65 the 64-key padding of
    the build grid."""
    pk, sig, msg, exp = many_keys
    with _committee(pk[:k]) as c:
        assert c.digit_bits == 4 and c.table_bytes == k * COMPACT_BYTES
        got = c.verify_flags(np.arange(k, dtype=np.uint32), sig[:k], msg[:k])
        assert (got == exp[:k]).all(), np.nonzero(got != exp[:k])[0][:8]
        # the last key's table is the one a short final run would leave unbuilt
        assert c.index(pk[k - 1]) == k - 1


# ---- 6. transactions ------------------------------------------------------------------
def test_transactions_match_the_oracle_and_a_full_committee(oracle_lib):
    from hsverify import _testing, mempool
    key_ids = np.where(np.arange(1000) % 2 == 0, np.arange(1000) % 3, 3 + np.arange(1000) % 5)
    txs = _signed(131, key_ids)
    buf, offsets = mempool.pack(txs)
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    member = key_ids < 3
    assert (exp[member] & o.STRICT_OK).any() and not (exp[member] & o.STRICT_OK).all()
    assert (exp[~member] & o.STRICT_OK).any()
    keys = np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in TX_SEEDS[:3]])
    hits = int(member.sum())
    counts = {}
    for compact in (False, True):
        with _committee(keys, compact=compact) as c:
            assert c.digit_bits == (4 if compact else 8)
            got = c.verify_transactions(txs)                             # the host form
            assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
            host_counts = _testing.committee_tx_counts()
            counts[compact] = _check_tx(c, buf, exp, (hits, 1000 - hits), offsets=offsets, base=3)
            assert host_counts[:2] == counts[compact][:2]
    assert counts[True] == counts[False]


# ---- 7. whole messages ----------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged1000(oracle_lib):
    """tests/test_committee_msgs.py's batch: 1000 ragged items, each under a key
    of its own, one in eight corrupted, and the oracle's flags."""
    pk, sig, msgs, bad = ragged_batch(51, 1000)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
    for a in (pk, sig, exp):
        a.setflags(write=False)
    return pk, sig, msgs, exp


def test_ragged_messages_match_the_oracle_and_a_full_committee(ragged1000, oracle_lib):
    from hsverify import _testing, verifier
    pk, sig, msgs, exp = ragged1000
    buf, offsets = verifier.pack_msgs(msgs)
    keys = pk[::2]
    hits = _hits(keys, pk)                            # a corrupted item may carry another item's key
    assert 400 < hits < 600
    victim = 86                                       # a member's item in wave 1: its offsets decrease
    off = offsets.copy()
    assert off[victim] > 0
    off[victim + 1] = off[victim] - 1                 # the next message starts one byte early
    want = exp.copy()
    want[victim] = 0
    nxt = buf[int(off[victim + 1]):int(off[victim + 2])].tobytes()
    want[victim + 1] = oracle_lib.oracle_verify_flags(pk[victim + 1].tobytes(), sig[victim + 1].tobytes(), nxt,
                                                      len(nxt))
    assert exp[victim + 1] & o.STRICT_OK and not want[victim + 1] & o.STRICT_OK
    assert (want[[victim - 1, victim + 2]] == exp[[victim - 1, victim + 2]]).all()
    counts = {}
    for compact in (False, True):
        with _committee(keys, compact=compact) as c:
            got = c.verify_msgs(pk, sig, msgs)                           # the host form
            assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
            assert _testing.committee_msgs_counts()[:2] == (hits, 1000 - hits)
            a = _check_msgs(c, pk, sig, buf, exp, (hits, 1000 - hits), offsets=offsets, shift=3)
            b = _check_msgs(c, pk, sig, buf, want, (hits - 1, 1000 - hits), offsets=off, shift=3)
            counts[compact] = (a, b)
    assert counts[True] == counts[False]


@pytest.mark.parametrize("stride", [61, 0], ids=["stride", "shared"])
def test_fixed_length_messages_match_the_oracle_and_a_full_committee(stride, oracle_lib):
    """msg_len bytes per item at a wider stride, and one shared message
    (msg_stride 0): keys 0..2 of 5 are members."""
    from test_verify_msgs import sign_ragged
    rnd = np.random.default_rng(64 + stride)
    n, length = 131, 45
    rows = rnd.integers(0, 256, (n if stride else 1, stride or length), dtype=np.uint8)
    msgs = [rows[i if stride else 0, :length].tobytes() for i in range(n)]
    key_ids = np.arange(n) % 5
    seeds = np.random.default_rng(2025).integers(0, 256, (8, 32), dtype=np.uint8)
    pk, sig = sign_ragged(seeds[key_ids], msgs)
    sig[::9, 2] ^= 8
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp[np.arange(n) % 9 != 0] & o.STRICT_OK).all() and not (exp[::9] & o.STRICT_OK).any()
    hits = int((key_ids < 3).sum())
    keys = np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in seeds[:3]])
    counts = {}
    for compact in (False, True):
        with _committee(keys, compact=compact) as c:
            counts[compact] = _check_msgs(c, pk, sig, rows, exp, (hits, n - hits), shift=5, msg_len=length,
                                          msg_stride=stride)
    assert counts[True] == counts[False]


# ---- 8. the self-check reaches the caller -----------------------------------------------
def test_injected_table_corruption_is_a_device_fault(many_keys):
    """HSV_ERR_DEVICE_FAULT is the library's own code for a failed curve
    self-check of a final point: the hook is a flag in the kernel's arguments
    that makes the first key entry read back as zeros; no memory is touched."""
    from hsverify import _lib, _testing
    pk, sig, msg, exp = many_keys
    n = 300
    idx = np.arange(n, dtype=np.uint32)
    with _committee(pk[:n]) as c:
        assert (c.verify_flags(idx, sig[:n], msg[:n]) == exp[:n]).all()
        with _testing.injected_fault(_testing.INJECT_ZERO_TABLES):
            with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_DEVICE_FAULT"):
                c.verify_flags(idx, sig[:n], msg[:n])
            assert "self-check" in _lib.last_error()
            _, fault = _device_votes(c, idx, sig[:n], msg[:n])
            assert fault[0] != 0
        got = c.verify_flags(idx, sig[:n], msg[:n])
        assert (got == exp[:n]).all()
        dgot, fault = _device_votes(c, idx, sig[:n], msg[:n])
        assert (dgot == exp[:n]).all() and fault == [0, 0]


# ---- 9. side by side --------------------------------------------------------------------
def test_full_and_compact_committees_side_by_side(many_keys):
    import torch
    pk, sig, msg, exp = many_keys
    nk, n = 100, 300
    rows = np.arange(n)
    idx = (rows * 37 % nk).astype(np.int32)                              # every member, out of order
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(idx).to(dev)
    # item i carries the signature of key idx[i] over that key's digest
    d_sig, d_msg = torch.from_numpy(sig[idx].copy()).to(dev), torch.from_numpy(msg[idx].copy()).to(dev)
    want = exp[idx]
    assert (want & o.STRICT_OK).any() and not (want & o.STRICT_OK).all()
    full, compact = _committee(pk[:nk], compact=False), _committee(pk[:nk], compact=True)
    try:
        assert (full.digit_bits, compact.digit_bits) == (8, 4)
        assert (full.table_bytes, compact.table_bytes) == (nk * FULL_BYTES, nk * COMPACT_BYTES)
        outs = []
        for c in (full, compact, full, compact, compact, full):           # alternately, one stream
            f = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            c.verify_device(d_idx, d_sig, d_msg, f, fault=fault)
            outs.append((f, fault))
        torch.cuda.synchronize()
        for f, fault in outs:
            assert (f.cpu().numpy() == want).all() and fault.cpu().tolist() == [0, 0]
        host = sig[idx], msg[idx]
        assert (full.verify_flags(idx, *host) == want).all() and (compact.verify_flags(idx, *host) == want).all()
        full.close()
        assert (compact.verify_flags(idx, *host) == want).all()
        full = _committee(pk[:nk], compact=False)
        compact.close()
        assert (full.verify_flags(idx, *host) == want).all()
    finally:
        full.close()
        compact.close()
