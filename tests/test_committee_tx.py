"""Mempool transactions of known signers (hsv_committee_verify_transactions*).

A transaction whose pk bytes equal a committee member's is verified from the
member's comb table, any other by the generic kernels; which it is, is
decided on the device (route kernel, comb pass, generic pass: DESIGN.md 4g).
The flags must be those of hsv_verify_transactions* bit for bit, so every
case is compared with the C oracle (or the committed golden flags) and with
hsv_verify_transactions* on the same bytes, and the split itself with
hsv_test_committee_tx_counts.  The whole module runs on libhsv_test.so, which
exports that hook.
"""
import hashlib

import numpy as np
import pytest

import ed25519_ref as o
from conftest import oracle_tx_flags

pytestmark = pytest.mark.gpu

FAULT_MATCH = "HSV_ERR_DEVICE_FAULT"


@pytest.fixture(scope="module", autouse=True)
def tlib(hsv):
    from hsverify import _testing
    with _testing.test_library() as lib:
        yield lib


def _committee(keys):
    from hsverify.committee import Committee
    return Committee(np.ascontiguousarray(keys, np.uint8).reshape(-1, 32))


def _pack_bits(strict):
    n = strict.size
    padded = np.zeros((n + 31) // 32 * 32, np.uint32)
    padded[:n] = strict
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def _device(c, buf, offsets=None, tx_size=0, n=None, base=3):
    """The device form on a copy of buf at an odd address, outputs pre-filled
    with ones: (flags, strict words, fault words, (hits, misses, fallback))."""
    import torch
    from hsverify import _testing
    dev = torch.device("cuda:0")
    if n is None:
        n = len(offsets) - 1 if offsets is not None else buf.size // tx_size
    backing = torch.zeros(buf.size + 64, dtype=torch.uint8, device=dev)
    d_txs = backing[base:base + buf.size]
    d_txs.copy_(torch.from_numpy(np.array(buf, dtype=np.uint8)))
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev) if offsets is not None else None
    flags = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    fault = torch.zeros(2, dtype=torch.int32, device=dev)
    c.verify_transactions_device(d_txs, d_off, tx_size=tx_size, n=n, flags=flags, strict_bits=bits, fault=fault)
    torch.cuda.synchronize()
    return (flags.cpu().numpy(), bits.cpu().numpy().view(np.uint32), fault.cpu().numpy(),
            _testing.committee_tx_counts())


def _check_device(c, buf, exp, counts=None, **kw):
    got, words, fault, cnt = _device(c, buf, **kw)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert (words == _pack_bits(exp & o.STRICT_OK)).all()  # every word written, no bit past n
    assert not fault.any()
    if counts is not None:
        assert cnt[:2] == counts, (cnt, counts)
    assert cnt[2] <= cnt[1]
    return cnt


def _pk_of(tx):
    return tx[-96:-64]


SEEDS = np.random.default_rng(2024).integers(0, 256, (8, 32), dtype=np.uint8)


def _signed(seed, key_ids, max_msg=1105):
    """Ragged transactions (lengths 96 .. 1200) signed by SEEDS[key_ids]; about
    1 in 13 with a bad R or s, and one message byte flipped."""
    from hsverify import verifier
    key_ids = np.asarray(key_ids)
    n = key_ids.size
    rnd = np.random.default_rng(seed)
    lens = rnd.integers(0, max_msg, n)
    msgs = [rnd.integers(0, 256, int(m), dtype=np.uint8).tobytes() for m in lens]
    dig = np.stack([np.frombuffer(hashlib.sha512(m).digest()[:32], np.uint8) for m in msgs])
    pk, sig = verifier.sign_many(SEEDS[key_ids], dig)
    sig[::13, 7] ^= 2                      # bad R
    sig[5::29, 40] ^= 1                    # bad s
    txs = [m + pk[i].tobytes() + sig[i].tobytes() for i, m in enumerate(msgs)]
    if n > 6:
        txs[6] = b"\x55" + txs[6]          # message changed -> digest changed
    return txs


@pytest.fixture(scope="module")
def member_keys():
    """SEEDS[0..2] are the committee of the ragged cases, SEEDS[3..] strangers."""
    return np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in SEEDS])


# ---- 1. the golden transactions, three committees ---------------------------------
def test_golden_three_committees(tx_golden, oracle_lib):
    from hsverify import _testing, mempool
    txs, want = tx_golden["txs"], tx_golden["flags"]
    assert len(txs) == 47 and min(len(t) for t in txs) >= 96
    buf, offsets = mempool.pack(txs)
    assert (oracle_tx_flags(oracle_lib, buf, offsets) == want).all()
    assert (mempool.verify_transactions(txs) == want).all()
    pks = [_pk_of(t) for t in txs]
    distinct = list(dict.fromkeys(pks))
    half = set(distinct[::2])
    strangers = np.random.default_rng(5).integers(0, 256, (8, 32), dtype=np.uint8)
    n_half = sum(p in half for p in pks)
    assert 0 < n_half < 47
    for keys, counts in ((pks, (47, 0)), (sorted(half), (n_half, 47 - n_half)), ([bytes(k) for k in strangers], (0, 47))):
        with _committee(np.frombuffer(b"".join(keys), np.uint8)) as c:
            got = c.verify_transactions(txs)  # the host form
            assert (got == want).all(), [(tx_golden["cases"][i], int(got[i])) for i in np.nonzero(got != want)[0]]
            assert _testing.committee_tx_counts()[:2] == counts
            _check_device(c, buf, want, counts, offsets=offsets)


# ---- 2. wave edges ------------------------------------------------------------------
PATTERNS = {
    "all": lambda i: i % 3,
    "none": lambda i: 3 + i % 2,
    "alternating": lambda i: np.where(i % 2 == 0, i % 3, 3 + i % 2),
    "member_in_lane_0": lambda i: np.where(i % 64 == 0, i % 3, 3 + i % 2),
    "stranger_in_lane_63": lambda i: np.where(i % 64 == 63, 3 + i % 2, i % 3),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_wave_edges(pattern, member_keys, oracle_lib):
    from hsverify import mempool
    key_ids = np.asarray(PATTERNS[pattern](np.arange(1000)))
    txs = _signed(100 + len(pattern), key_ids)
    buf, offsets = mempool.pack(txs)
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    assert (mempool.verify_transactions(txs) == exp).all()
    assert (exp[key_ids < 3] & o.STRICT_OK).any() or pattern == "none"
    with _committee(member_keys[:3]) as c:
        for n in (1, 2, 63, 64, 65, 129, 257, 1000):
            hits = int((key_ids[:n] < 3).sum())
            _check_device(c, buf[:int(offsets[n])], exp[:n], (hits, n - hits), offsets=offsets[:n + 1].copy())
        assert (c.verify_transactions(txs) == exp).all()


# ---- 3. short and malformed transactions -----------------------------------------
def test_short_and_malformed(member_keys, oracle_lib):
    from hsverify import _lib, mempool
    key_ids = np.arange(300) % 5
    txs = _signed(7, key_ids)
    txs[10] = txs[10][:50]
    txs[100] = txs[100][:95]
    buf, offsets = mempool.pack(txs)
    offsets[201] = offsets[200] - 5        # transaction 200: decreasing offsets
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    assert exp[10] == 0 and exp[100] == 0 and exp[200] == 0
    assert (exp[[9, 11, 99, 101, 199]] & o.STRICT_OK).all()
    bad = {10, 100, 200}
    hits = sum(1 for i in range(300) if key_ids[i] < 3 and i not in bad)
    with _committee(member_keys[:3]) as c:
        _check_device(c, buf, exp, (hits, 300 - 3 - hits), offsets=offsets)
        out = np.full(300, 0xee, np.uint8)
        p = lambda a: a.ctypes.data
        rc = c._lib.hsv_committee_verify_transactions(c._h, p(buf), p(offsets), 0, 300, p(out))
        assert rc == -3 and "shorter than 96" in _lib.last_error()
        assert (out == 0xee).all()
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            c.verify_transactions_fixed(np.zeros((4, 95), np.uint8))


# ---- 4. keys that are almost a member's ---------------------------------------------
def test_near_member_keys_miss(member_keys, oracle_lib):
    from hsverify import mempool
    key_ids = np.arange(96) % 3
    txs = [bytearray(t) for t in _signed(8, key_ids, max_msg=300)]
    for i, t in enumerate(txs):
        if i % 4 == 1:
            t[-65] ^= 0x80                 # bit 255 of pk
        elif i % 4 == 2:
            t[-65] ^= 0x01                 # byte 31
        elif i % 4 == 3:
            t[-96 + 8] ^= 0x10             # byte 8: the lookup's tag word matches, the key does not
    txs = [bytes(t) for t in txs]
    buf, offsets = mempool.pack(txs)
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    assert (mempool.verify_transactions(txs) == exp).all()
    assert not (exp[np.arange(96) % 4 != 0] & o.STRICT_OK).any()
    with _committee(member_keys[:3]) as c:
        _check_device(c, buf, exp, (24, 72), offsets=offsets)


# ---- 5. lattice fallback among the misses -------------------------------------------
def test_fallback_among_misses(member_keys, oracle_lib):
    from hsverify import _testing, mempool
    n = 12000
    key_ids = np.arange(n) % 8
    txs = _signed(31, key_ids, max_msg=700)
    buf, offsets = mempool.pack(txs)
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    assert (exp & o.STRICT_OK).sum() > n // 2
    prev = _testing.set_lattice_bits(128)
    try:
        with _committee(member_keys[:4]) as c:
            runs = [_device(c, buf, offsets=offsets, base=5) for _ in range(2)]
    finally:
        _testing.set_lattice_bits(prev)
    for got, words, fault, cnt in runs:
        assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
        assert (words == _pack_bits(exp & o.STRICT_OK)).all()
        assert not fault.any()
        assert cnt[:2] == (n // 2, n // 2) and 0 < cnt[2] <= n // 2
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all() and runs[0][3] == runs[1][3]


# ---- 6. fixed size ----------------------------------------------------------------------
@pytest.mark.parametrize("size", [96, 97, 208, 512])
def test_fixed_size(size, oracle_lib):
    from hsverify import mempool, synth
    w = synth.transactions(1000, tx_size=size, seed=size, corrupt_frac=0.05)
    exp = oracle_tx_flags(oracle_lib, w.txs.reshape(-1), tx_size=size, n=w.n)
    assert (mempool.verify_transactions_fixed(w.txs) == exp).all()
    pks = w.txs[:, size - 96:size - 64]
    members = {bytes(k) for k in pks[:500]}
    hits = sum(bytes(k) in members for k in pks)
    with _committee(pks[:500]) as c:
        got = c.verify_transactions_fixed(w.txs)
        assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
        assert ((got & o.STRICT_OK) != 0).tolist() == w.accept.tolist()
        _check_device(c, w.txs.reshape(-1), exp, (hits, 1000 - hits), tx_size=size, n=w.n, base=0)
        _check_device(c, w.txs.reshape(-1), exp, (hits, 1000 - hits), tx_size=size, n=w.n, base=7)


# ---- 7. the 2^22 round boundary ---------------------------------------------------------
def test_round_boundary():
    import torch
    from hsverify import _testing, mempool
    from hsverify.signer import Signer
    dev = torch.device("cuda:0")
    n = (1 << 22) + 65
    seeds = np.random.default_rng(77).integers(0, 256, (64, 32), dtype=np.uint8)
    gen = torch.Generator(device="cpu").manual_seed(3)
    key_idx = torch.randint(0, 64, (n,), generator=gen, dtype=torch.int32).to(dev)
    txs = torch.zeros((n, 96), dtype=torch.uint8, device=dev)
    with Signer(seeds) as s:
        s.sign_transactions_device(txs, key_idx=key_idx)
        pks = s.public_keys()
    txs[::4099, 70] ^= 1                   # one s byte of every 4099th item
    torch.cuda.synchronize()
    words = (n + 31) // 32
    ref_f = torch.zeros(n, dtype=torch.uint8, device=dev)
    ref_b = torch.zeros(words, dtype=torch.int32, device=dev)
    mempool.verify_transactions_device(txs, None, tx_size=96, n=n, flags=ref_f, strict_bits=ref_b)
    got_f = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
    got_b = torch.full((words,), -1, dtype=torch.int32, device=dev)
    fault = torch.zeros(2, dtype=torch.int32, device=dev)
    with _committee(pks[:48]) as c:
        c.verify_transactions_device(txs, None, tx_size=96, n=n, flags=got_f, strict_bits=got_b, fault=fault)
        torch.cuda.synchronize()
        cnt = _testing.committee_tx_counts()
    assert torch.equal(got_f, ref_f) and torch.equal(got_b, ref_b)
    assert not fault.cpu().numpy().any()
    strict = (ref_f & 1).to(torch.int64)
    assert int(strict.sum()) == n - len(range(0, n, 4099)) and not strict[::4099].any()
    hits = int((key_idx < 48).sum())
    assert cnt[:2] == (hits, n - hits) and 0 < hits < n


# ---- 8. idempotence and isolation -------------------------------------------------------
def test_idempotent_and_leaves_the_committee_calls_alone(member_keys, oracle_lib):
    import torch
    from hsverify import mempool, synth
    dev = torch.device("cuda:0")
    # votes by the committee, through the existing device call, before and after
    v = synth.independent_triples(600, seed=12, corrupt_frac=0.05)
    key_ids = np.arange(20000) % 5
    txs = _signed(9, key_ids, max_msg=400)
    buf, offsets = mempool.pack(txs)
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    with _committee(np.concatenate([v.pk, member_keys[:3]])) as c:
        idx = torch.arange(v.n, dtype=torch.int32, device=dev)
        sig, msg = torch.from_numpy(v.sig).to(dev), torch.from_numpy(v.msg).to(dev)

        def votes():
            f = torch.zeros(v.n, dtype=torch.uint8, device=dev)
            c.verify_device(idx, sig, msg, f)
            torch.cuda.synchronize()
            return f.cpu().numpy()

        before = votes()
        assert ((before & 1) != 0).tolist() == v.accept.tolist()
        d_txs = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
        outs = []
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        for st in streams:
            f = torch.full((len(txs),), 0xff, dtype=torch.uint8, device=dev)
            b = torch.full(((len(txs) + 31) // 32,), -1, dtype=torch.int32, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            st.wait_stream(torch.cuda.current_stream(dev))
            c.verify_transactions_device(d_txs, d_off, flags=f, strict_bits=b, stream=st.cuda_stream, fault=fault)
            outs.append((f, b, fault))
        torch.cuda.synchronize()
        for f, b, fault in outs:
            assert (f.cpu().numpy() == exp).all()
            assert (b.cpu().numpy().view(np.uint32) == _pack_bits(exp & o.STRICT_OK)).all()
            assert not fault.cpu().numpy().any()
        assert (votes() == before).all()


# ---- 9. the self-checks reach the caller --------------------------------------------------
def test_injected_table_corruption_is_a_device_fault(member_keys):
    """HSV_ERR_DEVICE_FAULT is the library's own code for a failed curve
    self-check of a final point (the hook makes table entries read back as
    zeros); no memory fault is involved."""
    from hsverify import _lib, _testing
    key_ids = np.arange(500) % 5
    txs = _signed(10, key_ids, max_msg=300)
    with _committee(member_keys[:3]) as members, _committee(np.zeros((0, 32), np.uint8)) as nobody:
        want = members.verify_transactions(txs)
        assert (want & 1).any() and (nobody.verify_transactions(txs) == want).all()
        with _testing.injected_fault(_testing.INJECT_ZERO_TABLES):
            for c in (members, nobody):    # the comb route's check, the generic route's
                with pytest.raises(_lib.HsvLibraryError, match=FAULT_MATCH):
                    c.verify_transactions(txs)
            assert "self-check" in _lib.last_error()
        assert (members.verify_transactions(txs) == want).all()


# ---- 10. the Python call shapes -------------------------------------------------------------
def test_mempool_call_shapes_take_a_committee(tx_golden):
    from hsverify import mempool
    txs = tx_golden["txs"]
    honest = [t for t, case in zip(txs, tx_golden["cases"]) if case.startswith("honest")]
    with _committee(np.frombuffer(b"".join(_pk_of(t) for t in honest), np.uint8)) as c:
        assert mempool.filter_transactions(txs, committee=c) == mempool.filter_transactions(txs) == honest
        assert mempool.verify_batch_transactions(honest, committee=c)
        assert not mempool.verify_batch_transactions(txs, committee=c)
        assert mempool.verify_batch_transactions([], committee=c) is True
