"""Whole messages of known signers (hsv_committee_verify_msgs*).

An item whose pk bytes equal a committee member's is verified from the
member's comb table, any other by the generic kernels; which it is, is
decided on the device (route kernel, comb pass, generic pass: DESIGN.md 4h).
The flags must be those of hsv_verify_msgs* bit for bit, so every case is
compared with the C oracle (or the committed golden flags), with
hsv_verify_msgs* on the same bytes, and the split itself with
hsv_test_committee_msgs_counts.  The whole module runs on libhsv_test.so,
which exports that hook.  The generators are those of tests/test_verify_msgs.py.
"""
import numpy as np
import pytest

import ed25519_ref as o
from test_verify_msgs import MSG_LENS, oracle_msgs, ragged_batch, run_device, sign_ragged

pytestmark = pytest.mark.gpu

FAULT_MATCH = "HSV_ERR_DEVICE_FAULT"
# the fixed key set of the cases that need one: SEEDS[:3] are members, the rest strangers
SEEDS = np.random.default_rng(2025).integers(0, 256, (8, 32), dtype=np.uint8)


@pytest.fixture(scope="module", autouse=True)
def tlib(hsv):
    from hsverify import _testing
    with _testing.test_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def member_keys():
    return np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in SEEDS])


@pytest.fixture(scope="module")
def ragged1000(oracle_lib):
    """1000 ragged items, each under a key of its own, one in eight corrupted,
    and the oracle's flags (computed once, read-only); smaller batches are
    prefixes.  ragged_batch's own claim is kept: corrupted => not STRICT_OK,
    honest => STRICT_OK, so what verifies here rests on the oracle alone."""
    pk, sig, msgs, bad = ragged_batch(51, 1000)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
    for a in (pk, sig, exp):
        a.setflags(write=False)
    return {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}


def _committee(keys):
    from hsverify.committee import Committee
    return Committee(np.ascontiguousarray(keys, np.uint8).reshape(-1, 32))


def _pack_bits(strict):
    n = strict.size
    padded = np.zeros((n + 31) // 32 * 32, np.uint32)
    padded[:n] = strict != 0
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def _hits(keys, pk):
    """items of pk whose 32 bytes are one of keys"""
    members = {bytes(k) for k in np.asarray(keys, np.uint8).reshape(-1, 32)}
    return sum(bytes(p) in members for p in pk)


def _device(c, pk, sig, buf, offsets=None, shift=3, msg_len=0, msg_stride=None, want_flags=True, want_bits=True,
            stream=None):
    """The device form with the message bytes `shift` bytes into an allocation
    (an odd address) and the outputs pre-filled with ones: (flags or None,
    strict words or None, fault words, (hits, misses, fallback items))."""
    import torch
    from hsverify import _testing
    dev = torch.device("cuda:0")
    n = pk.shape[0]
    buf = np.asarray(buf, np.uint8).reshape(-1)
    backing = torch.zeros(buf.size + shift + 16, dtype=torch.uint8, device=dev)
    backing[shift:shift + buf.size].copy_(torch.from_numpy(np.array(buf, dtype=np.uint8)))
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev) if offsets is not None else None
    flags = torch.full((n,), 0xff, dtype=torch.uint8, device=dev) if want_flags else None
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev) if want_bits else None
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    c.verify_msgs_device(torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev), backing[shift:],
                         d_off, msg_len=msg_len, msg_stride=msg_stride, flags=flags, strict_bits=bits, fault=fault,
                         stream=stream)
    torch.cuda.synchronize()
    return (flags.cpu().numpy() if want_flags else None, bits.cpu().numpy().view(np.uint32) if want_bits else None,
            fault.cpu().tolist(), _testing.committee_msgs_counts())


def _check(c, pk, sig, buf, exp, counts=None, **kw):
    """The device form against exp (every flag byte, every strict word with no
    bit past n, no fault word) and the split against counts."""
    flags, words, fault, cnt = _device(c, pk, sig, buf, **kw)
    if flags is not None:
        assert (flags == exp).all(), np.nonzero(flags != exp)[0][:8]
    if words is not None:
        assert (words == _pack_bits(exp & o.STRICT_OK)).all()
    assert fault == [0, 0]
    if counts is not None:
        assert cnt[:2] == counts, (cnt, counts)
    assert cnt[2] <= cnt[1]
    return cnt


def _same_as_generic(pk, sig, buf, exp, **kw):
    """hsv_verify_msgs_device on the same bytes gives exp as well"""
    flags, bits, fault = run_device(pk, sig, np.asarray(buf, np.uint8).reshape(-1), **kw)
    assert (flags == exp).all() and (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]


# ---- 1. the golden edge vectors, three committees -------------------------------------
def test_golden_three_committees(golden):
    from hsverify import _testing, verifier
    n = golden["n_edge"]
    pk, sig = golden["pk"][:n].copy(), golden["sig"][:n].copy()
    msg = np.ascontiguousarray(golden["msg"][:n]).reshape(-1)
    want = golden["flags"][:n]
    offsets = np.arange(n + 1, dtype=np.uint64) * 32
    assert (verifier.verify_msgs(pk, sig, (msg, offsets)) == want).all()
    _same_as_generic(pk, sig, msg, want, msg_len=32)
    distinct = list(dict.fromkeys(bytes(p) for p in pk))
    half = distinct[::2]
    strangers = [bytes(k) for k in np.random.default_rng(5).integers(0, 256, (8, 32), dtype=np.uint8)]
    n_half = _hits(np.frombuffer(b"".join(half), np.uint8), pk)
    assert 0 < n_half < n and _hits(np.frombuffer(b"".join(strangers), np.uint8), pk) == 0
    assert (want & o.A_OK == 0).any() and (want & o.SMALL_A).any()    # such keys become members below
    for keys, counts in ((distinct, (n, 0)), (half, (n_half, n - n_half)), (strangers, (0, n))):
        with _committee(np.frombuffer(b"".join(keys), np.uint8)) as c:
            got = c.verify_msgs(pk, sig, (msg, offsets))                 # the host form
            assert (got == want).all(), [(golden["cases"][i], int(got[i])) for i in np.nonzero(got != want)[0]]
            assert _testing.committee_msgs_counts()[:2] == counts
            _check(c, pk, sig, msg, want, counts, msg_len=32)
            _check(c, pk, sig, msg, want, counts, offsets=offsets, shift=7)


# ---- 2. wave edges ----------------------------------------------------------------------
PATTERNS = {   # the items whose keys are members
    "all": lambda i: np.ones_like(i, bool),
    "none": lambda i: np.zeros_like(i, bool),
    "alternating": lambda i: i % 2 == 0,
    "member_in_lane_0": lambda i: i % 64 == 0,
    "stranger_in_lane_63": lambda i: i % 64 != 63,
}


def test_wave_edges(ragged1000):
    from hsverify import verifier
    pk, sig, msgs, exp = (ragged1000[k] for k in ("pk", "sig", "msgs", "exp"))
    assert set(len(m) for m in msgs) == set(MSG_LENS)
    buf, offsets = verifier.pack_msgs(msgs)
    _same_as_generic(pk, sig, buf, exp, offsets=offsets, shift=3)
    strangers = np.random.default_rng(6).integers(0, 256, (8, 32), dtype=np.uint8)
    seen_hit = seen_miss = False
    for name, pattern in PATTERNS.items():
        keys = pk[pattern(np.arange(1000))] if name != "none" else strangers
        with _committee(keys) as c:
            for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
                hits = _hits(keys, pk[:n])
                seen_hit |= hits > 0
                seen_miss |= hits < n
                args = (c, pk[:n], sig[:n], buf[:int(offsets[n])], exp[:n], (hits, n - hits))
                _check(*args, offsets=offsets[:n + 1].copy(), shift=1 + (n * 7) % 15)
            _check(*args, offsets=offsets, shift=5, want_flags=False)    # d_flags NULL
            _check(*args, offsets=offsets, shift=9, want_bits=False)     # d_strict_bits NULL
            assert (c.verify_msgs(pk, sig, msgs) == exp).all()
    assert seen_hit and seen_miss


# ---- 3. one shared message, and the fixed length / stride form --------------------------
@pytest.mark.parametrize("length", [0, 1, 111, 112, 300])
def test_one_shared_message(length, member_keys, oracle_lib):
    import ctypes
    rnd = np.random.default_rng(60 + length)
    n = 67
    msg = rnd.integers(0, 256, length, dtype=np.uint8)
    key_ids = np.arange(n) % 5                      # keys 0..2 members, 3..4 strangers
    pk, sig = sign_ragged(SEEDS[key_ids], [msg.tobytes()] * n)
    sig[5, 33] ^= 1                                 # a member's item
    sig[8, 33] ^= 1                                 # a stranger's
    exp = oracle_msgs(oracle_lib, pk, sig, [msg.tobytes()] * n)
    assert (exp & o.STRICT_OK).sum() == n - 2 and (pk == member_keys[key_ids]).all()
    hits = int((key_ids < 3).sum())
    _same_as_generic(pk, sig, msg, exp, shift=3, msg_len=length, msg_stride=0)
    with _committee(member_keys[:3]) as c:
        _check(c, pk, sig, msg, exp, (hits, n - hits), shift=3, msg_len=length, msg_stride=0)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        got = np.full(n, 0xee, np.uint8)
        assert c._lib.hsv_committee_verify_msgs(c._h, p(pk), p(sig), p(msg) if length else None, None, length, 0, n,
                                                p(got)) == 0
        assert (got == exp).all()


def test_fixed_length_at_a_wider_stride(member_keys, oracle_lib):
    rnd = np.random.default_rng(61)
    n, length, stride = 131, 45, 61
    rows = rnd.integers(0, 256, (n, stride), dtype=np.uint8)
    msgs = [rows[i, :length].tobytes() for i in range(n)]
    key_ids = np.arange(n) % 4
    pk, sig = sign_ragged(SEEDS[key_ids], msgs)
    sig[::9, 2] ^= 8
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp[np.arange(n) % 9 != 0] & o.STRICT_OK).all() and not (exp[::9] & o.STRICT_OK).any()
    hits = int((key_ids < 3).sum())
    _same_as_generic(pk, sig, rows, exp, shift=5, msg_len=length, msg_stride=stride)
    with _committee(member_keys[:3]) as c:
        _check(c, pk, sig, rows, exp, (hits, n - hits), shift=5, msg_len=length, msg_stride=stride)


# ---- 4. keys that are almost a member's, and a key listed twice ------------------------
def test_near_member_keys_miss_and_the_first_duplicate_wins(member_keys, oracle_lib):
    from hsverify import verifier
    rnd = np.random.default_rng(62)
    n = 100
    key_ids = np.arange(n) % 3
    msgs = [rnd.integers(0, 256, int(rnd.integers(0, 300)), dtype=np.uint8).tobytes() for _ in range(n)]
    pk, sig = sign_ragged(SEEDS[key_ids], msgs)
    for byte, k in ((0, 1), (7, 2), (8, 3), (31, 4)):
        pk[k::5, byte] ^= 0x10 if byte != 31 else 0x80   # items 0, 5, 10, ... keep a member's key
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp[::5] & o.STRICT_OK).all() and not (exp[np.arange(n) % 5 != 0] & o.STRICT_OK).any()
    buf, offsets = verifier.pack_msgs(msgs)
    _same_as_generic(pk, sig, buf, exp, offsets=offsets, shift=3)
    with _committee(member_keys[:3]) as c:
        _check(c, pk, sig, buf, exp, (n // 5, n - n // 5), offsets=offsets)
    twice = np.concatenate([member_keys[:3], member_keys[1:2], member_keys[:1]])
    with _committee(twice) as c:
        assert [c.index(member_keys[k]) for k in range(3)] == [0, 1, 2]
        _check(c, pk, sig, buf, exp, (n // 5, n - n // 5), offsets=offsets)


# ---- 5. lattice fallback among the misses -----------------------------------------------
def test_fallback_among_misses(oracle_lib):
    from hsverify import _testing, verifier
    pk, sig, msgs, bad = ragged_batch(53, 257)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
    buf, offsets = verifier.pack_msgs(msgs)
    keys = pk[::2]
    hits = _hits(keys, pk)
    assert 0 < hits < 257
    with _committee(keys) as c:
        prev = _testing.set_lattice_bits(128)
        try:
            low = _check(c, pk, sig, buf, exp, (hits, 257 - hits), offsets=offsets, shift=9)
            assert (c.verify_msgs(pk, sig, msgs) == exp).all()
        finally:
            _testing.set_lattice_bits(prev)
        assert low[2] > 0                           # about one miss in seven has no short pair at 128 bits
        default = _check(c, pk, sig, buf, exp, (hits, 257 - hits), offsets=offsets, shift=9)
        assert default[2] < low[2]


# ---- 6. one long message among short ones -----------------------------------------------
def test_one_long_message_among_short_ones(member_keys, oracle_lib):
    from hsverify import verifier
    rnd = np.random.default_rng(63)
    n = 130
    msgs = [rnd.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    key_ids = np.arange(n) % 5
    assert key_ids[70] == 0 and key_ids[103] == 3   # a member's long message and a stranger's
    msgs[70] = rnd.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    msgs[103] = rnd.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    pk, sig = sign_ragged(SEEDS[key_ids], msgs)
    sig[3, 40] ^= 1
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp & o.STRICT_OK).sum() == n - 1 and exp[70] & o.STRICT_OK and exp[103] & o.STRICT_OK
    buf, offsets = verifier.pack_msgs(msgs)
    hits = int((key_ids < 3).sum())
    _same_as_generic(pk, sig, buf, exp, offsets=offsets, shift=7)
    with _committee(member_keys[:3]) as c:
        _check(c, pk, sig, buf, exp, (hits, n - hits), offsets=offsets, shift=7)
        buf2 = buf.copy()
        buf2[int(offsets[71]) - 1] ^= 1             # the last byte of the member's long message counts
        exp2 = exp.copy()
        exp2[70] = oracle_lib.oracle_verify_flags(pk[70].tobytes(), sig[70].tobytes(),
                                                  buf2[int(offsets[70]):int(offsets[71])].tobytes(), 1 << 20)
        assert not exp2[70] & o.STRICT_OK
        _check(c, pk, sig, buf2, exp2, (hits, n - hits), offsets=offsets, shift=7)


# ---- 7. decreasing offsets --------------------------------------------------------------
def test_decreasing_offsets(ragged1000, oracle_lib):
    from hsverify import _lib, verifier
    n = 130
    pk, sig, msgs = ragged1000["pk"][:n], ragged1000["sig"][:n], ragged1000["msgs"][:n]
    exp = ragged1000["exp"][:n].copy()
    buf, offsets = verifier.pack_msgs(msgs)
    keys = pk[::2]
    for victim in (21, 86):                         # a stranger's item in wave 0, a member's in wave 1
        off = offsets.copy()
        assert off[victim] > 0
        off[victim + 1] = off[victim] - 1           # the next message starts one byte early
        want = exp.copy()
        want[victim] = 0
        nxt = buf[int(off[victim + 1]):int(off[victim + 2])].tobytes()
        want[victim + 1] = oracle_lib.oracle_verify_flags(pk[victim + 1].tobytes(), sig[victim + 1].tobytes(), nxt,
                                                          len(nxt))
        _same_as_generic(pk, sig, buf, want, offsets=off, shift=5)
        with _committee(keys) as c:
            hits = _hits(keys, np.delete(pk, victim, axis=0))
            assert 0 < hits < n - 1
            flags, words, fault, cnt = _device(c, pk, sig, buf, offsets=off, shift=5)
            assert (flags == want).all(), np.nonzero(flags != want)[0][:8]
            assert flags[victim] == 0 and not (words[victim // 32] >> (victim % 32)) & 1
            assert (words == _pack_bits(want & o.STRICT_OK)).all() and fault == [0, 0]
            assert cnt[:2] == (hits, n - 1 - hits)  # the void item is on no list
            mates = (np.arange(n) != victim) & (np.arange(n) != victim + 1)
            assert (flags[mates] == exp[mates]).all()   # members and strangers of its wave: as without it
            with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
                c.verify_msgs(pk, sig, (buf, off))
            assert "decrease" in _lib.last_error()


# ---- 8. the 2^22 round boundary ---------------------------------------------------------
def test_round_boundary():
    import torch
    from hsverify import _testing, verifier
    from hsverify.signer import Signer
    dev = torch.device("cuda:0")
    n = (1 << 22) + 65
    gen = torch.Generator(device="cpu").manual_seed(4)
    key_idx = torch.randint(0, 4, (n,), generator=gen, dtype=torch.int32).to(dev)
    backing = torch.randint(0, 256, (n * 32 + 16,), generator=gen, dtype=torch.uint8).to(dev)
    d_msgs = backing[1:1 + n * 32]                  # an odd address
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    with Signer(SEEDS[:4]) as s:
        s.sign_device(d_msgs.view(n, 32), d_sig, key_idx=key_idx, msg_len=32)
        pks = s.public_keys()
    d_sig[::4099, 38] ^= 1                          # one s byte of every 4099th item
    d_pk = torch.from_numpy(pks).to(dev)[key_idx.to(torch.int64)].contiguous()
    torch.cuda.synchronize()
    words = (n + 31) // 32
    ref_f = torch.zeros(n, dtype=torch.uint8, device=dev)
    ref_b = torch.zeros(words, dtype=torch.int32, device=dev)
    verifier.verify_msgs_device(d_pk, d_sig, d_msgs, msg_len=32, flags=ref_f, strict_bits=ref_b)
    got_f = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
    got_b = torch.full((words,), -1, dtype=torch.int32, device=dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    with _committee(pks[:3]) as c:
        c.verify_msgs_device(d_pk, d_sig, d_msgs, msg_len=32, flags=got_f, strict_bits=got_b, fault=fault)
        torch.cuda.synchronize()
        cnt = _testing.committee_msgs_counts()
    assert torch.equal(got_f, ref_f) and torch.equal(got_b, ref_b)
    assert fault.cpu().tolist() == [0, 0]
    strict = (ref_f & 1).to(torch.int64)
    assert int(strict.sum()) == n - len(range(0, n, 4099)) and not strict[::4099].any()
    hits = int((key_idx < 3).sum())
    assert cnt[:2] == (hits, n - hits) and 0 < hits < n   # summed over both rounds


# ---- 9. two streams, two committees, and the older calls beside them --------------------
def test_two_streams_and_the_older_committee_calls(member_keys, ragged1000):
    import torch
    from hsverify import _testing, synth, verifier
    dev = torch.device("cuda:0")
    pk, sig, msgs, exp = (ragged1000[k] for k in ("pk", "sig", "msgs", "exp"))
    buf, offsets = verifier.pack_msgs(msgs)
    v = synth.independent_triples(600, seed=12, corrupt_frac=0.05)
    w = synth.transactions(300, tx_size=208, seed=208, corrupt_frac=0.05)
    tx_pks = w.txs[:, 208 - 96:208 - 64]
    with _committee(np.concatenate([v.pk, tx_pks[:150], pk[::2]])) as c1, _committee(pk[1::3]) as c2:
        idx = torch.arange(v.n, dtype=torch.int32, device=dev)
        d_vsig, d_vmsg = torch.from_numpy(v.sig).to(dev), torch.from_numpy(v.msg).to(dev)
        d_txs = torch.from_numpy(w.txs.reshape(-1).copy()).to(dev)

        def older():
            f = torch.zeros(v.n, dtype=torch.uint8, device=dev)
            t = torch.zeros(w.n, dtype=torch.uint8, device=dev)
            c1.verify_device(idx, d_vsig, d_vmsg, f)
            c1.verify_transactions_device(d_txs, None, tx_size=208, n=w.n, flags=t)
            torch.cuda.synchronize()
            return f.cpu().numpy(), t.cpu().numpy(), _testing.committee_tx_counts()

        before = older()
        assert ((before[0] & 1) != 0).tolist() == v.accept.tolist()
        assert ((before[1] & 1) != 0).tolist() == w.accept.tolist() and before[2][0] >= 150
        d_pk, d_sig = torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev)
        backing = torch.zeros(buf.size + 32, dtype=torch.uint8, device=dev)
        backing[11:11 + buf.size].copy_(torch.from_numpy(np.array(buf, dtype=np.uint8)))
        d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
        outs, streams = [], [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        for c, st in zip((c1, c2), streams):
            f = torch.full((1000,), 0xff, dtype=torch.uint8, device=dev)
            b = torch.full((32,), -1, dtype=torch.int32, device=dev)
            fault = torch.ones(2, dtype=torch.int32, device=dev)
            st.wait_stream(torch.cuda.current_stream(dev))
            c.verify_msgs_device(d_pk, d_sig, backing[11:], d_off, flags=f, strict_bits=b, stream=st.cuda_stream,
                                 fault=fault)
            outs.append((f, b, fault))
        torch.cuda.synchronize()
        assert _testing.committee_msgs_counts()[:2] == (_hits(pk[1::3], pk), 1000 - _hits(pk[1::3], pk))
        assert _testing.committee_tx_counts() == before[2]               # the other hook keeps its own slot
        for f, b, fault in outs:
            assert (f.cpu().numpy() == exp).all()
            assert (b.cpu().numpy().view(np.uint32) == _pack_bits(exp & o.STRICT_OK)).all()
            assert fault.cpu().tolist() == [0, 0]
        after = older()
        assert (after[0] == before[0]).all() and (after[1] == before[1]).all() and after[2] == before[2]


# ---- 10. the self-checks reach the caller -----------------------------------------------
def test_injected_table_corruption_is_a_device_fault(ragged1000):
    """HSV_ERR_DEVICE_FAULT is the library's own code for a failed curve
    self-check of a final point (the hook makes table entries read back as
    zeros, held in registers); no memory access changes."""
    from hsverify import _lib, _testing, verifier
    n = 300
    pk, sig, msgs, exp = ragged1000["pk"][:n], ragged1000["sig"][:n], ragged1000["msgs"][:n], ragged1000["exp"][:n]
    buf, offsets = verifier.pack_msgs(msgs)
    with _committee(pk) as members, _committee(np.zeros((0, 32), np.uint8)) as nobody:
        assert (members.verify_msgs(pk, sig, msgs) == exp).all() and (nobody.verify_msgs(pk, sig, msgs) == exp).all()
        with _testing.injected_fault(_testing.INJECT_ZERO_TABLES):
            for c in (members, nobody):             # the comb route's check, the generic route's
                with pytest.raises(_lib.HsvLibraryError, match=FAULT_MATCH):
                    c.verify_msgs(pk, sig, msgs)
                assert "self-check" in _lib.last_error()
                _, _, fault, _ = _device(c, pk, sig, buf, offsets=offsets)
                assert fault[0] == 1
        assert (members.verify_msgs(pk, sig, msgs) == exp).all()         # the hook is off again
        _check(members, pk, sig, buf, exp, (n, 0), offsets=offsets)
        _check(nobody, pk, sig, buf, exp, (0, n), offsets=offsets)


# ---- 11. the Python call shapes ---------------------------------------------------------
def test_python_call_shapes(ragged1000):
    import torch
    from hsverify import verifier
    n = 70
    pk, sig, msgs, exp = ragged1000["pk"][:n], ragged1000["sig"][:n], ragged1000["msgs"][:n], ragged1000["exp"][:n]
    buf, offsets = verifier.pack_msgs(msgs)
    with _committee(pk[::2]) as c:
        assert (c.verify_msgs(pk, sig, msgs) == exp).all()               # a list of bytes
        assert (c.verify_msgs(pk, sig, (buf, offsets)) == exp).all()     # (buffer, offsets)
        assert c.verify_msgs(pk[:0], sig[:0], []).size == 0
        with pytest.raises(ValueError):
            c.verify_msgs(pk, sig, msgs[:-1])
        # the device wrapper's defaults: the current stream, msg_stride = msg_len, no fault words
        dev = torch.device("cuda:0")
        rows = np.stack([np.frombuffer(m[:1].ljust(1, b"\0"), np.uint8) for m in msgs])   # 1-byte messages
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        ref = torch.zeros(n, dtype=torch.uint8, device=dev)
        args = (torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev),
                torch.from_numpy(rows.reshape(-1).copy()).to(dev))
        c.verify_msgs_device(*args, msg_len=1, flags=flags)
        verifier.verify_msgs_device(*args, msg_len=1, flags=ref)
        torch.cuda.synchronize()
        assert torch.equal(flags, ref)
        one = np.array([len(m) == 1 for m in msgs])
        assert one.any() and (flags.cpu().numpy()[one] == exp[one]).all()
