"""Whole messages by member index (hsv_committee_verify_msgs_indexed*).

The caller names each item's signer by its index in the committee, as
hsv_committee_verify* does, so there is no lookup and no route for strangers
(DESIGN.md 4m): at most 2^12 items on a committee with 8-bit tables take ONE
launch of the latency form (hsv_cmsg_quad_kernel), everything else a round of
two launches (hsv_cmsg_index_kernel and the comb pass).  The flags must be those
of hsv_verify_msgs* for (member's key bytes, sig, message) bit for bit, so every
case is compared with the C oracle or the committed golden flags, and with
hsv_committee_verify_msgs_device and hsv_verify_msgs_device on the same bytes.
The cases run through both routes by hsv_test_cmsg_indexed_form: quad and bulk
on a full committee, bulk on a compact one.  The whole module runs on
libhsv_test.so, which exports the hooks.
"""
import ctypes

import numpy as np
import pytest

import ed25519_ref as o
from test_verify_msgs import oracle_msgs, run_device, sign_ragged

pytestmark = pytest.mark.gpu

# the 64-byte head R || A leaves 64 message bytes in block 0; one padded block
# holds up to 47 message bytes, two up to 175, three up to 303
BOUNDARY_LENS = (0, 1, 47, 48, 63, 64, 65, 175, 176, 191, 192, 193, 303, 304, 1000)
SEEDS = np.random.default_rng(2026).integers(0, 256, (8, 32), dtype=np.uint8)
# (compact committee, forced form): quad and bulk on full tables, bulk on compact ones
ROUTES = ((False, 1), (False, 0), (True, 0))


@pytest.fixture(scope="module", autouse=True)
def tlib(hsv):
    from hsverify import _testing
    with _testing.test_library() as lib:
        yield lib
        _testing.cmsg_indexed_form(-1)


@pytest.fixture(scope="module")
def keys():
    return np.stack([np.frombuffer(o.public_key(bytes(s)), np.uint8) for s in SEEDS])


@pytest.fixture(scope="module")
def committees(keys):
    """{compact: Committee} over the eight keys of SEEDS"""
    from hsverify.committee import Committee
    cs = {False: Committee(keys), True: Committee(keys, compact=True)}
    yield cs
    for c in cs.values():
        c.close()


class forced:
    """the route forced for a block, the product's rule afterwards"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from hsverify import _testing
        _testing.cmsg_indexed_form(self.mode)

    def __exit__(self, *exc):
        from hsverify import _testing
        _testing.cmsg_indexed_form(-1)


def _device(c, idx, sig, buf, offsets=None, shift=3, msg_len=0, msg_stride=None, stream=None):
    """The device form with the message bytes `shift` bytes into an allocation,
    the flags pre-filled with ones and one guard byte past m: (flags, fault words)."""
    import torch
    dev = torch.device("cuda:0")
    m = len(idx)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    backing = torch.zeros(buf.size + shift + 16, dtype=torch.uint8, device=dev)
    backing[shift:shift + buf.size].copy_(torch.from_numpy(np.array(buf, dtype=np.uint8)))
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev) if offsets is not None else None
    flags = torch.full((m + 1,), 0xff, dtype=torch.uint8, device=dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, np.uint32).view(np.int32).copy()).to(dev)
    c.verify_msgs_indexed_device(d_idx, torch.from_numpy(sig.copy()).to(dev), backing[shift:], d_off, msg_len=msg_len,
                                 msg_stride=msg_stride, flags=flags[:m], stream=stream, fault=fault)
    torch.cuda.synchronize()
    got = flags.cpu().numpy()
    assert got[m] == 0xff, "the byte past m was written"
    return got[:m], fault.cpu().tolist()


def _both_routes(cs, idx, sig, buf, exp, **kw):
    """exp from each of the three routes, no fault word"""
    for compact, mode in ROUTES:
        with forced(mode):
            got, fault = _device(cs[compact], idx, sig, buf, **kw)
        assert (got == exp).all(), (compact, mode, np.nonzero(got != exp)[0][:8], got[got != exp][:8])
        assert fault == [0, 0], (compact, mode)


def _older_calls(c, pk, sig, buf, exp, **kw):
    """hsv_verify_msgs_device and hsv_committee_verify_msgs_device give exp on the same bytes"""
    import torch
    flags, _, fault = run_device(pk, sig, np.asarray(buf, np.uint8).reshape(-1), **kw)
    assert (flags == exp).all() and fault == [0, 0]
    dev = torch.device("cuda:0")
    shift = kw.pop("shift", 0)
    offsets = kw.pop("offsets", None)
    b = np.asarray(buf, np.uint8).reshape(-1)
    backing = torch.zeros(b.size + shift + 16, dtype=torch.uint8, device=dev)
    backing[shift:shift + b.size].copy_(torch.from_numpy(b.copy()))
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev) if offsets is not None else None
    out = torch.full((len(exp) + 1,), 0xff, dtype=torch.uint8, device=dev)
    c.verify_msgs_device(torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev), backing[shift:],
                         d_off, flags=out[:len(exp)], **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:-1] == exp).all() and got[-1] == 0xff


def _signed(key_ids, msgs):
    """(pk, sig) of msgs[i] under SEEDS[key_ids[i]]"""
    return sign_ragged(SEEDS[np.asarray(key_ids)], msgs)


# ---- 1. the golden edge vectors by member index -------------------------------------------
def test_golden_edge_vectors(golden):
    from hsverify.committee import Committee
    n = golden["n_edge"]
    assert n == 145
    pk, sig = golden["pk"][:n].copy(), golden["sig"][:n].copy()
    msg = np.ascontiguousarray(golden["msg"][:n]).reshape(-1)
    want = golden["flags"][:n]
    distinct = list(dict.fromkeys(bytes(p) for p in pk))
    where = {k: i for i, k in enumerate(distinct)}
    idx = np.array([where[bytes(p)] for p in pk], np.uint32)
    assert (want & o.A_OK == 0).any() and (want & o.SMALL_A).any()    # such keys are members
    karr = np.frombuffer(b"".join(distinct), np.uint8).reshape(-1, 32)
    cs = {False: Committee(karr), True: Committee(karr, compact=True)}
    try:
        for m in (1, 3, 4, 5, 8, 9, 145):          # 4 votes per block: edges at 4 / 5 and 8 / 9
            _both_routes(cs, idx[:m], sig[:m], msg[:32 * m], want[:m], msg_len=32)
        offsets = np.arange(n + 1, dtype=np.uint64) * 32
        _both_routes(cs, idx, sig, msg, want, offsets=offsets, shift=7)
        _older_calls(cs[False], pk, sig, msg, want, msg_len=32)
        for c in cs.values():
            assert (c.verify_msgs_indexed(idx, sig, (msg, offsets)) == want).all()    # the host form
        # an index >= size and 0xffffffff: flags 0, the neighbours exact
        honest = np.nonzero(want & o.STRICT_OK)[0][:2]
        bad_idx, exp = idx.copy(), want.copy()
        bad_idx[honest[0]], bad_idx[honest[1]] = len(distinct), 0xFFFFFFFF
        exp[honest] = 0
        _both_routes(cs, bad_idx, sig, msg, exp, msg_len=32)
        for c in cs.values():
            assert (c.verify_msgs_indexed(bad_idx, sig, (msg, offsets)) == exp).all()
    finally:
        for c in cs.values():
            c.close()


# ---- 2. block boundaries of the 64-byte head ---------------------------------------------
@pytest.fixture(scope="module")
def boundary(oracle_lib, keys):
    """one item per length of BOUNDARY_LENS, honest and corrupted in turn, and the oracle's flags"""
    rnd = np.random.default_rng(71)
    msgs = [rnd.integers(0, 256, n, dtype=np.uint8).tobytes() for n in BOUNDARY_LENS]
    kid = np.arange(len(msgs)) % 8
    pk, sig = _signed(kid, msgs)
    for i in range(2, len(msgs), 3):               # every third: a flipped last message byte (s where empty)
        if msgs[i]:
            msgs[i] = msgs[i][:-1] + bytes([msgs[i][-1] ^ 1])
        else:
            sig[i, 33] ^= 1
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    bad = np.zeros(len(msgs), bool)
    bad[2::3] = True
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all() and (pk == keys[kid]).all()
    return {"idx": kid.astype(np.uint32), "pk": pk, "sig": sig, "msgs": msgs, "exp": exp}


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_block_boundaries(boundary, committees, shift):
    from hsverify import verifier
    idx, pk, sig, msgs, exp = (boundary[k] for k in ("idx", "pk", "sig", "msgs", "exp"))
    for i, msg in enumerate(msgs):                 # each length alone
        _both_routes(committees, idx[i:i + 1], sig[i:i + 1], np.frombuffer(msg, np.uint8), exp[i:i + 1], shift=shift,
                     offsets=np.array([0, len(msg)], np.uint64))
    buf, offsets = verifier.pack_msgs(msgs)        # all together, ragged
    _both_routes(committees, idx, sig, buf, exp, offsets=offsets, shift=shift)
    _older_calls(committees[False], pk, sig, buf, exp, offsets=offsets, shift=shift)
    for c in committees.values():
        assert (c.verify_msgs_indexed(idx, sig, msgs) == exp).all()


# ---- 3. the hash wave's trip count is the block's longest message ------------------------
@pytest.mark.parametrize("slot", [0, 3])
def test_one_long_message_in_a_block(oracle_lib, committees, slot):
    from hsverify import verifier
    rnd = np.random.default_rng(72 + slot)
    m = 6                                          # blocks of 4: a partial last block
    lens = [32] * m
    lens[slot] = 65536
    lens[4 if slot else 5] = 4096                  # in the partial block
    msgs = [rnd.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    kid = (np.arange(m) * 3) % 8
    pk, sig = _signed(kid, msgs)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp & o.STRICT_OK).all()
    buf, offsets = verifier.pack_msgs(msgs)
    _both_routes(committees, kid, sig, buf, exp, offsets=offsets, shift=5)
    flipped = np.array(buf, dtype=np.uint8)
    flipped[int(offsets[slot + 1]) - 1] ^= 0x80      # the long message's last byte
    msgs2 = list(msgs)
    msgs2[slot] = flipped[int(offsets[slot]):int(offsets[slot + 1])].tobytes()
    exp2 = oracle_msgs(oracle_lib, pk, sig, msgs2)
    assert not exp2[slot] & o.EQ_OK and (np.delete(exp2, slot) == np.delete(exp, slot)).all()
    _both_routes(committees, kid, sig, flipped, exp2, offsets=offsets, shift=5)
    _older_calls(committees[False], pk, sig, flipped, exp2, offsets=offsets, shift=5)


# ---- 4. one shared message, and a fixed length at a wider stride -------------------------
@pytest.mark.parametrize("length", [0, 32, 200])
def test_one_shared_message(oracle_lib, committees, length):
    rnd = np.random.default_rng(80 + length)
    m = 67
    msg = rnd.integers(0, 256, length, dtype=np.uint8)
    kid = np.arange(m) % 8
    pk, sig = _signed(kid, [msg.tobytes()] * m)
    sig[5, 33] ^= 1
    sig[8, 2] ^= 1
    exp = oracle_msgs(oracle_lib, pk, sig, [msg.tobytes()] * m)
    assert (exp & o.STRICT_OK).sum() == m - 2
    _both_routes(committees, kid, sig, msg, exp, shift=3, msg_len=length, msg_stride=0)
    _older_calls(committees[False], pk, sig, msg, exp, shift=3, msg_len=length, msg_stride=0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for c in committees.values():                  # the host form, stride 0
        got = np.full(m, 0xee, np.uint8)
        assert c._lib.hsv_committee_verify_msgs_indexed(c._h, p(kid.astype(np.uint32)), p(sig),
                                                        p(msg) if length else None, None, length, 0, m, p(got)) == 0
        assert (got == exp).all()


def test_fixed_length_at_a_wider_stride(oracle_lib, committees):
    rnd = np.random.default_rng(81)
    m, length, stride = 131, 100, 128
    rows = rnd.integers(0, 256, (m, stride), dtype=np.uint8)
    msgs = [rows[i, :length].tobytes() for i in range(m)]
    kid = (np.arange(m) * 5) % 8
    pk, sig = _signed(kid, msgs)
    rows[7, length - 1] ^= 1                       # a message byte
    rows[9, length] ^= 1                           # a byte between two messages: nothing changes
    msgs[7] = rows[7, :length].tobytes()
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp & o.STRICT_OK).sum() == m - 1 and not exp[7] & o.EQ_OK
    _both_routes(committees, kid, sig, rows, exp, shift=9, msg_len=length, msg_stride=stride)
    _older_calls(committees[False], pk, sig, rows, exp, shift=9, msg_len=length, msg_stride=stride)


# ---- 5. the index decides the key ---------------------------------------------------------
def test_wrong_member_and_a_key_listed_twice(oracle_lib, keys):
    from hsverify.committee import Committee
    from hsverify import verifier
    rnd = np.random.default_rng(82)
    m = 21
    msgs = [rnd.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rnd.integers(0, 300, m)]
    kid = np.arange(m) % 8
    _, sig = _signed(kid, msgs)
    twice = np.concatenate([keys, keys[2:3]])      # member 8 is member 2 again
    idx = kid.astype(np.uint32)
    idx[3] = 4                                     # an honest signature under another member's index
    idx[10] = 8                                    # key 2 through its second index
    pk = twice[idx]
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert not exp[3] & o.EQ_OK and exp[3] & o.PARSE_OK and (np.delete(exp, 3) & o.STRICT_OK).all()
    buf, offsets = verifier.pack_msgs(msgs)
    cs = {False: Committee(twice), True: Committee(twice, compact=True)}
    try:
        _both_routes(cs, idx, sig, buf, exp, offsets=offsets, shift=1)
        first = idx.copy()
        first[idx == 8] = 2
        _both_routes(cs, first, sig, buf, exp, offsets=offsets, shift=1)
    finally:
        for c in cs.values():
            c.close()


# ---- 6. decreasing offsets -----------------------------------------------------------------
def test_decreasing_offsets(oracle_lib, committees):
    from hsverify import _lib, verifier
    rnd = np.random.default_rng(83)
    first = [rnd.integers(0, 256, 40 + 13 * i, dtype=np.uint8).tobytes() for i in range(5)]
    # items 0..4 lie back to back; item 5 runs from the end of item 4 back to byte 0; items 6..10 sign
    # the bytes of items 0..4 again under other keys, so every neighbour of item 5 keeps an honest range
    msgs = first + [b""] + first
    m = len(msgs)
    kid = (np.arange(m) * 3) % 8
    pk, sig = _signed(kid, msgs)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp & o.STRICT_OK).all()
    buf, off5 = verifier.pack_msgs(first)
    off = np.concatenate([off5, off5]).astype(np.uint64)
    assert off[5] > off[6] and len(off) == m + 1
    exp[5] = 0
    _both_routes(committees, kid, sig, buf, exp, offsets=off, shift=2)
    for c in committees.values():
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            c.verify_msgs_indexed(kid, sig, (buf, off))


# ---- 7. the product's routing ---------------------------------------------------------------
def test_product_routing(oracle_lib, committees):
    from hsverify import _lib, _testing
    rnd = np.random.default_rng(84)
    msg = rnd.integers(0, 256, 32, dtype=np.uint8)
    kid = np.arange(4097) % 8
    pk, sig = _signed(kid, [msg.tobytes()] * 4097)
    exp = oracle_msgs(oracle_lib, pk[:8], sig[:8], [msg.tobytes()] * 8)
    assert (exp & o.STRICT_OK).all()
    full, compact = committees[False], committees[True]
    pkc = np.ascontiguousarray(pk[:5])
    full.verify_msgs(pkc, sig[:5], [msg.tobytes()] * 5)
    older = _testing.committee_msgs_counts()
    _testing.cmsg_indexed_form(-1)
    for m in (1, 67, 667, 4096):
        before = _testing.cmsg_indexed_counts()
        got, fault = _device(full, kid[:m], sig[:m], msg, msg_len=32, msg_stride=0)
        after = _testing.cmsg_indexed_counts()
        assert (got & o.STRICT_OK).all() and fault == [0, 0]
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, 0, 0), (m, before, after)
    before = _testing.cmsg_indexed_counts()
    got, fault = _device(full, kid, sig, msg, msg_len=32, msg_stride=0)
    after = _testing.cmsg_indexed_counts()
    assert (got & o.STRICT_OK).all() and fault == [0, 0]
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, 1, 4097)
    before = after
    bad = kid[:5].astype(np.uint32)
    bad[1] = 8                                     # out of range: not on the hit list
    got, fault = _device(compact, bad, sig[:5], msg, msg_len=32, msg_stride=0)
    after = _testing.cmsg_indexed_counts()
    assert got[1] == 0 and (np.delete(got, 1) & o.STRICT_OK).all()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, 1, 4)
    with forced(1):                                # the latency form needs 8-bit tables
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            _device(compact, kid[:5], sig[:5], msg, msg_len=32, msg_stride=0)
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            compact.verify_msgs_indexed(kid[:5], sig[:5], [msg.tobytes()] * 5)
    assert _testing.cmsg_indexed_counts() == after
    assert _testing.committee_msgs_counts() == older    # the pk-addressed call's hook: untouched


# ---- 8. larger shapes, the product's route -------------------------------------------------
def test_larger_shapes(oracle_lib, committees):
    import torch
    from hsverify import verifier
    rnd = np.random.default_rng(85)
    m = (1 << 12) + 1
    lens = rnd.choice(np.array([0, 32, 100, 416]), m, p=[0.1, 0.5, 0.2, 0.2])
    msgs = [rnd.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    kid = rnd.integers(0, 8, m)
    pk, sig = _signed(kid, msgs)
    corrupt = rnd.random(m) < 0.2
    for i in np.nonzero(corrupt)[0]:
        sig[i, int(rnd.integers(0, 64))] ^= 1 << int(rnd.integers(0, 8))
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert 0.1 * m < (exp & o.STRICT_OK == 0).sum() <= corrupt.sum()
    buf, offsets = verifier.pack_msgs(msgs)
    for c in committees.values():
        got, fault = _device(c, kid, sig, buf, offsets=offsets, shift=11)
        assert (got == exp).all() and fault == [0, 0]
    # 2^22 + 65 items tiled from 1000 of these, across the round boundary, against the pk-addressed call
    dev = torch.device("cuda:0")
    big = (1 << 22) + 65
    pick = np.nonzero(lens == 32)[0][:1000]
    assert pick.size == 1000
    tile = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).repeat(big // 1000 + 1, 1)[:big].contiguous()
    d_idx = tile(kid[pick].astype(np.int32)[:, None]).reshape(-1)
    d_sig, d_pk = tile(sig[pick]), tile(pk[pick])
    d_msg = tile(np.stack([np.frombuffer(msgs[i], np.uint8) for i in pick]))
    c = committees[False]
    a = torch.full((big + 1,), 0xff, dtype=torch.uint8, device=dev)
    b = torch.full((big + 1,), 0xff, dtype=torch.uint8, device=dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    c.verify_msgs_indexed_device(d_idx, d_sig, d_msg, msg_len=32, flags=a[:big], fault=fault)
    c.verify_msgs_device(d_pk, d_sig, d_msg, msg_len=32, flags=b[:big])
    torch.cuda.synchronize()
    assert torch.equal(a, b) and int(a[big]) == 0xff and fault.cpu().tolist() == [0, 0]
    assert (a[:1000].cpu().numpy() == exp[pick]).all()


# ---- 9. two streams, two committees, the older calls beside them ----------------------------
def test_two_streams_and_the_older_calls(oracle_lib, committees, keys):
    import torch
    from hsverify import verifier
    from hsverify.committee import Committee
    rnd = np.random.default_rng(86)
    m = 300
    msgs = [rnd.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rnd.integers(0, 500, m)]
    kid = rnd.integers(0, 8, m)
    pk, sig = _signed(kid, msgs)
    sig[::7, 40] ^= 4
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    buf, offsets = verifier.pack_msgs(msgs)
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d_sig, d_buf, d_off, d_pk = d(sig), d(buf), d(offsets.view(np.int64)), d(pk)
    digests = rnd.integers(0, 256, (m, 32), dtype=np.uint8)
    pk32, sig32 = sign_ragged(SEEDS[kid], [bytes(r) for r in digests])
    exp32 = oracle_msgs(oracle_lib, pk32, sig32, [bytes(r) for r in digests])
    rev = np.ascontiguousarray(keys[::-1])
    with Committee(rev) as c2:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [torch.full((m,), 0xff, dtype=torch.uint8, device=dev) for _ in range(4)]
        faults = [torch.ones(2, dtype=torch.int32, device=dev) for _ in range(4)]
        d_idx1, d_idx2 = d(kid.astype(np.int32)), d((7 - kid).astype(np.int32))
        d_sig32, d_dig = d(sig32), d(digests)
        torch.cuda.synchronize()
        c1 = committees[False]
        for _ in range(3):
            c1.verify_msgs_indexed_device(d_idx1, d_sig, d_buf, d_off, flags=outs[0], stream=s1.cuda_stream,
                                          fault=faults[0])
            c2.verify_msgs_indexed_device(d_idx2, d_sig, d_buf, d_off, flags=outs[1], stream=s2.cuda_stream,
                                          fault=faults[1])
            c1.verify_device(d_idx1, d_sig32, d_dig, outs[2], stream=s2.cuda_stream, fault=faults[2])
            c2.verify_msgs_device(d_pk, d_sig, d_buf, d_off, flags=outs[3], stream=s1.cuda_stream, fault=faults[3])
        torch.cuda.synchronize()
        for i, want in enumerate((exp, exp, exp32, exp)):
            assert (outs[i].cpu().numpy() == want).all(), i
            assert faults[i].cpu().tolist() == [0, 0], i


# ---- 10. the Python call shapes --------------------------------------------------------------
def test_python_call_shapes(boundary, committees):
    import torch
    from hsverify import verifier
    idx, sig, msgs, exp = (boundary[k] for k in ("idx", "sig", "msgs", "exp"))
    c = committees[False]
    buf, offsets = verifier.pack_msgs(msgs)
    assert (c.verify_msgs_indexed(idx, sig, msgs) == exp).all()                   # list of bytes
    assert (c.verify_msgs_indexed(list(idx), sig, (buf, offsets)) == exp).all()   # (array, offsets)
    assert c.verify_msgs_indexed(np.zeros(0, np.uint32), np.zeros((0, 64), np.uint8), []).size == 0
    with pytest.raises(ValueError):
        c.verify_msgs_indexed(idx[:-1], sig, msgs)
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(idx.view(np.int32).copy()).to(dev)
    flags = torch.zeros(len(idx), dtype=torch.uint8, device=dev)
    c.verify_msgs_indexed_device(d_idx, torch.from_numpy(sig.copy()).to(dev), torch.from_numpy(buf.copy()).to(dev),
                                 torch.from_numpy(offsets.view(np.int64).copy()).to(dev), flags=flags)
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() == exp).all()
    with pytest.raises(ValueError):
        c.verify_msgs_indexed_device(d_idx, torch.from_numpy(sig.copy()).to(dev), torch.from_numpy(buf.copy()),
                                     flags=flags)


# ---- 11. the device self-check, once per route ----------------------------------------------
@pytest.mark.parametrize("compact,mode", ROUTES)
def test_self_check_reports_a_wrong_table_entry(boundary, committees, compact, mode):
    from hsverify import _lib, _testing
    idx, sig, msgs, exp = (boundary[k] for k in ("idx", "sig", "msgs", "exp"))
    from hsverify import verifier
    buf, offsets = verifier.pack_msgs(msgs)
    c = committees[compact]
    with forced(mode):
        with _testing.injected_fault(1):
            _, fault = _device(c, idx, sig, buf, offsets=offsets)
            assert fault[0] == 1
            with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_DEVICE_FAULT"):
                c.verify_msgs_indexed(idx, sig, msgs)
        got, fault = _device(c, idx, sig, buf, offsets=offsets)    # injection off: the same call verifies again
        assert (got == exp).all() and fault == [0, 0]
        assert (c.verify_msgs_indexed(idx, sig, msgs) == exp).all()
