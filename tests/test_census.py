"""The signer census on the GPU (hsv_census_keys*, hsv_census_transactions*):
the distinct 32-byte signer keys of a batch and how often each occurs.

The expected value of every case is a collections.Counter over the key bytes
of the well-formed items; nothing is signed except in the end-to-end case.
The whole module runs on libhsv_test.so, which exports the seed hook
(hsv_test_census_seed) and hsv_test_committee_tx_counts.
"""
import collections
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS = 4096
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def tlib(hsv):
    from hsverify import _testing
    with _testing.test_library() as lib:
        yield lib


def keytab_hash(seed, key):
    """csrc/hsv_keytab.hpp keytab_hash over the key's 32 bytes, restated."""
    h = seed & M64
    for i in range(4):
        w = int.from_bytes(key[8 * i:8 * i + 8], "little")
        h = ((h ^ w) * 0xbf58476d1ce4e5b9) & M64
        h ^= h >> 31
    return h


def _keys(k, seed):
    """k distinct random keys, (k, 32) uint8"""
    return np.random.default_rng(seed).integers(0, 256, (k, 32), dtype=np.uint8)


def _draw(keys, n, seed):
    """(n, 32): every one of the min(len(keys), n) first keys occurs, in a shuffled order"""
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    k = min(len(keys), n)
    return keys[np.random.default_rng(seed).permutation(n) % k]


def _spans(buf, offsets=None, tx_size=0, n=None):
    """the key bytes of each item as the library addresses them, None for a malformed one"""
    out = []
    for i in range(n):
        lo, hi = (int(offsets[i]), int(offsets[i + 1])) if offsets is not None else (i * tx_size, (i + 1) * tx_size)
        out.append(bytes(buf[hi - 96:hi - 64]) if hi >= lo and hi - lo >= 96 else None)
    return out


def _ragged(pks, seed, lo=96, hi=300):
    """transactions of lo..hi bytes around pks: (buffer, offsets)"""
    rnd = np.random.default_rng(seed)
    lens = rnd.integers(lo, hi + 1, len(pks))
    offsets = np.zeros(len(pks) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = rnd.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    for i, pk in enumerate(pks):
        e = int(offsets[i + 1])
        buf[e - 96:e - 64] = pk
    return buf, offsets


def _fixed(pks, size, seed):
    buf = np.random.default_rng(seed).integers(0, 256, (len(pks), size), dtype=np.uint8)
    if len(pks):
        buf[:, size - 96:size - 64] = pks
    return buf.reshape(-1)


class Out:
    """device outputs pre-filled with ones, and what a call left in them"""

    def __init__(self, slots, dev="cuda:0"):
        import torch
        self.slots = slots
        self.keys = torch.full((slots, 32), 0xff, dtype=torch.uint8, device=dev)
        self.counts = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        self.summary = torch.full((6,), -1, dtype=torch.int64, device=dev)

    def read(self):
        s = [int(x) for x in self.summary.cpu().numpy().view(np.uint64)]
        summary = dict(items=s[0], counted=s[1], members=s[2], malformed=s[3], overflow=s[4],
                       distinct=s[5] & 0xffffffff, reserved=s[5] >> 32)
        return self.keys.cpu().numpy(), self.counts.cpu().numpy().view(np.uint32), summary


def _to_device(buf, base=1):
    """a copy of buf on the device at an odd address (a tensor sliced at [base:])"""
    import torch
    backing = torch.zeros(buf.size + 64, dtype=torch.uint8, device="cuda:0")
    t = backing[base:base + buf.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(buf, np.uint8).reshape(-1)))
    assert base % 2 == 0 or buf.size == 0 or t.data_ptr() % 2 == 1
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def census_keys_device(pk, n, out, skip=None, stream=None):
    """hsv_census_keys_device over the rows of a (n, stride) uint8 tensor"""
    import torch
    from hsverify import _lib
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().hsv_census_keys_device(skip._h if skip is not None else None, _p(pk), pk.stride(0) if n else 32, n,
                                            out.slots, _p(out.keys), _p(out.counts), _p(out.summary),
                                            ctypes.c_void_p(stream))
    _lib.check(rc, "hsv_census_keys_device")


def census_tx_device(txs, offsets, tx_size, n, out, skip=None, stream=None):
    from hsverify import mempool
    mempool.census_device(txs, offsets, tx_size=tx_size, n=n, skip=skip, slots=out.slots, keys_out=out.keys,
                          counts_out=out.counts, summary_out=out.summary, stream=stream)


def run_mode(mode, pks, seed, out, skip=None, stream=None):
    """enqueue one census of the keys pks (n, 32) in the given input mode; returns the tensors to keep alive"""
    import torch
    n = len(pks)
    if mode in ("keys32", "keys128"):
        stride = 32 if mode == "keys32" else 128
        rows = np.random.default_rng(seed).integers(0, 256, (max(n, 1), stride), dtype=np.uint8)
        rows[:n, :32] = pks
        t = torch.from_numpy(rows).to("cuda:0")
        census_keys_device(t, n, out, skip, stream)
        return t
    if mode == "ragged":
        buf, offsets = _ragged(pks, seed)
        t, off = _to_device(buf), torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
        census_tx_device(t, off, 0, n, out, skip, stream)
        return t, off
    assert mode == "fixed97"
    t = _to_device(_fixed(pks, 97, seed))
    census_tx_device(t, None, 97, n, out, skip, stream)
    return t


def check_exact(out, want, items, members=0, malformed=0):
    """the outputs hold exactly the Counter `want`, then zeros; the summary adds up"""
    keys, counts, s = out.read()
    d = s["distinct"]
    assert d == len(want), (d, len(want))
    got = {(bytes(keys[j]), int(counts[j])) for j in range(d)}
    assert len(got) == d
    assert got == set(want.items())
    assert not keys[d:].any() and not counts[d:].any()
    assert s["reserved"] == 0 and s["overflow"] == 0
    assert s["items"] == items and s["members"] == members and s["malformed"] == malformed
    assert s["counted"] == sum(want.values())
    assert s["items"] == s["counted"] + s["members"] + s["malformed"] + s["overflow"]


MODES = ["keys32", "keys128", "ragged", "fixed97"]


# ---- 1. wave and block edges --------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("mode", MODES)
def test_wave_and_block_edges(mode, n):
    import torch
    pool = _keys(1000, 11)
    for k in sorted({1, 2, 63, 64, 65, max(n, 1)}):
        pks = _draw(pool[:k], n, 100 * n + k)
        out = Out(SLOTS)
        keep = run_mode(mode, pks, n + k, out)
        torch.cuda.synchronize()
        want = collections.Counter(bytes(p) for p in pks)
        assert len(want) == min(k, n)
        check_exact(out, want, n)
        del keep


# ---- 2. malformed transactions ---------------------------------------------------------
def test_malformed_transactions_are_counted_apart():
    import torch
    rnd = np.random.default_rng(5)
    pool = _keys(6, 21)
    lens = [96] + [int(x) for x in rnd.choice([0, 95, 96, 97, 200], 299)]
    lens[64], lens[65], lens[127], lens[128] = 0, 95, 95, 0
    lens[200] = lens[201] = 97
    offsets = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = rnd.integers(0, 256, int(offsets[-1]) + 400, dtype=np.uint8)
    n = len(lens)
    for i in range(n):
        e = int(offsets[i + 1])
        if lens[i] >= 96:
            buf[e - 96:e - 64] = pool[i % 6]
    # one decreasing pair: item 200 ends before it starts, item 201 spans back up (and is long enough)
    offsets[201] = offsets[200] - 50
    want_keys = _spans(buf, offsets, n=n)
    assert want_keys[0] is not None and int(offsets[0]) == 0 and int(offsets[1]) == 96
    assert want_keys[200] is None and want_keys[201] is not None
    malformed = sum(k is None for k in want_keys)
    assert malformed > 50
    t, off = _to_device(buf), torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    out = Out(SLOTS)
    census_tx_device(t, off, 0, n, out)
    torch.cuda.synchronize()
    check_exact(out, collections.Counter(k for k in want_keys if k is not None), n, malformed=malformed)
    # the host form counts the same
    from hsverify import mempool
    txs = [bytes(buf[int(offsets[i]):int(offsets[i + 1])]) for i in range(200)]
    keys, counts, s = mempool.census(txs, slots=SLOTS)
    want = collections.Counter(k for k in want_keys[:200] if k is not None)
    assert {(bytes(k), int(c)) for k, c in zip(keys, counts)} == set(want.items())
    assert s["malformed"] == sum(k is None for k in want_keys[:200]) and s["items"] == 200


# ---- 3. contention -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("mode", ["keys32", "fixed97"])
def test_contention_on_few_keys(mode, k):
    import torch
    n = 1 << 16
    pks = _draw(_keys(k, 31), n, 32)
    out = Out(SLOTS)
    keep = run_mode(mode, pks, 33, out)
    torch.cuda.synchronize()
    want = collections.Counter(bytes(p) for p in pks)
    assert len(want) == k and sum(want.values()) == n
    check_exact(out, want, n)
    del keep


# ---- 4. a collision cluster that wraps ----------------------------------------------------------
@pytest.mark.parametrize("seed", [0x9e3779b97f4a7c15, 0x0123456789abcdef])
def test_cluster_wraps_past_the_table_end(seed):
    import torch
    from hsverify import _testing
    rnd = np.random.default_rng(7)
    cluster = []
    while len(cluster) < 8:
        key = rnd.integers(0, 256, 32, dtype=np.uint8)
        if keytab_hash(seed, bytes(key)) & 15 == 13:
            cluster.append(key)
    pks = _draw(np.stack(cluster), 8 * 37, 9)
    _testing.census_seed(seed)
    try:
        out = Out(16)
        keep = run_mode("keys32", pks, 1, out)
        torch.cuda.synchronize()
    finally:
        _testing.census_seed(0)
    want = collections.Counter(bytes(p) for p in pks)
    assert len(want) == 8
    check_exact(out, want, len(pks))
    del keep


# ---- 5. overflow -----------------------------------------------------------------------------
def test_overflow_keeps_its_invariants():
    import torch
    pks = _keys(1000, 41)
    assert len({bytes(p) for p in pks}) == 1000
    out = Out(16)
    keep = run_mode("keys32", pks, 2, out)  # returns HSV_OK (census_keys_device checks the code)
    torch.cuda.synchronize()
    keys, counts, s = out.read()
    d = s["distinct"]
    assert 0 < d <= 16
    given = {bytes(p) for p in pks}
    written = [bytes(keys[j]) for j in range(d)]
    assert len(set(written)) == d and set(written) <= given
    assert (counts[:d] == 1).all()
    assert not keys[d:].any() and not counts[d:].any()
    assert s["counted"] == d and s["counted"] + s["overflow"] == 1000
    assert s["items"] == 1000 and s["members"] == 0 and s["malformed"] == 0
    del keep


# ---- 6. leaving a committee's members out ---------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
def test_skip_records_only_strangers(hsv, compact):
    import torch
    from hsverify.committee import Committee
    seeds = np.random.default_rng(51).integers(0, 256, (8, 32), dtype=np.uint8)
    members = np.zeros((8, 32), np.uint8)
    for i in range(8):
        assert hsv.hsv_public_key(ctypes.c_void_p(seeds[i].ctypes.data), ctypes.c_void_p(members[i].ctypes.data)) == 0
    strangers = _keys(5, 52)
    pks = _draw(np.concatenate([members, strangers]), 700, 53)
    is_member = np.array([bytes(p) in {bytes(m) for m in members} for p in pks])
    for mode in ("keys32", "ragged"):
        with Committee(members, compact=compact) as c:
            assert c.digit_bits == (4 if compact else 8)
            out = Out(SLOTS)
            keep = run_mode(mode, pks, 54, out, skip=c)
            torch.cuda.synchronize()
            want = collections.Counter(bytes(p) for p in pks[~is_member])
            assert len(want) == 5
            check_exact(out, want, 700, members=int(is_member.sum()))
            # an empty committee leaves nobody out
        with Committee(np.zeros((0, 32), np.uint8)) as empty:
            out = Out(SLOTS)
            keep = run_mode(mode, pks, 54, out, skip=empty)
            torch.cuda.synchronize()
            check_exact(out, collections.Counter(bytes(p) for p in pks), 700)
        out = Out(SLOTS)
        keep = run_mode(mode, pks, 54, out)
        torch.cuda.synchronize()
        want = collections.Counter(bytes(p) for p in pks)
        assert len(want) == 13
        check_exact(out, want, 700)
        del keep


# ---- 7. two streams at once --------------------------------------------------------------------------
def test_two_streams_with_different_inputs():
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = _draw(_keys(300, 61), 20000, 62)
    b = _draw(_keys(7, 63), 30000, 64)
    out_a, out_b = Out(SLOTS), Out(SLOTS)
    torch.cuda.synchronize()
    keep = [run_mode("keys32", a, 65, out_a, stream=s1.cuda_stream),
            run_mode("fixed97", b, 66, out_b, stream=s2.cuda_stream),
            run_mode("ragged", a, 67, out_a, stream=s1.cuda_stream),
            run_mode("keys128", b, 68, out_b, stream=s2.cuda_stream)]
    torch.cuda.synchronize()
    check_exact(out_a, collections.Counter(bytes(p) for p in a), len(a))
    check_exact(out_b, collections.Counter(bytes(p) for p in b), len(b))
    del keep


# ---- 8. end to end: learn the clients, verify from their tables ----------------------------------------
def test_learn_then_verify_from_comb_tables():
    from hsverify import _lib, _testing, mempool
    from hsverify.committee import Committee
    from hsverify.signer import Signer
    rnd = np.random.default_rng(71)
    seeds = rnd.integers(0, 256, (54, 32), dtype=np.uint8)  # 0..2 the clients, 3..52 one-off keys, 53 a late client
    key_idx = np.concatenate([rnd.integers(0, 3, 1950), np.arange(3, 53)]).astype(np.uint32)
    rnd.shuffle(key_idx)
    blank = rnd.integers(0, 256, (2000, 128), dtype=np.uint8)
    with Signer(seeds) as signer:
        pk = signer.public_keys()
        txs = signer.sign_transactions(blank, key_idx)
        late = signer.sign_transactions(blank[:300], np.where(np.arange(300) % 2 == 0, 53, key_idx[:300]))
    txs[7, 100] ^= 1  # one bad signature among them
    with Committee.learn(txs, min_count=2) as c:
        assert len(c) == 3
        assert {c.index(pk[i]) for i in range(3)} == {0, 1, 2}
        assert all(c.index(pk[i]) == -1 for i in range(3, 54))
        flags = c.verify_transactions_fixed(txs)
        hits, misses, _ = _testing.committee_tx_counts()
        assert (flags == mempool.verify_transactions_fixed(txs)).all()
        assert int((flags & _lib.STRICT_OK != 0).sum()) == 1999
        assert hits == int((key_idx < 3).sum()) == 1950 and misses == 50
        # growing: the late client joins, the members keep their indices
        with Committee.learn(late, min_count=2, skip=c) as c2:
            assert len(c2) == 4 and [c2.index(pk[i]) for i in range(3)] == [c.index(pk[i]) for i in range(3)]
            assert c2.index(pk[53]) == 3
    # min_count and max_keys
    with Committee.learn(txs, min_count=1, max_keys=10) as c3:
        assert len(c3) == 10 and {c3.index(pk[i]) for i in range(3)} == {0, 1, 2}


# ---- 9. the host forms: sorted, capped ---------------------------------------------------------------
def test_host_forms_sort_and_cap():
    from hsverify import _lib, mempool
    pool = _keys(10, 81)
    times = [5, 5, 5, 3, 3, 9, 1, 1, 1, 1]
    pks = np.concatenate([np.repeat(pool[i:i + 1], t, axis=0) for i, t in enumerate(times)])
    pks = pks[np.random.default_rng(82).permutation(len(pks))]
    want = sorted(collections.Counter(bytes(p) for p in pks).items(), key=lambda kv: (-kv[1], kv[0]))
    lib = _lib.load()
    rows = np.zeros((len(pks), 48), np.uint8)  # a stride of 48 and an odd address: the host form takes both
    rows[:, :32] = pks
    flat = np.zeros(rows.size + 1, np.uint8)
    flat[1:] = rows.reshape(-1)
    for cap in (16, 10, 4, 0):
        keys = np.full((16, 32), 0xee, np.uint8)
        counts = np.full(16, 0xeeeeeeee, np.uint32)
        s = mempool.CensusSummary()
        rc = lib.hsv_census_keys(None, ctypes.c_void_p(flat.ctypes.data + 1), 48, len(pks), 64,
                                 ctypes.c_void_p(keys.ctypes.data) if cap else None,
                                 ctypes.c_void_p(counts.ctypes.data) if cap else None, cap, ctypes.byref(s))
        assert rc == 0, _lib.last_error()
        w = min(cap, 10)
        assert [(bytes(keys[j]), int(counts[j])) for j in range(w)] == want[:w]
        assert (keys[w:] == 0xee).all() and (counts[w:] == 0xeeeeeeee).all()
        assert s.distinct == 10 and s.items == len(pks) == s.counted and s.overflow == 0 and s.reserved == 0
    # the transaction form through the Python helper, ragged and fixed
    buf, offsets = _ragged(pks, 83)
    txs = [bytes(buf[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(pks))]
    keys, counts, s = mempool.census(txs)
    assert [(bytes(k), int(c)) for k, c in zip(keys, counts)] == want and s["distinct"] == 10
    keys, counts, s = mempool.census(_fixed(pks, 128, 84).reshape(-1, 128), slots=16)
    assert [(bytes(k), int(c)) for k, c in zip(keys, counts)] == want and s["items"] == len(pks)
    keys, counts, s = mempool.census([])
    assert keys.shape == (0, 32) and counts.size == 0 and s["items"] == 0 and s["distinct"] == 0
