"""Mempool transactions signed on the GPU (hsv_signer_sign_transactions*): byte
for byte what the host route produces -- hashlib's SHA-512(message)[..32]
signed by verifier.sign_many on the same seeds -- at every message length
where a SHA-512 padding boundary falls, at byte addresses where neighbouring
transactions share a 32-bit word, and at the item counts where the kernels'
grouping changes shape."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MSG_LENS = (0, 1, 111, 112, 127, 128, 239, 240, 416)   # message-only padding boundaries; 416: the 512-byte transaction
TX_SIZES = tuple(n + 96 for n in MSG_LENS)
FILL = 0xCC                                            # the unsigned tail, so an untouched one shows


@pytest.fixture(scope="module")
def group(hsv):
    from hsverify import _lib
    return _lib.load_test().hsv_test_signer_group(0)


@pytest.fixture(scope="module")
def ref(hsv, group):
    """One pool of seeds with the host signer's keys, and per transaction size
    64 G + 1 unsigned transactions with their signed form (computed once,
    read-only); 4097 of them for the 512-byte size."""
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(51)
    n = max(4097, 64 * group + 1)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    out = {"n": n, "seeds": seeds, "raw": {}, "signed": {}}
    for size in TX_SIZES:
        m = n if size == 512 else 64 * group + 1
        raw = np.full((m, size), FILL, np.uint8)
        raw[:, :size - 96] = rnd.integers(0, 256, (m, size - 96), dtype=np.uint8)
        out["raw"][size] = raw
        out["signed"][size] = sign_rows(sign_many, seeds[:m], raw)
    out["pk"] = out["signed"][512][:, 416:448].copy()
    for a in (seeds, out["pk"], *out["raw"].values(), *out["signed"].values()):
        a.setflags(write=False)
    return out


def digests_of(msgs):
    return np.stack([np.frombuffer(hashlib.sha512(bytes(m)).digest()[:32], np.uint8) for m in msgs])


def sign_rows(sign_many, seeds, raw):
    """The host route on an (m, size) array of unsigned transactions."""
    size = raw.shape[1]
    pk, sig = sign_many(np.ascontiguousarray(seeds), digests_of(raw[:, :size - 96]))
    out = raw.copy()
    out[:, size - 96:size - 64], out[:, size - 64:] = pk, sig
    return out


def sign_list(seeds, msgs):
    """The host route on a list of messages: the signed transactions, as bytes."""
    from hsverify.verifier import sign_many
    pk, sig = sign_many(np.ascontiguousarray(seeds), digests_of(msgs))
    return [bytes(m) + bytes(pk[i]) + bytes(sig[i]) for i, m in enumerate(msgs)]


@pytest.fixture(scope="module")
def signer(ref):
    from hsverify import Signer
    with Signer(ref["seeds"]) as s:
        yield s


def carve(data: bytes, off: int):
    """`data` at byte 16 + off of an aligned device allocation filled with
    0xa5 (16 guard bytes before and at least 16 after): (whole, view)."""
    import torch
    whole = torch.full((16 + off + len(data) + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert whole.data_ptr() % 16 == 0
    view = whole[16 + off:16 + off + len(data)]
    view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert view.data_ptr() % 16 == off
    return whole, view


def image(data: bytes, off: int) -> bytes:
    return bytes([0xA5]) * (16 + off) + data + bytes([0xA5]) * 32


@pytest.mark.parametrize("size", TX_SIZES)
def test_fixed_size_matches_host_route(ref, group, signer, size):
    """Host form, key_idx = None: item i signs with key i; the whole buffer is
    the host route's."""
    for m in (1, 63, 65, 64 * group + 1):
        got = signer.sign_transactions(ref["raw"][size][:m])
        bad = np.nonzero((got != ref["signed"][size][:m]).any(axis=1))[0]
        assert bad.size == 0, (size, m, bad[:8].tolist())


@pytest.mark.parametrize("size", (97, 207, 512))
@pytest.mark.parametrize("off", (1, 3, 15))
def test_device_form_in_place_at_odd_addresses(ref, group, signer, size, off):
    """At sizes 97 and 207 the tail of transaction i and the message of
    transaction i + 1 share a word, and neighbouring lanes write them at the
    same time: every message byte and both guards must come back unchanged."""
    import torch
    m = 64 * group + 1
    whole, txs = carve(ref["raw"][size][:m].tobytes(), off)
    fault = torch.ones(2, dtype=torch.int32, device="cuda:0")
    signer.sign_transactions_device(txs, tx_size=size, fault=fault)
    torch.cuda.synchronize()
    assert bytes(whole.cpu().numpy()) == image(ref["signed"][size][:m].tobytes(), off)
    assert fault.cpu().tolist() == [0, 0]


def ragged_items(ref, rnd, count):
    lens = [MSG_LENS[k % len(MSG_LENS)] for k in range(count)]
    rnd.shuffle(lens)
    return [rnd.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]


def test_ragged_batch_host_form(ref, group, signer):
    rnd = np.random.default_rng(52)
    m = 64 * group + 1
    msgs = ragged_items(ref, rnd, m)
    want = sign_list(ref["seeds"][:m], msgs)
    offsets = np.cumsum([0] + [len(t) for t in want]).astype(np.uint64)
    raw = np.frombuffer(b"".join(x + bytes([FILL]) * 96 for x in msgs), np.uint8)
    got = signer.sign_transactions(raw, offsets=offsets)
    assert bytes(got) == b"".join(want)
    assert bytes(raw[-96:]) == bytes([FILL]) * 96, "the caller's array is not the one signed"


def test_ragged_batch_with_short_items_device_form(ref, group, signer):
    """A 95-byte item and an empty one are left untouched, at an odd base
    address; the items around them are exact."""
    import torch
    rnd = np.random.default_rng(53)
    m = 64 * group + 1
    msgs = ragged_items(ref, rnd, m)
    want = sign_list(ref["seeds"][:m], msgs)
    raw = [x + bytes([FILL]) * 96 for x in msgs]
    for at, short in ((5, rnd.integers(0, 256, 95, dtype=np.uint8).tobytes()), (70, b"")):
        raw[at] = want[at] = short
    offsets = torch.from_numpy(np.cumsum([0] + [len(t) for t in raw]).astype(np.int64)).to("cuda:0")
    whole, txs = carve(b"".join(raw), 3)
    fault = torch.ones(2, dtype=torch.int32, device="cuda:0")
    signer.sign_transactions_device(txs, offsets=offsets, fault=fault)
    torch.cuda.synchronize()
    assert bytes(whole.cpu().numpy()) == image(b"".join(want), 3)
    assert fault.cpu().tolist() == [0, 0]


def test_decreasing_offsets_skip_that_item_only(ref, signer):
    """offsets[2] < offsets[1]: item 1 is left alone, items 0 and 2 (whose
    spans the offsets still describe) are signed, nothing else is written."""
    import torch
    rnd = np.random.default_rng(54)
    msgs = [rnd.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (17, 111)]
    tx0, tx2 = sign_list(ref["seeds"][[0, 2]], msgs)   # no key_idx: item i signs with key i
    gap, rest = bytes([0x5A]) * 64, bytes([0x3C]) * 120
    unsigned = [x + bytes([FILL]) * 96 for x in msgs]
    data = gap + unsigned[1] + unsigned[0] + rest      # item 2 lies BEFORE item 0
    o2, o0 = len(gap), len(gap) + len(unsigned[1])
    offsets = torch.tensor([o0, o0 + len(unsigned[0]), o2, o2 + len(unsigned[1])], dtype=torch.int64, device="cuda:0")
    whole, txs = carve(data, 15)
    signer.sign_transactions_device(txs, offsets=offsets)
    torch.cuda.synchronize()
    assert bytes(whole.cpu().numpy()) == image(gap + tx2 + tx0 + rest, 15)


@pytest.mark.parametrize("size", (97, 512))
def test_key_index_with_repeats_and_out_of_range(ref, group, signer, size):
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(55)
    m = 64 * group + 1
    idx = rnd.integers(0, 50, m).astype(np.uint32)      # 50 keys over m items: many repeats
    raw = ref["raw"][size][:m]
    exp = sign_rows(sign_many, ref["seeds"][idx], raw)
    a, b = m // 2, m - 2
    idx[a], idx[b] = ref["n"], 0xFFFFFFFF                # the first index past the keys, and the last of all
    exp[a, size - 96:] = 0
    exp[b, size - 96:] = 0
    got = signer.sign_transactions(raw, key_idx=idx)
    assert (got == exp).all()


def test_more_items_than_keys_needs_an_index(ref):
    from hsverify import Signer, _lib
    with Signer(ref["seeds"][:2]) as s:
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            s.sign_transactions(ref["raw"][97][:3])
        with pytest.raises(_lib.HsvLibraryError, match="shorter than 96"):
            s.sign_transactions(np.zeros((2, 95), np.uint8))
        got = s.sign_transactions(ref["raw"][97][:3], key_idx=[0, 1, 0])
        assert (got[:2] == ref["signed"][97][:2]).all()


def test_round_trip_through_the_mempool_verifier(ref, signer):
    """sign_transactions_device, then verify_transactions_device on the same
    tensor and stream with no synchronisation between them; 4097 items, so
    both grids have more than one block.  One flipped message bit costs that
    item, and only that item, its STRICT_OK."""
    import torch
    from hsverify import STRICT_OK, mempool
    m, size = 4097, 512
    dev = torch.device("cuda:0")
    txs = torch.from_numpy(ref["raw"][size][:m].copy()).to(dev)
    flags = torch.zeros(m, dtype=torch.uint8, device=dev)
    f_sign = torch.ones(2, dtype=torch.int32, device=dev)
    f_ver = torch.ones(2, dtype=torch.int32, device=dev)
    signer.sign_transactions_device(txs, fault=f_sign)
    mempool.verify_transactions_device(txs, tx_size=size, flags=flags, fault=f_ver)
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() & STRICT_OK).all()
    assert f_sign.cpu().tolist() == [0, 0] and f_ver.cpu().tolist() == [0, 0]
    assert (txs.cpu().numpy() == ref["signed"][size][:m]).all()
    victim = 2051
    txs[victim, 200] ^= 4
    mempool.verify_transactions_device(txs, tx_size=size, flags=flags)
    torch.cuda.synchronize()
    ok = (flags.cpu().numpy() & STRICT_OK) != 0
    assert not ok[victim] and ok.sum() == m - 1


def test_synth_transactions_gpu_equals_the_host_workload(hsv):
    from hsverify import synth
    gpu = synth.transactions_gpu(257, 512, 7)
    host = synth.transactions(257, 512, 7, corrupt_frac=0.0)
    assert gpu.txs.shape == (257, 512) and (gpu.txs == host.txs).all()
    assert gpu.honest.all() and gpu.accept.all() and (gpu.kind == -1).all()


def test_batches_above_one_launch(ref):
    """The launch boundary (2^22 items in the product) lowered to 300 through
    the test library's hook: 700 items are three launches, and each must start
    at its own key, offsets and bytes.  Host and device form, fixed and
    ragged, implicit and explicit key index."""
    import torch
    from hsverify import Signer, _testing
    rnd = np.random.default_rng(56)
    m = 700
    with _testing.test_library() as lib:
        assert lib.hsv_test_tx_sign_chunk(300) == 1 << 22
        try:
            with Signer(ref["seeds"][:m]) as s:
                for size in (97, 512):
                    raw, want = ref["raw"][512][:m, 512 - size:], ref["signed"][512][:m]
                    if size != 512:   # other messages: sign them on the host
                        from hsverify.verifier import sign_many
                        want = sign_rows(sign_many, ref["seeds"][:m], np.ascontiguousarray(raw))
                    assert (s.sign_transactions(raw) == want).all(), size
                    assert (s.sign_transactions(raw, key_idx=np.arange(m, dtype=np.uint32)) == want).all(), size
                    whole, txs = carve(np.ascontiguousarray(raw).tobytes(), 1)
                    s.sign_transactions_device(txs, tx_size=size)
                    torch.cuda.synchronize()
                    assert bytes(whole.cpu().numpy()) == image(want.tobytes(), 1), size
                msgs = ragged_items(ref, rnd, m)
                want = sign_list(ref["seeds"][:m], msgs)
                offsets = np.cumsum([0] + [len(t) for t in want])
                data = b"".join(x + bytes([FILL]) * 96 for x in msgs)
                got = s.sign_transactions(np.frombuffer(data, np.uint8), offsets=offsets.astype(np.uint64))
                assert bytes(got) == b"".join(want)
                whole, txs = carve(data, 3)
                s.sign_transactions_device(txs, offsets=torch.from_numpy(offsets.astype(np.int64)).to("cuda:0"))
                torch.cuda.synchronize()
                assert bytes(whole.cpu().numpy()) == image(b"".join(want), 3)
        finally:
            lib.hsv_test_tx_sign_chunk(0)
