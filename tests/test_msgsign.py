"""Whole messages of differing lengths signed on the GPU (hsv_signer_sign_msgs*):
byte for byte what the host signer (verifier.sign_many, grouped by length)
produces, at every message length where either of the signer's two hashes
changes its block count or a staging window ends, at every base address within
a 16-byte line, ragged inside one wave, and across the round boundary.  All
comparisons are exact bytes.  The CPU side is tests/test_msgsign_host.py."""
import numpy as np
import pytest

from test_msgsign_host import BASES, SIGN_MSG_LENS

pytestmark = pytest.mark.gpu


def sign_ragged(seeds, msgs):
    """Host signer (hsv_sign_many) over messages of mixed lengths: (pk, sig)."""
    from hsverify.verifier import sign_many
    n = len(msgs)
    pk, sig = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    lens = np.array([len(m) for m in msgs])
    for length in sorted(set(lens.tolist())):
        idx = np.nonzero(lens == length)[0]
        m = np.frombuffer(b"".join(msgs[i] for i in idx), np.uint8).reshape(len(idx), length)
        pk[idx], sig[idx] = sign_many(np.ascontiguousarray(seeds[idx]), m)
    return pk, sig


@pytest.fixture(scope="module")
def group(hsv):
    from hsverify import _lib
    return _lib.load_test().hsv_test_signer_group(0)


@pytest.fixture(scope="module")
def ref(hsv, group):
    """64 G + 90 keys and as many messages, every SIGN_MSG_LENS length among
    them, shuffled; the host signer's keys and signatures with key_idx = None
    (item i, key i) and with 50 keys repeated.  Computed once, read-only."""
    rnd = np.random.default_rng(61)
    n = 64 * group + 90
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = [SIGN_MSG_LENS[k % len(SIGN_MSG_LENS)] for k in range(n)]
    # the first 63 items hold every length once, so the smallest batches see them all
    head = list(lens[:len(SIGN_MSG_LENS)])
    rnd.shuffle(head)
    tail = lens[len(SIGN_MSG_LENS):]
    rnd.shuffle(tail)
    lens = head + tail
    msgs = [rnd.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    pk, sig = sign_ragged(seeds, msgs)
    idx = rnd.integers(0, 50, n).astype(np.uint32)
    _, sig_idx = sign_ragged(seeds[idx], msgs)
    for a in (seeds, pk, sig, idx, sig_idx):
        a.setflags(write=False)
    return {"n": n, "seeds": seeds, "msgs": msgs, "pk": pk, "sig": sig, "idx": idx, "sig_idx": sig_idx}


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
    if data:
        view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert view.data_ptr() % 16 == off
    return whole, view


def image(data: bytes, off: int) -> bytes:
    return bytes([0xA5]) * (16 + off) + data + bytes([0xA5]) * 32


def offsets_of(msgs):
    return np.cumsum([0] + [len(m) for m in msgs]).astype(np.int64)


def records(pk, m):
    """(m, 96) device records pk || 0xa5 x 64, and the (m, 64) view the signatures go to."""
    import torch
    rec = torch.full((m, 96), 0xA5, dtype=torch.uint8, device="cuda:0")
    rec[:, :32] = torch.from_numpy(pk[:m].copy()).to("cuda:0")
    return rec, rec[:, 32:]


def test_host_form_every_length(ref, group, signer):
    """A shuffled list holding every length, item i with key i and with keys
    repeated through key_idx, at the item counts where the grouping changes."""
    assert set(len(x) for x in ref["msgs"][:63]) == set(SIGN_MSG_LENS)
    for m in (1, 63, 65, 64 * group + 1):
        got = signer.sign_msgs(ref["msgs"][:m])
        bad = np.nonzero((got != ref["sig"][:m]).any(axis=1))[0]
        assert bad.size == 0, (m, bad[:8].tolist(), [len(ref["msgs"][i]) for i in bad[:8]])
        got = signer.sign_msgs(ref["msgs"][:m], key_idx=ref["idx"][:m])
        bad = np.nonzero((got != ref["sig_idx"][:m]).any(axis=1))[0]
        assert bad.size == 0, (m, bad[:8].tolist(), [len(ref["msgs"][i]) for i in bad[:8]])


@pytest.mark.parametrize("off", BASES)
def test_device_form_ragged_at_every_base(ref, group, signer, off):
    """Messages back to back at each base offset inside a guarded allocation,
    signatures at stride 96 into pk || R || s records: the pk bytes, the
    message bytes and the guards come back unchanged."""
    import torch
    m = 64 * group + 1
    data = b"".join(ref["msgs"][:m])
    whole, buf = carve(data, off)
    offsets = torch.from_numpy(offsets_of(ref["msgs"][:m])).to("cuda:0")
    rec, sig = records(ref["pk"], m)
    fault = torch.ones(2, dtype=torch.int32, device="cuda:0")
    signer.sign_msgs_device(buf, sig, offsets=offsets, fault=fault)
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    assert (got[:, :32] == ref["pk"][:m]).all()
    bad = np.nonzero((got[:, 32:] != ref["sig"][:m]).any(axis=1))[0]
    assert bad.size == 0, (off, bad[:8].tolist(), [len(ref["msgs"][i]) for i in bad[:8]])
    assert bytes(whole.cpu().numpy()) == image(data, off)
    assert fault.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("length", (32, 33, 111, 416))
def test_fixed_form_equals_sign_device(ref, group, signer, length):
    """msg_stride > msg_len, and stride 0 as one shared message: byte for byte
    the existing Signer.sign_device on the same inputs."""
    import torch
    rnd = np.random.default_rng(62 + length)
    m, stride = 64 * group + 1, length + 9
    rows = torch.from_numpy(rnd.integers(0, 256, (m, stride), dtype=np.uint8)).to("cuda:0")
    old = torch.zeros((m, 64), dtype=torch.uint8, device="cuda:0")
    new = torch.full((m, 64), 0xA5, dtype=torch.uint8, device="cuda:0")
    signer.sign_device(rows, old, msg_len=length)
    signer.sign_msgs_device(rows, new, msg_len=length, msg_stride=stride)
    torch.cuda.synchronize()
    assert old.cpu().numpy().any() and (old.cpu().numpy() == new.cpu().numpy()).all()
    shared = rows[5, 3:3 + length]
    old.zero_()
    new.fill_(0xA5)
    signer.sign_device(shared, old)
    signer.sign_msgs_device(shared, new, msg_len=length, msg_stride=0)
    torch.cuda.synchronize()
    assert old.cpu().numpy().any() and (old.cpu().numpy() == new.cpu().numpy()).all()


def test_one_long_message_in_a_wave_of_short_ones(ref, signer):
    """63 short messages and one of 256 KiB in one wave: the trip count is
    the wave's longest message, and every lane leaves the loop with its own hash."""
    import torch
    rnd = np.random.default_rng(63)
    msgs = [bytes(x) for x in ref["msgs"][:64]]
    msgs[37] = rnd.integers(0, 256, 256 * 1024, dtype=np.uint8).tobytes()
    _, want = sign_ragged(ref["seeds"][:64], msgs)
    whole, buf = carve(b"".join(msgs), 3)
    sig = torch.zeros((64, 64), dtype=torch.uint8, device="cuda:0")
    signer.sign_msgs_device(buf, sig, offsets=torch.from_numpy(offsets_of(msgs)).to("cuda:0"))
    torch.cuda.synchronize()
    assert (sig.cpu().numpy() == want).all()


def test_bad_index_and_decreasing_offsets_zero_that_item_only(ref, signer):
    """An index out of range and a decreasing pair of offsets: 64 zero bytes,
    no fault, and the neighbours are signed."""
    import torch
    msgs = [bytes(x) for x in ref["msgs"][:6]]
    idx = np.array([0, 1, ref["n"], 3, 0xFFFFFFFF, 5], np.uint32)
    want = ref["sig"][:6].copy()
    want[[2, 4]] = 0
    got = signer.sign_msgs(msgs, key_idx=idx)
    assert (got == want).all()
    # device form: item 1 = [end of item 0, start of item 2) with item 2 lying BEFORE item 0
    m0, m2 = msgs[0], msgs[2]
    data = m2 + m0
    offsets = torch.tensor([len(m2), len(m2) + len(m0), 0, len(m2)], dtype=torch.int64, device="cuda:0")
    whole, buf = carve(data, 15)
    sig = torch.full((3, 64), 0xA5, dtype=torch.uint8, device="cuda:0")
    fault = torch.ones(2, dtype=torch.int32, device="cuda:0")
    signer.sign_msgs_device(buf, sig, offsets=offsets, fault=fault)
    torch.cuda.synchronize()
    got = sig.cpu().numpy()
    assert (got[0] == ref["sig"][0]).all() and (got[2] == ref["sig"][2]).all() and not got[1].any()
    assert fault.cpu().tolist() == [0, 0]
    assert bytes(whole.cpu().numpy()) == image(data, 15)


def test_rounds_and_staged_bytes(ref, group):
    """The round boundary (2^22 items in the product) lowered to 300, and the
    bytes staged per launch of the host form lowered to 4096, through the test
    library's hooks: 64 G + 90 items take several rounds, each starting at its
    own key, offsets and bytes; the results equal the unchunked run."""
    import torch
    from hsverify import Signer, _testing
    m = 64 * group + 90
    msgs = ref["msgs"][:m]
    with _testing.test_library() as lib:
        assert lib.hsv_test_msg_sign_chunk(300) == 1 << 22
        try:
            with Signer(ref["seeds"][:m]) as s:
                assert (s.sign_msgs(msgs) == ref["sig"][:m]).all()
                assert (s.sign_msgs(msgs, key_idx=ref["idx"][:m]) == ref["sig_idx"][:m]).all()
                whole, buf = carve(b"".join(msgs), 1)
                sig = torch.zeros((m, 64), dtype=torch.uint8, device="cuda:0")
                s.sign_msgs_device(buf, sig, offsets=torch.from_numpy(offsets_of(msgs)).to("cuda:0"))
                torch.cuda.synchronize()
                assert (sig.cpu().numpy() == ref["sig"][:m]).all()
                lib.hsv_test_msg_sign_chunk(0)
                assert lib.hsv_test_stage_bytes(4096) == 1 << 29
                assert (s.sign_msgs(msgs) == ref["sig"][:m]).all()
                assert (s.sign_msgs(msgs, key_idx=ref["idx"][:m]) == ref["sig_idx"][:m]).all()
        finally:
            lib.hsv_test_msg_sign_chunk(0)
            lib.hsv_test_stage_bytes(0)


def test_more_items_than_keys_needs_an_index(ref):
    from hsverify import Signer, _lib
    with Signer(ref["seeds"][:2]) as s:
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            s.sign_msgs(ref["msgs"][:3])
        got = s.sign_msgs(ref["msgs"][:3], key_idx=[0, 1, 0])
        assert (got[:2] == ref["sig"][:2]).all()


def test_round_trip_through_the_message_verifier(ref, group, signer):
    """sign_msgs_device, then verify_msgs_device on the same tensors and stream
    with no synchronisation between them: every item STRICT_OK."""
    import torch
    from hsverify import STRICT_OK, verifier
    m = 64 * group + 1
    msgs = ref["msgs"][:m]
    whole, buf = carve(b"".join(msgs), 4)
    offsets = torch.from_numpy(offsets_of(msgs)).to("cuda:0")
    pk = torch.from_numpy(ref["pk"][:m].copy()).to("cuda:0")
    sig = torch.zeros((m, 64), dtype=torch.uint8, device="cuda:0")
    flags = torch.zeros(m, dtype=torch.uint8, device="cuda:0")
    signer.sign_msgs_device(buf, sig, offsets=offsets)
    verifier.verify_msgs_device(pk, sig, buf, offsets=offsets, flags=flags)
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() & STRICT_OK).all()


def test_synth_messages_gpu_verifies(hsv):
    import torch
    from hsverify import STRICT_OK, synth, verifier
    lens = [SIGN_MSG_LENS[k % len(SIGN_MSG_LENS)] for k in range(257)]
    pk, sig, buf, offsets = synth.messages_gpu(lens, seed=7)
    assert pk.shape == (257, 32) and sig.shape == (257, 64) and offsets.tolist()[-1] == sum(lens) == buf.numel()
    flags = torch.zeros(257, dtype=torch.uint8, device=pk.device)
    verifier.verify_msgs_device(pk, sig, buf, offsets=offsets, flags=flags)
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() & STRICT_OK).all()
