"""hsv_verify_msgs* at <= 2^13 items: the message instantiations of the four
small-batch kernels (quad, joint, row, pair), one launch whose
prepass wave hashes the block's whole messages beside the point waves.

The test library's hsv_test_msgs_small forces one form at every such n (1 quad,
2 joint, 3 row, 4 pair; 0 = the message prepass + point pass, two launches,
as larger batches; -1 = by n).  Unless a test says otherwise it runs under every
forced form, expects the C oracle's oracle_verify_flags(pk, sig, msg, len) --
all 8 bits -- the strict bits of those flags and fault words [0, 0], and
compares the form's outputs byte for byte with mode 0 on the same inputs."""
import contextlib
import ctypes

import numpy as np
import pytest

import ed25519_ref as o
from test_verify_msgs import oracle_msgs, ragged_batch, run_device, sign_ragged

pytestmark = pytest.mark.gpu

FORMS = {1: "quad", 2: "joint", 3: "row", 4: "pair"}
FORM_IDS = [pytest.param(m, id=name) for m, name in FORMS.items()]
# sizes at each form's block edges (joint: 3 items per block, row: 6, pair: 64)
EDGE_SIZES = [(1, 1), (1, 3), (2, 1), (2, 3), (2, 4), (2, 7), (3, 5), (3, 6), (3, 7), (3, 13),
              (4, 1), (4, 63), (4, 64), (4, 65), (4, 129)]


@pytest.fixture
def tlib(hsv):
    """Every hsverify call of the test goes to libhsv_test.so, whose route
    switch the test may move; the default route is back afterwards."""
    from hsverify import _testing
    with _testing.test_library() as lib:
        assert lib.hsv_test_msgs_small(-1) == -1
        try:
            yield lib
        finally:
            lib.hsv_test_msgs_small(-1)


@contextlib.contextmanager
def route(lib, mode):
    prev = lib.hsv_test_msgs_small(mode)
    assert prev != -2
    try:
        yield
    finally:
        lib.hsv_test_msgs_small(prev)


def form_counts(lib):
    out = (ctypes.c_uint64 * 5)()
    assert lib.hsv_test_msgs_form_counts(out) == 0
    return np.array(list(out), np.int64)


def check_against(lib, mode, exp, call):
    """call() -> (flags or None, bits or None, fault) under `mode` and under
    mode 0: the oracle's flags and strict bits, no fault, the form's launch
    counted, and the two routes' outputs identical."""
    before = form_counts(lib)
    with route(lib, mode):
        got = call()
    moved = form_counts(lib) - before
    assert moved[mode] >= 1 and moved.sum() == moved[mode], (FORMS[mode], moved.tolist())
    with route(lib, 0):
        two = call()
    for (flags, bits, fault), what in ((got, FORMS[mode]), (two, "two launches")):
        if flags is not None:
            assert (flags == exp).all(), (what, np.nonzero(flags != exp)[0][:8], flags[flags != exp][:8])
        if bits is not None:
            assert (bits == (exp & o.STRICT_OK)).all(), (what, np.nonzero(bits != (exp & o.STRICT_OK))[0][:8])
        assert fault == [0, 0], what
    for a, b in zip(got[:2], two[:2]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ragged(hsv, oracle_lib):
    """129 ragged items (lengths from MSG_LENS: 0, 47/48, 175/176, 64, 192, ...;
    one in eight corrupted) and the oracle's flags, computed once, read-only;
    the smaller batches are prefixes."""
    pk, sig, msgs, bad = ragged_batch(61, 129)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
    for a in (pk, sig, exp):
        a.setflags(write=False)
    return {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}


@pytest.mark.parametrize("mode,n", EDGE_SIZES, ids=[f"{FORMS[m]}-{n}" for m, n in EDGE_SIZES])
def test_sizes_at_each_forms_block_edges(tlib, ragged, mode, n):
    """Ragged lengths inside one block, the message bytes 1..15 bytes off a
    16-byte boundary (both outputs, then bits only) and once aligned (flags
    only)."""
    from hsverify import verifier
    pk, sig, msgs, exp = ragged["pk"][:n], ragged["sig"][:n], ragged["msgs"][:n], ragged["exp"][:n]
    buf, offsets = verifier.pack_msgs(msgs)
    shift = 1 + (n * 7 + mode) % 15
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, offsets, shift=shift))
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, offsets, shift=0, want_bits=False))
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, offsets, shift=16 - shift, want_flags=False))


@pytest.fixture(scope="module")
def one_long(hsv, oracle_lib):
    """66 items: a 64 KiB message last (and, swapped, first), the others empty
    or 32 bytes; one short item corrupted."""
    rnd = np.random.default_rng(62)
    n = 66
    msgs = [rnd.integers(0, 256, 32 * (i % 2), dtype=np.uint8).tobytes() for i in range(n)]
    msgs[-1] = rnd.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()
    out = {}
    for where in ("last", "first"):
        if where == "first":
            msgs = [msgs[-1]] + msgs[:-1]
        seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
        pk, sig = sign_ragged(seeds, msgs)
        sig[1, 40] ^= 1
        out[where] = (pk, sig, list(msgs))
    return out


# a partial last block per form: 2 of 3 (joint), 2 of 6 (row), 2 of 64 (pair)
@pytest.mark.parametrize("mode,n", [(1, 2), (2, 5), (3, 8), (4, 66)], ids=list(FORMS.values()))
def test_one_long_message_in_a_partial_last_block(tlib, oracle_lib, one_long, mode, n):
    """The prepass wave's idle lanes hash an item of their own block again:
    they follow the block's trip count (513 blocks here) and read no byte
    outside a message.  Long message last: the batch is the last n items of
    the fixture; long message first: its first n."""
    from hsverify import verifier
    for where in ("last", "first"):
        pk, sig, msgs = one_long[where]
        sl = slice(len(msgs) - n, None) if where == "last" else slice(0, n)
        pk, sig, msgs = pk[sl], sig[sl], msgs[sl]
        assert len(msgs[-1 if where == "last" else 0]) == 1 << 16 and len(msgs) == n
        exp = oracle_msgs(oracle_lib, pk, sig, msgs)
        assert exp[-1 if where == "last" else 0] & o.STRICT_OK
        buf, offsets = verifier.pack_msgs(msgs)
        check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, offsets, shift=7))


@pytest.fixture(scope="module")
def votes(hsv, oracle_lib):
    """The QC shape: 67 signers over one 100-byte message, and over the empty
    message; two items corrupted in each."""
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(63)
    n = 67
    out = {}
    for length in (0, 100):
        msg = rnd.integers(0, 256, length, dtype=np.uint8)
        seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
        pk, sig = sign_many(seeds, np.repeat(msg[None], n, 0))
        sig[5, 33] ^= 1
        pk[40] = pk[41]
        exp = oracle_msgs(oracle_lib, pk, sig, [msg.tobytes()] * n)
        assert (exp & o.STRICT_OK).sum() == n - 2
        out[length] = (pk, sig, msg, exp)
    return out


@pytest.mark.parametrize("mode", FORM_IDS)
def test_empty_and_shared_batch_wide_messages(tlib, votes, mode):
    """msg_len = 0 with d_msgs one past an allocation (nothing is loaded), and
    msg_stride = 0: 67 votes over one 100-byte message."""
    import torch
    from hsverify import _lib
    dev = torch.device("cuda:0")

    def empty():
        pk, sig, _, _ = votes[0]
        n = pk.shape[0]
        backing = torch.zeros(64, dtype=torch.uint8, device=dev)
        flags = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
        bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
        fault = torch.ones(2, dtype=torch.int32, device=dev)
        d_pk, d_sig = torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev)
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
        # (an empty torch slice has no address: the C ABI directly, on torch's current stream)
        rc = _lib.load().hsv_verify_msgs_device(p(d_pk), 32, p(d_sig), 64, p(backing, 64), None, 0, 0, n, p(flags),
                                                p(bits), p(fault),
                                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(rc, "hsv_verify_msgs_device")
        torch.cuda.synchronize()
        b = bits.cpu().numpy().view(np.uint32)
        return (flags.cpu().numpy(), ((b[np.arange(n) // 32] >> (np.arange(n) % 32)) & 1).astype(np.uint8),
                fault.cpu().tolist())

    check_against(tlib, mode, votes[0][3], empty)
    pk, sig, msg, exp = votes[100]
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, msg, shift=3, msg_len=100, msg_stride=0))


@pytest.fixture(scope="module")
def long_ragged(hsv, oracle_lib):
    """129 items, every message longer than 32 bytes."""
    pk, sig, msgs, bad = ragged_batch(64, 129, lens_pool=(33, 47, 48, 100, 176, 193))
    return pk, sig, msgs, oracle_msgs(oracle_lib, pk, sig, msgs)


@pytest.mark.parametrize("mode", FORM_IDS)
def test_fallback_items_take_k_from_the_record(tlib, long_ragged, fallback_records, oracle_lib, mode):
    """At a 128-bit lattice bound most items have no short pair and run the
    full-length path, whose k mod l comes from the LDS record: a form that
    hashed 32 bytes again for such an item would reject these (every message
    is longer).  Then the lattice-fallback fixtures as 32-byte messages at 133
    bits."""
    from hsverify import _testing, verifier
    pk, sig, msgs, exp = long_ragged
    buf, offsets = verifier.pack_msgs(msgs)
    prev = _testing.set_lattice_bits(128)
    try:
        check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, offsets, shift=9))
        _testing.set_lattice_bits(133)
        fpk, fsig, fmsg = fallback_records["pk"], fallback_records["sig"], fallback_records["msg"]
        fexp = oracle_msgs(oracle_lib, fpk, fsig, [m.tobytes() for m in fmsg])
        assert (fexp == fallback_records["flags"]).all()
        check_against(tlib, mode, fexp, lambda: run_device(fpk, fsig, fmsg.reshape(-1), shift=0, msg_len=32))
    finally:
        _testing.set_lattice_bits(prev)


@pytest.mark.parametrize("mode", FORM_IDS)
def test_void_items_among_valid_ones(tlib, oracle_lib, ragged, mode):
    """Device form, two items whose offsets decrease: flags 0 and strict bit 0
    for them, their neighbours as the oracle says (the item after a victim
    starts one byte early)."""
    from hsverify import verifier
    n = 65 if mode == 4 else 13
    pk, sig, msgs, exp = ragged["pk"][:n], ragged["sig"][:n], ragged["msgs"][:n], ragged["exp"][:n].copy()
    buf, offsets = verifier.pack_msgs(msgs)
    off = offsets.copy()
    for victim in (2, 9):
        assert off[victim] > 0 and off[victim + 2] >= off[victim] - 1
        off[victim + 1] = off[victim] - 1
        exp[victim] = 0
        nxt = buf[int(off[victim + 1]):int(off[victim + 2])].tobytes()
        exp[victim + 1] = oracle_lib.oracle_verify_flags(pk[victim + 1].tobytes(), sig[victim + 1].tobytes(), nxt,
                                                         len(nxt))
    assert (exp & o.STRICT_OK).sum() > n // 2
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, buf, off, shift=5))


@pytest.mark.parametrize("mode", FORM_IDS)
def test_edge_vectors_as_32_byte_messages(tlib, oracle_lib, golden, mode):
    n = golden["n_edge"]
    assert n == 145
    pk, sig, msg = golden["pk"][:n].copy(), golden["sig"][:n].copy(), np.ascontiguousarray(golden["msg"][:n])
    exp = oracle_msgs(oracle_lib, pk, sig, [m.tobytes() for m in msg])
    assert (exp == golden["flags"][:n]).all()
    check_against(tlib, mode, exp, lambda: run_device(pk, sig, msg.reshape(-1), shift=0, msg_len=32))


@pytest.mark.parametrize("inject", [1, 2, 3])
@pytest.mark.parametrize("mode", FORM_IDS)
def test_self_check_injection(tlib, votes, mode, inject):
    """Corrupted table values (zeroed, flipped bits) or an overwritten canary
    word: the message forms answer as tests/test_fault.py requires of the
    digest forms -- the call's fault word is set, the host form returns
    HSV_ERR_DEVICE_FAULT -- and verify again once the hook is off."""
    from hsverify import _lib, _testing, verifier
    pk, sig, msg, exp = votes[100]
    msgs = [msg.tobytes()] * pk.shape[0]
    with route(tlib, mode):
        with _testing.injected_fault(inject):
            _, _, fault = run_device(pk, sig, msg, shift=3, msg_len=100, msg_stride=0)
            assert [bool(w) for w in fault] == [inject != 2, inject == 2], fault
            with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_DEVICE_FAULT"):
                verifier.verify_msgs(pk, sig, msgs)
        flags, _, fault = run_device(pk, sig, msg, shift=3, msg_len=100, msg_stride=0)
        assert (flags == exp).all() and fault == [0, 0]
        assert (verifier.verify_msgs(pk, sig, msgs) == exp).all()


@pytest.fixture(scope="module")
def many(hsv, oracle_lib):
    """8193 items of 0, 32 or 100 bytes, one in eight corrupted, and the
    oracle's flags; the routing sizes are prefixes."""
    pk, sig, msgs, _ = ragged_batch(65, 8193, lens_pool=(0, 32, 100))
    return pk, sig, msgs, oracle_msgs(oracle_lib, pk, sig, msgs)


def test_routing_by_size(tlib, many):
    """The default route: one call at n = 1 is a small form's launch, one at
    8193 the two-launch form's; at each digest-path cut-over and its successor
    exactly one small-form counter moves, and the flags are the oracle's.
    Which form a size takes is the measured table's business."""
    from hsverify import verifier
    pk, sig, msgs, exp = many

    def call(n):
        buf, offsets = verifier.pack_msgs(msgs[:n])
        before = form_counts(tlib)
        flags, bits, fault = run_device(pk[:n], sig[:n], buf, offsets, shift=11)
        assert (flags == exp[:n]).all(), (n, np.nonzero(flags != exp[:n])[0][:8])
        assert (bits == (exp[:n] & o.STRICT_OK)).all() and fault == [0, 0], n
        return form_counts(tlib) - before

    moved = call(1)
    assert moved[0] == 0 and moved[1:].sum() == 1, moved.tolist()
    moved = call(8193)
    assert moved.tolist() == [1, 0, 0, 0, 0]
    for n in (256, 257, 768, 769, 3072, 3073, 8192):
        moved = call(n)
        assert moved[0] == 0 and sorted(moved[1:].tolist()) == [0, 0, 0, 1], (n, moved.tolist())


@pytest.mark.parametrize("mode", [pytest.param(-1, id="default")] + FORM_IDS)
def test_stream_order_after_the_gpu_signer(tlib, oracle_lib, mode):
    """Signer.sign_device, then verify_msgs_device at n = 67 on the same
    stream with no synchronisation between them: all accepted."""
    import torch
    from hsverify import Signer, verifier
    rnd = np.random.default_rng(66)
    m, length = 67, 100
    seeds = rnd.integers(0, 256, (m, 32), dtype=np.uint8)
    msgs = rnd.integers(0, 256, (m, length), dtype=np.uint8)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with route(tlib, mode), Signer(seeds) as s:
        pks = s.public_keys()
        with torch.cuda.stream(st):
            raw = torch.zeros(m * length + 19, dtype=torch.uint8, device=dev)
            d_msgs = raw[3:3 + m * length].view(m, length)
            d_msgs.copy_(torch.from_numpy(msgs))
            rec = torch.zeros((m, 96), dtype=torch.uint8, device=dev)
            rec[:, :32] = torch.from_numpy(pks).to(dev)
            flags = torch.zeros(m, dtype=torch.uint8, device=dev)
            f_sign = torch.ones(2, dtype=torch.int32, device=dev)
            f_ver = torch.ones(2, dtype=torch.int32, device=dev)
            s.sign_device(d_msgs, rec[:, 32:], msg_len=length, fault=f_sign)
            verifier.verify_msgs_device(rec[:, :32], rec[:, 32:], raw[3:], msg_len=length, flags=flags, fault=f_ver)
        st.synchronize()
    got_rec = rec.cpu().numpy()
    exp = oracle_msgs(oracle_lib, got_rec[:, :32], got_rec[:, 32:], [msgs[i].tobytes() for i in range(m)])
    assert (exp & o.STRICT_OK).all()
    assert (flags.cpu().numpy() == exp).all()
    assert f_sign.cpu().tolist() == [0, 0] and f_ver.cpu().tolist() == [0, 0]
