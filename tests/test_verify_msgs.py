"""Ed25519 verification over messages of any length on the GPU
(hsv_verify_msgs, hsv_verify_msgs_device): flags bit-exact with the C oracle's
oracle_verify_flags(pk, sig, msg, msg_len) at every length where the padding or
the block count of SHA-512(R || A || M) changes, at every alignment, ragged
inside a wave, through the full-length fallback path, and across the 2^22-item
launch boundary.  The CPU side (the hash core against hashlib) is
tests/test_msg_host.py."""
import numpy as np
import pytest

import ed25519_ref as o
from test_msg_host import MSG_LENS

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
        pk[idx], sig[idx] = sign_many(seeds[idx], m)
    return pk, sig


def ragged_batch(seed, n, lens_pool=MSG_LENS):
    """n items whose lengths are drawn from lens_pool; one item in eight is
    corrupted: a flipped message byte (a flipped s bit where the message is
    empty), a flipped s bit, s + l, or a wrong key."""
    rnd = np.random.default_rng(seed)
    lens = rnd.choice(np.array(lens_pool), n)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rnd.integers(0, 256, int(length), dtype=np.uint8).tobytes() for length in lens]
    pk, sig = sign_ragged(seeds, msgs)
    bad = np.zeros(n, bool)
    for i in range(3, n, 8):
        kind = (i // 8) % 4
        bad[i] = True
        if kind == 0 and msgs[i]:
            m = bytearray(msgs[i])
            m[int(rnd.integers(0, len(m)))] ^= 0x10
            msgs[i] = bytes(m)
        elif kind in (0, 1):
            sig[i, 32 + int(rnd.integers(0, 31))] ^= 4
        elif kind == 2:
            s = int.from_bytes(sig[i, 32:].tobytes(), "little") + o.L
            sig[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
        else:
            pk[i] = pk[(i + 1) % n] if n > 1 else pk[i] ^ 1
    return pk, sig, msgs, bad


def oracle_msgs(lib, pk, sig, msgs):
    return np.array([lib.oracle_verify_flags(pk[i].tobytes(), sig[i].tobytes(), msgs[i], len(msgs[i]))
                     for i in range(len(msgs))], np.uint8)


def unpack_bits(bits, n):
    b = bits.cpu().numpy().view(np.uint32)
    return ((b[np.arange(n) // 32] >> (np.arange(n) % 32)) & 1).astype(np.uint8)


def run_device(pk, sig, buf, offsets=None, shift=0, msg_len=0, msg_stride=None, want_bits=True, want_flags=True):
    """Device form on cuda:0 with the message bytes `shift` bytes into an
    allocation; returns (flags or None, strict bits or None, fault words)."""
    import torch
    from hsverify import verifier
    dev = torch.device("cuda:0")
    n = pk.shape[0]
    backing = torch.zeros(buf.size + shift + 16, dtype=torch.uint8, device=dev)
    backing[shift:shift + buf.size].copy_(torch.from_numpy(np.array(buf, dtype=np.uint8)))
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev) if offsets is not None else None
    flags = torch.full((n,), 0xff, dtype=torch.uint8, device=dev) if want_flags else None
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev) if want_bits else None
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    verifier.verify_msgs_device(torch.from_numpy(pk.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev),
                                backing[shift:], d_off, msg_len=msg_len, msg_stride=msg_stride, flags=flags,
                                strict_bits=bits, fault=fault)
    torch.cuda.synchronize()
    return (flags.cpu().numpy() if want_flags else None, unpack_bits(bits, n) if want_bits else None,
            fault.cpu().tolist())


_REFERENCE = {}   # computed once per process, read-only: tests/test_stage_cap.py shares it


def ragged_reference(oracle_lib):
    """257 ragged items and the oracle's flags."""
    if "ragged" not in _REFERENCE:
        pk, sig, msgs, bad = ragged_batch(51, 257)
        exp = oracle_msgs(oracle_lib, pk, sig, msgs)
        assert not (exp[bad] & o.STRICT_OK).any() and (exp[~bad] & o.STRICT_OK).all()
        for a in (pk, sig, exp):
            a.setflags(write=False)
        _REFERENCE["ragged"] = {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}
    return _REFERENCE["ragged"]


def ragged_over_the_cap(oracle_lib):
    """The same 257 items with item 100 replaced by a valid message of 5000
    bytes, longer than the lowered staging cap of 4096: it goes alone in its
    launch."""
    if "over_the_cap" not in _REFERENCE:
        ragged = ragged_reference(oracle_lib)
        at = 100
        long = np.random.default_rng(57).integers(0, 256, 5000, dtype=np.uint8).tobytes()
        pk, sig, msgs, exp = ragged["pk"].copy(), ragged["sig"].copy(), list(ragged["msgs"]), ragged["exp"].copy()
        pk[at:at + 1], sig[at:at + 1] = sign_ragged(np.full((1, 32), 9, np.uint8), [long])
        msgs[at] = long
        exp[at] = oracle_msgs(oracle_lib, pk[at:at + 1], sig[at:at + 1], [long])[0]
        assert exp[at] & o.STRICT_OK and 0 < (exp & o.STRICT_OK).sum() < len(msgs)
        for a in (pk, sig, exp):
            a.setflags(write=False)
        _REFERENCE["over_the_cap"] = {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}
    return _REFERENCE["over_the_cap"]


@pytest.fixture(scope="module")
def ragged(hsv, oracle_lib):
    """257 ragged items and the oracle's flags (computed once, read-only);
    the smaller batches are prefixes."""
    return ragged_reference(oracle_lib)


def test_edge_vectors_as_32_byte_messages(hsv, golden):
    """Every record of tests/golden/edge_vectors.json with msg_len = 32: all 8
    flag bits, at the fixed stride and through offsets."""
    import ctypes
    from hsverify import verifier
    n = golden["n_edge"]
    pk, sig = golden["pk"][:n].copy(), golden["sig"][:n].copy()
    msg = np.ascontiguousarray(golden["msg"][:n])
    exp = golden["flags"][:n]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    got = np.zeros(n, np.uint8)
    assert hsv.hsv_verify_msgs(p(pk), p(sig), p(msg), None, 32, 32, n, p(got)) == 0
    assert (got == exp).all(), [(golden["cases"][i], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
    offsets = np.arange(n + 1, dtype=np.uint64) * 32
    got = verifier.verify_msgs(pk, sig, (msg.reshape(-1), offsets))
    assert (got == exp).all(), [(golden["cases"][i], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
    for kw in ({"msg_len": 32}, {"offsets": offsets}):
        flags, bits, fault = run_device(pk, sig, msg.reshape(-1), shift=0, **kw)
        assert (flags == exp).all() and (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0], kw


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_unaligned_batches(hsv, ragged, n):
    """Lengths mix inside a wave; messages packed back to back from a base
    pointer 1..15 bytes past a 16-byte boundary.  Host form, and the device
    form with and without strict bits."""
    from hsverify import verifier
    pk, sig, msgs, exp = ragged["pk"][:n], ragged["sig"][:n], ragged["msgs"][:n], ragged["exp"][:n]
    got = verifier.verify_msgs(pk, sig, msgs)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    buf, offsets = verifier.pack_msgs(msgs)
    shift = 1 + (n * 7) % 15
    flags, bits, fault = run_device(pk, sig, buf, offsets, shift=shift)
    assert (flags == exp).all(), np.nonzero(flags != exp)[0][:8]
    assert (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]
    flags, _, fault = run_device(pk, sig, buf, offsets, shift=16 - shift, want_bits=False)
    assert (flags == exp).all() and fault == [0, 0]
    _, bits, fault = run_device(pk, sig, buf, offsets, shift=shift, want_flags=False)
    assert (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]


@pytest.mark.parametrize("length", [0, 1, 200])
def test_one_shared_message(hsv, oracle_lib, length):
    """msg_stride = 0: 67 signers over one message."""
    import ctypes
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(52 + length)
    n = 67
    msg = rnd.integers(0, 256, length, dtype=np.uint8)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    pk, sig = sign_many(seeds, np.repeat(msg[None], n, 0))
    sig[5, 33] ^= 1
    pk[40] = pk[41]
    exp = oracle_msgs(oracle_lib, pk, sig, [msg.tobytes()] * n)
    assert (exp & o.STRICT_OK).sum() == n - 2
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    got = np.zeros(n, np.uint8)
    assert hsv.hsv_verify_msgs(p(pk), p(sig), p(msg) if length else None, None, length, 0, n, p(got)) == 0
    assert (got == exp).all()
    flags, bits, fault = run_device(pk, sig, msg, shift=3, msg_len=length, msg_stride=0)
    assert (flags == exp).all() and (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]


def test_fallback_path_reads_k_from_the_record(hsv, oracle_lib):
    """With the lattice bound lowered to 128 bits about one item in seven has
    no short pair (278 of 2,000 random challenges, counted with
    tests/native/msg_host.cpp --prep 128) and takes the full-length path, whose
    k mod l the point pass reads from the prepass record (the only cover of
    that path)."""
    from hsverify import _testing
    pk, sig, msgs, bad = ragged_batch(53, 257)
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    from hsverify import verifier
    buf, offsets = verifier.pack_msgs(msgs)
    with _testing.test_library():
        prev = _testing.set_lattice_bits(128)
        try:
            flags, bits, fault = run_device(pk, sig, buf, offsets, shift=9)
            got_host = verifier.verify_msgs(pk, sig, msgs)
        finally:
            _testing.set_lattice_bits(prev)
    assert (flags == exp).all(), np.nonzero(flags != exp)[0][:8]
    assert (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]
    assert (got_host == exp).all()


def test_one_long_message_among_short_ones(hsv, oracle_lib):
    """130 items: one message of 1 MiB, the rest 32 bytes.  Only its own wave
    of the prepass loops over it; the point pass never reads a message."""
    from hsverify import verifier
    rnd = np.random.default_rng(54)
    n = 130
    msgs = [rnd.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    msgs[70] = rnd.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    pk, sig = sign_ragged(seeds, msgs)
    sig[3, 40] ^= 1
    exp = oracle_msgs(oracle_lib, pk, sig, msgs)
    assert (exp & o.STRICT_OK).sum() == n - 1 and exp[70] & o.STRICT_OK
    buf, offsets = verifier.pack_msgs(msgs)
    flags, bits, fault = run_device(pk, sig, buf, offsets, shift=7)
    assert (flags == exp).all() and (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]
    m = bytearray(msgs[70])
    m[-1] ^= 1                                  # the last byte of the long message counts
    msgs[70] = bytes(m)
    got = verifier.verify_msgs(pk, sig, msgs)
    exp2 = exp.copy()
    exp2[70] = oracle_msgs(oracle_lib, pk[70:71], sig[70:71], msgs[70:71])[0]
    assert not (exp2[70] & o.STRICT_OK) and (got == exp2).all()


def test_decreasing_offsets(hsv, oracle_lib, ragged):
    """Device form: the item whose offsets decrease gets flags 0, its
    neighbours the oracle's flags.  Host form: HSV_ERR_INVALID_ARG."""
    from hsverify import _lib, verifier
    n = 65
    pk, sig, msgs, exp = ragged["pk"][:n], ragged["sig"][:n], ragged["msgs"][:n], ragged["exp"][:n].copy()
    buf, offsets = verifier.pack_msgs(msgs)
    # offsets[victim + 1] one below offsets[victim]: the victim's pair decreases, and
    # the next item's message starts one byte early (the oracle says what that gives)
    victim = 21
    off = offsets.copy()
    assert off[victim] > 0
    off[victim + 1] = off[victim] - 1
    exp[victim] = 0
    nxt = buf[int(off[victim + 1]):int(off[victim + 2])].tobytes()
    exp[victim + 1] = oracle_lib.oracle_verify_flags(pk[victim + 1].tobytes(), sig[victim + 1].tobytes(), nxt, len(nxt))
    flags, bits, fault = run_device(pk, sig, buf, off, shift=5)
    assert (flags == exp).all(), np.nonzero(flags != exp)[0][:8]
    assert (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0]
    assert flags[victim] == 0 and flags[victim - 1] == ragged["exp"][victim - 1]
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        verifier.verify_msgs(pk, sig, (buf, off))


@pytest.mark.parametrize("length", [0, 47, 176, 1000])
def test_round_trip_with_the_gpu_signer(hsv, oracle_lib, length):
    """Signer.sign_device writes into packed pk || R || s records and
    verify_msgs_device runs next on the same stream, no synchronisation
    between them.  Flipping one message byte clears exactly that item."""
    import torch
    from hsverify import Signer, verifier
    rnd = np.random.default_rng(55 + length)
    m = 70
    seeds = rnd.integers(0, 256, (m, 32), dtype=np.uint8)
    msgs = rnd.integers(0, 256, (m, length), dtype=np.uint8)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with Signer(seeds) as s:
        pks = s.public_keys()
        with torch.cuda.stream(st):
            raw = torch.zeros(m * length + 19, dtype=torch.uint8, device=dev)
            d_msgs = raw[3:3 + m * length].view(m, length)
            d_msgs.copy_(torch.from_numpy(msgs))
            rec = torch.zeros((m, 96), dtype=torch.uint8, device=dev)
            rec[:, :32] = torch.from_numpy(pks).to(dev)
            flags = torch.zeros(m, dtype=torch.uint8, device=dev)
            flags2 = torch.zeros(m, dtype=torch.uint8, device=dev)
            f_sign = torch.ones(2, dtype=torch.int32, device=dev)
            f_ver = torch.ones(2, dtype=torch.int32, device=dev)
            s.sign_device(d_msgs, rec[:, 32:], msg_len=length, fault=f_sign)
            verifier.verify_msgs_device(rec[:, :32], rec[:, 32:], raw[3:], msg_len=length, flags=flags, fault=f_ver)
            if length:
                raw[3 + 17 * length + length // 2] ^= 1       # a byte of message 17
                verifier.verify_msgs_device(rec[:, :32], rec[:, 32:], raw[3:], msg_len=length, flags=flags2)
        st.synchronize()
    got_rec = rec.cpu().numpy()
    exp = oracle_msgs(oracle_lib, got_rec[:, :32], got_rec[:, 32:], [msgs[i].tobytes() for i in range(m)])
    assert (exp & o.STRICT_OK).all()
    assert (flags.cpu().numpy() == exp).all()
    assert f_sign.cpu().tolist() == [0, 0] and f_ver.cpu().tolist() == [0, 0]
    if length:
        msgs[17, length // 2] ^= 1
        exp2 = oracle_msgs(oracle_lib, got_rec[:, :32], got_rec[:, 32:], [msgs[i].tobytes() for i in range(m)])
        assert [i for i in range(m) if not exp2[i] & o.STRICT_OK] == [17]
        assert (flags2.cpu().numpy() == exp2).all()


def test_batches_above_one_launch(hsv):
    """2^22 + 65 items over one shared 32-byte message run as two launches;
    one corrupted item on each side of the seam.  The yardstick here is
    hsv_verify_device on the same triples (the oracle would take minutes)."""
    import torch
    from hsverify import Signer, verifier
    rnd = np.random.default_rng(56)
    m = (1 << 22) + 65
    seeds = rnd.integers(0, 256, (1024, 32), dtype=np.uint8)
    digest = rnd.integers(0, 256, 32, dtype=np.uint8)
    idx = (np.arange(m) % 1024).astype(np.uint32)
    with Signer(seeds) as s:
        pks = s.public_keys()
        sig = s.sign(digest, idx)
    sig[(1 << 22) - 1, 35] ^= 1
    sig[(1 << 22) + 1, 2] ^= 1
    dev = torch.device("cuda:0")
    d_pk = torch.from_numpy(pks).to(dev)[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous()
    d_sig = torch.from_numpy(sig).to(dev)
    backing = torch.zeros(48, dtype=torch.uint8, device=dev)
    backing[16:48].copy_(torch.from_numpy(digest))
    ref = torch.zeros(m, dtype=torch.uint8, device=dev)
    got = torch.zeros(m, dtype=torch.uint8, device=dev)
    bits = torch.zeros((m + 31) // 32, dtype=torch.int32, device=dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    verifier.verify_device(d_pk, d_sig, backing[16:48], flags=ref)
    verifier.verify_msgs_device(d_pk, d_sig, backing[16:48], msg_len=32, msg_stride=0, flags=got, strict_bits=bits,
                                fault=fault)
    torch.cuda.synchronize()
    ref, got = ref.cpu().numpy(), got.cpu().numpy()
    assert (got == ref).all(), np.nonzero(got != ref)[0][:8]
    rejected = np.nonzero((ref & o.STRICT_OK) == 0)[0].tolist()
    assert rejected == [(1 << 22) - 1, (1 << 22) + 1]
    assert (unpack_bits(bits, m) == (ref & o.STRICT_OK)).all() and fault.cpu().tolist() == [0, 0]


def test_agrees_with_the_32_byte_path(hsv):
    """2^15 random 32-byte triples with the usual corruption mix: identical
    flags and strict bits from hsv_verify_msgs_device and hsv_verify_device."""
    import torch
    from hsverify import synth, verifier
    w = synth.independent_triples(1 << 15, seed=57, corrupt_frac=0.05)
    dev = torch.device("cuda:0")
    d_pk, d_sig, d_msg = (torch.from_numpy(a).to(dev) for a in (w.pk, w.sig, w.msg))
    n = w.n
    out = []
    for fn, kw in ((verifier.verify_device, {}), (verifier.verify_msgs_device, {"msg_len": 32})):
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        bits = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
        fault = torch.ones(2, dtype=torch.int32, device=dev)
        fn(d_pk, d_sig, d_msg if not kw else d_msg.view(-1), flags=flags, strict_bits=bits, fault=fault, **kw)
        torch.cuda.synchronize()
        assert fault.cpu().tolist() == [0, 0]
        out.append((flags.cpu().numpy(), bits.cpu().numpy()))
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all()
    assert ((out[0][0] & o.STRICT_OK) != 0).tolist() == w.accept.tolist()


def test_host_form_across_its_byte_cap(hsv, oracle_lib, ragged):
    """The host form stages at most 2^29 message bytes per launch; the test
    library's hsv_test_stage_bytes lowers that to 4096.  The 257 ragged,
    unaligned messages then take a dozen launches, each with its offsets
    rebased to its first byte, and one message of 5000 bytes -- longer than
    the cap -- goes alone.  Flags equal the oracle's, and those of the same
    call at the product's cap."""
    from hsverify import _testing, verifier
    ref = ragged_over_the_cap(oracle_lib)
    pk, sig, msgs, exp = ref["pk"], ref["sig"], ref["msgs"], ref["exp"]
    with _testing.test_library() as lib:
        whole = verifier.verify_msgs(pk, sig, msgs)
        assert lib.hsv_test_stage_bytes(4096) == 1 << 29
        try:
            got = verifier.verify_msgs(pk, sig, msgs)
        finally:
            assert lib.hsv_test_stage_bytes(0) == 4096
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert (got == whole).all()
