"""Batch key derivation and signing on the GPU (hsv_signer_*): byte for byte
the host signer's (hsv_sign_many) keys and signatures, at every item count
where the kernels' grouping changes shape and every message length where a
SHA-512 padding boundary falls."""
import ctypes

import numpy as np
import pytest

from test_sign_host import RFC8032

pytestmark = pytest.mark.gpu

# 32 + len and 64 + len bytes hashed: 32 is the one-block fast path, 48 closes
# the second hash's block (112), 80 the first's, 112 / 416 span blocks
LENS = (0, 32, 48, 80, 112, 416)


@pytest.fixture(scope="module")
def group(hsv):
    """G of the product launches: items per lane, 64 G per wave."""
    from hsverify import _lib
    return _lib.load_test().hsv_test_signer_group(0)


@pytest.fixture(scope="module")
def ref(hsv, group):
    """One pool of seeds and, per message length, messages with the host
    signer's keys and signatures (computed once, read-only)."""
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(41)
    n = max(4097, 64 * group + 1)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    out = {"n": n, "seeds": seeds, "msgs": {}, "sig": {}}
    for length in LENS:
        msgs = rnd.integers(0, 256, (n, length), dtype=np.uint8)
        pk, sig = sign_many(seeds, msgs)
        out["msgs"][length], out["sig"][length], out["pk"] = msgs, sig, pk
    for a in (seeds, out["pk"], *out["msgs"].values(), *out["sig"].values()):
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def signer(ref):
    from hsverify import Signer
    with Signer(ref["seeds"]) as s:
        yield s


def sizes(group):
    return (1, 63, 65, 64 * group - 1, 64 * group + 1, 4097)


def test_public_keys_match_host_signer(ref, group, signer):
    from hsverify import Signer
    for n in (1, 63, 65, 64 * group + 1):
        with Signer(ref["seeds"][:n]) as s:
            assert len(s) == n
            assert (s.public_keys() == ref["pk"][:n]).all(), n
    assert (signer.public_keys() == ref["pk"]).all()
    with Signer(np.zeros((0, 32), np.uint8)) as s:  # an empty signer is valid
        assert len(s) == 0 and s.public_keys().shape == (0, 32)
        assert s.sign(np.zeros((0, 32), np.uint8)).shape == (0, 64)


@pytest.mark.parametrize("length", LENS)
def test_sign_matches_host_signer(ref, group, signer, length):
    """key_idx = None: item i signs with key i."""
    for m in sizes(group):
        got = signer.sign(ref["msgs"][length][:m])
        bad = np.nonzero((got != ref["sig"][length][:m]).any(axis=1))[0]
        assert bad.size == 0, (length, m, bad[:8].tolist())


@pytest.mark.parametrize("length", (32, 80))
def test_key_index_with_repeats_and_one_out_of_range(ref, group, signer, length):
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(42)
    m = 64 * group + 1
    idx = rnd.integers(0, 50, m).astype(np.uint32)  # 50 keys over m items: many repeats
    victim = m // 2
    msgs = ref["msgs"][length][:m]
    _, exp = sign_many(ref["seeds"][idx], msgs)
    idx[victim] = ref["n"]                          # first index past the keys
    exp[victim] = 0
    got = signer.sign(msgs, idx)
    assert (got == exp).all()
    idx[victim] = 0xffffffff
    assert (signer.sign(msgs, idx) == exp).all()


@pytest.mark.parametrize("length", (32, 48))
def test_one_shared_message(ref, signer, length):
    """msg_stride == 0: a committee signing one digest."""
    from hsverify.verifier import sign_many
    msg = ref["msgs"][length][7]
    m = 131
    _, exp = sign_many(ref["seeds"][:m], np.repeat(msg[None], m, 0))
    assert (signer.sign(msg, np.arange(m, dtype=np.uint32)) == exp).all()
    idx = np.array([5, 5, 0, 130, 5], np.uint32)
    assert (signer.sign(msg, idx) == exp[idx]).all()


@pytest.mark.parametrize("length", (32, 80))
def test_unaligned_messages_into_packed_vote_records(ref, group, signer, length):
    """Device form: messages at an odd address, signatures written at stride
    96 into pk || R || s records; the pk part and the bytes between rows stay."""
    import torch
    m = 64 * group + 1
    dev = torch.device("cuda:0")
    raw = torch.zeros(m * length + 3, dtype=torch.uint8, device=dev)
    msg = raw[3:].view(m, length)
    msg.copy_(torch.from_numpy(ref["msgs"][length][:m].copy()))
    assert msg.data_ptr() % 4 == 3
    rec = torch.full((m, 96), 0xa5, dtype=torch.uint8, device=dev)
    rec[:, :32] = torch.from_numpy(ref["pk"][:m].copy()).to(dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    signer.sign_device(msg, rec[:, 32:], fault=fault)
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    assert (got[:, :32] == ref["pk"][:m]).all()
    assert (got[:, 32:] == ref["sig"][length][:m]).all()
    assert fault.cpu().tolist() == [0, 0]


def test_rfc8032_vectors(hsv):
    from hsverify import Signer
    for seed, pk, msg, sig in RFC8032:
        with Signer(bytes.fromhex(seed)) as s:
            assert bytes(s.public_keys()[0]) == bytes.fromhex(pk)
            m = np.frombuffer(bytes.fromhex(msg), np.uint8).reshape(1, -1)
            assert bytes(s.sign(m)[0]) == bytes.fromhex(sig)


def test_more_items_than_keys_needs_an_index(ref):
    from hsverify import Signer, _lib
    with Signer(ref["seeds"][:2]) as s:
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            s.sign(ref["msgs"][32][:3])
        assert (s.sign(ref["msgs"][32][:3], [0, 1, 0])[2] == s.sign(ref["msgs"][32][2:3], [0])[0]).all()


def test_sign_then_verify_on_one_stream(ref, group, signer):
    """sign_device and verify_device enqueued back to back, no synchronisation
    between them: the verifier reads what the signer wrote."""
    import torch
    from hsverify import STRICT_OK, verifier
    m = 64 * group + 1
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        pk = torch.from_numpy(ref["pk"][:m].copy()).to(dev, non_blocking=False)
        msg = torch.from_numpy(ref["msgs"][32][:m].copy()).to(dev)
        sig = torch.zeros((m, 64), dtype=torch.uint8, device=dev)
        flags = torch.zeros(m, dtype=torch.uint8, device=dev)
        f_sign = torch.ones(2, dtype=torch.int32, device=dev)
        f_ver = torch.ones(2, dtype=torch.int32, device=dev)
        signer.sign_device(msg, sig, fault=f_sign)
        verifier.verify_device(pk, sig, msg, flags=flags, fault=f_ver)
    st.synchronize()
    assert (flags.cpu().numpy() & STRICT_OK).all()
    assert f_sign.cpu().tolist() == [0, 0] and f_ver.cpu().tolist() == [0, 0]
    assert (sig.cpu().numpy() == ref["sig"][32][:m]).all()


def test_committee_signatures_pass_the_drop_in(hsv, ref):
    """67 members sign one QC digest; crypto::Signature::verify_batch's drop-in accepts."""
    from hsverify import Signer
    digest = np.ascontiguousarray(ref["msgs"][32][11])
    with Signer(ref["seeds"][:67]) as s:
        sigs = s.sign(digest)
        pks = s.public_keys()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert hsv.hsv_verify_batch(p(digest), p(pks), p(sigs), 67) == 1
    sigs[40, 3] ^= 1
    assert hsv.hsv_verify_batch(p(digest), p(pks), p(sigs), 67) == 0


def test_batches_above_one_launch(hsv, ref):
    """More than 2^22 items run as several launches; the second starts at the
    right key, message and signature.  Checked against the host signer at the
    seam (the only size at which this path exists), and the implicit key index
    against the explicit one everywhere."""
    from hsverify import Signer, crypto
    rnd = np.random.default_rng(43)
    m = (1 << 22) + 65
    seeds = rnd.integers(0, 256, (m, 32), dtype=np.uint8)
    digest = np.ascontiguousarray(ref["msgs"][32][3])
    with Signer(seeds) as s:
        pks = s.public_keys()
        implicit = s.sign(digest)
        explicit = s.sign(digest, np.arange(m, dtype=np.uint32))
    assert (implicit == explicit).all()
    for i in (0, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, m - 1):
        assert bytes(pks[i]) == crypto.public_key_from_seed(bytes(seeds[i])).data, i
        sig = (ctypes.c_uint8 * 64)()
        assert hsv.hsv_sign(bytes(seeds[i]), bytes(digest), 32, sig) == 0
        assert bytes(implicit[i]) == bytes(sig), i


def test_every_built_group_signs_the_same(ref):
    """The measurement hook's other G (1 = one inversion per item ... 16): same bytes."""
    from hsverify import Signer, _testing
    m = 64 * 16 + 1
    with _testing.test_library() as lib:
        try:
            for g in (1, 2, 4, 8, 16):
                assert lib.hsv_test_signer_group(g) > 0
                with Signer(ref["seeds"][:m]) as s:
                    assert (s.public_keys() == ref["pk"][:m]).all(), g
                    for length in (32, 48):
                        assert (s.sign(ref["msgs"][length][:m]) == ref["sig"][length][:m]).all(), (g, length)
        finally:
            lib.hsv_test_signer_group(0)
