"""The staged host forms across their byte cap, and the device forms' stream check.

hsv_verify_transactions*, hsv_verify_msgs and hsv_signer_sign_transactions
stage at most 2^29 bytes per launch, which no quick test reaches.  The test
library's hsv_test_stage_bytes lowers that cap to 4096 bytes, so a few hundred
items take many launches: every launch after the first starts at its own item,
key and byte, and a ragged one gets offsets rebased to its first byte
(csrc/hsv_batch.hpp; the walk itself is checked on the CPU by
tests/test_batch_host.py).  hsv_verify_msgs' case is in tests/test_verify_msgs.py,
next to its fixture.  The committee host forms (hsv_committee_verify_transactions,
hsv_committee_verify_msgs) run the same two walks and take the same inputs
over many launches here; their list lengths accumulate over a call's launches.
"""
import contextlib

import numpy as np
import pytest

from conftest import oracle_tx_flags
from test_txsign import FILL, sign_list, sign_rows
from test_verify_msgs import ragged_over_the_cap

pytestmark = pytest.mark.gpu

CAP = 4096
N = 257


@contextlib.contextmanager
def stage_cap(cap=CAP, items=0):
    """hsverify calls run on the test library with its byte cap (and, for
    hsv_signer_sign_transactions, its items per launch) lowered."""
    from hsverify import _testing
    with _testing.test_library() as lib:
        assert lib.hsv_test_stage_bytes(cap) == 1 << 29
        if items:
            assert lib.hsv_test_tx_sign_chunk(items) == 1 << 22
        try:
            yield lib
        finally:
            lib.hsv_test_tx_sign_chunk(0)
            assert lib.hsv_test_stage_bytes(0) == cap


def test_verify_ragged_golden_transactions_over_many_launches(hsv, oracle_lib, tx_golden):
    """47 transactions of 96..1096 bytes, 17157 in all: five launches."""
    from hsverify import mempool
    buf, offsets = mempool.pack(tx_golden["txs"])
    exp = oracle_tx_flags(oracle_lib, buf, offsets)
    assert (exp == tx_golden["flags"]).all()
    with stage_cap():
        got = mempool.verify_transactions(tx_golden["txs"])
    assert (got == exp).all(), [(tx_golden["cases"][i], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]


@pytest.mark.parametrize("size", [97, 512])
def test_verify_fixed_size_transactions_over_many_launches(hsv, oracle_lib, size):
    """257 transactions: 42 per launch at 97 bytes, 8 at 512; the last launch
    is a short one."""
    from hsverify import mempool, synth
    w = synth.transactions(N, tx_size=size, seed=size, corrupt_frac=0.1)
    exp = oracle_tx_flags(oracle_lib, w.txs.reshape(-1), tx_size=size, n=N)
    assert 0 < (exp & 1).sum() < N
    with stage_cap():
        got = mempool.verify_transactions_fixed(w.txs)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]


# ---- the committee host forms: the same walks, the same inputs ---------------------
def _committee(keys, compact=False):
    from hsverify.committee import Committee
    return Committee(np.ascontiguousarray(keys, np.uint8).reshape(-1, 32), compact=compact)


def test_committee_verify_ragged_golden_transactions_over_many_launches(hsv, oracle_lib, tx_golden):
    """The 47 golden transactions in five launches against every second
    distinct key: the golden flags, those of mempool.verify_transactions under
    the same cap, and list lengths summed over the launches."""
    from hsverify import _testing, mempool
    txs, want = tx_golden["txs"], tx_golden["flags"]
    assert len(txs) == 47 and sum(len(t) for t in txs) == 17157
    pks = [t[-96:-64] for t in txs]
    half = set(list(dict.fromkeys(pks))[::2])
    n_half = sum(p in half for p in pks)
    assert 0 < n_half < 47
    with stage_cap(), _committee(np.frombuffer(b"".join(sorted(half)), np.uint8)) as c:
        got = c.verify_transactions(txs)
        counts = _testing.committee_tx_counts()
        generic = mempool.verify_transactions(txs)
    assert (got == want).all(), [(tx_golden["cases"][i], int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]
    assert (got == generic).all()
    assert counts[:2] == (n_half, 47 - n_half)


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
@pytest.mark.parametrize("size", [97, 512])
def test_committee_verify_fixed_size_transactions_over_many_launches(hsv, oracle_lib, size, compact):
    """257 transactions, 42 or 8 per launch, the first 128 rows' keys the
    committee."""
    from hsverify import _testing, synth
    w = synth.transactions(N, tx_size=size, seed=size, corrupt_frac=0.1)
    exp = oracle_tx_flags(oracle_lib, w.txs.reshape(-1), tx_size=size, n=N)
    assert 0 < (exp & 1).sum() < N
    with stage_cap(), _committee(w.txs[:128, size - 96:size - 64], compact=compact) as c:
        got = c.verify_transactions_fixed(w.txs)
        counts = _testing.committee_tx_counts()
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert counts[0] + counts[1] == N


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_committee_verify_ragged_msgs_over_many_launches(hsv, oracle_lib, compact):
    """The 257 ragged messages of test_verify_msgs.py's case, the 5000-byte one
    alone in its launch, against half of the distinct keys."""
    from hsverify import _testing, verifier
    ref = ragged_over_the_cap(oracle_lib)
    pk, sig, msgs, exp = ref["pk"], ref["sig"], ref["msgs"], ref["exp"]
    distinct = list(dict.fromkeys(bytes(k) for k in pk))
    with stage_cap(), _committee(np.frombuffer(b"".join(distinct[::2]), np.uint8), compact=compact) as c:
        got = c.verify_msgs(pk, sig, msgs)
        counts = _testing.committee_msgs_counts()
        generic = verifier.verify_msgs(pk, sig, msgs)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert (got == generic).all()
    assert counts[0] + counts[1] == len(msgs) == N


@pytest.fixture(scope="module")
def sign_ref(hsv):
    """257 seeds; per fixed size the unsigned rows and the host signer's
    bytes, with item i under key i and under a key index with repeats; one
    ragged batch likewise (computed once, read-only)."""
    from hsverify.verifier import sign_many
    rnd = np.random.default_rng(61)
    seeds = rnd.integers(0, 256, (N, 32), dtype=np.uint8)
    idx = rnd.integers(0, 40, N).astype(np.uint32)
    out = {"seeds": seeds, "idx": idx, "raw": {}, "own": {}, "indexed": {}}
    for size in (97, 512):
        raw = np.full((N, size), FILL, np.uint8)
        raw[:, :size - 96] = rnd.integers(0, 256, (N, size - 96), dtype=np.uint8)
        out["raw"][size] = raw
        out["own"][size] = sign_rows(sign_many, seeds, raw)
        out["indexed"][size] = sign_rows(sign_many, seeds[idx], raw)
    lens = rnd.choice(np.array([0, 1, 111, 112, 240, 416]), N)
    lens[131] = 5000   # longer than the cap: alone in its launch
    msgs = [rnd.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    out["msgs"] = msgs
    out["ragged_own"] = sign_list(seeds, msgs)
    out["ragged_indexed"] = sign_list(seeds[idx], msgs)
    for a in (seeds, idx, *out["raw"].values(), *out["own"].values(), *out["indexed"].values()):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("items", [0, 64])
@pytest.mark.parametrize("size", [97, 512])
def test_sign_fixed_size_transactions_over_many_launches(sign_ref, size, items):
    """Bytes equal the host signer's, message bytes included, with the key of
    item i implicit (launch k starts at key a_k) and explicit."""
    from hsverify import Signer
    raw = sign_ref["raw"][size]
    with stage_cap(items=items), Signer(sign_ref["seeds"]) as s:
        got = s.sign_transactions(raw)
        got_idx = s.sign_transactions(raw, key_idx=sign_ref["idx"])
    assert (got == sign_ref["own"][size]).all(), np.nonzero((got != sign_ref["own"][size]).any(axis=1))[0][:8]
    assert (got_idx == sign_ref["indexed"][size]).all()
    assert (got[:, :size - 96] == raw[:, :size - 96]).all() and (got_idx[:, :size - 96] == raw[:, :size - 96]).all()


@pytest.mark.parametrize("items", [0, 64])
def test_sign_ragged_transactions_over_many_launches(sign_ref, items):
    """Ragged, with empty messages and one transaction above the cap."""
    from hsverify import Signer
    msgs = sign_ref["msgs"]
    data = np.frombuffer(b"".join(m + bytes([FILL]) * 96 for m in msgs), np.uint8)
    offsets = np.cumsum([0] + [len(m) + 96 for m in msgs]).astype(np.uint64)
    with stage_cap(items=items), Signer(sign_ref["seeds"]) as s:
        got = bytes(s.sign_transactions(data, offsets=offsets))
        got_idx = bytes(s.sign_transactions(data, offsets=offsets, key_idx=sign_ref["idx"]))
    assert got == b"".join(sign_ref["ragged_own"])          # every byte: tails and messages
    assert got_idx == b"".join(sign_ref["ragged_indexed"])
    for i in (0, 131, N - 1):
        a = int(offsets[i])
        assert got[a:a + len(msgs[i])] == msgs[i]


# ---- a stream of another device ------------------------------------------------
def _second_device_stream():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    return torch.cuda.Stream(device=1)


def test_signer_sign_device_refuses_a_stream_of_another_device(hsv):
    import torch
    from hsverify import Signer, _lib
    stream = _second_device_stream()
    rnd = np.random.default_rng(62)
    with torch.cuda.device(0), Signer(rnd.integers(0, 256, (4, 32), dtype=np.uint8)) as s:
        msg = torch.from_numpy(rnd.integers(0, 256, (4, 32), dtype=np.uint8)).to("cuda:0")
        sig = torch.full((4, 64), 0xA5, dtype=torch.uint8, device="cuda:0")
        fault = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            s.sign_device(msg, sig, stream=stream.cuda_stream, fault=fault)
        torch.cuda.synchronize(0)
        stream.synchronize()
        assert (sig.cpu().numpy() == 0xA5).all() and fault.cpu().tolist() == [7, 7]
        s.sign_device(msg, sig)   # the device's own stream still works
        torch.cuda.synchronize(0)
        assert (sig.cpu().numpy() != 0xA5).any()


def test_committee_verify_device_refuses_a_stream_of_another_device(hsv, golden):
    import torch
    from hsverify import _lib, committee
    stream = _second_device_stream()
    with torch.cuda.device(0), committee.Committee(golden["pk"][:4]) as c:
        idx = torch.arange(4, dtype=torch.int32, device="cuda:0")
        sig = torch.from_numpy(golden["sig"][:4].copy()).to("cuda:0")
        msg = torch.from_numpy(golden["msg"][:4].copy()).to("cuda:0")
        flags = torch.full((4,), 0xA5, dtype=torch.uint8, device="cuda:0")
        fault = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
        with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
            c.verify_device(idx, sig, msg, flags, stream=stream.cuda_stream, fault=fault)
        torch.cuda.synchronize(0)
        stream.synchronize()
        assert (flags.cpu().numpy() == 0xA5).all() and fault.cpu().tolist() == [7, 7]
        c.verify_device(idx, sig, msg, flags)
        torch.cuda.synchronize(0)
        assert (flags.cpu().numpy() == golden["flags"][:4]).all()
