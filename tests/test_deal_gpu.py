"""The dealt point pass on the GPU: hsv_prep_kernel / hsv_msg_prep_kernel put
every item on the list of its column class, hsv_verify_hp_kernel takes 64-item
batches from the lists, longest need first (csrc/hsv_pointpass.hpp deal_append,
DealOffsets), over 2-bit columns with digits in {-1 .. 2}
(csrc/hsv_verify_hc.hpp recode_cols).  Flags and STRICT_OK bits against the
oracle, dealt and in index order (the test library's hsv_test_deal), and the
class lists' lengths against a host histogram.  tests/test_cols_host.py checks
the same headers on the host.
"""
import hashlib
import subprocess

import numpy as np
import pytest

import ed25519_ref as o
from conftest import oracle_flags, oracle_tx_flags

pytestmark = pytest.mark.gpu

N_MIXED = 8192 + 577  # just above the small forms' 2^13: 138 batches, the last one partial
N_EDGE = 8192 + 1     # the last batch is one item and 63 idle lanes
L = 2**252 + 27742317777372353535851937790883648493


def _unpack_bits(bits, n):
    b = bits.cpu().numpy().view(np.uint32)
    return ((b[np.arange(n) // 32] >> (np.arange(n) % 32)) & 1).astype(np.uint8)


def _run(pk, sig, msg):
    """hsv_verify_device_bits on cuda:0: (flags, unpacked STRICT_OK bits, bits
    past the batch's end, fault words)."""
    import torch
    from hsverify import verifier
    dev = torch.device("cuda:0")
    n = pk.shape[0]
    t = [torch.from_numpy(np.array(x)).to(dev) for x in (pk, sig, msg)]  # a copy: the reference is read-only
    flags = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    verifier.verify_device(t[0], t[1], t[2], flags, bits, fault=fault)
    torch.cuda.synchronize()
    words = bits.cpu().numpy().view(np.uint32)
    tail = int(words[-1] >> (n % 32)) if n % 32 else 0
    return flags.cpu().numpy(), _unpack_bits(bits, n), tail, fault.cpu().tolist()


@pytest.fixture(scope="module")
def tlib(hsv):
    """The test library (default variant: the two launches above 2^13 items),
    committee cache off."""
    from hsverify import _testing
    with _testing.test_library() as lib:
        lib.hsv_set_auto_committee(0)
        try:
            yield lib
        finally:
            _testing.set_deal(_testing.DEAL_ON)
            lib.hsv_set_auto_committee(1)


@pytest.fixture(scope="module")
def mixed(oracle_lib, fallback_records):
    """8192 + 577 seeded triples, 10 % corrupted so that every kind of synth
    occurs many times, with the oracle's flags; and the same batch with the
    lattice-fallback fixtures at random places.  Computed once, read-only."""
    from hsverify import synth
    w = synth.independent_triples(N_MIXED, seed=0xdea1, corrupt_frac=0.10, nthreads=8)
    assert set(w.kind[w.kind >= 0].tolist()) == set(range(len(synth.CORRUPTIONS)))
    exp = oracle_flags(oracle_lib, w.pk, w.sig, w.msg)
    fb = fallback_records
    pos = np.sort(np.random.default_rng(0xfb).choice(N_MIXED, 150, replace=False))
    src = np.arange(pos.size) % len(fb["flags"])
    pk, sig, msg, fexp = w.pk.copy(), w.sig.copy(), w.msg.copy(), exp.copy()
    pk[pos], sig[pos], msg[pos], fexp[pos] = fb["pk"][src], fb["sig"][src], fb["msg"][src], fb["flags"][src]
    out = {"plain": (w.pk, w.sig, w.msg, exp), "fallback": (pk, sig, msg, fexp)}
    for arrs in out.values():
        for a in arrs:
            a.setflags(write=False)
    return out


def _both_orders(pk, sig, msg, exp):
    from hsverify import _testing
    res = {}
    for mode in (_testing.DEAL_ON, 0):
        prev = _testing.set_deal(mode)
        try:
            res[mode] = _run(pk, sig, msg)
        finally:
            _testing.set_deal(prev)
        flags, bits, tail, fault = res[mode]
        bad = np.nonzero(flags != exp)[0]
        assert bad.size == 0, (mode, [(int(i), hex(flags[i]), hex(exp[i])) for i in bad[:8]])
        assert (bits == (exp & o.STRICT_OK)).all() and tail == 0, mode
        assert fault == [0, 0], mode
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()


def test_mixed_batch_dealt_and_in_index_order(tlib, mixed):
    """Every corruption kind of synth at 8192 + 577 items: flags and STRICT_OK
    bits bit-exact against the oracle with dealing on and off, and the two
    runs identical."""
    pk, sig, msg, exp = mixed["plain"]
    assert 0.85 * N_MIXED < int((exp & o.STRICT_OK).sum()) < N_MIXED
    _both_orders(pk, sig, msg, exp)


def test_fallback_list_and_classes_together(tlib, mixed):
    """The same batch with the lattice-fallback fixtures mixed in and the bound
    lowered to 133: full-length batches first, then the class lists."""
    from hsverify import _testing
    pk, sig, msg, exp = mixed["fallback"]
    prev = _testing.set_lattice_bits(133)
    try:
        _both_orders(pk, sig, msg, exp)
    finally:
        _testing.set_lattice_bits(prev)


def test_partial_and_straddling_batches(tlib, mixed):
    """8192 + 1 items: the last batch is almost all idle lanes, and every class
    but the last ends inside a batch."""
    pk, sig, msg, exp = (a[:N_EDGE] for a in mixed["plain"])
    _both_orders(pk, sig, msg, exp)


def test_whole_messages_krec_point_pass(tlib, oracle_lib):
    """verify_msgs at 2^13 + 65 ragged items (hsv_msg_prep_kernel writes the
    records and the lists, the KREC point pass reads them), dealt and in index
    order, against the oracle."""
    from hsverify import _testing
    from test_verify_msgs import ragged_reference, run_device
    ref = ragged_reference(oracle_lib)
    n = (1 << 13) + 65
    idx = np.arange(n) % len(ref["msgs"])
    msgs = [ref["msgs"][i] for i in idx]
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs])
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    exp = ref["exp"][idx]
    got = {}
    for mode in (_testing.DEAL_ON, 0):
        prev = _testing.set_deal(mode)
        try:
            flags, bits, fault = run_device(ref["pk"][idx], ref["sig"][idx], buf, offsets, shift=3)
        finally:
            _testing.set_deal(prev)
        assert (flags == exp).all(), (mode, np.nonzero(flags != exp)[0][:8])
        assert (bits == (exp & o.STRICT_OK)).all() and fault == [0, 0], mode
        got[mode] = flags
    assert (got[0] == got[1]).all()


def test_transactions_fused_launch_reads_the_new_digits(tlib, oracle_lib):
    """verify_transactions_device at 2^13 + 65: the fused launch keeps index
    order; its record phase writes and its point phase reads the {-1 .. 2}
    columns.  Against the oracle."""
    import torch
    from hsverify import mempool, synth
    n = (1 << 13) + 65
    w = synth.transactions(n, tx_size=200, seed=0xdea2, corrupt_frac=0.05, nthreads=8)
    exp = oracle_tx_flags(oracle_lib, w.txs.reshape(-1), None, 200, w.n)
    d = torch.from_numpy(w.txs.reshape(-1)).to("cuda:0")
    f = torch.full((n,), 0xff, dtype=torch.uint8, device="cuda:0")
    fault = torch.ones(2, dtype=torch.int32, device="cuda:0")
    mempool.verify_transactions_device(d, None, tx_size=200, n=n, flags=f, fault=fault)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert fault.cpu().tolist() == [0, 0]


def _cols(c):
    m = 0
    while 3 * c >= 2 * 4 ** m + 1:
        m += 1
    return m


def _host_histogram(pk, sig, msg, bits):
    """[items per class, longest first], fallback items: k with hashlib, the
    lattice pair with the host build of csrc/hsv_lattice.hpp."""
    from test_kernel_host import BIN, _build
    core = _build(BIN)
    ks = [int.from_bytes(hashlib.sha512(bytes(sig[i, :32]) + bytes(pk[i]) + bytes(msg[i])).digest(), "little") % L
          for i in range(len(pk))]
    out = subprocess.run([core, "--lattice", str(bits)], input="\n".join(f"{k:064x}" for k in ks) + "\n",
                         capture_output=True, text=True, check=True).stdout.split()
    hist, nfb = [0] * 6, 0
    for i in range(len(ks)):
        ok, c0, c1 = int(out[4 * i]), int(out[4 * i + 2], 16), int(out[4 * i + 3], 16)
        if not ok:
            nfb += 1
            continue
        hist[67 - min(max(_cols(c0), _cols(c1), 62), 67)] += 1
    return hist, nfb


@pytest.mark.parametrize("which,bits", [("plain", 138), ("fallback", 133)])
def test_class_counts_match_the_host_histogram(tlib, mixed, which, bits):
    """The lengths of the class lists after a launch (hsv_test_deal_counts)
    equal the histogram of max(cols(|c0|), cols(c1)) computed on the host; the
    fallback items are on no list; an index-order launch keeps no lists."""
    from hsverify import _testing
    pk, sig, msg, exp = mixed[which]
    hist, nfb = _host_histogram(pk, sig, msg, bits)
    assert sum(hist) + nfb == N_MIXED and (nfb >= 48 if which == "fallback" else nfb == 0)
    assert hist[3] > 0.4 * N_MIXED and hist[2] > 0.3 * N_MIXED  # 64 and 65 columns: 52 % and 41 %
    prev_bits = _testing.set_lattice_bits(0 if bits == 138 else bits)
    prev = _testing.set_deal(_testing.DEAL_ON | _testing.DEAL_COUNTS)
    try:
        flags, _, _, fault = _run(pk, sig, msg)
        counts = _testing.deal_counts()
        _testing.set_deal(_testing.DEAL_COUNTS)
        _run(pk, sig, msg)
        counts_off = _testing.deal_counts()
    finally:
        _testing.set_deal(prev)
        _testing.set_lattice_bits(prev_bits)
    assert (flags == exp).all() and fault == [0, 0]
    assert counts == hist, (counts, hist)
    assert counts_off == [0] * 6
