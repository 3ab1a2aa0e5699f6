"""The host forms of the benchmark's sample transactions (no GPU):
hsv_client_bursts against a line-by-line restatement of node/src/client.rs:121-135,
hsv_batch_samples_bincode against wire.decode_batch plus the filter of
mempool/src/batch_maker.rs:120-125 restated here, and hsverify.benchlog against
literal strings.  No expected value comes from the calls under test."""
import ctypes
import struct

import numpy as np
import pytest

FILL = 0xA5
M64 = 2**64


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def client_rs(n, size, burst, counter0, r0):
    """client.rs:121-135, n transactions' worth: one loop with `counter` and `r`.
    -> (transactions, the counters of the samples sent, r afterwards)"""
    txs, sent, counter, r = [], [], counter0, r0
    while len(txs) < n:
        for x in range(burst):
            if len(txs) == n:
                break
            if x == counter % burst:
                sent.append(counter)
                tx = bytes([0]) + struct.pack(">Q", counter)
            else:
                r = (r + 1) % M64
                tx = bytes([1]) + struct.pack(">Q", r)
            txs.append(tx + bytes(size - len(tx)))  # tx.resize(self.size, 0u8)
        counter = (counter + 1) % M64
    return txs, sent, r


def seal_filter(txs):
    """batch_maker.rs:120-125 and :116 -> (ids, size); an empty transaction, on
    which tx[0] would panic, is not a sample"""
    ids = [int.from_bytes(t[1:9], "big") for t in txs if len(t) > 8 and t[0] == 0]
    return ids, sum(len(t) for t in txs)


def run_bursts(lib, n, tx_size, trailer, counter0, burst, r0, base):
    """hsv_client_bursts into a filled buffer at byte `base` -> (rc, the whole buffer, r_out)"""
    raw = np.full(base + n * tx_size + 64 + 16, FILL, np.uint8)
    shift = (-raw.ctypes.data) % 16  # so that `base` is the address mod 16
    r = ctypes.c_uint64(12345)
    rc = lib.hsv_client_bursts(ctypes.c_void_p(raw.ctypes.data + shift + base), tx_size, trailer, counter0, burst, r0,
                               n, ctypes.byref(r))
    return rc, raw, shift + base, r.value


CASES = [  # n, tx_size, trailer, counter0, burst, r0
    (7, 9, 0, 0, 1, 0),
    (7, 105, 96, 5, 2, 7),
    (23, 128, 96, 3, 5, M64 - 2),       # n no multiple of burst; c % burst wraps 3, 4, 0, ..; r wraps
    (23, 105, 96, 3, 5, 0),
    (11, 128, 0, M64 - 2, 5, 1 << 63),  # the counter itself wraps inside the call
    (10, 9, 0, 9, 5, 0),
    (4, 512, 96, 1500, 1000, 99),       # one open burst whose sample (position 500) lies beyond n
]


@pytest.mark.parametrize("base", [0, 1, 15])
@pytest.mark.parametrize("case", CASES)
def test_client_bursts_equal_the_client_loop(lib, case, base):
    n, tx_size, trailer, counter0, burst, r0 = case
    body = tx_size - trailer
    want, sent, r_next = client_rs(n, body, burst, counter0, r0)
    rc, raw, at, r_out = run_bursts(lib, n, tx_size, trailer, counter0, burst, r0, base)
    assert rc == 0
    assert r_out == r_next
    assert (raw[:at] == FILL).all() and (raw[at + n * tx_size:] == FILL).all()  # canaries around
    for i in range(n):
        tx = raw[at + i * tx_size: at + (i + 1) * tx_size]
        assert tx[:body].tobytes() == want[i], i
        assert (tx[body:] == FILL).all(), i  # the trailer is never written
    # exactly one sample per whole burst, and the ids seal() would report are the counters sent
    assert seal_filter(want)[0] == sent
    assert len(sent) >= n // burst


def test_client_bursts_python_form(lib):
    from hsverify import synth
    txs, r = synth.client_bursts(23, 128, 5, counter0=3, r0=10)
    want, _, r_next = client_rs(23, 32, 5, 3, 10)
    assert r == r_next
    assert [bytes(t[:32]) for t in txs] == want and not txs[:, 32:].any()
    out = np.full((4, 20), FILL, np.uint8)
    txs, r = synth.client_bursts(4, 20, 2, trailer=0, out=out)
    assert txs is out and [bytes(t) for t in txs] == client_rs(4, 20, 2, 0, 0)[0]


def test_client_bursts_argument_errors(lib):
    buf = np.full(256, FILL, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    r = ctypes.c_uint64(77)
    assert lib.hsv_client_bursts(p, 16, 0, 0, 0, 0, 1, ctypes.byref(r)) == -3     # burst == 0
    assert lib.hsv_client_bursts(p, 8, 0, 0, 1, 0, 1, None) == -3                 # size < 9
    assert lib.hsv_client_bursts(p, 104, 96, 0, 1, 0, 1, None) == -3              # tx_size < 9 + trailer
    assert lib.hsv_client_bursts(p, 50, 96, 0, 1, 0, 1, None) == -3               # trailer > tx_size
    assert lib.hsv_client_bursts(None, 16, 0, 0, 1, 0, 1, None) == -3             # null txs
    assert lib.hsv_client_bursts(p, 16, 0, 0, 1, 0, 1 << 32, None) == -3          # n > 2^32 - 1
    assert r.value == 77 and (buf == FILL).all()
    assert lib.hsv_client_bursts(None, 16, 0, 4, 3, 21, 0, ctypes.byref(r)) == 0  # n == 0 does nothing
    assert r.value == 21 and (buf == FILL).all()
    # the device form checks the same arguments before it looks for a device
    assert lib.hsv_client_bursts_device(p, 16, 0, 0, 0, 0, 1, None, None) == -3
    assert lib.hsv_client_bursts_device(p, 104, 96, 0, 1, 0, 1, None, None) == -3
    assert lib.hsv_client_bursts_device(None, 16, 0, 4, 3, 21, 0, ctypes.byref(r), None) == 0


# ---- hsv_batch_samples_bincode ------------------------------------------------------

def sample(i, size):
    return bytes([0]) + struct.pack(">Q", i) + bytes(size - 9)


BATCHES = {
    "lengths 0, 8, 9 and first bytes 0, 1, 255": [
        b"", bytes(8), bytes(9), bytes([1]) + bytes(8), bytes([255]) + bytes(40), sample(7, 9), bytes([0]) * 8,
        sample((1 << 63) | 5, 12), bytes([1]) + struct.pack(">Q", 7), b"", sample(M64 - 1, 100), b"\x00"],
    "count 0": [],
    "one sample": [sample(3, 512)],
    "no sample": [bytes([1]) + bytes(20), bytes([2]) * 9],
}


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_samples_equal_decode_and_filter(lib, name):
    from hsverify import mempool, wire
    txs = BATCHES[name]
    buf = wire.encode_batch(txs)
    assert wire.decode_batch(buf) == txs
    ids, size = seal_filter(wire.decode_batch(buf))
    want = {"status": 0, "n_tx": len(txs), "size": size, "n_samples": len(ids), "first_sample": 0}
    assert size == len(buf) - 12 - 8 * len(txs)
    got, got_ids = mempool.batch_samples(buf)
    assert got == want and got_ids.dtype == np.uint64 and got_ids.tolist() == ids
    got, none = mempool.batch_samples(buf, count_only=True)  # ids_out == NULL only counts
    assert got == want and none is None
    if name.startswith("lengths"):
        assert ids == [0, 7, (1 << 63) | 5, M64 - 1]  # bytes(9) is a sample with id 0
    # ids_cap too small: HSV_ERR_INVALID_ARG, res still written, nothing past the cap
    if ids:
        res = mempool.BatchSamples()
        out = np.full(len(ids) + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        rc = lib.hsv_batch_samples_bincode(buf, len(buf), ctypes.byref(res), ctypes.c_void_p(out.ctypes.data),
                                           len(ids) - 1)
        assert rc == -3 and res.as_dict() == want
        assert out[:len(ids) - 1].tolist() == ids[:-1] and (out[len(ids) - 1:] == 0x5A5A5A5A5A5A5A5A).all()


def malformed_batches():
    from hsverify import wire
    good = wire.encode_batch([sample(1, 9), bytes(30), b"", sample(2, 20)])
    yield from (("truncated at %d" % k, good[:k]) for k in range(len(good)))
    yield "trailing byte", good + b"\x00"
    yield "tag 1", struct.pack("<IQ", 1, 0)
    yield "tag 2", b"\x02" + good[1:]
    yield "tag with a high byte", good[:3] + b"\x01" + good[4:]
    yield "count beyond the buffer", struct.pack("<IQ", 0, 2) + struct.pack("<Q", 0)
    yield "count 2^64 - 1", struct.pack("<IQ", 0, M64 - 1) + bytes(64)
    yield "length 2^64 - 1", struct.pack("<IQQ", 0, 1, M64 - 1) + bytes(16)
    yield "length with a high bit", struct.pack("<IQQ", 0, 1, (1 << 63) | 4) + bytes(4)
    yield "length one past the end", struct.pack("<IQQ", 0, 1, 10) + bytes(9)
    yield "batch request", wire.encode_batch_request([bytes(32)], bytes(32))


def test_malformed_batches_are_parse_errors(lib):
    from hsverify import mempool
    seen = 0
    for name, buf in malformed_batches():
        res = mempool.BatchSamples(9, 9, 9, 9, 9, 9)
        ids = np.full(8, 77, np.uint64)
        rc = lib.hsv_batch_samples_bincode(buf, len(buf), ctypes.byref(res), ctypes.c_void_p(ids.ctypes.data), 8)
        assert rc == -6, name
        assert res.as_dict() == {"status": 9, "n_tx": 9, "size": 9, "n_samples": 9, "first_sample": 9}, name
        assert (ids == 77).all(), name
        seen += 1
    assert seen > 100
    assert lib.hsv_batch_samples_bincode(None, 5, None, None, 0) == -3
    assert lib.hsv_batch_samples_bincode(None, 0, None, None, 0) == -6  # no bytes: a truncated header


# ---- hsverify.benchlog -----------------------------------------------------------------

def test_benchlog_lines_are_the_reference_s():
    from hsverify import benchlog
    digest = bytes(range(32))
    b64 = "AAECAwQFBgcICQoLDA0ODxAREhMUFRYXGBkaGxwdHh8="  # Digest's Debug form: base64 with padding
    assert benchlog.sending_sample_line(42) == "Sending sample transaction 42"
    assert benchlog.batch_sample_lines(digest, [0, 7, M64 - 1]) == [
        "Batch " + b64 + " contains sample tx 0",
        "Batch " + b64 + " contains sample tx 7",
        "Batch " + b64 + " contains sample tx 18446744073709551615"]
    assert benchlog.batch_sample_lines(np.frombuffer(digest, np.uint8), np.array([-1], np.int64)) == [
        "Batch " + b64 + " contains sample tx 18446744073709551615"]  # an id read back as int64
    assert benchlog.batch_sample_lines(digest, []) == []
    assert benchlog.batch_size_line(digest, 500224) == "Batch " + b64 + " contains 500224 B"
    with pytest.raises(ValueError):
        benchlog.batch_size_line(bytes(31), 1)
