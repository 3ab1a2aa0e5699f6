"""The serialized-batch calls that need no GPU (hsv_batch_parse_bincode, and the
argument checks of hsv_batch*_verify_bincode*, which come before any device is
looked for): parser vectors against hsverify.wire.encode_batch, the rejection
rules, the error codes and the exports."""
import ctypes
import struct

import numpy as np
import pytest

NO_DEVICE, INVALID_ARG, ALIGN, PARSE = -1, -3, -5, -6


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def _tx(rnd, n):
    return rnd.integers(0, 256, n, dtype=np.uint8).tobytes()


def _parse(lib, buf, with_spans=True):
    """(rc, n_tx, spans) of hsv_batch_parse_bincode on an exact-size copy"""
    arr = np.frombuffer(bytes(buf), np.uint8).copy()
    n = ctypes.c_size_t(12345)
    spans = np.full(2 * (len(buf) // 8 + 1), 0xEE, np.uint64)
    rc = lib.hsv_batch_parse_bincode(ctypes.c_void_p(arr.ctypes.data) if arr.size else None, arr.size, ctypes.byref(n),
                                     ctypes.c_void_p(spans.ctypes.data) if with_spans else None, spans.size)
    return rc, n.value, spans


@pytest.mark.parametrize("lens", [[], [136], [0, 95, 96, 97, 0, 1, 400, 96]], ids=["empty", "one", "ragged"])
def test_parser_round_trips_the_encoder(lib, lens):
    from hsverify import wire
    rnd = np.random.default_rng(len(lens))
    txs = [_tx(rnd, n) for n in lens]
    enc = wire.encode_batch(txs)
    assert enc[:12] == struct.pack("<IQ", 0, len(txs)) and len(enc) == 12 + sum(8 + n for n in lens)
    rc, n, spans = _parse(lib, enc)
    assert (rc, n) == (1, len(txs))
    assert [enc[int(spans[2 * i]): int(spans[2 * i + 1])] for i in range(n)] == txs
    assert (spans[2 * n:] == 0xEE).all()  # nothing past the pairs is written
    assert _parse(lib, enc, with_spans=False)[:2] == (1, len(txs))
    assert wire.decode_batch(enc) == txs


def test_parser_rejections(lib):
    from hsverify import _lib, wire
    rnd = np.random.default_rng(7)
    txs = [_tx(rnd, n) for n in (0, 95, 96, 3)]
    enc = wire.encode_batch(txs)
    for cut in range(len(enc)):  # truncation at every byte
        rc, n, spans = _parse(lib, enc[:cut])
        assert rc == PARSE and n == 12345 and (spans == 0xEE).all(), cut
    assert _parse(lib, enc + b"\x00")[0] == PARSE  # one trailing byte
    assert "trailing" in _lib.last_error()
    for tag in (1, 2):
        assert _parse(lib, struct.pack("<I", tag) + enc[4:])[0] == PARSE
    assert "Batch" in _lib.last_error()
    assert _parse(lib, wire.encode_batch_request([bytes(32)] * 3, bytes(32)))[0] == PARSE
    for count in (len(txs) + 1, len(enc), 2 ** 64 - 1, 2 ** 61):  # a count beyond the buffer
        assert _parse(lib, enc[:4] + struct.pack("<Q", count) + enc[12:])[0] == PARSE
    for length in (2 ** 64 - 1, 2 ** 63, 2 ** 32, len(enc)):  # a length past the end, with and without overflow
        assert _parse(lib, enc[:12] + struct.pack("<Q", length) + enc[20:])[0] == PARSE
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_PARSE"):
        wire.decode_batch(enc[:-1])


def test_parse_argument_errors(lib):
    from hsverify import wire
    enc = np.frombuffer(wire.encode_batch([bytes(100), bytes(7)]), np.uint8)
    p = ctypes.c_void_p(enc.ctypes.data)
    spans = np.zeros(4, np.uint64)
    assert lib.hsv_batch_parse_bincode(None, 5, None, None, 0) == INVALID_ARG
    assert lib.hsv_batch_parse_bincode(p, enc.size, None, ctypes.c_void_p(spans.ctypes.data), 3) == INVALID_ARG
    assert not spans.any()
    assert lib.hsv_batch_parse_bincode(p, enc.size, None, ctypes.c_void_p(spans.ctypes.data), 4) == 1
    assert spans.tolist() == [20, 120, 128, 135]
    assert lib.hsv_batch_parse_bincode(None, 0, None, None, 0) == PARSE  # an empty buffer is a truncated header


def test_verify_calls_check_their_arguments_before_any_device(lib):
    """Argument and parse errors are reported with or without a GPU; only a
    call that passed them looks for a device (HSV_ERR_NO_DEVICE without one)."""
    from hsverify import wire
    good = wire.encode_batch([bytes(136), bytes(200)])
    bufs = np.frombuffer(good + good, np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    off = np.array([0, len(good), 2 * len(good)], np.uint64)
    dec = np.array([0, len(good), len(good) - 1], np.uint64)
    res = (wire.BatchResult * 2)()
    flags = np.full(4, 0xff, np.uint8)
    rp = ctypes.cast(res, ctypes.c_void_p)
    assert lib.hsv_batches_verify_bincode(None, None, None, 0, None, None, 0) == 0
    assert lib.hsv_batches_verify_bincode(None, p(bufs), None, 2, rp, p(flags), 4) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode(None, p(bufs), p(dec), 2, rp, p(flags), 4) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode(None, None, p(off), 2, rp, p(flags), 4) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode(None, p(bufs), p(off), 2, rp, p(flags), 3) == INVALID_ARG  # flags_cap < 4
    assert (flags == 0xff).all()
    assert lib.hsv_batch_verify_bincode(None, None, 5, None) == INVALID_ARG
    assert lib.hsv_batch_verify_bincode(None, good[:-1], len(good) - 1, None) == PARSE
    assert lib.hsv_batch_verify_bincode(None, good + b"\x00", len(good) + 1, None) == PARSE
    # the device form: nulls, sizes and alignment before the pointers matter
    words = np.zeros(16, np.uint64)
    assert lib.hsv_batches_verify_bincode_device(None, None, None, 0, 0, None, None, None, None) == 0
    assert lib.hsv_batches_verify_bincode_device(None, None, p(off), 2, 4, p(words), None, None, None) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode_device(None, p(bufs), None, 2, 4, p(words), None, None, None) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode_device(None, p(bufs), p(off), 2, 4, None, None, None, None) == INVALID_ARG
    assert lib.hsv_batches_verify_bincode_device(None, p(bufs), p(off), 2, 2 ** 32, p(words), None, None,
                                                 None) == INVALID_ARG
    odd = ctypes.c_void_p(words.ctypes.data + 4)
    assert lib.hsv_batches_verify_bincode_device(None, p(bufs), odd, 2, 4, p(words), None, None, None) == ALIGN
    assert lib.hsv_batches_verify_bincode_device(None, p(bufs), p(off), 2, 4, odd, None, None, None) == ALIGN
    if lib.hsv_device_count() <= 0:
        assert lib.hsv_batches_verify_bincode(None, p(bufs), p(off), 2, rp, p(flags), 4) == NO_DEVICE
        assert lib.hsv_batch_verify_bincode(None, good, len(good), None) == NO_DEVICE
        # a malformed batch beside a good one is no error of the call: it still needs the device
        one_bad = np.frombuffer(good + good[:-1], np.uint8)
        off2 = np.array([0, len(good), 2 * len(good) - 1], np.uint64)
        assert lib.hsv_batches_verify_bincode(None, p(one_bad), p(off2), 2, rp, p(flags), 4) == NO_DEVICE
        assert lib.hsv_batches_verify_bincode_device(None, p(bufs), p(off), 2, 4, p(words), None, None,
                                                     None) == NO_DEVICE
        assert (flags == 0xff).all()


def test_exports_and_mirrors(lib):
    from test_capi import declared_symbols, exported_symbols
    from hsverify import _lib, mempool, wire
    new = {"hsv_batch_parse_bincode", "hsv_batches_verify_bincode", "hsv_batch_verify_bincode",
           "hsv_batches_verify_bincode_device"}
    assert new <= set(declared_symbols())
    assert exported_symbols(_lib.LIB_PATH) == declared_symbols() or not _lib.LIB_PATH.endswith("libhsv.so")
    assert new <= set(exported_symbols(_lib.TEST_LIB_PATH))
    assert ctypes.sizeof(wire.BatchResult) == 24
    assert (wire.BATCH_OK, wire.BATCH_TX, wire.BATCH_PARSE, wire.BATCH_OVERFLOW) == (0, 1, 2, 3)
    assert wire.batch_results(np.array([1 | (5 << 32), 9, 3], np.uint64)) == [(1, 5, 9, 3)]
    # malformed bytes and a BatchRequest are rejections of make_vote, not errors
    assert mempool.verify_serialized_batch(wire.encode_batch([bytes(136)])[:-1]) is False
    assert mempool.verify_serialized_batch(wire.encode_batch_request([bytes(32)], bytes(32))) is False
