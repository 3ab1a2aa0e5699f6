"""The C ABI of the transaction signer (hsv_signer_sign_transactions,
hsv_signer_sign_transactions_device): exports, argument checks and the
no-device answer.  No GPU needed; the GPU behaviour is tests/test_txsign.py."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

SYMBOLS = ("hsv_signer_sign_transactions", "hsv_signer_sign_transactions_device")


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


@pytest.fixture()
def handle():
    """Something non-NULL where a signer is expected.  Every check below is
    made before the signer is looked at (no device: there cannot be one)."""
    buf = (ctypes.c_uint64 * 16)()
    return ctypes.cast(buf, ctypes.c_void_p), buf


def test_symbols_are_declared_listed_and_prototyped(lib):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    vmap = open(os.path.join(PKG, "csrc", "libhsv.map")).read()
    globs = re.findall(r"[\w*]+(?=;)", vmap.split("global:")[1].split("local:")[0])
    for s in SYMBOLS:
        assert re.search(r"HSV_API int %s\(" % s, hdr), s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        fn = getattr(lib, s)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, s
    assert len(lib.hsv_signer_sign_transactions.argtypes) == 6
    assert len(lib.hsv_signer_sign_transactions_device.argtypes) == 8
    # the header's comment on the new calls says what this path is and is not
    doc = hdr.split("HSV_API int hsv_signer_sign_transactions(")[0].rsplit("/*", 1)[1]
    assert "NOT constant time" in doc and "load generation" in doc
    assert "neither pipelined" in doc and "SHA-512(message)[..32]" in doc
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr) and lib.hsv_abi_version() == 3


def test_chunk_hook_is_a_test_library_export_only(lib):
    from hsverify import _lib
    assert "hsv_test_tx_sign_chunk" in _lib.HOOKS
    assert getattr(lib, "hsv_test_tx_sign_chunk", None) is None or _lib.LIB_PATH == _lib.TEST_LIB_PATH
    t = _lib.load_test()
    prev = t.hsv_test_tx_sign_chunk(300)
    assert prev == 1 << 22                       # the product's launch size
    assert t.hsv_test_tx_sign_chunk(0) == 300 and t.hsv_test_tx_sign_chunk(0) == 1 << 22


def test_stage_bytes_hook_is_a_test_library_export_only(lib):
    from hsverify import _lib
    assert "hsv_test_stage_bytes" in _lib.HOOKS
    assert getattr(lib, "hsv_test_stage_bytes", None) is None or _lib.LIB_PATH == _lib.TEST_LIB_PATH
    t = _lib.load_test()
    prev = t.hsv_test_stage_bytes(4096)
    assert prev == 1 << 29                       # the product's bytes per launch
    assert t.hsv_test_stage_bytes(0) == 4096 and t.hsv_test_stage_bytes(0) == 1 << 29


def test_python_layer_exports():
    from hsverify import Signer, synth
    assert callable(Signer.sign_transactions) and callable(Signer.sign_transactions_device)
    assert callable(synth.transactions_gpu)
    with pytest.raises(ValueError):
        synth.transactions_gpu(4, 95)


def test_null_signer_and_null_buffer(lib, handle):
    h, _ = handle
    buf = (ctypes.c_uint8 * 96)()
    assert lib.hsv_signer_sign_transactions(None, None, buf, None, 96, 1) == -3
    assert lib.hsv_signer_sign_transactions(h, None, None, None, 96, 1) == -3
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_transactions_device(None, None, p(1027), None, 96, 1, None, None) == -3
    assert lib.hsv_signer_sign_transactions_device(h, None, None, None, 96, 1, None, None) == -3


def test_empty_batches_are_no_ops(lib):
    assert lib.hsv_signer_sign_transactions(None, None, None, None, 512, 0) == 0
    assert lib.hsv_signer_sign_transactions_device(None, None, None, None, 512, 0, None, None) == 0


def test_short_transactions_are_refused_before_any_device_work(lib, handle):
    """The host form makes hsv_verify_transactions' length check, and makes it
    before anything is written; so the answer is -3 with or without a GPU."""
    h, _ = handle
    buf = np.full(300, 0xCC, np.uint8)
    ptr = ctypes.c_void_p(buf.ctypes.data)
    assert lib.hsv_signer_sign_transactions(h, None, ptr, None, 95, 3) == -3           # fixed size 95
    assert b"shorter than 96" in lib.hsv_last_error()
    short = (ctypes.c_uint64 * 3)(0, 96, 191)                                           # second one: 95 bytes
    assert lib.hsv_signer_sign_transactions(h, None, ptr, short, 0, 2) == -3
    assert b"transaction 1" in lib.hsv_last_error()
    down = (ctypes.c_uint64 * 4)(0, 100, 90, 290)                                       # offsets decrease
    assert lib.hsv_signer_sign_transactions(h, None, ptr, down, 0, 3) == -3
    assert (buf == 0xCC).all()
    # device form: a fixed size below 96 is refused as hsv_verify_transactions_device refuses it,
    # and the offsets are 8-byte words
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_transactions_device(h, None, p(1027), None, 95, 2, None, None) == -3
    assert lib.hsv_signer_sign_transactions_device(h, None, p(1027), p(4100), 0, 2, None, None) == -5
    assert lib.hsv_signer_sign_transactions_device(h, p(4098), p(1027), None, 96, 2, None, None) == -5


def test_no_device_is_an_error_not_a_fallback(lib, handle):
    """Without a GPU both calls answer HSV_ERR_NO_DEVICE and write nothing:
    hashlib plus hsv_sign_many stays the host route.  The buffers of both
    forms sit at odd addresses on purpose: any alignment is accepted."""
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    h, _ = handle
    buf = np.full(1 + 2 * 97, 0xCC, np.uint8)
    assert lib.hsv_signer_sign_transactions(h, None, ctypes.c_void_p(buf.ctypes.data + 1), None, 97, 2) == -1
    offs = (ctypes.c_uint64 * 3)(0, 96, 193)
    assert lib.hsv_signer_sign_transactions(h, None, ctypes.c_void_p(buf.ctypes.data + 1), offs, 0, 2) == -1
    assert (buf == 0xCC).all()
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_transactions_device(h, None, p(1027), None, 97, 2, None, None) == -1
    from hsverify import _lib, synth
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        synth.transactions_gpu(4, 128)
