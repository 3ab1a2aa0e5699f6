"""The C ABI of the message signer (hsv_signer_sign_msgs,
hsv_signer_sign_msgs_device): exports, argument checks and the no-device
answer.  No GPU needed; the GPU behaviour is tests/test_msgsign.py."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

SYMBOLS = ("hsv_signer_sign_msgs", "hsv_signer_sign_msgs_device")


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
    assert len(lib.hsv_signer_sign_msgs.argtypes) == 8
    assert len(lib.hsv_signer_sign_msgs_device.argtypes) == 11
    # the header's comment on the new calls says what this path is and is not
    doc = hdr.split("HSV_API int hsv_signer_sign_msgs(")[0].rsplit("/*", 1)[1]
    assert "NOT constant time" in doc and "load generation" in doc
    assert "neither pipelined nor sharded" in doc and "hsv_verify_msgs*" in doc
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr) and lib.hsv_abi_version() == 3


def test_chunk_hook_is_a_test_library_export_only(lib):
    from hsverify import _lib
    assert "hsv_test_msg_sign_chunk" in _lib.HOOKS
    assert getattr(lib, "hsv_test_msg_sign_chunk", None) is None or _lib.LIB_PATH == _lib.TEST_LIB_PATH
    t = _lib.load_test()
    prev = t.hsv_test_msg_sign_chunk(300)
    assert prev == 1 << 22                       # the product's round size
    assert t.hsv_test_msg_sign_chunk(0) == 300 and t.hsv_test_msg_sign_chunk(0) == 1 << 22


def test_python_layer_exports():
    from hsverify import Signer, synth
    assert callable(Signer.sign_msgs) and callable(Signer.sign_msgs_device)
    assert callable(synth.messages_gpu)
    with pytest.raises(ValueError):
        synth.messages_gpu([3, -1])


def test_null_signer_and_null_output(lib, handle):
    h, _ = handle
    msg = (ctypes.c_uint8 * 64)()
    sig = (ctypes.c_uint8 * 64)()
    assert lib.hsv_signer_sign_msgs(None, None, msg, None, 64, 64, 1, sig) == -3
    assert lib.hsv_signer_sign_msgs(h, None, msg, None, 64, 64, 1, None) == -3
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_msgs_device(None, None, p(1027), None, 64, 64, 1, p(4096), 64, None, None) == -3
    assert lib.hsv_signer_sign_msgs_device(h, None, p(1027), None, 64, 64, 1, None, 64, None, None) == -3


def test_empty_batches_are_no_ops(lib):
    assert lib.hsv_signer_sign_msgs(None, None, None, None, 64, 64, 0, None) == 0
    assert lib.hsv_signer_sign_msgs_device(None, None, None, None, 64, 64, 0, None, 0, None, None) == 0


def test_bad_addressing_is_refused_before_any_device_work(lib, handle):
    """Decreasing offsets and overlapping messages are refused before anything
    is written, so the answer is -3 with or without a GPU."""
    h, _ = handle
    msgs = np.full(300, 0xCC, np.uint8)
    sig = np.full(3 * 64, 0xCC, np.uint8)
    mp, sp = ctypes.c_void_p(msgs.ctypes.data + 1), ctypes.c_void_p(sig.ctypes.data)
    down = (ctypes.c_uint64 * 4)(0, 100, 90, 290)
    assert lib.hsv_signer_sign_msgs(h, None, mp, down, 0, 0, 3, sp) == -3
    assert b"message 1" in lib.hsv_last_error()
    assert lib.hsv_signer_sign_msgs(h, None, mp, None, 64, 63, 3, sp) == -3        # stride below the length
    assert lib.hsv_signer_sign_msgs(h, None, None, None, 64, 64, 3, sp) == -3      # bytes, but no buffer
    assert (sig == 0xCC).all() and (msgs == 0xCC).all()
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_msgs_device(h, None, p(1027), None, 64, 63, 3, p(4096), 64, None, None) == -3
    assert lib.hsv_signer_sign_msgs_device(h, None, p(1027), None, 64, 64, 3, p(4096), 48, None, None) == -3


def test_device_form_alignment(lib, handle):
    """d_sig and sig_stride multiples of 16, d_key_idx 4-byte and d_offsets
    8-byte aligned: HSV_ERR_ALIGN, before anything else is looked at (even a
    NULL signer).  The messages may sit anywhere."""
    h, _ = handle
    p = ctypes.c_void_p
    for s in (h, None):
        assert lib.hsv_signer_sign_msgs_device(s, None, p(1027), None, 64, 64, 2, p(4104), 64, None, None) == -5
        assert lib.hsv_signer_sign_msgs_device(s, None, p(1027), None, 64, 64, 2, p(4096), 72, None, None) == -5
        assert lib.hsv_signer_sign_msgs_device(s, None, p(1027), p(8196), 0, 0, 2, p(4096), 64, None, None) == -5
        assert lib.hsv_signer_sign_msgs_device(s, p(4098), p(1027), None, 64, 64, 2, p(4096), 64, None, None) == -5


def test_no_device_is_an_error_not_a_fallback(lib, handle):
    """Without a GPU both calls answer HSV_ERR_NO_DEVICE and write nothing:
    hsv_sign_many stays the host route."""
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    h, _ = handle
    msgs = np.full(1 + 2 * 97, 0xCC, np.uint8)
    sig = np.full(2 * 64, 0xCC, np.uint8)
    mp, sp = ctypes.c_void_p(msgs.ctypes.data + 1), ctypes.c_void_p(sig.ctypes.data)
    assert lib.hsv_signer_sign_msgs(h, None, mp, None, 97, 97, 2, sp) == -1
    offs = (ctypes.c_uint64 * 3)(0, 96, 193)
    assert lib.hsv_signer_sign_msgs(h, None, mp, offs, 0, 0, 2, sp) == -1
    assert (sig == 0xCC).all() and (msgs == 0xCC).all()
    p = ctypes.c_void_p
    assert lib.hsv_signer_sign_msgs_device(h, None, p(1027), None, 97, 97, 2, p(4096), 64, None, None) == -1
    from hsverify import _lib, synth
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        synth.messages_gpu([0, 5, 97])
