"""The batch signer's C ABI (hsv_signer_*): exports, argument checks and the
no-device answer.  No GPU needed; the GPU behaviour is tests/test_signer.py."""
import ctypes
import os

import pytest

from conftest import ROOT

SYMBOLS = ("hsv_signer_create", "hsv_signer_destroy", "hsv_signer_size", "hsv_signer_public_keys",
           "hsv_signer_sign", "hsv_signer_sign_device")


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def test_symbols_load_and_are_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    for s in SYMBOLS:
        assert getattr(lib, s).argtypes is not None, s
        assert f"{s}(" in hdr, s
    assert "typedef struct hsv_signer hsv_signer;" in hdr
    # the header says what this path is not
    assert "NOT constant time" in hdr and "secret" in hdr


def test_group_hook_is_a_test_library_export_only(lib):
    from hsverify import _lib
    assert "hsv_test_signer_group" in _lib.HOOKS
    assert getattr(lib, "hsv_test_signer_group", None) is None or _lib.LIB_PATH == _lib.TEST_LIB_PATH
    t = _lib.load_test()
    g = t.hsv_test_signer_group(0)          # the value in effect: the product's
    assert g in (1, 2, 4, 8, 16)
    assert t.hsv_test_signer_group(3) == -1  # not built
    assert t.hsv_test_signer_group(1) == g and t.hsv_test_signer_group(0) == 1
    assert t.hsv_test_signer_group(0) == g


def test_bad_arguments(lib):
    h = ctypes.c_void_p()
    sig = (ctypes.c_uint8 * 64)()
    assert lib.hsv_signer_create(bytes(32), 1, None) == -3          # no place for the handle
    assert lib.hsv_signer_create(None, 1, ctypes.byref(h)) == -3    # seeds missing
    assert lib.hsv_signer_public_keys(None, sig) == -3
    assert lib.hsv_signer_sign(None, None, bytes(32), 32, 32, 1, sig) == -3      # no signer
    assert lib.hsv_signer_sign_device(None, None, ctypes.c_void_p(64), 32, 32, 1, ctypes.c_void_p(128), 64,
                                      None, None) == -3
    assert lib.hsv_signer_size(None) == 0
    lib.hsv_signer_destroy(None)                                    # a no-op, as free(NULL)


def test_misaligned_signature_buffer(lib):
    """d_sig and sig_stride must be multiples of 16; rejected before any device work."""
    for d_sig, stride in ((8, 64), (128, 72), (132, 96)):
        assert lib.hsv_signer_sign_device(None, None, ctypes.c_void_p(64), 32, 32, 1, ctypes.c_void_p(d_sig), stride,
                                          None, None) == -5
    # the message may sit anywhere: an odd d_msg gets past the alignment check (to the null signer)
    assert lib.hsv_signer_sign_device(None, None, ctypes.c_void_p(67), 32, 32, 1, ctypes.c_void_p(128), 96,
                                      None, None) == -3


def test_empty_batches_are_no_ops(lib):
    assert lib.hsv_signer_sign(None, None, None, 32, 32, 0, None) == 0
    assert lib.hsv_signer_sign_device(None, None, None, 32, 32, 0, None, 64, None, None) == 0


def test_no_device_is_an_error_not_a_fallback(lib):
    """Without a GPU there is no signer: hsv_sign_many stays the host path."""
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    assert lib.hsv_signer_create(bytes(32), 1, ctypes.byref(h)) == -1
    assert not h.value
    from hsverify import Signer, _lib
    with pytest.raises(_lib.HsvLibraryError):
        Signer(bytes(32))
