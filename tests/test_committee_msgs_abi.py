"""The C ABI of hsv_committee_verify_msgs* without a GPU: exports, the
argument checks made before any device work, and the no-device answer.  The
GPU behaviour is tests/test_committee_msgs.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

SYMBOLS = ("hsv_committee_verify_msgs", "hsv_committee_verify_msgs_device")
INVALID_ARG, ALIGN, NO_DEVICE = -3, -5, -1


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def test_symbols_are_exported_declared_and_prototyped(lib):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "hsverify", "libhsv.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in exported, s
        assert re.search(r"HSV_API int %s\(" % s, hdr), s
        fn = getattr(lib, s)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, s
    assert "hsv_test_committee_msgs_counts" not in exported      # the hook: libhsv_test.so only
    assert len(lib.hsv_committee_verify_msgs.argtypes) == 9
    assert len(lib.hsv_committee_verify_msgs_device.argtypes) == 14
    assert "hsv_committee_verify_msgs" in hdr.split("#ifndef HSV_H_")[0], "file-header mapping line"
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr) and lib.hsv_abi_version() == 3


def test_empty_batch_is_ok_without_a_committee(lib):
    assert lib.hsv_committee_verify_msgs(None, None, None, None, None, 0, 0, 0, None) == 0
    assert lib.hsv_committee_verify_msgs_device(None, None, 32, None, 64, None, None, 0, 0, 0, None, None, None,
                                                None) == 0


def _host(lib, cm, pk=bytes(64), sig=bytes(128), msgs=bytes(9), offs=(0, 5, 9), msg_len=0, msg_stride=0, out=True):
    flags = (ctypes.c_uint8 * 2)(0xee, 0xee)
    o = (ctypes.c_uint64 * 3)(*offs) if offs else None
    rc = lib.hsv_committee_verify_msgs(cm, pk, sig, msgs, o, msg_len, msg_stride, 2, flags if out else None)
    assert list(flags) == [0xee, 0xee]
    return rc


def _device(lib, cm, **kw):
    p = ctypes.c_void_p
    opt = lambda v: p(v) if v else None
    return lib.hsv_committee_verify_msgs_device(
        cm, p(kw.get("pk", 256)), kw.get("pks", 32), p(kw.get("sig", 512)), kw.get("sigs", 64),
        opt(kw.get("msgs", 1027)), opt(kw.get("offs", 0)), kw.get("len", 32), kw.get("stride", 32), 2,
        opt(kw.get("flags", 4096)), opt(kw.get("bits", 0)), None, None)


def test_bad_arguments_are_refused_before_any_device_work(lib):
    from hsverify import _lib
    # no committee
    assert _host(lib, None) == INVALID_ARG and "null" in _lib.last_error()
    assert _device(lib, None) == INVALID_ARG and "null" in _lib.last_error()
    # every other check comes before the handle is read, so an opaque non-NULL one will do
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    assert _host(lib, fake, pk=None) == INVALID_ARG
    assert _host(lib, fake, out=False) == INVALID_ARG
    assert _host(lib, fake, offs=(0, 5, 4)) == INVALID_ARG and "decrease" in _lib.last_error()
    assert _host(lib, fake, msgs=None) == INVALID_ARG                    # bytes wanted, none given
    assert _host(lib, fake, msgs=None, offs=None, msg_len=7, msg_stride=7) == INVALID_ARG
    assert _host(lib, fake, msgs=bytes(16), offs=None, msg_len=8, msg_stride=4) == INVALID_ARG   # messages overlap
    assert _device(lib, fake, flags=0, bits=0) == INVALID_ARG            # both outputs NULL
    assert "no output" in _lib.last_error()
    for kw in ({"pk": 264}, {"sig": 520}, {"pks": 40}, {"sigs": 72}):
        assert _device(lib, fake, **kw) == ALIGN, kw
    assert _device(lib, fake, offs=1028) == ALIGN                        # offsets: 8-byte words
    assert _device(lib, fake, msgs=0) == INVALID_ARG                     # NULL msgs with a non-empty message
    assert _device(lib, fake, pks=16) == INVALID_ARG and _device(lib, fake, sigs=48) == INVALID_ARG
    assert _device(lib, fake, len=64, stride=48) == INVALID_ARG


def test_no_device_is_an_error_not_a_fallback(lib):
    """Without a GPU both calls answer HSV_ERR_NO_DEVICE once their arguments
    have passed: nothing is verified on the CPU.  (No committee can exist
    without a device, so the handle is an opaque block the calls never read.)"""
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    assert _host(lib, fake) == NO_DEVICE
    assert _host(lib, fake, msgs=None, offs=None) == NO_DEVICE           # empty messages
    assert _device(lib, fake, len=33, stride=35) == NO_DEVICE            # msgs at an odd address
    assert _device(lib, fake, flags=0, bits=8192) == NO_DEVICE           # strict bits alone


class _NoCommittee:
    """Committee's wrappers over a NULL handle (a committee cannot be built
    without a device)."""

    def __init__(self):
        from hsverify import _lib
        self._lib = _lib.load()
        self._h = None


def test_python_wrappers_raise_on_those_codes(lib):
    from hsverify import _lib, _testing
    from hsverify.committee import Committee
    assert callable(Committee.verify_msgs) and callable(Committee.verify_msgs_device)
    assert callable(_testing.committee_msgs_counts)
    assert "hsv_test_committee_msgs_counts" in _lib.HOOKS
    c = _NoCommittee()
    pk, sig = np.zeros((2, 32), np.uint8), np.zeros((2, 64), np.uint8)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_msgs(c, pk, sig, [b"abc", b""])
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_msgs(c, pk, sig, (np.zeros(9, np.uint8), np.array([0, 5, 9], np.uint64)))
    with pytest.raises(ValueError):
        Committee.verify_msgs(c, pk, sig, [b"abc"])                      # one message per item
    assert Committee.verify_msgs(c, pk[:0], sig[:0], []).size == 0
    import torch
    t = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):  # refused before the pointers matter
        Committee.verify_msgs_device(c, t(2, 32), t(2, 64), t(64), msg_len=32, flags=t(2), stream=0)
