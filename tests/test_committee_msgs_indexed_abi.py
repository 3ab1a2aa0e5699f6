"""The C ABI of hsv_committee_verify_msgs_indexed* without a GPU: exports, the
argument checks made before any device work, and the no-device answer.  The
GPU behaviour is tests/test_committee_msgs_indexed.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

SYMBOLS = ("hsv_committee_verify_msgs_indexed", "hsv_committee_verify_msgs_indexed_device")
HOOKS = ("hsv_test_cmsg_indexed_form", "hsv_test_cmsg_indexed_counts")
INVALID_ARG, ALIGN, NO_DEVICE = -3, -5, -1


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def _exports(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "hsverify", name)], capture_output=True,
                        text=True, check=True).stdout
    return {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_symbols_are_exported_declared_and_prototyped(lib):
    from hsverify import _lib
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    hooks_hdr = open(os.path.join(PKG, "csrc", "hsv_test_hooks.h")).read()
    product, test = _exports("libhsv.so"), _exports("libhsv_test.so")
    for s in SYMBOLS:
        assert s in product and s in test, s
        assert re.search(r"HSV_API int %s\(" % s, hdr), s
        fn = getattr(lib, s)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, s
    for h in HOOKS:                                # the hooks: libhsv_test.so only
        assert h in test and h not in product, h
        assert re.search(r"HSV_API int %s\(" % h, hooks_hdr) and h not in hdr, h
        assert h in _lib.HOOKS
    assert len(lib.hsv_committee_verify_msgs_indexed.argtypes) == 9
    assert len(lib.hsv_committee_verify_msgs_indexed_device.argtypes) == 12
    assert "hsv_committee_verify_msgs_indexed" in hdr.split("#ifndef HSV_H_")[0], "file-header mapping line"
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr) and lib.hsv_abi_version() == 3


def test_the_route_hook_needs_no_device():
    from hsverify import _testing
    with _testing.test_library():
        assert _testing.cmsg_indexed_form(0) == -1
        assert _testing.cmsg_indexed_form(1) == 0
        assert _testing.cmsg_indexed_form(-1) == 1
        with pytest.raises(ValueError):
            _testing.cmsg_indexed_form(2)
        assert _testing.cmsg_indexed_form(-1) == -1
        assert len(_testing.cmsg_indexed_counts()) == 3           # before any launch: nothing to read on a device


def test_empty_batch_is_ok_without_a_committee(lib):
    assert lib.hsv_committee_verify_msgs_indexed(None, None, None, None, None, 0, 0, 0, None) == 0
    assert lib.hsv_committee_verify_msgs_indexed_device(None, None, None, 64, None, None, 0, 0, 0, None, None,
                                                        None) == 0


def _host(lib, cm, idx=True, sig=bytes(128), msgs=bytes(9), offs=(0, 5, 9), msg_len=0, msg_stride=0, out=True):
    flags = (ctypes.c_uint8 * 2)(0xee, 0xee)
    o = (ctypes.c_uint64 * 3)(*offs) if offs else None
    ki = (ctypes.c_uint32 * 2)(0, 1) if idx else None
    rc = lib.hsv_committee_verify_msgs_indexed(cm, ki, sig, msgs, o, msg_len, msg_stride, 2, flags if out else None)
    assert list(flags) == [0xee, 0xee]
    return rc


def _device(lib, cm, **kw):
    p = ctypes.c_void_p
    opt = lambda v: p(v) if v else None
    return lib.hsv_committee_verify_msgs_indexed_device(
        cm, opt(kw.get("idx", 256)), opt(kw.get("sig", 512)), kw.get("sigs", 64), opt(kw.get("msgs", 1027)),
        opt(kw.get("offs", 0)), kw.get("len", 32), kw.get("stride", 32), 2, opt(kw.get("flags", 4096)), None, None)


def test_bad_arguments_are_refused_before_any_device_work(lib):
    from hsverify import _lib
    # no committee
    assert _host(lib, None) == INVALID_ARG and "null" in _lib.last_error()
    assert _device(lib, None) == INVALID_ARG and "null" in _lib.last_error()
    # every other check comes before the handle is read, so an opaque non-NULL one will do
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    assert _host(lib, fake, idx=False) == INVALID_ARG
    assert _host(lib, fake, sig=None) == INVALID_ARG
    assert _host(lib, fake, out=False) == INVALID_ARG
    assert _host(lib, fake, offs=(0, 5, 4)) == INVALID_ARG and "decrease" in _lib.last_error()
    assert _host(lib, fake, msgs=None) == INVALID_ARG                    # bytes wanted, none given
    assert _host(lib, fake, msgs=None, offs=None, msg_len=7, msg_stride=7) == INVALID_ARG
    assert _host(lib, fake, msgs=bytes(16), offs=None, msg_len=8, msg_stride=4) == INVALID_ARG   # messages overlap
    assert _device(lib, fake, idx=0) == INVALID_ARG and _device(lib, fake, sig=0) == INVALID_ARG
    assert _device(lib, fake, flags=0) == INVALID_ARG                    # d_flags is required
    for kw in ({"sig": 520}, {"sigs": 72}):
        assert _device(lib, fake, **kw) == ALIGN, kw
    assert _device(lib, fake, idx=258) == ALIGN                          # indices: 4-byte words
    assert _device(lib, fake, offs=1028) == ALIGN                        # offsets: 8-byte words
    assert _device(lib, fake, msgs=0) == INVALID_ARG                     # NULL msgs with a non-empty message
    assert _device(lib, fake, sigs=48) == INVALID_ARG                    # signatures overlap
    assert _device(lib, fake, len=64, stride=48) == INVALID_ARG          # messages overlap


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
    assert _device(lib, fake, idx=260, len=0, stride=0, msgs=0) == NO_DEVICE


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
    assert callable(_testing.cmsg_indexed_form) and callable(_testing.cmsg_indexed_counts)
    c = _NoCommittee()
    idx, sig = np.zeros(2, np.uint32), np.zeros((2, 64), np.uint8)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_msgs_indexed(c, idx, sig, [b"abc", b""])
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_msgs_indexed(c, idx, sig, (np.zeros(9, np.uint8), np.array([0, 5, 9], np.uint64)))
    with pytest.raises(ValueError):
        Committee.verify_msgs_indexed(c, idx, sig, [b"abc"])             # one message per item
    assert Committee.verify_msgs_indexed(c, idx[:0], sig[:0], []).size == 0
    import torch
    t = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):  # refused before the pointers matter
        Committee.verify_msgs_indexed_device(c, torch.zeros(2, dtype=torch.int32), t(2, 64), t(64), msg_len=32,
                                             flags=t(2), stream=0)
