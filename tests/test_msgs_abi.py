"""The C ABI of verification over messages of any length (hsv_verify_msgs,
hsv_verify_msgs_device): exports, argument checks and the no-device answer.
No GPU needed; the GPU behaviour is tests/test_verify_msgs.py."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

SYMBOLS = ("hsv_verify_msgs", "hsv_verify_msgs_device")


@pytest.fixture(scope="module")
def hsv_lib_cpu():
    from hsverify import _lib
    return _lib.load(require=True)


def test_symbols_are_declared_listed_and_prototyped(hsv_lib_cpu):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    vmap = open(os.path.join(PKG, "csrc", "libhsv.map")).read()
    globs = re.findall(r"[\w*]+(?=;)", vmap.split("global:")[1].split("local:")[0])
    for s in SYMBOLS:
        assert re.search(r"HSV_API int %s\(" % s, hdr), s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        fn = getattr(hsv_lib_cpu, s)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, s
    assert len(hsv_lib_cpu.hsv_verify_msgs.argtypes) == 8
    assert len(hsv_lib_cpu.hsv_verify_msgs_device.argtypes) == 13
    # the header says what the host form is not, and names the scheme
    assert "RFC 8032 5.1.7" in hdr and "neither pipelined" in hdr
    assert "hsv_verify_msgs" in hdr.split("#ifndef HSV_H_")[0], "file-header mapping line"


def test_abi_version_is_still_3(hsv_lib_cpu):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr)
    assert hsv_lib_cpu.hsv_abi_version() == 3


def test_python_layer_exports():
    import hsverify
    from hsverify import verifier
    assert hsverify.verify_msgs is verifier.verify_msgs
    assert hsverify.verify_msgs_device is verifier.verify_msgs_device
    buf, offsets = verifier.pack_msgs([b"", b"ab", b"c"])
    assert buf.tobytes() == b"abc" and offsets.tolist() == [0, 0, 2, 3]


def test_empty_batches_are_no_ops(hsv_lib_cpu):
    assert hsv_lib_cpu.hsv_verify_msgs(None, None, None, None, 0, 0, 0, None) == 0
    assert hsv_lib_cpu.hsv_verify_msgs_device(None, 32, None, 64, None, None, 0, 0, 0, None, None, None, None) == 0
    from hsverify import verifier
    assert verifier.verify_msgs(np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), []).size == 0


def test_bad_arguments_are_refused_before_any_device_work(hsv_lib_cpu):
    lib = hsv_lib_cpu
    pk, sig, out = bytes(64), bytes(128), (ctypes.c_uint8 * 2)()
    good = (ctypes.c_uint64 * 3)(0, 5, 9)
    bad = (ctypes.c_uint64 * 3)(0, 5, 4)
    assert lib.hsv_verify_msgs(None, sig, bytes(9), good, 0, 0, 2, out) == -3        # no keys
    assert lib.hsv_verify_msgs(pk, sig, bytes(9), good, 0, 0, 2, None) == -3         # no place for the flags
    assert lib.hsv_verify_msgs(pk, sig, bytes(9), bad, 0, 0, 2, out) == -3           # offsets decrease
    assert b"decrease" in lib.hsv_last_error()
    assert lib.hsv_verify_msgs(pk, sig, None, good, 0, 0, 2, out) == -3              # bytes wanted, none given
    assert lib.hsv_verify_msgs(pk, sig, None, None, 7, 7, 2, out) == -3
    assert lib.hsv_verify_msgs(pk, sig, bytes(16), None, 8, 4, 2, out) == -3         # messages overlap
    p = ctypes.c_void_p
    dev = lambda **kw: lib.hsv_verify_msgs_device(
        p(kw.get("pk", 256)), kw.get("pks", 32), p(kw.get("sig", 512)), kw.get("sigs", 64), p(kw.get("msgs", 1027)),
        p(kw.get("offs", 0)) if kw.get("offs", 0) else None, kw.get("len", 32), kw.get("stride", 32), 2,
        p(kw.get("flags", 4096)) if kw.get("flags", 4096) else None, None, None, None)
    for kw in ({"pk": 264}, {"sig": 520}, {"pks": 40}, {"sigs": 72}):
        assert dev(**kw) == -5, kw                                                    # HSV_ERR_ALIGN
    assert dev(offs=1028) == -5                                                       # offsets: 8-byte words
    assert dev(flags=0) == -3                                                         # no output at all
    assert dev(msgs=0) == -3
    assert dev(pks=16) == -3 and dev(sigs=48) == -3                                   # records overlap
    assert dev(len=64, stride=48) == -3


def test_no_device_is_an_error_not_a_fallback(hsv_lib_cpu):
    """Without a GPU both calls answer HSV_ERR_NO_DEVICE: nothing is verified
    on the CPU.  The message pointer of the device form is odd on purpose: any
    alignment is accepted."""
    lib = hsv_lib_cpu
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    out = (ctypes.c_uint8 * 2)()
    offs = (ctypes.c_uint64 * 3)(0, 5, 9)
    assert lib.hsv_verify_msgs(bytes(64), bytes(128), bytes(9), offs, 0, 0, 2, out) == -1
    assert lib.hsv_verify_msgs(bytes(64), bytes(128), None, None, 0, 0, 2, out) == -1  # empty messages
    p = ctypes.c_void_p
    assert lib.hsv_verify_msgs_device(p(256), 32, p(512), 64, p(1027), None, 33, 35, 2, p(4096), None, None,
                                      None) == -1
    from hsverify import _lib, verifier
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        verifier.verify_msgs(np.zeros((2, 32), np.uint8), np.zeros((2, 64), np.uint8), [b"abc", b""])
