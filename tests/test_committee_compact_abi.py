"""The C ABI of compact committees (hsv_committee_create_ex,
hsv_committee_digit_bits, hsv_committee_table_bytes) without a GPU: exports,
the width check made before any device work, and the no-device answer.  The
GPU behaviour is tests/test_committee_compact.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

SYMBOLS = {"hsv_committee_create_ex": "int", "hsv_committee_digit_bits": "int",
           "hsv_committee_table_bytes": "uint64_t"}
INVALID_ARG, NO_DEVICE = -3, -1


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def test_symbols_are_listed_declared_exported_and_prototyped(lib):
    hdr = open(os.path.join(ROOT, "include", "hsv.h")).read()
    vmap = open(os.path.join(PKG, "csrc", "libhsv.map")).read()
    globs = re.findall(r"[\w*]+(?=;)", vmap.split("global:")[1].split("local:")[0])
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "hsverify", "libhsv.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for s, ret in SYMBOLS.items():
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        assert re.search(r"HSV_API %s %s\(" % (ret, s), hdr), s
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.hsv_committee_create_ex.argtypes) == 4
    assert lib.hsv_committee_table_bytes.restype is ctypes.c_uint64
    assert re.search(r"#define HSV_COMMITTEE_DIGITS_FULL 8\b", hdr)
    assert re.search(r"#define HSV_COMMITTEE_DIGITS_COMPACT 4\b", hdr)
    assert re.search(r"#define HSV_ABI_VERSION 3\b", hdr) and lib.hsv_abi_version() == 3
    # the header says what a compact committee costs and lacks
    doc = hdr.split("HSV_API int hsv_committee_create_ex(")[0].rsplit("HSV_API int hsv_committee_create(", 1)[1]
    assert "384 KiB" in doc and "48 KiB" in doc
    assert "no latency form" in doc and "resident service" in doc and "zero-copy" in doc
    assert "committee_compact_bench_2p20.json" in doc


def test_other_widths_are_refused_before_any_device_work(lib):
    from hsverify import _lib
    keys = bytes(range(32)) * 2
    for bits in (5, 0, -4, 16, 3):
        h = ctypes.c_void_p(0x1234)
        assert lib.hsv_committee_create_ex(keys, 2, bits, ctypes.byref(h)) == INVALID_ARG, bits
        assert "digit_bits" in _lib.last_error()
        assert h.value == 0x1234                                  # nothing was written
    h = ctypes.c_void_p()
    assert lib.hsv_committee_create_ex(None, 2, 4, ctypes.byref(h)) == INVALID_ARG      # the older checks hold
    assert lib.hsv_committee_create_ex(keys, 2, 4, None) == INVALID_ARG
    assert lib.hsv_committee_create_ex(keys, (1 << 20) + 1, 4, ctypes.byref(h)) == INVALID_ARG


def test_null_committee_has_no_width_and_no_tables(lib):
    assert lib.hsv_committee_digit_bits(None) == 0
    assert lib.hsv_committee_table_bytes(None) == 0


def test_a_valid_call_needs_a_device(lib):
    """Without a GPU both widths answer HSV_ERR_NO_DEVICE: nothing is built on
    the CPU.  With one, the committee exists and reports its width."""
    keys = bytes(range(32)) * 2
    for bits, per_key in ((4, 49152), (8, 393216)):
        h = ctypes.c_void_p()
        rc = lib.hsv_committee_create_ex(keys, 2, bits, ctypes.byref(h))
        if lib.hsv_device_count() <= 0:
            assert rc == NO_DEVICE and not h.value
            continue
        assert rc == 0 and h.value
        assert lib.hsv_committee_digit_bits(h) == bits and lib.hsv_committee_table_bytes(h) == 2 * per_key
        lib.hsv_committee_destroy(h)


def test_python_wrapper_exposes_the_width():
    import inspect

    from hsverify.committee import Committee
    assert inspect.signature(Committee.__init__).parameters["compact"].default is False
    assert isinstance(Committee.digit_bits, property) and isinstance(Committee.table_bytes, property)
