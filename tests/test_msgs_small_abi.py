"""The two test hooks of the small-batch message forms (hsv_verify_msgs* at
<= 2^13 items): hsv_test_msgs_small picks the route,
hsv_test_msgs_form_counts reports the launches by form.  Both are exported by
libhsv_test.so only and answer without a device.  No GPU needed; the GPU
behaviour is tests/test_msgs_small.py."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import PKG
from test_capi import declared_symbols, exported_symbols

HOOKS = ("hsv_test_msgs_small", "hsv_test_msgs_form_counts")


@pytest.fixture(scope="module")
def tlib():
    from hsverify import _lib
    return _lib.load_test()


def test_hooks_are_declared_and_exported_by_the_test_library_only():
    from hsverify import _lib
    declared = declared_symbols(os.path.join(PKG, "csrc", "hsv_test_hooks.h"))
    product = exported_symbols(os.path.join(os.path.dirname(_lib.TEST_LIB_PATH), "libhsv.so"))
    test = exported_symbols(_lib.TEST_LIB_PATH)
    for s in HOOKS:
        assert s in declared, s
        assert s in _lib.HOOKS, s
        assert s in test, s
        assert s not in product, s
    # no public symbol came with them
    assert not [s for s in declared_symbols() if "msgs_small" in s or "form_counts" in s]


def test_route_switch_answers_without_a_device(tlib):
    """Set and restore; every mode is accepted and handed back as the previous
    one; an unknown mode gives -2 and changes nothing."""
    sw = tlib.hsv_test_msgs_small
    assert sw.restype is ctypes.c_int
    prev = sw(0)
    try:
        assert prev == -1, "the default route is chosen by n"
        last = 0
        for mode in (1, 2, 3, 4, -1, 0):
            assert sw(mode) == last
            last = mode
        for bad in (5, -2, -3, 100):
            assert sw(bad) == -2
        assert sw(0) == 0, "an unknown mode left the route alone"
    finally:
        sw(-1)
    assert sw(-1) == -1


def test_form_counts_read_zero_before_any_launch():
    """A fresh process that has loaded the test library and launched nothing:
    all five counts are 0 (and the call needs no device)."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hsverify import _lib\n"
            "lib = _lib.load_test()\n"
            "out = (ctypes.c_uint64 * 5)(*[7] * 5)\n"
            "assert lib.hsv_test_msgs_form_counts(out) == 0\n"
            "assert list(out) == [0] * 5, list(out)\n"
            "assert lib.hsv_test_msgs_small(3) == -1 and lib.hsv_test_msgs_small(-1) == 3\n"
            "assert list(out) == [0] * 5\n" % PKG)
    env = dict(os.environ, HSV_NO_TORCH="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
