"""The signer census at the C ABI, without a GPU: the four entry points are
exported by libhsv.so, hsv_census_summary is 48 bytes, and every argument
error is reported before any device work (so it is the same answer on a
machine with no device).  The seed hook is exported by libhsv_test.so only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

NO_DEVICE, INVALID_ARG, ALIGN = -1, -3, -5
ENTRY_POINTS = ("hsv_census_keys", "hsv_census_keys_device", "hsv_census_transactions",
                "hsv_census_transactions_device")


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class _Bufs:
    """Host arrays in the place of device buffers: the checks under test never
    read them.  numpy allocations are 16-byte aligned."""

    def __init__(self, slots=16):
        self.pk = np.zeros(64 * 32, np.uint8)
        self.txs = np.zeros(4 * 128, np.uint8)
        self.offsets = np.arange(5, dtype=np.uint64) * 128
        self.keys = np.full(32 * slots, 0xab, np.uint8)
        self.counts = np.full(slots + 2, 0xabababab, np.uint32)
        self.summary = np.full(8, 0xabababab, np.uint64)
        for a in (self.pk, self.keys, self.counts, self.summary):
            assert a.ctypes.data % 16 == 0

    def untouched(self):
        return (self.keys == 0xab).all() and (self.counts == 0xabababab).all() and (self.summary == 0xabababab).all()


def test_symbols_and_struct_size(lib):
    from hsverify import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "hsverify", "libhsv.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported
    assert "hsv_test_census_seed" not in exported
    assert "hsv_test_census_seed" in _lib.HOOKS
    header = open(os.path.join(ROOT, "include", "hsv.h")).read()
    body = re.search(r"typedef struct hsv_census_summary \{(.*?)\} hsv_census_summary;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+);", body)
    assert [f for _, f in fields] == ["items", "counted", "members", "malformed", "overflow", "distinct", "reserved"]
    assert sum(8 if t == "uint64_t" else 4 for t, _ in fields) == 48
    from hsverify.mempool import CensusSummary
    assert ctypes.sizeof(CensusSummary) == 48
    assert [n for n, _ in CensusSummary._fields_] == [f for _, f in fields]


@pytest.mark.parametrize("slots", [0, 15, 24, 1 << 23])
def test_slots_must_be_a_power_of_two_in_range(lib, slots):
    b = _Bufs()
    assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 4, slots, _p(b.keys), _p(b.counts), _p(b.summary),
                                      None) == INVALID_ARG
    assert lib.hsv_census_transactions_device(None, _p(b.txs), _p(b.offsets), 0, 4, slots, _p(b.keys), _p(b.counts),
                                              _p(b.summary), None) == INVALID_ARG
    assert lib.hsv_census_keys(None, _p(b.pk), 32, 4, slots, _p(b.keys), _p(b.counts), 16, _p(b.summary)) == INVALID_ARG
    assert lib.hsv_census_transactions(None, _p(b.txs), _p(b.offsets), 0, 4, slots, _p(b.keys), _p(b.counts), 16,
                                       _p(b.summary)) == INVALID_ARG
    from hsverify import _lib
    assert "slots" in _lib.last_error()
    assert b.untouched()


def test_null_outputs_and_inputs(lib):
    b = _Bufs()
    k, c, s = _p(b.keys), _p(b.counts), _p(b.summary)
    for outs in ((None, c, s), (k, None, s), (k, c, None)):
        assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 4, 16, *outs, None) == INVALID_ARG
        assert lib.hsv_census_transactions_device(None, _p(b.txs), _p(b.offsets), 0, 4, 16, *outs, None) == INVALID_ARG
        # an empty batch still writes its outputs, so it needs them too
        assert lib.hsv_census_keys_device(None, None, 32, 0, 16, *outs, None) == INVALID_ARG
    assert lib.hsv_census_keys_device(None, None, 32, 4, 16, k, c, s, None) == INVALID_ARG
    assert lib.hsv_census_transactions_device(None, None, _p(b.offsets), 0, 4, 16, k, c, s, None) == INVALID_ARG
    # host forms: a summary always, the arrays once keys_cap is not 0
    assert lib.hsv_census_keys(None, _p(b.pk), 32, 4, 16, k, c, 16, None) == INVALID_ARG
    assert lib.hsv_census_keys(None, _p(b.pk), 32, 4, 16, None, c, 16, s) == INVALID_ARG
    assert lib.hsv_census_keys(None, _p(b.pk), 32, 4, 16, k, None, 16, s) == INVALID_ARG
    assert lib.hsv_census_keys(None, None, 32, 4, 16, k, c, 16, s) == INVALID_ARG
    assert lib.hsv_census_transactions(None, _p(b.txs), _p(b.offsets), 0, 4, 16, None, c, 1, s) == INVALID_ARG
    assert lib.hsv_census_transactions(None, None, _p(b.offsets), 0, 4, 16, k, c, 16, s) == INVALID_ARG
    assert b.untouched()


def test_misaligned_device_arguments(lib):
    b = _Bufs()
    k, c, s = _p(b.keys), _p(b.counts), _p(b.summary)
    off = lambda a, d: ctypes.c_void_p(a.ctypes.data + d)
    assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 4, 16, k, off(b.counts, 4), s, None) == ALIGN
    assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 4, 16, k, c, off(b.summary, 4), None) == ALIGN
    assert lib.hsv_census_keys_device(None, off(b.pk, 8), 32, 4, 16, k, c, s, None) == ALIGN
    assert lib.hsv_census_keys_device(None, _p(b.pk), 40, 4, 16, k, c, s, None) == ALIGN
    assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 4, 16, off(b.keys, 4), c, s, None) == ALIGN
    assert lib.hsv_census_transactions_device(None, _p(b.txs), _p(b.offsets), 0, 4, 16, k, off(b.counts, 4), s,
                                              None) == ALIGN
    assert lib.hsv_census_transactions_device(None, _p(b.txs), _p(b.offsets), 0, 4, 16, k, c, off(b.summary, 4),
                                              None) == ALIGN
    assert lib.hsv_census_transactions_device(None, _p(b.txs), off(b.offsets, 4), 0, 3, 16, k, c, s, None) == ALIGN
    # a key stride of 16 is aligned but the records would overlap; a fixed size below 96 holds no key
    assert lib.hsv_census_keys_device(None, _p(b.pk), 16, 4, 16, k, c, s, None) == INVALID_ARG
    assert lib.hsv_census_transactions_device(None, _p(b.txs), None, 95, 4, 16, k, c, s, None) == INVALID_ARG
    assert b.untouched()


def test_item_bounds(lib):
    b = _Bufs()
    k, c, s = _p(b.keys), _p(b.counts), _p(b.summary)
    assert lib.hsv_census_keys(None, _p(b.pk), 32, (1 << 22) + 1, 16, k, c, 16, s) == INVALID_ARG
    assert lib.hsv_census_transactions(None, _p(b.txs), None, 128, (1 << 22) + 1, 16, k, c, 16, s) == INVALID_ARG
    assert lib.hsv_census_keys_device(None, _p(b.pk), 32, 1 << 32, 16, k, c, s, None) == INVALID_ARG
    assert lib.hsv_census_transactions_device(None, _p(b.txs), None, 128, 1 << 32, 16, k, c, s, None) == INVALID_ARG
    assert lib.hsv_census_keys(None, _p(b.pk), 16, 4, 16, k, c, 16, s) == INVALID_ARG
    assert lib.hsv_census_transactions(None, _p(b.txs), None, 95, 4, 16, k, c, 16, s) == INVALID_ARG
    assert b.untouched()


def test_accepted_arguments_reach_the_device_question(lib):
    """keys_cap 0 with keys_out NULL is accepted: the call goes on to look for
    a device.  Without one the host forms answer HSV_ERR_NO_DEVICE."""
    b = _Bufs()
    rc = lib.hsv_census_keys(None, _p(b.pk), 32, 4, 16, None, None, 0, _p(b.summary))
    rc_tx = lib.hsv_census_transactions(None, _p(b.txs), _p(b.offsets), 0, 4, 16, None, None, 0, _p(b.summary))
    if lib.hsv_device_count() <= 0:
        assert rc == NO_DEVICE and rc_tx == NO_DEVICE
        assert lib.hsv_census_keys(None, None, 32, 0, 16, None, None, 0, _p(b.summary)) == NO_DEVICE
        assert b.untouched()
    else:
        assert rc == 0 and rc_tx == 0
        assert b.summary[0] == 4 and b.summary[5] == 1  # four all-zero keys: one distinct key


def test_python_call_shapes():
    from hsverify import mempool
    from hsverify.committee import Committee
    assert callable(mempool.census) and callable(mempool.census_device) and callable(Committee.learn)
    assert mempool.default_census_slots(0) == 16 and mempool.default_census_slots(4) == 16
    assert mempool.default_census_slots(5) == 32 and mempool.default_census_slots(1000) == 4096
    assert mempool.default_census_slots(1 << 20) == 1 << 22 and mempool.default_census_slots(1 << 22) == 1 << 22
    with pytest.raises(ValueError):
        mempool.census([b"\0" * 128], slots=24)
