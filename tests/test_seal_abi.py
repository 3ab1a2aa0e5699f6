"""hsv_seal_* at the C ABI, without a GPU: the three entry points are exported
by libhsv.so, hsv_seal_summary is 64 bytes in the documented order, every
argument error is reported before any device work (so it is the same answer on a
machine with no device), and hsv_seal_bound is plain arithmetic."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

NO_DEVICE, INVALID_ARG, ALIGN = -1, -3, -5
ENTRY_POINTS = ("hsv_seal_bound", "hsv_seal_transactions_device", "hsv_seal_transactions")
FIELDS = ["items", "sealed", "rejected", "malformed", "held", "held_first", "bytes", "n_batches", "status"]


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def _p(a, d=0):
    return ctypes.c_void_p(a.ctypes.data + d)


class _Bufs:
    """Host arrays in the place of device buffers: the checks under test never
    read them.  numpy allocations are 16-byte aligned."""

    def __init__(self):
        self.txs = np.zeros(4 * 128, np.uint8)
        self.offsets = np.arange(6, dtype=np.uint64) * 128
        self.flags = np.ones(4, np.uint8)
        self.out = np.full(1024, 0xab, np.uint8)
        self.boff = np.full(8, 0xabababababababab, np.uint64)
        self.dig = np.full(6 * 32, 0xab, np.uint8)
        self.summary = np.full(9, 0xabababababababab, np.uint64)
        self.hflags = np.full(4, 0xab, np.uint8)

    def untouched(self):
        return ((self.out == 0xab).all() and (self.boff == 0xabababababababab).all() and (self.dig == 0xab).all()
                and (self.summary == 0xabababababababab).all() and (self.hflags == 0xab).all())

    def device(self, lib, **kw):
        a = dict(txs=_p(self.txs), offsets=_p(self.offsets), tx_size=0, n=4, flags=_p(self.flags), batch_size=200,
                 flush=1, out=_p(self.out), out_cap=1024, boff=_p(self.boff), bcap=6, dig=_p(self.dig),
                 summary=_p(self.summary))
        a.update(kw)
        return lib.hsv_seal_transactions_device(a["txs"], a["offsets"], a["tx_size"], a["n"], a["flags"],
                                                a["batch_size"], a["flush"], a["out"], a["out_cap"], a["boff"],
                                                a["bcap"], a["dig"], a["summary"], None)

    def host(self, lib, **kw):
        a = dict(txs=_p(self.txs), offsets=_p(self.offsets), tx_size=0, n=4, batch_size=200, flush=1, out=_p(self.out),
                 out_cap=1024, boff=_p(self.boff), bcap=6, dig=_p(self.dig), hflags=_p(self.hflags),
                 summary=_p(self.summary))
        a.update(kw)
        return lib.hsv_seal_transactions(None, a["txs"], a["offsets"], a["tx_size"], a["n"], a["batch_size"],
                                         a["flush"], a["out"], a["out_cap"], a["boff"], a["bcap"], a["dig"],
                                         a["hflags"], a["summary"])


def test_symbols_and_struct(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "hsverify", "libhsv.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported
    assert "hsv_test_seal_stages" not in exported
    header = open(os.path.join(ROOT, "include", "hsv.h")).read()
    body = re.search(r"typedef struct hsv_seal_summary \{(.*?)\} hsv_seal_summary;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint64_t|uint32_t)\s+([\w\s,]+);", body):
        fields += [(typ, name.strip()) for name in names.split(",")]
    assert [f for _, f in fields] == FIELDS
    assert sum(8 if t == "uint64_t" else 4 for t, _ in fields) == 64
    from hsverify.mempool import SealSummary
    assert ctypes.sizeof(SealSummary) == 64
    assert [n for n, _ in SealSummary._fields_] == FIELDS
    assert [ctypes.sizeof(t) for _, t in SealSummary._fields_] == [8 if t == "uint64_t" else 4 for t, _ in fields]
    assert re.search(r"#define HSV_SEAL_OK 0u", header) and re.search(r"#define HSV_SEAL_OVERFLOW 1u", header)


def test_device_form_argument_errors(lib):
    b = _Bufs()
    assert b.device(lib, batch_size=0) == INVALID_ARG
    assert b.device(lib, n=1 << 32) == INVALID_ARG
    assert b.device(lib, offsets=None, tx_size=0) == INVALID_ARG
    assert b.device(lib, boff=None) == INVALID_ARG
    assert b.device(lib, summary=None) == INVALID_ARG
    assert b.device(lib, out=None) == INVALID_ARG
    assert b.device(lib, txs=None) == INVALID_ARG
    # an empty batch still writes its offsets and its summary, so it needs them too
    assert b.device(lib, n=0, txs=None, offsets=None, boff=None) == INVALID_ARG
    assert b.device(lib, n=0, txs=None, offsets=None, summary=None) == INVALID_ARG
    assert b.device(lib, boff=_p(b.boff, 4)) == ALIGN
    assert b.device(lib, summary=_p(b.summary, 4)) == ALIGN
    assert b.device(lib, offsets=_p(b.offsets, 4)) == ALIGN
    assert b.untouched()


def test_output_must_not_overlap_a_fixed_size_input(lib):
    b = _Bufs()
    big = np.full(4096, 0xab, np.uint8)
    for out_at, cap in ((0, 1024), (511, 1024), (256, 16)):
        assert lib.hsv_seal_transactions_device(_p(big, 512), None, 128, 4, None, 200, 1, _p(big, 512 + out_at), cap,
                                                _p(b.boff), 6, None, _p(b.summary), None) == INVALID_ARG
    from hsverify import _lib
    assert "overlap" in _lib.last_error()
    assert (big == 0xab).all() and b.untouched()


def test_host_form_argument_errors(lib):
    b = _Bufs()
    assert b.host(lib, batch_size=0) == INVALID_ARG
    assert b.host(lib, offsets=None, tx_size=0) == INVALID_ARG
    assert b.host(lib, boff=None) == INVALID_ARG
    assert b.host(lib, summary=None) == INVALID_ARG
    assert b.host(lib, out=None) == INVALID_ARG
    assert b.host(lib, txs=None) == INVALID_ARG
    assert b.host(lib, offsets=None, tx_size=128, n=(1 << 22) + 1) == INVALID_ARG
    assert b.host(lib, offsets=None, tx_size=(1 << 29) // 4 + 1) == INVALID_ARG
    assert b.untouched()


def test_host_form_without_a_device(lib):
    b = _Bufs()
    rc = b.host(lib, offsets=None, tx_size=128)
    if lib.hsv_device_count() <= 0:
        assert rc == NO_DEVICE
        assert b.host(lib, n=0, txs=None, offsets=None) == NO_DEVICE
        assert b.untouched()
    else:
        assert rc == 0
        assert b.summary[0] == 4 and b.summary[2] == 4  # four all-zero transactions: all rejected


def _bound(total, n, batch_size):
    """The documented bound: a batch closes at a kept transaction (at most n),
    and every batch but a flushed last one holds at least batch_size bytes."""
    batches = 0 if n == 0 else min(n, total // batch_size + 1)
    return total + 8 * n + 12 * batches, batches


@pytest.mark.parametrize("total,n,batch_size", [(0, 0, 1), (0, 5, 1), (512 << 20, 1 << 20, 500_000), (1000, 3, 100),
                                                (96, 1, 96), (95, 1, 96), (10_000, 100, 1), (1 << 40, 1 << 32, 7),
                                                (12345, 67, (1 << 64) - 1)])
def test_bound_is_the_formula(lib, total, n, batch_size):
    from hsverify import mempool
    assert mempool.seal_bound(total, n, batch_size) == _bound(total, n, batch_size)


def test_bound_argument_errors(lib):
    x, y = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.hsv_seal_bound(100, 1, 0, ctypes.byref(x), ctypes.byref(y)) == INVALID_ARG
    assert lib.hsv_seal_bound((1 << 64) - 8, 1, 1, ctypes.byref(x), ctypes.byref(y)) == INVALID_ARG
    assert x.value == 7 and y.value == 7
    assert lib.hsv_seal_bound(100, 1, 10, None, None) == 0


def test_python_call_shapes():
    from hsverify import mempool
    assert callable(mempool.seal) and callable(mempool.seal_device) and callable(mempool.seal_bound)
    s = mempool.SealSummary.from_words(np.arange(8, dtype=np.int64))
    assert s.as_dict()["held_first"] == 5 and s.n_batches == 7 and s.status == 0
