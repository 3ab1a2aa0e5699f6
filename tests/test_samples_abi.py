"""The ABI of the benchmark's sample-transaction calls (no GPU): include/hsv.h
declares them, libhsv.so exports them, hsv_batch_samples is 40 bytes with the
header's layout (a compiled C probe), and the ABI generation is still 3."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ("hsv_batch_samples_bincode", "hsv_batches_samples_bincode_device", "hsv_client_bursts",
       "hsv_client_bursts_device")
HEADER = os.path.join(ROOT, "include", "hsv.h")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "hsv.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(hsv_batch_samples), offsetof(hsv_batch_samples, status),
         offsetof(hsv_batch_samples, pad), offsetof(hsv_batch_samples, n_tx), offsetof(hsv_batch_samples, size),
         offsetof(hsv_batch_samples, n_samples), offsetof(hsv_batch_samples, first_sample), HSV_ABI_VERSION);
  return 0;
}
"""


def test_header_declares_the_four_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"HSV_API int " + name + r"\(", text), name
    assert "the last: the benchmark's sample transactions" in open(HEADER).read()


def test_library_exports_the_four_calls():
    from hsverify import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= exported
    lib = _lib.load(require=True)
    for name in NEW:
        assert getattr(lib, name).restype is ctypes.c_int, name


def test_struct_layout_and_abi_version(tmp_path):
    from hsverify import _lib, mempool
    assert ctypes.sizeof(mempool.BatchSamples) == 40
    assert [getattr(mempool.BatchSamples, f).offset for f, _ in mempool.BatchSamples._fields_] == [0, 4, 8, 16, 24, 32]
    assert _lib.load(require=True).hsv_abi_version() == 3
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [40, 0, 4, 8, 16, 24, 32, 3]
