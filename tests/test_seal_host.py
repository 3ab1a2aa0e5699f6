"""The arithmetic of hsv_seal_transactions* (csrc/hsv_seal.hpp) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer: the functions the kernels of
csrc/hsv_seal.hip are built from.  The harness is tests/native/seal_host.cpp, a
stand-alone program; no GPU is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "seal_host_asan")


@pytest.fixture(scope="module")
def seal_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "native", "seal_host.cpp"),
                    "-o", BIN], check=True)
    return BIN


def test_seal_arithmetic_under_asan_ubsan(seal_bin):
    """300 transactions (kept, rejected, malformed, some empty), batch_size 1, 96,
    97, 1000, above the total and 2^64 - 1, flush on and off: the cut walk gives
    BatchMaker::run's batches, offsets and held count; the places of seal_dst
    and the chunk copy reproduce a naive serializer's bytes between guards, from
    an input and into an output at odd positions; hsv_seal_bound's arithmetic
    is never below the need.  The chunk copy alone for every (source mod 16,
    destination mod 16) and lengths 0..80: the destination's other bytes keep
    their fill and no source chunk without a source byte is read."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([seal_bin], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "seal host ok" in r.stdout
