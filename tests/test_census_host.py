"""The insert step of the signer census (csrc/hsv_census.hpp) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer: the function the lanes of
hsv_census_count_kernel run per distinct key, with the __atomic builtins in
the place of the device atomics.  The harness is tests/native/census_host.cpp,
a stand-alone program; no GPU is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "census_host_asan")


@pytest.fixture(scope="module")
def census_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-pthread",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "native", "census_host.cpp"),
                    "-o", BIN], check=True)
    return BIN


def test_census_insert_under_asan_ubsan(census_bin):
    """0, 1, 15, 16, 17 and 1000 distinct keys under two seeds; duplicates and
    the batch twice over; one-bit neighbours in bytes 0, 7, 8 and 31 as keys of
    their own; a group's population count in one insert; an 8-key cluster at
    home slot 13 of a 16-slot table that wraps past its end, under two seeds; a
    full 16-slot table (every recorded count exact, overflow = the rest, every
    walk ends); a walk given up after 256 occupied slots and one of 201 that
    reaches its empty slot; the same items from 8 threads at once, the same
    multiset out."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([census_bin], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "census host ok" in r.stdout
