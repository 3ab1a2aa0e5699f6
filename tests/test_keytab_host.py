"""The device key table of hsv_committee_verify_transactions*
(csrc/hsv_keytab.hpp) on the host, under AddressSanitizer +
UndefinedBehaviorSanitizer: the builder the committee runs once and
keytab_find, the lookup the route kernel runs per transaction on
attacker-chosen key bytes.  The harness is tests/native/keytab_host.cpp, a
stand-alone program; no GPU is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "keytab_host_asan")


@pytest.fixture(scope="module")
def keytab_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "keytab_host.cpp"), "-o", BIN], check=True)
    return BIN


def test_keytab_builder_and_find_under_asan_ubsan(keytab_bin):
    """Key counts 0, 1, 31, 32, 33 and 1000: every member at its first index
    (duplicates included), one-bit neighbours in bytes 0, 7, 8 and 31 miss, a
    20-key cluster that wraps past the end of a 64-slot table resolves, and two
    seeds give two layouts with the same answers."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([keytab_bin], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "keytab host ok" in r.stdout
