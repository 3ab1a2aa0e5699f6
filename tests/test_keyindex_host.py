"""The host key index of the QC paths (csrc/hsv_keyindex.hpp) under
AddressSanitizer + UndefinedBehaviorSanitizer: KeyIndex, which the explicit
committee and the automatic cache probe with attacker-chosen key bytes, and
KeyHash against the device table's mix.  The harness is
tests/native/keyindex_host.cpp, a stand-alone program; no GPU is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "keyindex_host_asan")


@pytest.fixture(scope="module")
def keyindex_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "keyindex_host.cpp"), "-o", BIN], check=True)
    return BIN


def test_keyindex_against_a_scan_under_asan_ubsan(keyindex_bin):
    """Against a brute-force scan of the key list, for 0, 1, 31, 32, 33, 1000
    and 4097 keys (up to eight grow()s): an empty index finds nothing, every
    member is found at its first index (duplicates included), one-bit
    neighbours in bytes 0 and 7 (the tag changes) and 8 and 31 (the full
    compare decides) miss; an index and its copy, grown with different keys,
    each answer for their own; and KeyHash equals hsv::keytab_hash under
    KeyHash's seed on 1000 random keys."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([keyindex_bin], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "keyindex host ok" in r.stdout
