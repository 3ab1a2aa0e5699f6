"""The compact comb core (verify_one_comb4_k, verify_one_comb4 and the table
builder comb4_build_group, csrc/hsv_comb.hpp) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer: the 4-bit digit tables behind
hsv_committee_create_ex(..., 4, ...).  The harness is
tests/native/comb4_host.cpp, a stand-alone program that builds both table
widths on the host for the keys of tests/test_comb_k_host.py and checks every
line of that generator against the flag bytes of oracle/ed25519_ref.py, then
crafted challenges (k = 0, 1, 7, 8, 9, l - 1 and three digit patterns) against
a plain double-and-add.  No GPU is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT
from test_comb_k_host import _items

BIN = os.path.join(ROOT, "build", "comb4_host_asan")
CRAFTED = 6 + 3      # k = 0, 1, 7, 8, 9, l - 1; nibbles all 0x0, all 0xF, alternating


@pytest.fixture(scope="module")
def comb4_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "comb4_host.cpp"), "-o", BIN], check=True)
    return BIN


def test_compact_comb_core_matches_the_oracle_and_plain_double_and_add(comb4_bin):
    keys, lines = _items()
    assert len(keys) == 5
    text = "\n".join([str(len(keys))] + [k.hex() for k in keys] + lines) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([comb4_bin], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    # items, 32-byte items (3 + 2), crafted k, crafted checks (accept + reject each),
    # compact entries found byte for byte in the full tables (4 decodable keys x 32 x 8 x 2)
    assert r.stdout.split() == ["comb4", "host", "ok", str(len(lines)), "5", str(CRAFTED), str(2 * CRAFTED),
                                str(4 * 32 * 8 * 2)]
