"""The device walk of a serialized mempool batch (csrc/hsv_batchscan.hpp, the
core of the parse kernels of csrc/hsv_batchwire.hip) compiled for the host and
run under AddressSanitizer + UndefinedBehaviorSanitizer against the host parser
(hsvw::parse_batch, csrc/hsv_wire_parse.cpp).  The harness is
tests/native/batchscan_host.cpp, a stand-alone program; no GPU is involved and
nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "batchscan_host_asan")


@pytest.fixture(scope="module")
def batchscan_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    csrc = os.path.join(PKG, "csrc")
    tmp = f"{BIN}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", csrc,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "batchscan_host.cpp"),
                    os.path.join(csrc, "hsv_wire_parse.cpp"), "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def test_device_walk_equals_the_host_parser_under_asan_ubsan(batchscan_bin):
    """Counts, spans and statuses of the window walk equal parse_batch's at every
    misalignment 0..15 and with three fill patterns around the batch: the empty
    batch, one transaction, ragged lengths with 0, 95 and 96; truncation at
    every byte, counts beyond the buffer, lengths of 2^64 - 1 and with high bits
    set, tags 1 and 2, a trailing byte; stepped batches of 8 and 15 windows
    whose prefixes land on every residue mod 16 and straddle a window edge at
    every split 1..7 (asserted from the spans); transactions of several
    windows."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([batchscan_bin], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "batchscan host ok" in r.stdout
