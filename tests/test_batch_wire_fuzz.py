"""The serialized-batch parser (hsvw::parse_batch, csrc/hsv_wire_parse.cpp) and
the device walk's core (csrc/hsv_batchscan.hpp, compiled for the host) fuzzed
under AddressSanitizer + UndefinedBehaviorSanitizer.  They read untrusted
network bytes: a batch arrives as a TCP frame and Core::make_vote reads it back
from the store (consensus/src/core.rs:113-142).  The harness is
tests/native/batch_wire_fuzz.cpp, a program of its own linked with the
sanitizers; no GPU is involved and nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "batch_wire_fuzz_asan")


@pytest.fixture(scope="module")
def fuzz_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    csrc = os.path.join(PKG, "csrc")
    tmp = f"{BIN}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", csrc,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "batch_wire_fuzz.cpp"),
                    os.path.join(csrc, "hsv_wire_parse.cpp"), "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def test_batch_parsers_fuzz_under_asan_ubsan(fuzz_bin):
    """A fixed seed, about a second: valid encodings round-trip, every prefix,
    extension and foreign tag is rejected, and on 100 000 mutated inputs the
    parser and the walk agree on verdict, count and spans with no sanitizer
    report."""
    # the program carries its own sanitizer runtime; as tests/test_wire_fuzz.py, it does not insist on being the
    # first library of the process where the environment preloads one of its own
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "100000", "20261021"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "batch wire fuzz ok" in r.stdout
