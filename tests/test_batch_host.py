"""The batch walk of the staged host calls, compiled for the host.

tests/native/batch_host.cpp includes csrc/hsv_batch.hpp -- the chunk end, chunk
geometry and length validation that hsv_verify_transactions*, hsv_verify_msgs
and hsv_signer_sign_transactions share -- and checks it with g++ against a
brute-force walk of its own: ragged batches with random lengths (0 included,
one item above the byte cap), fixed strides and stride 0, at item caps 1, 3, n
and byte caps from 1 to several items.  The program exits non-zero at its first
failed check and names it.
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "batch_host")


@pytest.fixture(scope="module")
def batch_host():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "batch_host.cpp")
    tmp = f"{BIN}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), src, "-o", tmp],
                   check=True)
    os.replace(tmp, BIN)
    return BIN


def _run(binary, mode):
    r = subprocess.run([binary, mode], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    word, checks = r.stdout.split()
    assert word == "ok"
    return int(checks)


def test_chunks_partition_respect_caps_and_are_maximal(batch_host):
    """Every chunk equals the brute-force walk's: in order, within both caps
    unless it is one item, maximal; first byte, span and relative offsets
    (0 .. span, nothing written past them) as summed from the items."""
    assert _run(batch_host, "--walk") > 10000


def test_validator_returns_the_first_bad_item(batch_host):
    """Decreasing offsets and too-short items, fixed cases and random batches."""
    assert _run(batch_host, "--validate") > 200


def test_unknown_mode_fails(batch_host):
    assert subprocess.run([batch_host, "--nothing"], capture_output=True).returncode == 2
