"""A proposal as one verification batch, compiled for the host.

tests/native/proposal_host.cpp includes csrc/hsv_proposal.hpp -- the assembly
of a Block's author signature, QC votes and TC votes into one batch with
per-item digests, and the reduction of the batch's flags to the reference's
verdict (consensus/src/messages.rs:55-76) -- and checks it with plain g++: the
item order, the genesis-QC skip (also for a genesis QC that carries votes), the
empty non-genesis QC, and on synthetic flag arrays that PARSE_OK|EQ_OK without
STRICT_OK passes in the QC segment and fails in the TC segment and as author,
that the first failing stage in the reference's order wins, and that the lowest
failing vote is reported.  The program exits non-zero at its first failed check
and names it.  Its digests are compared with hashlib here.
"""
import hashlib
import os
import struct
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "proposal_host")


@pytest.fixture(scope="module")
def proposal_host():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "proposal_host.cpp")
    tmp = f"{BIN}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    "-I", os.path.join(ROOT, "include"), src, "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def test_batch_assembly_and_verdict_reduction(proposal_host):
    r = subprocess.run([proposal_host, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) > 100


def test_digests_match_hashlib(proposal_host):
    """Block::digest (empty payload and 3 digests), QC / Vote::digest and
    Timeout::digest of the program's fixed inputs (messages.rs:80-89, 149-156,
    201-207, 268-275)."""
    r = subprocess.run([proposal_host, "--digests"], capture_output=True, text=True, check=True)
    got = r.stdout.split()
    author, qc_hash = bytes(range(32)), bytes(range(0x20, 0x40))
    round_le = struct.pack("<Q", 0x0102030405060708)
    payload = b"".join(bytes([0xa0 + k]) * 32 for k in range(3))
    h = lambda b: hashlib.sha512(b).digest()[:32].hex()
    assert got == [h(author + round_le + qc_hash),
                   h(author + round_le + payload + qc_hash),
                   h(qc_hash + struct.pack("<Q", 7)),
                   h(struct.pack("<QQ", 9, 8))]


def test_unknown_mode_fails(proposal_host):
    assert subprocess.run([proposal_host, "--nothing"], capture_output=True).returncode == 2
