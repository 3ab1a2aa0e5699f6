"""The any-length message hash of the verifier, compiled for the host.

tests/native/msg_host.cpp includes csrc/hsv_msghash.hpp -- the header
hsv_msg_prep_kernel (csrc/hsv_msgs.hip) hashes SHA-512(R || A || M) with --
and runs it with g++ against hashlib, at every length where the padding or the
block count changes and at every start alignment.  It also runs the split
scalar prepass (prep_from_hash, csrc/hsv_verify_hc.hpp) against the unsplit
prep_scalars (test infrastructure; the product never hashes on the CPU).
"""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "msg_host")

# 64 + len crosses the padding boundary (111/112 mod 128) at 47/48 and 175/176;
# 64 and 192 are block edges; 1023 is RFC 8032's long case
MSG_LENS = (0, 1, 31, 32, 33, 46, 47, 48, 49, 63, 64, 65, 111, 112, 127, 128, 174, 175, 176, 177, 191, 192, 193, 1023)
PREP_WORDS = 19


@pytest.fixture(scope="module")
def msg_host():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "msg_host.cpp")
    tmp = f"{BIN}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"), src,
                    "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def _run(binary, args, text):
    r = subprocess.run([binary, *args], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    return r.stdout.split("\n")


def test_hash_matches_hashlib_at_every_length_and_alignment(msg_host):
    """Every length of MSG_LENS at every start offset 0..15 mod 16.  The
    program's chunk loader aborts on a load outside the chunks of the
    message's first and last byte, and on any load for an empty message; the
    message ends flush with its buffer."""
    rnd = random.Random(21)
    cases = [(sh, rnd.randbytes(64), rnd.randbytes(n)) for n in MSG_LENS for sh in range(16)]
    got = _run(msg_host, ["--hash"], "".join(f"{sh} {h.hex()} {m.hex() or '-'}\n" for sh, h, m in cases))
    bad = [(len(m), sh) for (sh, h, m), g in zip(cases, got) if g != hashlib.sha512(h + m).hexdigest()]
    assert not bad, bad[:8]
    assert len(got) >= len(cases)


def test_block_count_and_length_field_far_past_one_block(msg_host):
    """Several whole blocks and a tail: lengths around 8 blocks, unaligned."""
    rnd = random.Random(22)
    cases = [(sh, rnd.randbytes(64), rnd.randbytes(n)) for n in (959, 960, 961, 1087, 1088, 4096 + 7) for sh in (0, 5, 15)]
    got = _run(msg_host, ["--hash"], "".join(f"{sh} {h.hex()} {m.hex()}\n" for sh, h, m in cases))
    assert [g for (sh, h, m), g in zip(cases, got)] == [hashlib.sha512(h + m).hexdigest() for sh, h, m in cases]


def _prep(binary, bits, golden, count):
    n = min(count, len(golden["pk"]))
    text = "".join(f"{golden['pk'][i].tobytes().hex()} {golden['sig'][i].tobytes().hex()} "
                   f"{golden['msg'][i].tobytes().hex()}\n" for i in range(n))
    rows = [l.split() for l in _run(binary, ["--prep", str(bits)], text) if l]
    assert len(rows) == n
    return rows


@pytest.mark.parametrize("bits", [138, 128])
def test_split_prepass_equals_unsplit(msg_host, golden, bits):
    """prep_from_hash on SHA-512(R || A || M) writes prep_scalars' record, word
    for word, on 32-byte messages (edge vectors and random ones).  Its KREC
    form differs in one place only: a fallback item's eight b words carry
    k mod l.  At the lowered bound (128 bits) many items are fallback items.
    An item marked void gets the meta word 8 alone and is never a fallback."""
    rows = _prep(msg_host, bits, golden, 600)
    nfb = 0
    for f0, f1, f2, f3, meta_void, r0, r1, r2, k in rows:
        assert r0 == r1 and f0 == f1 == f2, "split and unsplit prepass differ"
        assert f3 == "0" and meta_void == "00000008"
        w1 = [r1[8 * j:8 * j + 8] for j in range(PREP_WORDS)]
        w2 = [r2[8 * j:8 * j + 8] for j in range(PREP_WORDS)]
        assert w2[:10] == w1[:10] and w2[18] == w1[18]
        fallback = bool(int(w1[18], 16) & 4)
        assert fallback == (f1 == "1")
        if fallback:
            nfb += 1
            assert "".join(w2[10:18]) == k
        else:
            assert w2[10:18] == w1[10:18]
    if bits == 128:
        assert nfb > 20, "the lowered bound must send items down the full-length path"
