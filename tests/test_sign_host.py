"""The signing kernels' per-lane core, compiled for the host, against the oracle.

tests/native/sign_host.cpp includes csrc/hsv_sign_core.hpp -- the header
hsv_keygen_kernel and hsv_sign_kernel are built from -- and runs it with g++
in 64-lane waves, the way the kernels deal items out (test infrastructure; the
product library never signs with it on the CPU).
"""
import os
import random
import subprocess

import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "sign_host")

# RFC 8032 section 7.1, TEST 1-3: (seed, public key, message, signature)
RFC8032 = [
    ("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
     "",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
     "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
    ("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c",
     "72",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
     "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
    ("c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7",
     "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025",
     "af82",
     "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac"
     "18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"),
]

MSG_LENS = (0, 1, 2, 32, 47, 48, 79, 80, 111, 112, 175, 176, 416, 1023)


@pytest.fixture(scope="module")
def sign_host():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "sign_host.cpp")
    tmp = f"{BIN}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"), src,
                    "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


@pytest.fixture(scope="module")
def group(sign_host):
    return int(subprocess.run([sign_host, "--group"], capture_output=True, text=True, check=True).stdout)


def _run(binary, mode, text):
    return subprocess.run([binary, mode], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def _sign(binary, batches):
    """batches: (wb, msg_len, items [(seed, msg)], inject_item, grouped) -> per batch ([(pk, sig)], fault)"""
    text = []
    for wb, msg_len, items, inject, grouped in batches:
        text.append(f"B {wb} {msg_len} {len(items)} {inject} {int(grouped)}")
        text += [f"{s.hex()} {m.hex() or '-'}" for s, m in items]
    lines = _run(binary, "--sign", "\n".join(text) + "\n")
    out, at = [], 0
    for wb, msg_len, items, inject, grouped in batches:
        rows = [tuple(bytes.fromhex(x) for x in lines[at + i].split()) for i in range(len(items))]
        fault = int(lines[at + len(items)].split()[1])
        at += len(items) + 1
        out.append((rows, fault))
    return out


def test_fixed_base_comb_matches_oracle(sign_host):
    """[x]B for the whole range x < 2^256, both digit widths: the ends, the
    recoding's extreme digits (0x7fff: the largest positive digit everywhere;
    0x8000 and 0xffff: every digit carries into the next and out of the top)."""
    rnd = random.Random(11)
    digits = lambda d: sum(d << (16 * j) for j in range(16))
    xs = [0, 1, o.L - 1, 2**252, digits(0x7fff), digits(0x8000), digits(0xffff)]
    xs += [rnd.randrange(o.L) for _ in range(200)]
    for wb in (8, 16):
        got = _run(sign_host, "--comb", "".join(f"{wb} {x.to_bytes(32, 'little').hex()}\n" for x in xs))
        bad = [hex(x) for x, g in zip(xs, got)
               if bytes.fromhex(g) != o.compress(o.to_affine(o.scalar_mult(x, o.BASEPOINT)))]
        assert not bad, (wb, bad[:4])


def test_rfc8032_vectors(sign_host):
    cases = [(wb, grouped, v) for wb in (8, 16) for grouped in (False, True) for v in RFC8032]
    batches = [(wb, len(v[2]) // 2, [(bytes.fromhex(v[0]), bytes.fromhex(v[2]))], -1, grouped) for wb, grouped, v in cases]
    for (wb, grouped, (seed, pk, msg, sig)), (rows, fault) in zip(cases, _sign(sign_host, batches)):
        assert rows[0] == (bytes.fromhex(pk), bytes.fromhex(sig)) and fault == 0, (wb, grouped, msg)


def test_expand_and_sign_match_oracle(sign_host):
    """Every padding boundary of SHA-512(prefix || M) (32 + len) and of
    SHA-512(R || pk || M) (64 + len): 111/112 and 239/240 bytes hashed close a
    block; 416 is the message of the 512-byte transaction, 1023 RFC 8032's
    long case; 32 takes the one-block fast path."""
    rnd = random.Random(12)
    batches = []
    for n in MSG_LENS:
        items = [(rnd.randbytes(32), rnd.randbytes(n)) for _ in range(5)]
        batches.append((8, n, items, -1, True))
    batches.append((16, 32, [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(5)], -1, True))
    batches.append((16, 80, [(rnd.randbytes(32), rnd.randbytes(80)) for _ in range(5)], -1, True))
    for (wb, n, items, _, _), (rows, fault) in zip(batches, _sign(sign_host, batches)):
        assert fault == 0
        for (seed, msg), (pk, sig) in zip(items, rows):
            assert pk == o.public_key(seed), (wb, n)
            assert sig == o.sign(seed, msg), (wb, n)


def test_grouped_encoding_matches_ungrouped(sign_host, group):
    """Item counts around the group (G items per lane) and the wave (64 G):
    a partly filled lane, a partly filled wave, one item in a second wave."""
    rnd = random.Random(13)
    for m in (1, group, group + 1, 64 * group - 1, 64 * group + 1):
        items = [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(m)]
        (g_rows, g_fault), (u_rows, u_fault) = _sign(sign_host, [(8, 32, items, -1, True), (8, 32, items, -1, False)])
        assert g_fault == 0 and u_fault == 0
        assert g_rows == u_rows, m
        for i in sorted({0, m // 2, m - 1}):  # and the ungrouped result is the oracle's
            assert u_rows[i] == (o.public_key(items[i][0]), o.sign(*items[i])), (m, i)


def test_corrupted_table_entry_is_contained(sign_host, group):
    """One item reads a zeroed table entry: its point fails the self-check, it
    gets a zero signature and the fault bit, and it enters its lane's product
    as 1 -- the other items of its group (same lane: every 64th item) and of
    its wave stay bit-exact."""
    rnd = random.Random(14)
    m = 64 * group + 1
    items = [(rnd.randbytes(32), rnd.randbytes(32)) for _ in range(m)]
    victim = 64 * (group // 2) + 5  # lane 5, a middle slot of its group
    (bad_rows, bad_fault), (rows, fault) = _sign(sign_host, [(8, 32, items, victim, True), (8, 32, items, -1, True)])
    assert fault == 0 and bad_fault == 1
    assert bad_rows[victim][1] == bytes(64)
    assert rows[victim][1] == o.sign(*items[victim])
    assert [r for i, r in enumerate(bad_rows) if i != victim] == [r for i, r in enumerate(rows) if i != victim]
