"""The k-taking comb core (verify_one_comb_k, csrc/hsv_comb.hpp) on the host,
under AddressSanitizer + UndefinedBehaviorSanitizer: the comb pass of
hsv_committee_verify_msgs* feeds it k = SHA-512(R || A || M) mod l from the
route kernel's record instead of hashing a 32-byte message.  The harness is
tests/native/comb_k_host.cpp, a stand-alone program that builds the comb tables
on the host; the expected flag bytes come from oracle/ed25519_ref.py.  No GPU
is involved."""
import os
import shutil
import subprocess

import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "comb_k_host_asan")
LENGTHS = (0, 1, 32, 47, 48, 111, 112, 175, 176, 1000)  # 32: verify_one_comb's own length


@pytest.fixture(scope="module")
def comb_k_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "comb_k_host.cpp"), "-o", BIN], check=True)
    return BIN


def _items():
    """(keys, lines): three honest keys, a small-order key and an undecodable
    one; per length an honest signature, one with a flipped s bit and one over
    a changed message (an s + l signature where the message is empty)."""
    seeds = [bytes([7 * i + 1]) * 32 for i in range(3)]
    small = next(e for e in o.small_order_encodings() if o.decompress(e) is not None and e != bytes([1]) + bytes(31))
    keys = [o.public_key(s) for s in seeds] + [small, o.find_undecodable_y()]
    lines, honest, rejected = [], 0, 0
    for j, length in enumerate(LENGTHS):
        k = j % 3
        msg = bytes((5 * j + 3 * i + 1) & 0xff for i in range(length))
        sig = o.sign(seeds[k], msg)
        flipped = sig[:40] + bytes([sig[40] ^ 4]) + sig[41:]
        if length:
            other_msg, other_sig = msg[:-1] + bytes([msg[-1] ^ 0x10]), sig
        else:
            s = int.from_bytes(sig[32:], "little") + o.L
            other_msg, other_sig = msg, sig[:32] + s.to_bytes(32, "little")
        for m, s in ((msg, sig), (msg, flipped), (other_msg, other_sig)):
            f = o.verify_flags(keys[k], s, m)
            honest += bool(f & o.STRICT_OK)
            rejected += not f & o.STRICT_OK
            lines.append(f"{k} {s.hex()} {m.hex() or '-'} {f:02x}")
        if length in (32, 112):   # the keys whose flags come from the stored key flags
            for k2 in (3, 4):
                f = o.verify_flags(keys[k2], sig, msg)
                assert not f & o.PARSE_OK or f & o.SMALL_A
                lines.append(f"{k2} {sig.hex()} {msg.hex()} {f:02x}")
    assert honest == len(LENGTHS) and rejected == 2 * len(LENGTHS)
    return keys, lines


def test_comb_core_from_k_matches_the_oracle_and_the_hashing_form(comb_k_bin):
    keys, lines = _items()
    text = "\n".join([str(len(keys))] + [k.hex() for k in keys] + lines) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([comb_k_bin], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split() == ["comb", "k", "host", "ok", str(len(lines)), "5"]   # 3 + 2 items of 32 bytes
