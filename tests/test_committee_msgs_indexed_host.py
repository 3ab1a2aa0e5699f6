"""What hsv_committee_verify_msgs_indexed* computes per item, on the host under
AddressSanitizer + UndefinedBehaviorSanitizer: k from the head_*<64> block
arithmetic over (R, the member's key, M) and the k-taking comb cores of both
table widths.  The harness is tests/native/cmsg_indexed_host.cpp, a stand-alone
program; the expected flag bytes come from oracle/ed25519_ref.py.  The lengths
are the block boundaries tests/test_committee_msgs_indexed.py runs on the GPU.
No GPU is involved."""
import os
import shutil
import subprocess

import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "cmsg_indexed_host_asan")
LENGTHS = (0, 1, 47, 48, 63, 64, 65, 175, 176, 191, 192, 193, 303, 304, 1000)


@pytest.fixture(scope="module")
def host_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "cmsg_indexed_host.cpp"), "-o", BIN], check=True)
    return BIN


def _items():
    """(keys, lines): three honest members, a small-order member and an
    undecodable one; per length an honest signature and one corrupted in s, in R
    or in the last message byte (in turn; s where the message is empty), and at
    two lengths the honest signature under the two odd members' indices."""
    seeds = [bytes([11 * i + 3]) * 32 for i in range(3)]
    small = next(e for e in o.small_order_encodings() if o.decompress(e) is not None and e != bytes([1]) + bytes(31))
    keys = [o.public_key(s) for s in seeds] + [small, o.find_undecodable_y()]
    lines, honest, rejected, kinds = [], 0, 0, set()
    for j, length in enumerate(LENGTHS):
        k = j % 3
        msg = bytes((7 * j + 5 * i + 2) & 0xff for i in range(length))
        sig = o.sign(seeds[k], msg)
        kind = ("s", "R", "msg")[j % 3] if length else "s"
        if kind == "s":
            bad_msg, bad_sig = msg, sig[:40] + bytes([sig[40] ^ 4]) + sig[41:]
        elif kind == "R":
            bad_msg, bad_sig = msg, bytes([sig[0] ^ 2]) + sig[1:]
        else:
            bad_msg, bad_sig = msg[:-1] + bytes([msg[-1] ^ 0x10]), sig
        kinds.add(kind)
        for m, s in ((msg, sig), (bad_msg, bad_sig)):
            f = o.verify_flags(keys[k], s, m)
            honest += bool(f & o.STRICT_OK)
            rejected += not f & o.STRICT_OK
            lines.append(f"{k} {s.hex()} {m.hex() or '-'} {f:02x}")
        if length in (64, 192):   # the members whose flags come from the stored key flags
            for k2 in (3, 4):
                f = o.verify_flags(keys[k2], sig, msg)
                assert not f & o.PARSE_OK or f & o.SMALL_A
                lines.append(f"{k2} {sig.hex()} {msg.hex()} {f:02x}")
    assert honest == len(LENGTHS) and rejected == len(LENGTHS) and kinds == {"s", "R", "msg"}
    return keys, lines


def test_head_hash_and_comb_cores_match_the_oracle(host_bin):
    keys, lines = _items()
    text = "\n".join([str(len(keys))] + [k.hex() for k in keys] + lines) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([host_bin], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split() == ["cmsg", "indexed", "host", "ok", str(len(lines))]
