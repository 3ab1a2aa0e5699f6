"""The message signer's per-lane code, compiled for the host, against the oracle.

tests/native/msgsign_host.cpp includes csrc/hsv_msgsign.hpp -- the header the
three launches of hsv_signer_sign_msgs* are built from -- and runs the nonce
item, sign_lane with the point-only store, and the response item with g++ in
64-lane waves (test infrastructure; the product library never signs with it on
the CPU).  The hash is hsv_msghash.hpp's head_msg_hash for heads of 32 and 64
bytes, the block arithmetic the kernels' staged loop uses.

Expected bytes: ed25519_ref.sign(seed, message), memoised over a small pool.
The message buffer is allocated as exactly the 16-byte lines it touches, the
signature array sits between 0xa5 guards.
"""
import os
import random
import subprocess

import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "msgsign_host")
SRC = os.path.join(ROOT, "tests", "native", "msgsign_host.cpp")

# every length at which either hash changes its block count (32 + len: 79 / 80,
# 207 / 208; 64 + len: 47 / 48, 175 / 176) or a staging window ends (96, 224 for
# r; 64, 192 for k)
SIGN_MSG_LENS = (0, 1, 31, 32, 33, 46, 47, 48, 49, 63, 64, 65, 78, 79, 80, 81, 95, 96, 97, 111, 112, 127, 128, 174,
                 175, 176, 177, 191, 192, 193, 206, 207, 208, 209, 223, 224, 225, 1023)
BASES = (0, 1, 3, 4, 15)  # byte offset of the buffer within a 16-byte line

_rnd = random.Random(41)
SEEDS = [_rnd.randbytes(32) for _ in range(3)]
POOL = {n: _rnd.randbytes(n) for n in SIGN_MSG_LENS}  # one message per length


def _build(out, extra=()):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = f"{out}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(PKG, "csrc"), SRC,
                    "-o", tmp], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def msgsign_host():
    return _build(BIN)


@pytest.fixture(scope="module")
def group(msgsign_host):
    return int(subprocess.run([msgsign_host, "--group"], capture_output=True, text=True, check=True).stdout)


_sigs = {}


def sig(seed: bytes, msg: bytes) -> bytes:
    key = (seed, msg)
    if key not in _sigs:
        _sigs[key] = o.sign(seed, msg)
    return _sigs[key]


class Batch:
    """items: (key index, message); fixed: every message has the length of the
    first and sits at `stride` (default: that length; 0: the first message is
    shared); else back to back by offsets.  idx: pass the key indices (else
    item i uses key i)."""

    def __init__(self, base, seeds, items, fixed, idx=False, inject=-1, stride=None, offsets=None, data=None):
        self.base, self.seeds, self.items, self.idx, self.inject = base, seeds, items, idx, inject
        self.msg_len, self.stride, self.offsets = -1, 0, offsets
        if fixed:
            self.msg_len = len(items[0][1])
            self.stride = self.msg_len if stride is None else stride
            if self.stride == 0:
                self.data = items[0][1]
            else:
                pad = bytes([0x5A]) * (self.stride - self.msg_len)
                self.data = pad.join(it[1] for it in items)
        else:
            if offsets is None:
                self.offsets = [0]
                for it in items:
                    self.offsets.append(self.offsets[-1] + len(it[1]))
            self.data = b"".join(it[1] for it in items) if data is None else data

    def text(self):
        out = [f"M {self.base} {len(self.items)} {self.msg_len} {self.stride} {self.inject} {len(self.seeds)} "
               f"{int(self.idx)} {len(self.data)}"]
        out += [s.hex() for s in self.seeds]
        if self.idx:
            out.append("I " + " ".join(str(it[0]) for it in self.items))
        if self.msg_len < 0:
            out.append("O " + " ".join(map(str, self.offsets)))
        out.append("D " + (self.data.hex() or "-"))
        return "\n".join(out) + "\n"

    def expected(self):
        return [bytes(64) if it[0] >= len(self.seeds) or it[1] is None else sig(self.seeds[it[0]], it[1])
                for it in self.items]


def run(binary, batches):
    """-> per batch (list of 64-byte signatures, guards intact, fault)"""
    r = subprocess.run([binary, "--sign"], input="".join(b.text() for b in batches), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert len(lines) >= 3 * len(batches), r.stdout[-200:]
    out = []
    for k in range(len(batches)):
        raw = bytes.fromhex(lines[3 * k])
        out.append(([raw[i:i + 64] for i in range(0, len(raw), 64)], int(lines[3 * k + 1].split()[1]),
                    int(lines[3 * k + 2].split()[1])))
    return out


def check(batch, result):
    got, guards, fault = result
    assert guards == 1, "a byte outside the signature array was written"
    want = batch.expected()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (batch.base, batch.msg_len, i, batch.items[i][0], len(batch.items[i][1] or b""))
    return fault


def ragged_all_lengths(base, rnd):
    lens = list(SIGN_MSG_LENS)
    rnd.shuffle(lens)
    return Batch(base, SEEDS, [(rnd.randrange(3), POOL[n]) for n in lens], fixed=False, idx=True)


def test_every_length_at_every_base_ragged(msgsign_host):
    """One wave holding all lengths shuffled -- an empty message and the
    longest among them -- at every base offset."""
    rnd = random.Random(42)
    batches = [ragged_all_lengths(base, rnd) for base in BASES]
    assert all(len(b.items) <= 64 for b in batches)
    for b, res in zip(batches, run(msgsign_host, batches)):
        assert check(b, res) == 0


def test_every_length_at_every_base_fixed(msgsign_host):
    """Equal messages of every length at their own stride, at every base."""
    batches = [Batch(base, SEEDS, [(k, POOL[n]) for k in range(3)], fixed=True)
               for n in SIGN_MSG_LENS for base in BASES]
    for b, res in zip(batches, run(msgsign_host, batches)):
        assert check(b, res) == 0


def test_fixed_stride_above_the_length_and_shared_message(msgsign_host):
    batches = []
    for n in (33, 111, 176):
        batches.append(Batch(3, SEEDS, [(k, POOL[n]) for k in range(3)], fixed=True, stride=n + 7))
        batches.append(Batch(15, SEEDS, [(k, POOL[n]) for k in range(3)], fixed=True, stride=0))
    for b, res in zip(batches, run(msgsign_host, batches)):
        assert check(b, res) == 0


def test_all_messages_empty_and_no_buffer(msgsign_host):
    """Every message empty: the buffer pointer is NULL and nothing is loaded."""
    batches = [Batch(0, SEEDS, [(k, b"") for k in range(3)], fixed=False),
               Batch(0, SEEDS, [(k, b"") for k in range(3)], fixed=True)]
    for b, res in zip(batches, run(msgsign_host, batches)):
        assert check(b, res) == 0


def test_item_counts_around_the_group_and_the_wave(msgsign_host, group):
    """1, G, 64 G - 1 and 64 G + 1 items (a partly filled lane, a partly
    filled wave, one item in a second wave); keys repeat through key_idx."""
    rnd = random.Random(43)
    lens = (0, 47, 48, 79, 80, 96, 175, 207, 224)
    batches = []
    for m in (1, group, 64 * group - 1, 64 * group + 1):
        items = [(rnd.randrange(3), POOL[lens[rnd.randrange(len(lens))]]) for _ in range(m)]
        batches.append(Batch(1, SEEDS, items, fixed=False, idx=True))
    for b, res in zip(batches, run(msgsign_host, batches)):
        assert check(b, res) == 0


def test_key_index_out_of_range_writes_zeros(msgsign_host):
    items = [(k, POOL[33]) for k in (0, 2, 3, 1, 0xFFFFFFFF, 2)]
    b = Batch(3, SEEDS, items, fixed=False, idx=True)
    got, guards, fault = res = run(msgsign_host, [b])[0]
    assert check(b, res) == 0, "an index past the keys is not a fault"
    assert got[2] == bytes(64) and got[4] == bytes(64)


def test_decreasing_offsets_zero_that_item_only(msgsign_host):
    """offsets[i + 1] < offsets[i]: item i gets 64 zero bytes and no fault;
    the items around it (whose spans the offsets still describe) are signed."""
    m0, m2 = POOL[81], POOL[47]
    data = m2 + m0
    offs = [len(m2), len(m2) + len(m0), 0, len(m2)]  # item 1 = [128, 0): decreasing
    b = Batch(4, SEEDS, [(0, m0), (1, None), (2, m2)], fixed=False, offsets=offs, data=data)
    got, guards, fault = res = run(msgsign_host, [b])[0]
    assert check(b, res) == 0
    assert got[1] == bytes(64) and got[0] != bytes(64) and got[2] != bytes(64)


def test_corrupted_table_entry_is_contained(msgsign_host, group):
    """One item reads a zeroed table entry (as tests/test_sign_host.py): it
    gets 64 zero bytes and raises the fault; every other byte of the output
    is what the clean run gives."""
    rnd = random.Random(44)
    m = 64 * group + 1
    lens = (1, 48, 111, 176)
    items = [(rnd.randrange(3), POOL[lens[rnd.randrange(len(lens))]]) for _ in range(m)]
    victim = 64 * (group // 2) + 5  # lane 5, a middle slot of its group
    clean = Batch(15, SEEDS, items, fixed=False, idx=True)
    hurt = Batch(15, SEEDS, items, fixed=False, idx=True, inject=victim)
    res_clean, res_hurt = run(msgsign_host, [clean, hurt])
    assert check(clean, res_clean) == 0
    got, guards, fault = res_hurt
    assert guards == 1 and fault == 1
    assert got[victim] == bytes(64)
    assert got[:victim] == res_clean[0][:victim] and got[victim + 1:] == res_clean[0][victim + 1:]


def test_sanitized_build_reads_no_byte_past_the_last_line(msgsign_host):
    """The same program under AddressSanitizer and UBSan, stand-alone: the
    message buffer is exactly the 16-byte lines the messages touch, so a chunk
    load past the last one aborts the run."""
    binary = _build(BIN + "_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    rnd = random.Random(45)
    batches = [ragged_all_lengths(base, rnd) for base in BASES]
    batches.append(Batch(0, SEEDS, [(k, b"") for k in range(3)], fixed=False))
    batches.append(Batch(0, SEEDS, [(k, b"") for k in range(3)], fixed=True))
    batches.append(Batch(0, SEEDS, [(0, POOL[0]), (1, POOL[1]), (2, POOL[0])], fixed=False))  # ends one byte into a line
    for b, res in zip(batches, run(binary, batches)):
        assert check(b, res) == 0
