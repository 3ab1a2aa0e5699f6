"""The transaction signer's per-lane code, compiled for the host, against the oracle.

tests/native/txsign_host.cpp includes csrc/hsv_txsign.hpp -- the header
hsv_tx_digest_kernel and hsv_tx_sign_kernel are built from -- and runs the
digest item, sign_lane with the transaction store, and the unaligned tail
store with g++ in 64-lane waves over one byte buffer (test infrastructure; the
product library never signs with it on the CPU).

Expected bytes: message || ed25519_ref.public_key(seed) ||
ed25519_ref.sign(seed, SHA-512(message)[..32]).  The buffer sits between 0xa5
guards; the program reports whether any byte outside it changed, and its word
stores trap when they are not on a 4-byte boundary.
"""
import hashlib
import os
import random
import subprocess

import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "txsign_host")

BASES = (0, 1, 3, 4, 15)                                 # byte offset of the buffer within a 16-byte line
MSG_LENS = (0, 1, 111, 112, 127, 128, 239, 240, 416)     # SHA-512 padding boundaries, and the 512-byte transaction
FILL = 0xCC                                              # the unsigned tail, so an untouched one shows


@pytest.fixture(scope="module")
def txsign_host():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "txsign_host.cpp")
    tmp = f"{BIN}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(PKG, "csrc"), src,
                    "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


@pytest.fixture(scope="module")
def group(txsign_host):
    return int(subprocess.run([txsign_host, "--group"], capture_output=True, text=True, check=True).stdout)


_tails = {}


def tail(seed: bytes, msg: bytes) -> bytes:
    """pk || R || s of one transaction, by the oracle (memoised: the large
    batches draw their items from a small pool)."""
    key = (seed, msg)
    if key not in _tails:
        _tails[key] = o.public_key(seed) + o.sign(seed, hashlib.sha512(msg).digest()[:32])
    return _tails[key]


class Batch:
    """seeds: the signer's keys; items: (key index, message) or (key index, raw
    bytes, None) for a transaction that is not to be signed; fixed: equal
    sizes (else offsets); idx: pass the key indices (else item i uses key i)."""

    def __init__(self, base, seeds, items, fixed, idx=False, inject=-1, offsets=None):
        self.base, self.seeds, self.items, self.idx, self.inject = base, seeds, items, idx, inject
        self.raw = [it[1] + bytes([FILL]) * 96 if len(it) == 2 else it[1] for it in items]
        self.fixed = len(self.raw[0]) if fixed else 0
        self.offsets = offsets
        if not fixed and offsets is None:
            self.offsets = [0]
            for r in self.raw:
                self.offsets.append(self.offsets[-1] + len(r))
        self.data = b"".join(self.raw)

    def text(self):
        out = [f"T {self.base} {len(self.items)} {self.fixed} {self.inject} {len(self.seeds)} {int(self.idx)} "
               f"{len(self.data)}"]
        out += [s.hex() for s in self.seeds]
        if self.idx:
            out.append("I " + " ".join(str(it[0]) for it in self.items))
        if not self.fixed:
            out.append("O " + " ".join(map(str, self.offsets)))
        out.append("D " + (self.data.hex() or "-"))
        return "\n".join(out) + "\n"

    def expected(self):
        """The signed buffer: every signable item's tail replaced."""
        out = []
        for it, raw in zip(self.items, self.raw):
            if len(it) == 3:
                out.append(raw)
            elif it[0] >= len(self.seeds):
                out.append(it[1] + bytes(96))
            else:
                out.append(it[1] + tail(self.seeds[it[0]], it[1]))
        return b"".join(out)


def run(binary, batches):
    """-> per batch (buffer bytes, guards intact, fault)"""
    r = subprocess.run([binary, "--sign"], input="".join(b.text() for b in batches), capture_output=True, text=True,
                       check=True)
    lines = r.stdout.split("\n")
    assert len(lines) >= 3 * len(batches), r.stdout[-200:]
    return [(bytes.fromhex(lines[3 * k]), int(lines[3 * k + 1].split()[1]), int(lines[3 * k + 2].split()[1]))
            for k in range(len(batches))]


def check(batch, result):
    got, guards, fault = result
    want = batch.expected()
    assert guards == 1, "a byte outside the buffer was written"
    at = 0
    for i, raw in enumerate(batch.raw):
        assert got[at:at + len(raw)] == want[at:at + len(raw)], (batch.base, batch.fixed, i, len(raw))
        at += len(raw)
    assert got == want
    return fault


def test_tail_store_writes_exactly_its_96_bytes(txsign_host):
    """tx_store_tail at every byte of two 16-byte lines: the 96 bytes land,
    and nothing before or after them changes."""
    rnd = random.Random(21)
    cases = [(base, rnd.randbytes(96)) for base in range(32)]
    r = subprocess.run([txsign_host, "--tail"], input="".join(f"{b} {d.hex()}\n" for b, d in cases),
                       capture_output=True, text=True, check=True)
    for (base, data), line in zip(cases, r.stdout.split("\n")):
        want = bytes([0xA5]) * (16 + base) + data + bytes([0xA5]) * (32 - base)
        assert bytes.fromhex(line) == want, base


def test_fixed_sizes_at_every_base(txsign_host):
    """Every message-only padding boundary (tx_size 96, 97, 207, ..., 512) at
    every base offset: with tx_size no multiple of 4, the tail of transaction
    i and the message of transaction i + 1 share a word."""
    rnd = random.Random(22)
    batches = []
    for n in MSG_LENS:
        for base in BASES:
            seeds = [rnd.randbytes(32) for _ in range(3)]
            batches.append(Batch(base, seeds, [(k, rnd.randbytes(n)) for k in range(3)], fixed=True))
    assert sorted({b.fixed for b in batches}) == [96, 97, 207, 208, 223, 224, 335, 336, 512]
    for b, res in zip(batches, run(txsign_host, batches)):
        assert check(b, res) == 0


def test_ragged_batch_mixes_all_lengths(txsign_host):
    """One batch with every length, a 95-byte transaction and an empty one
    (both untouched), at every base offset."""
    rnd = random.Random(23)
    batches = []
    for base in BASES:
        lens = list(MSG_LENS) * 2
        rnd.shuffle(lens)
        items = [(k, rnd.randbytes(n)) for k, n in enumerate(lens)]
        items.insert(5, (5, rnd.randbytes(95), None))
        items.insert(11, (11, b"", None))
        items = [(k,) + it[1:] for k, it in enumerate(items)]
        batches.append(Batch(base, [rnd.randbytes(32) for _ in items], items, fixed=False))
    for b, res in zip(batches, run(txsign_host, batches)):
        assert check(b, res) == 0


def test_decreasing_offsets_skip_that_item_only(txsign_host):
    """offsets[i + 1] < offsets[i]: item i is left alone; the items around it
    (whose spans the offsets still describe) are signed."""
    rnd = random.Random(24)
    seeds = [rnd.randbytes(32) for _ in range(4)]
    msgs = [rnd.randbytes(n) for n in (17, 111, 1)]
    # items 0, 2, 3 are transactions; item 1 is the pair (end of 0, start of 2 - 50): decreasing
    raw0, raw2, raw3 = (m + bytes([FILL]) * 96 for m in msgs)
    gap = bytes([0x5A]) * 64
    data = gap + raw2 + raw0 + raw3
    o2, o0 = len(gap), len(gap) + len(raw2)
    # offsets: item 0 = [o0, o0 + len0), item 1 = [o0 + len0, o2) decreasing, then item 2 has to start at o2
    offs = [o0, o0 + len(raw0), o2, o2 + len(raw2)]
    b = Batch(3, seeds, [(0, msgs[0]), (1, b"", None), (2, msgs[1])], fixed=False, offsets=offs)
    b.data = data
    got, guards, fault = run(txsign_host, [b])[0]
    want = gap + msgs[1] + tail(seeds[2], msgs[1]) + msgs[0] + tail(seeds[0], msgs[0]) + raw3
    assert guards == 1 and fault == 0
    assert got == want


def test_item_counts_around_the_group_and_the_wave(txsign_host, group):
    """1, G, 64 G - 1 and 64 G + 1 items (a partly filled lane, a partly
    filled wave, one item in a second wave) of 97 and 207 bytes, where
    neighbouring lanes write into one word; keys repeat through key_idx."""
    rnd = random.Random(25)
    seeds = [rnd.randbytes(32) for _ in range(8)]
    batches = []
    for m in (1, group, 64 * group - 1, 64 * group + 1):
        for n, base in ((1, 1), (111, 15)):
            pool = [(rnd.randrange(8), rnd.randbytes(n)) for _ in range(12)]
            batches.append(Batch(base, seeds, [pool[rnd.randrange(12)] for _ in range(m)], fixed=True, idx=True))
    for b, res in zip(batches, run(txsign_host, batches)):
        assert check(b, res) == 0


def test_key_index_out_of_range_writes_zeros(txsign_host):
    rnd = random.Random(26)
    seeds = [rnd.randbytes(32) for _ in range(4)]
    items = [(k, rnd.randbytes(17)) for k in (0, 3, 4, 1, 0xFFFFFFFF, 2)]
    b = Batch(3, seeds, items, fixed=True, idx=True)
    got, guards, fault = res = run(txsign_host, [b])[0]
    assert check(b, res) == 0, "an index past the keys is not a fault"
    assert got[2 * 113 + 17:3 * 113] == bytes(96) and got[4 * 113 + 17:5 * 113] == bytes(96)


def test_corrupted_table_entry_is_contained(txsign_host, group):
    """One item reads a zeroed table entry (as tests/test_sign_host.py): it
    gets its pk and a zero signature and raises the fault; every other byte
    of the buffer -- its lane's other items, its neighbours' shared words --
    is what the clean run gives."""
    rnd = random.Random(27)
    m = 64 * group + 1
    seeds = [rnd.randbytes(32) for _ in range(6)]
    pool = [(rnd.randrange(6), rnd.randbytes(111)) for _ in range(10)]
    items = [pool[rnd.randrange(10)] for _ in range(m)]
    victim = 64 * (group // 2) + 5  # lane 5, a middle slot of its group
    clean = Batch(15, seeds, items, fixed=True, idx=True)
    hurt = Batch(15, seeds, items, fixed=True, idx=True, inject=victim)
    res_clean, res_hurt = run(txsign_host, [clean, hurt])
    assert check(clean, res_clean) == 0
    got, guards, fault = res_hurt
    assert guards == 1 and fault == 1
    lo, hi = victim * 207, (victim + 1) * 207
    assert got[:lo] == res_clean[0][:lo] and got[hi:] == res_clean[0][hi:]
    assert got[lo:hi] == items[victim][1] + o.public_key(seeds[items[victim][0]]) + bytes(64)
