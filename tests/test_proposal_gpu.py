"""Block::verify, Timeout::verify and Vote::verify in one call each, on the GPU.

Keys and signatures come from hsv_sign_many.  Every verdict is derived here,
in Python, from the C oracle's per-item flags (conftest.oracle_flags) under the
reference's rules (consensus/src/messages.rs:55-76, 136-146, 250-265): the
author and every TC vote need STRICT_OK over their own digest, every vote of a
non-genesis QC needs PARSE_OK and EQ_OK, the first failing stage in the order
author, QC, TC is reported with its lowest failing vote -- never from the
library's own flags.  Each case runs on three routes, which must agree: c ==
NULL with the automatic committee cache warm, c == NULL with the cache off,
and an explicit committee (votes by member index).

Shapes: 1 + 3 + 3, 1 + 67 + 67 and 1 + 667 + 667 items (C1, C2, C3), blocks
without a TC, with a genesis QC, with an empty payload and with 3 digests; a
chain of 3 blocks, and one of 70 blocks of 1 + 67 items (4760 items: past the
4096-key limit of the cached latency path and past 2^12) with an unparsable
block among them.
"""
import copy
import ctypes
import dataclasses
import hashlib
import json
import os
import struct
from typing import List, Optional, Tuple

import numpy as np
import pytest

import ed25519_ref as o
from conftest import GOLDEN, oracle_flags

pytestmark = pytest.mark.gpu

OK, AUTHOR, QC, TC, PARSE = range(5)
BATCH = o.PARSE_OK | o.EQ_OK
NKEYS = 668  # 667 voters (a C3 quorum) and an author


def le(x):
    return struct.pack("<Q", x)


def h32(b):
    return hashlib.sha512(b).digest()[:32]


def flip(b: bytes, at: int, bit: int = 1) -> bytes:
    x = bytearray(b)
    x[at] ^= bit
    return bytes(x)


@dataclasses.dataclass
class Blk:
    author: bytes
    sig: bytes
    round: int
    payload: List[bytes]
    qc_hash: bytes
    qc_round: int
    qc_votes: List[Tuple[bytes, bytes]]
    tc_round: Optional[int] = None
    tc_votes: List[Tuple[bytes, bytes, int]] = dataclasses.field(default_factory=list)

    def digest(self):
        return h32(self.author + le(self.round) + b"".join(self.payload) + self.qc_hash)

    def encode(self):
        from hsverify import wire
        return wire.encode_block(wire.encode_qc(self.qc_hash, self.qc_round, self.qc_votes),
                                 None if self.tc_round is None else wire.encode_tc(self.tc_round, self.tc_votes),
                                 self.author, self.round, self.payload, self.sig)

    def items(self):
        """[(stage, index, pk, sig, digest)] in the order author, QC votes, TC
        votes; a QC with a zero hash and round 0 contributes none."""
        out = [(AUTHOR, 0, self.author, self.sig, self.digest())]
        if self.qc_hash != bytes(32) or self.qc_round != 0:
            d = h32(self.qc_hash + le(self.qc_round))
            out += [(QC, i, pk, sig, d) for i, (pk, sig) in enumerate(self.qc_votes)]
        if self.tc_round is not None:
            out += [(TC, i, pk, sig, h32(le(self.tc_round) + le(hqc))) for i, (pk, sig, hqc) in enumerate(self.tc_votes)]
        return out

    def but(self, **kw):
        b = copy.copy(self)
        for k, v in kw.items():
            setattr(b, k, v)
        return b


@dataclasses.dataclass
class Tmo:
    """consensus::Timeout: its items are a block's without a TC, the author's digest its own."""
    author: bytes
    sig: bytes
    round: int
    qc_hash: bytes
    qc_round: int
    qc_votes: List[Tuple[bytes, bytes]]

    def encode(self):
        from hsverify import wire
        return wire.encode_timeout(wire.encode_qc(self.qc_hash, self.qc_round, self.qc_votes), self.round,
                                   self.author, self.sig)

    def items(self):
        out = [(AUTHOR, 0, self.author, self.sig, h32(le(self.round) + le(self.qc_round)))]
        if self.qc_hash != bytes(32) or self.qc_round != 0:
            d = h32(self.qc_hash + le(self.qc_round))
            out += [(QC, i, pk, sig, d) for i, (pk, sig) in enumerate(self.qc_votes)]
        return out

    but = Blk.but


class World:
    """The committee's keys, the oracle with a memo of its answers, the routes."""

    def __init__(self, lib, oracle):
        from hsverify.committee import Committee
        self.lib, self.oracle, self.memo = lib, oracle, {}
        rnd = np.random.default_rng(20261020)
        self.seeds = rnd.integers(0, 256, (NKEYS, 32), dtype=np.uint8)
        self.rnd = rnd
        pk, _ = self._sign_rows(np.arange(NKEYS), np.zeros((NKEYS, 32), np.uint8))
        self.pk = [bytes(p) for p in pk]
        self.committee = Committee(pk)

    def _sign_rows(self, idx, msgs):
        from hsverify import verifier
        return verifier.sign_many(self.seeds[idx], msgs, nthreads=16)

    def sign(self, idx, digests) -> List[bytes]:
        """Key idx[i] signs digests[i] (bytes each)."""
        idx = np.asarray(idx)
        msgs = np.frombuffer(b"".join(digests), np.uint8).reshape(len(idx), 32)
        return [bytes(s) for s in self._sign_rows(idx, msgs)[1]]

    def block(self, n, tc=True, genesis=False, n_payload=3, round_=9, author=NKEYS - 1) -> Blk:
        """A valid block: voters 0 .. n-1 sign the QC (and the TC), `author` the block."""
        rnd = self.rnd
        payload = [bytes(rnd.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n_payload)]
        if genesis:  # skipped whatever votes it carries: these are garbage
            qc_hash, qc_round = bytes(32), 0
            qc_votes = [(self.pk[i], bytes(rnd.integers(0, 256, 64, dtype=np.uint8))) for i in range(min(n, 3))]
        else:
            qc_hash, qc_round = bytes(rnd.integers(0, 256, 32, dtype=np.uint8)), round_ - 1
            sigs = self.sign(range(n), [h32(qc_hash + le(qc_round))] * n)
            qc_votes = [(self.pk[i], sigs[i]) for i in range(n)]
        b = Blk(self.pk[author], b"", round_, payload, qc_hash, qc_round, qc_votes)
        if tc:
            b.tc_round = round_ - 1
            hqc = [round_ - 2 - i % 3 for i in range(n)]  # three distinct high_qc_rounds
            sigs = self.sign(range(n), [h32(le(b.tc_round) + le(r)) for r in hqc])
            b.tc_votes = [(self.pk[i], sigs[i], hqc[i]) for i in range(n)]
        b.sig = self.sign([author], [b.digest()])[0]
        return b

    # ---- the reference's verdict, from the oracle's flags -----------------
    def flags(self, items) -> np.ndarray:
        keys = [pk + sig + d for _, _, pk, sig, d in items]
        miss = [i for i, k in enumerate(keys) if k not in self.memo]
        if miss:
            arr = np.frombuffer(b"".join(keys[i] for i in miss), np.uint8).reshape(-1, 128)
            f = oracle_flags(self.oracle, arr[:, :32], arr[:, 32:96], arr[:, 96:])
            for i, v in zip(miss, f):
                self.memo[keys[i]] = int(v)
        return np.array([self.memo[k] for k in keys], np.uint8)

    def verdict(self, obj):
        for (stage, index, *_), f in zip(obj.items(), self.flags(obj.items())):
            good = (f & o.STRICT_OK) if stage != QC else (f & BATCH) == BATCH
            if not good:
                return False, (stage, index)
        return True, (OK, 0)

    # ---- routes --------------------------------------------------------------
    def warm(self):
        """Every key of the world in the automatic cache (they recur in batches, as a committee's do)."""
        lib = self.lib
        lib.hsv_set_auto_committee(1)
        if lib.hsv_auto_committee_size() >= NKEYS:
            return
        packed = b"".join(pk + bytes(64) for pk in self.pk)
        for _ in range(3):
            assert lib.hsv_verify_batch_packed(bytes(32), packed, NKEYS) == 0
        assert lib.hsv_auto_committee_wait(60000) == 1
        assert lib.hsv_auto_committee_size() >= NKEYS

    def on_routes(self, calls, committee=None):
        """calls: functions of a committee argument.  Runs all of them with the
        cache warm, then with the explicit committee, then with the cache off;
        the three lists of answers must be equal.  Returns one."""
        committee = self.committee if committee is None else committee
        self.warm()
        warm = [c(None) for c in calls]
        member = [c(committee) for c in calls]
        self.lib.hsv_set_auto_committee(0)
        try:
            assert self.lib.hsv_auto_committee_size() == 0
            off = [c(None) for c in calls]
        finally:
            self.lib.hsv_set_auto_committee(1)
        assert warm == member, [i for i, (a, b) in enumerate(zip(warm, member)) if a != b]
        assert warm == off, [i for i, (a, b) in enumerate(zip(warm, off)) if a != b]
        return warm


@pytest.fixture(scope="module")
def world(hsv, oracle_lib):
    w = World(hsv, oracle_lib)
    yield w
    hsv.hsv_set_auto_committee(1)


def block_call(buf):
    from hsverify import wire
    return lambda c: wire.block_verify(buf, committee=c)[:2]


# ---- blocks: shapes, routes, tampering -------------------------------------------
@pytest.mark.parametrize("n", [3, 67, 667])
def test_block_shapes_routes_and_tampering(world, n):
    from hsverify import wire
    base = world.block(n)
    last = n - 1
    k = n // 2
    qv, tv = base.qc_votes, base.tc_votes
    cases = {
        "valid": (base, (OK, 0)),
        "no_tc_empty_payload": (world.block(n, tc=False, n_payload=0), (OK, 0)),
        "genesis_qc_with_garbage_votes": (world.block(n, genesis=True), (OK, 0)),
        "author_signature": (base.but(sig=flip(base.sig, 40)), (AUTHOR, 0)),
        "payload_digest": (base.but(payload=[base.payload[0], flip(base.payload[1], 0), base.payload[2]]), (AUTHOR, 0)),
        "round": (base.but(round=base.round ^ 1), (AUTHOR, 0)),
        "first_qc_vote": (base.but(qc_votes=[(qv[0][0], flip(qv[0][1], 3))] + qv[1:]), (QC, 0)),
        "last_qc_vote": (base.but(qc_votes=qv[:last] + [(qv[last][0], flip(qv[last][1], 50))]), (QC, last)),
        "tc_vote_signature": (base.but(tc_votes=tv[:k] + [(tv[k][0], flip(tv[k][1], 33), tv[k][2])] + tv[k + 1:]),
                              (TC, k)),
        "tc_vote_high_qc_round": (base.but(tc_votes=tv[:last] + [(tv[last][0], tv[last][1], tv[last][2] + 1)]),
                                  (TC, last)),
        # two stages fail: the reference's order decides, and the lowest vote
        "qc_and_tc": (base.but(qc_votes=qv[:last] + [(qv[last][0], flip(qv[last][1], 50))],
                               tc_votes=[(tv[0][0], flip(tv[0][1], 1), tv[0][2])] + tv[1:]), (QC, last)),
    }
    names = list(cases)
    for name in names:  # the oracle and the rules decide; the table above only says what that must come to
        blk, want = cases[name]
        assert world.verdict(blk) == (want == (OK, 0), want), name
    got = world.on_routes([block_call(cases[name][0].encode()) for name in names])
    for name, g in zip(names, got):
        assert g == world.verdict(cases[name][0]), name
    # the decoded keys and counts, for the caller's quorum checks
    ok, res, n_qc, n_tc, pks = wire.block_verify(base.encode())
    assert (ok, res, n_qc, n_tc) == (True, (OK, 0), n, n)
    assert [bytes(p) for p in pks] == [base.author] + [v[0] for v in qv] + [v[0] for v in tv]
    ok, res, n_qc, n_tc, pks = wire.block_verify(cases["genesis_qc_with_garbage_votes"][0].encode())
    assert (ok, n_qc, n_tc, len(pks)) == (True, min(n, 3), n, 1 + min(n, 3) + n)

    # the same block as plain data: verdict and raw flags, flag for flag against the oracle
    def plain(blk):
        return lambda c: (lambda r: (r[0], r[1], r[2].tobytes()))(wire.proposal_verify(
            blk.author, blk.sig, blk.round, blk.payload, blk.qc_hash, blk.qc_round, blk.qc_votes, blk.tc_round,
            blk.tc_votes, committee=c))
    for name in ("valid", "qc_and_tc"):
        blk = cases[name][0]
        ok, res, flags = world.on_routes([plain(blk)])[0]
        assert (ok, res) == world.verdict(blk), name
        assert flags == world.flags(blk.items()).tobytes(), name


def _edge_batch_only(world, digest):
    """(pk, sig) of the golden edge vectors -- small-order and non-canonical
    encodings -- whose oracle flags over `digest` pass the batch rule and not
    the strict one (identity A and R with s = 0 satisfy the equation over any
    message)."""
    with open(os.path.join(GOLDEN, "edge_vectors.json")) as f:
        edge = json.load(f)["vectors"]
    cand = [(bytes.fromhex(e["pk"]), bytes.fromhex(e["sig"])) for e in edge
            if e["case"].startswith(("identity_R", "small_"))]
    f = world.flags([(QC, 0, pk, sig, digest) for pk, sig in cand])
    return [c for c, x in zip(cand, f) if (x & BATCH) == BATCH and not x & o.STRICT_OK]


def test_mixed_rules_in_one_batch(world):
    """One item with PARSE_OK | EQ_OK and without STRICT_OK: in the QC the
    block passes (verify_batch's rule), in the TC it fails at that index
    (verify_strict's), in the same batch of one call."""
    from hsverify.committee import Committee
    base = world.block(3)
    qc_digest = h32(base.qc_hash + le(base.qc_round))
    picks = _edge_batch_only(world, qc_digest)
    assert len({pk for pk, _ in picks}) >= 2, "the golden edge vectors hold a canonical and a non-canonical one"
    keys = sorted({pk for pk, _ in picks})
    committee = Committee(world.pk[:3] + [world.pk[-1]] + keys)
    blocks, wants = [], []
    for pk, sig in picks:
        in_qc = base.but(qc_votes=[base.qc_votes[0], (pk, sig), base.qc_votes[2]])
        in_tc = base.but(tc_votes=[base.tc_votes[0], (pk, sig, base.tc_votes[1][2]), base.tc_votes[2]])
        both = in_qc.but(tc_votes=in_tc.tc_votes)
        blocks += [in_qc, in_tc, both]
        wants += [(True, (OK, 0)), (False, (TC, 1)), (False, (TC, 1))]
    for blk, want in zip(blocks, wants):
        assert world.verdict(blk) == want
    assert world.on_routes([block_call(b.encode()) for b in blocks], committee) == wants


def test_non_member_voter_fails_its_stage_with_an_explicit_committee(world):
    """The reference rejects a non-member as UnknownAuthority; by member index
    a stranger gets flags 0: the QC stage at its index (the TC stage for a
    block whose QC is genesis)."""
    from hsverify import wire
    from hsverify.committee import Committee
    blk = world.block(3)
    assert world.verdict(blk) == (True, (OK, 0))
    no_author = Committee(world.pk[:3])
    members = Committee([world.pk[0], world.pk[2], world.pk[-1]])  # voter 1 is a stranger
    assert wire.block_verify(blk.encode(), committee=no_author)[:2] == (False, (AUTHOR, 0))
    assert wire.block_verify(blk.encode(), committee=members)[:2] == (False, (QC, 1))
    gen = world.block(3, genesis=True)
    assert wire.block_verify(gen.encode(), committee=members)[:2] == (False, (TC, 1))
    assert wire.block_verify(blk.encode(), committee=world.committee)[:2] == (True, (OK, 0))
    ok, res, flags = wire.proposal_verify(blk.author, blk.sig, blk.round, blk.payload, blk.qc_hash, blk.qc_round,
                                          blk.qc_votes, blk.tc_round, blk.tc_votes, committee=members)
    want = world.flags(blk.items())
    want[[2, 5]] = 0  # voter 1 in the QC and in the TC
    assert (ok, res) == (False, (QC, 1)) and (flags == want).all()


# ---- timeouts and votes ------------------------------------------------------------
def test_timeout_and_vote(world):
    from hsverify import wire
    blk = world.block(3, tc=False)
    author = NKEYS - 1
    t = Tmo(world.pk[author], b"", 12, blk.qc_hash, blk.qc_round, blk.qc_votes)
    t.sig = world.sign([author], [h32(le(t.round) + le(t.qc_round))])[0]
    qv = t.qc_votes
    gen = Tmo(world.pk[author], b"", 12, bytes(32), 0, [(world.pk[0], bytes(64))])
    gen.sig = world.sign([author], [h32(le(12) + le(0))])[0]
    cases = [(t, (OK, 0)),
             (t.but(sig=flip(t.sig, 0)), (AUTHOR, 0)),
             (t.but(round=13), (AUTHOR, 0)),
             (t.but(qc_votes=qv[:2] + [(qv[2][0], flip(qv[2][1], 63))]), (QC, 2)),
             (t.but(qc_round=t.qc_round + 1), (AUTHOR, 0)),  # the author signs high_qc.round too
             (gen, (OK, 0)),
             (gen.but(sig=flip(gen.sig, 9)), (AUTHOR, 0))]
    for obj, want in cases:
        assert world.verdict(obj) == (want == (OK, 0), want)
    got = world.on_routes([(lambda buf: lambda c: wire.timeout_verify(buf, committee=c)[:2])(obj.encode())
                           for obj, _ in cases])
    assert got == [world.verdict(obj) for obj, _ in cases]
    ok, res, n_qc, pks = wire.timeout_verify(t.encode())
    assert (ok, n_qc) == (True, 3) and [bytes(p) for p in pks] == [t.author] + [v[0] for v in qv]

    # Vote: strict over SHA-512(hash || round_le)[..32]
    vh, vr, voter = blk.digest(), blk.round, 5
    vsig = world.sign([voter], [h32(vh + le(vr))])[0]
    votes = [(vh, vr, world.pk[voter], vsig), (vh, vr, world.pk[voter], flip(vsig, 20)),
             (vh, vr + 1, world.pk[voter], vsig), (flip(vh, 31), vr, world.pk[voter], vsig),
             (vh, vr, world.pk[voter + 1], vsig)]
    want = [bool(world.flags([(AUTHOR, 0, pk, sig, h32(h + le(r)))])[0] & o.STRICT_OK) for h, r, pk, sig in votes]
    assert want == [True, False, False, False, False]
    got = world.on_routes([(lambda buf: lambda c: wire.vote_verify(buf, committee=c))(wire.encode_vote(*v))
                           for v in votes])
    assert got == want


# ---- chains ---------------------------------------------------------------------------
def test_chain_of_three_blocks(world):
    from hsverify import wire
    blocks = [world.block(3, round_=20), world.block(3, tc=False, n_payload=0, round_=21),
              world.block(3, genesis=True, round_=22)]
    tv = blocks[0].tc_votes
    bad = [blocks[0].but(tc_votes=tv[:1] + [(tv[1][0], flip(tv[1][1], 7), tv[1][2])] + tv[2:]), blocks[1],
           blocks[2].but(sig=flip(blocks[2].sig, 2))]
    for chain in (blocks, bad):
        want = [world.verdict(b)[1] for b in chain]
        got = world.on_routes([lambda c, bufs=[b.encode() for b in chain]: wire.blocks_verify(bufs, committee=c)])[0]
        assert got == (sum(w == (OK, 0) for w in want), want)
    assert [world.verdict(b)[1] for b in bad] == [(TC, 1), (OK, 0), (AUTHOR, 0)]


def test_chain_of_seventy_blocks_past_the_latency_limit(world):
    """70 blocks of 1 + 67 items and one that does not parse: 4760 items in one
    call -- past the 4096 keys of the cached latency path and past 2^12, so the
    generic path or the committee's comb pass -- with a bad vote in block 0, in
    a middle block and in the last one."""
    from hsverify import wire
    n, nb = 67, 70
    rnd = world.rnd
    hashes = [bytes(rnd.integers(0, 256, 32, dtype=np.uint8)) for _ in range(nb)]
    rounds = list(range(100, 100 + nb))
    voters = np.tile(np.arange(n), nb)
    sigs = world.sign(voters, [h32(hashes[b] + le(rounds[b] - 1)) for b in range(nb) for _ in range(n)])
    chain = []
    for b in range(nb):
        qv = [(world.pk[i], sigs[b * n + i]) for i in range(n)]
        chain.append(Blk(world.pk[n + b], b"", rounds[b], [hashes[b]], hashes[b], rounds[b] - 1, qv))
    asigs = world.sign([n + b for b in range(nb)], [blk.digest() for blk in chain])
    for blk, s in zip(chain, asigs):
        blk.sig = s
    for b, v in ((0, 66), (35, 0), (69, 30)):
        qv = chain[b].qc_votes
        chain[b] = chain[b].but(qc_votes=qv[:v] + [(qv[v][0], flip(qv[v][1], 45))] + qv[v + 1:])
    want = [world.verdict(blk)[1] for blk in chain]
    assert sum(len(blk.items()) for blk in chain) == 4760
    assert [w for w in want if w != (OK, 0)] == [(QC, 66), (QC, 0), (QC, 30)]
    bufs = [blk.encode() for blk in chain]
    bufs.insert(10, bufs[10][:-5])  # an unparsable block leaves its neighbours alone
    want.insert(10, (PARSE, 0))
    got = world.on_routes([lambda c: wire.blocks_verify(bufs, committee=c)])[0]
    assert got == (67, want)


# ---- routes ------------------------------------------------------------------------------
def test_a_whole_block_is_one_verification_call(world):
    """Through the request counters of the resident latency service (test
    library): a block of 1 + 2 + 1 items with every key cached is ONE request
    (one verification call of four items), where verify_strict + the QC call +
    the TC call on the same bytes are three."""
    from hsverify import _testing, wire
    blk = world.block(2)
    blk = blk.but(tc_votes=blk.tc_votes[:1])
    blk.sig = world.sign([NKEYS - 1], [blk.digest()])[0]
    assert world.verdict(blk) == (True, (OK, 0)) and len(blk.items()) == 4
    buf = blk.encode()
    qc = wire.encode_qc(blk.qc_hash, blk.qc_round, blk.qc_votes)
    tc = wire.encode_tc(blk.tc_round, blk.tc_votes)
    with _testing.test_library() as lib:
        def counts():
            p, a = ctypes.c_uint64(), ctypes.c_uint64()
            lib.hsv_test_resident_counts(ctypes.byref(p), ctypes.byref(a))
            return p.value, a.value
        lib.hsv_set_auto_committee(1)
        prev = lib.hsv_set_resident_service(1)
        try:
            for _ in range(2):  # a call of a few signatures teaches the cache its keys
                assert wire.block_verify(buf)[:2] == (True, (OK, 0))
            assert lib.hsv_auto_committee_wait(60000) == 1
            assert lib.hsv_auto_committee_size() >= 3
            p0, a0 = counts()
            assert wire.block_verify(buf)[:2] == (True, (OK, 0))
            p1, a1 = counts()
            assert (p1 - p0, a1 - a0) == (1, 1)
            assert lib.hsv_verify_strict(blk.digest(), blk.author, blk.sig) == 1
            assert wire.qc_verify(qc)[0] and wire.tc_verify(tc)[0]
            p2, a2 = counts()
            assert (p2 - p1, a2 - a1) == (3, 3)
            # the verdict does not depend on the service
            bad = blk.but(tc_votes=[(blk.tc_votes[0][0], flip(blk.tc_votes[0][1], 5), blk.tc_votes[0][2])]).encode()
            assert wire.block_verify(bad)[:2] == (False, (TC, 0))
            lib.hsv_set_resident_service(0)
            assert wire.block_verify(buf)[:2] == (True, (OK, 0)) and wire.block_verify(bad)[:2] == (False, (TC, 0))
            assert counts()[0] == p2 + 1
        finally:
            lib.hsv_set_resident_service(prev)


def test_seven_items_with_the_resident_service_on_and_off(world):
    """A 3-vote block with a TC is 7 items, above the service's 4: the same
    verdict and flags with the service on and off, and the oracle's."""
    from hsverify import wire
    blk = world.block(3)
    bad = blk.but(qc_votes=blk.qc_votes[:2] + [(blk.qc_votes[2][0], flip(blk.qc_votes[2][1], 12))])
    world.warm()
    prev = world.lib.hsv_set_resident_service(1)
    try:
        answers = []
        for mode in (1, 0):
            world.lib.hsv_set_resident_service(mode)
            answers.append([(lambda r: (r[0], r[1], r[2].tobytes()))(wire.proposal_verify(
                b.author, b.sig, b.round, b.payload, b.qc_hash, b.qc_round, b.qc_votes, b.tc_round, b.tc_votes))
                for b in (blk, bad)])
    finally:
        world.lib.hsv_set_resident_service(prev)
    assert answers[0] == answers[1]
    for b, (ok, res, flags) in zip((blk, bad), answers[0]):
        assert len(flags) == 7 and (ok, res) == world.verdict(b) and flags == world.flags(b.items()).tobytes()
    assert answers[0][1][1] == (QC, 2)
