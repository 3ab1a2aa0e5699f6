"""Blocks, votes and timeouts as bincode bytes: layout, parser errors, no device.

The encoders of hsverify/wire.py restate bincode 1.3's default encoding of the
reference's serde derives (consensus/src/messages.rs:16-24, 112-118, 222-228);
as for the QC (tests/test_wire.py) no Rust toolchain exists here, so the
layout is pinned against bytes assembled by hand from the documented rules,
not against a reference fixture.  The parser's error paths need no GPU: they
return HSV_ERR_PARSE before any device is looked for.  Without a GPU every new
verify entry answers HSV_ERR_NO_DEVICE on well-formed input.  The GPU tests are
in tests/test_proposal_gpu.py.
"""
import base64
import ctypes
import hashlib
import struct

import numpy as np
import pytest

PARSE, NO_DEVICE = -6, -1


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def _b(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def _key(pk):
    s = base64.b64encode(pk)
    assert len(s) == 44
    return [struct.pack("<Q", 44), s]


class Parts:
    """An object's encoding field by field, so that every field boundary is known."""

    def __init__(self):
        self.fields = []

    def add(self, *chunks):
        self.fields += [bytes(c) for c in chunks]
        return self

    def qc(self, h, round_, votes):
        self.add(h, struct.pack("<Q", round_), struct.pack("<Q", len(votes)))
        for pk, sig in votes:
            self.add(*_key(pk), sig[:32], sig[32:])
        return self

    def tc(self, round_, votes):
        self.add(struct.pack("<Q", round_), struct.pack("<Q", len(votes)))
        for pk, sig, hqc in votes:
            self.add(*_key(pk), sig[:32], sig[32:], struct.pack("<Q", hqc))
        return self

    def bytes(self):
        return b"".join(self.fields)

    def boundaries(self):
        """Every offset at which a field ends, the last (the whole object) excluded."""
        ends = np.cumsum([len(f) for f in self.fields]).tolist()
        return sorted(set(ends[:-1]) | {0})


QC_HASH, QC_ROUND = _b(1, 32), 6
QC_VOTES = [(_b(10 + i, 32), _b(20 + i, 64)) for i in range(2)]
TC_ROUND = 7
TC_VOTES = [(_b(30 + i, 32), _b(40 + i, 64), 5 + i) for i in range(2)]
AUTHOR, SIG, ROUND = _b(2, 32), _b(3, 64), 8
PAYLOAD = [_b(50, 32), _b(51, 32), _b(52, 32)]


def block_parts(tc=True, payload=PAYLOAD, qc_votes=QC_VOTES):
    p = Parts().qc(QC_HASH, QC_ROUND, qc_votes)
    p.add(b"\x01" if tc else b"\x00")
    if tc:
        p.tc(TC_ROUND, TC_VOTES)
    p.add(*_key(AUTHOR), struct.pack("<Q", ROUND), struct.pack("<Q", len(payload)), *payload)
    return p.add(SIG[:32], SIG[32:])


def timeout_parts():
    return Parts().qc(QC_HASH, QC_ROUND, QC_VOTES).add(struct.pack("<Q", ROUND), *_key(AUTHOR), SIG[:32], SIG[32:])


def vote_parts():
    return Parts().add(QC_HASH, struct.pack("<Q", ROUND), *_key(AUTHOR), SIG[:32], SIG[32:])


# ---- layout -----------------------------------------------------------------
def test_block_encoding_layout():
    from hsverify import wire
    qc = wire.encode_qc(QC_HASH, QC_ROUND, QC_VOTES)
    tc = wire.encode_tc(TC_ROUND, TC_VOTES)
    buf = wire.encode_block(qc, tc, AUTHOR, ROUND, PAYLOAD, SIG)
    assert buf == block_parts().bytes()
    nq, nt = len(qc), len(tc)
    assert nq == 48 + 2 * 116 and nt == 16 + 2 * 124
    assert len(buf) == nq + 1 + nt + 52 + 8 + 8 + 3 * 32 + 64
    assert buf[:nq] == qc and buf[nq] == 1 and buf[nq + 1:nq + 1 + nt] == tc
    at = nq + 1 + nt
    assert struct.unpack("<Q", buf[at:at + 8]) == (44,) and base64.b64decode(buf[at + 8:at + 52]) == AUTHOR
    assert struct.unpack("<QQ", buf[at + 52:at + 68]) == (ROUND, 3)
    assert buf[at + 68:at + 164] == b"".join(PAYLOAD) and buf[at + 164:] == SIG
    # Option::None is the one tag byte 0; an empty payload is its count alone
    none = wire.encode_block(qc, None, AUTHOR, ROUND, [], SIG)
    assert none == block_parts(tc=False, payload=[]).bytes()
    assert len(none) == nq + 1 + 52 + 16 + 64 and none[nq] == 0


def test_vote_and_timeout_encoding_layout():
    from hsverify import wire
    v = wire.encode_vote(QC_HASH, ROUND, AUTHOR, SIG)
    assert v == vote_parts().bytes() and len(v) == 32 + 8 + 52 + 64
    assert v[:32] == QC_HASH and struct.unpack("<Q", v[32:40]) == (ROUND,) and v[-64:] == SIG
    qc = wire.encode_qc(QC_HASH, QC_ROUND, QC_VOTES)
    t = wire.encode_timeout(qc, ROUND, AUTHOR, SIG)
    assert t == timeout_parts().bytes() and len(t) == len(qc) + 8 + 52 + 64
    assert t[:len(qc)] == qc and struct.unpack("<Q", t[len(qc):len(qc) + 8]) == (ROUND,)
    assert base64.b64decode(t[len(qc) + 16:len(qc) + 60]) == AUTHOR and t[-64:] == SIG


def test_digests_match_hashlib():
    """What the author of a block, a vote and a timeout signs (messages.rs:80-89,
    149-156, 268-275), spelt out against hashlib."""
    from hsverify import wire
    le = lambda x: struct.pack("<Q", x)
    assert wire.block_digest(AUTHOR, ROUND, PAYLOAD, QC_HASH) == \
        hashlib.sha512(AUTHOR + le(ROUND) + PAYLOAD[0] + PAYLOAD[1] + PAYLOAD[2] + QC_HASH).digest()[:32]
    assert wire.block_digest(AUTHOR, ROUND, [], QC_HASH) == hashlib.sha512(AUTHOR + le(ROUND) + QC_HASH).digest()[:32]
    assert wire.vote_digest(QC_HASH, ROUND) == hashlib.sha512(QC_HASH + le(ROUND)).digest()[:32]
    assert wire.timeout_digest(ROUND, QC_ROUND) == hashlib.sha512(le(ROUND) + le(QC_ROUND)).digest()[:32]


# ---- malformed input --------------------------------------------------------
def _calls(lib):
    """name -> rc of the entry point on buf (c == NULL)."""
    res = (ctypes.c_uint32 * 2)()
    return {
        "block": lambda buf: lib.hsv_block_verify_bincode(None, buf, len(buf), res, None, None, None),
        "timeout": lambda buf: lib.hsv_timeout_verify_bincode(None, buf, len(buf), res, None, None),
        "vote": lambda buf: lib.hsv_vote_verify_bincode(None, buf, len(buf)),
    }


def _rc(lib, kind, buf):
    from hsverify import _lib
    rc = _calls(lib)[kind](bytes(buf))
    if rc == PARSE:
        assert "bincode" in _lib.last_error()
    return rc


@pytest.mark.parametrize("kind,parts", [("block", block_parts()), ("block", block_parts(tc=False, payload=[])),
                                        ("timeout", timeout_parts()), ("vote", vote_parts())],
                         ids=["block", "block_no_tc", "timeout", "vote"])
def test_truncation_at_every_field_boundary_is_a_parse_error(lib, kind, parts):
    buf = parts.bytes()
    cuts = parts.boundaries()
    assert len(cuts) >= 6  # a vote: nothing, hash, round, key length, key, R
    for cut in cuts:
        assert _rc(lib, kind, buf[:cut]) == PARSE, cut
    # and one byte short of the whole object; trailing bytes
    assert _rc(lib, kind, buf[:-1]) == PARSE
    assert _rc(lib, kind, buf + b"\x00") == PARSE


def test_option_tag_other_than_0_or_1_is_a_parse_error(lib):
    buf = bytearray(block_parts().bytes())
    at = 48 + 2 * 116
    assert buf[at] == 1
    for tag in (2, 0xff):
        buf[at] = tag
        assert _rc(lib, "block", buf) == PARSE
    # tag 0 in front of a TC's bytes: the TC is read as the author's key and the rest
    buf[at] = 0
    assert _rc(lib, "block", buf) == PARSE


@pytest.mark.parametrize("kind,at", [("block", 40), ("block", 48 + 2 * 116 + 1 + 8),
                                     ("block", 48 + 2 * 116 + 1 + 16 + 2 * 124 + 52 + 8), ("timeout", 40)],
                         ids=["qc_votes", "tc_votes", "payload", "timeout_qc_votes"])
def test_count_larger_than_the_bytes_left_is_a_parse_error(lib, kind, at):
    parts = block_parts() if kind == "block" else timeout_parts()
    for count in (1 << 60, (1 << 64) - 1, 1000):
        buf = bytearray(parts.bytes())
        assert struct.unpack("<Q", buf[at:at + 8])[0] in (2, 3)
        buf[at:at + 8] = struct.pack("<Q", count)
        assert _rc(lib, kind, buf) == PARSE


def _key_offsets():
    """First base64 character of: QC vote 0, QC vote 1, TC vote 0, TC vote 1, the author (of block_parts())."""
    qc0 = 48 + 8
    tc0 = 48 + 2 * 116 + 1 + 16 + 8
    return {"qc_vote_0": qc0, "qc_vote_1": qc0 + 116, "tc_vote_0": tc0, "tc_vote_1": tc0 + 124,
            "author": 48 + 2 * 116 + 1 + 16 + 2 * 124 + 8}


@pytest.mark.parametrize("where", ["qc_vote_0", "qc_vote_1", "tc_vote_0", "tc_vote_1", "author"])
@pytest.mark.parametrize("how", ["bad_char", "padding_inside", "trailing_bits", "short_key"])
def test_bad_base64_key_is_a_parse_error(lib, where, how):
    good = block_parts().bytes()
    at = _key_offsets()[where]
    assert struct.unpack("<Q", good[at - 8:at]) == (44,) and good[at + 43] == ord("=")
    buf = bytearray(good)
    if how == "bad_char":
        buf[at + 5] = ord("*")
    elif how == "padding_inside":
        buf[at + 10] = ord("=")
    elif how == "trailing_bits":  # the last symbol carries non-zero unused bits
        alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
        buf[at + 42] = alphabet[alphabet.index(buf[at + 42]) ^ 1]
    elif how == "short_key":  # 40 characters decode to 30 bytes: the reference's slice fails
        enc = base64.b64encode(_b(99, 30))
        buf[at - 8:at + 44] = struct.pack("<Q", len(enc)) + enc
    assert _rc(lib, "block", buf) == PARSE
    assert _rc(lib, "block", good) != PARSE


@pytest.mark.parametrize("kind", ["timeout", "vote"])
def test_bad_author_key_of_timeout_and_vote_is_a_parse_error(lib, kind):
    parts = timeout_parts() if kind == "timeout" else vote_parts()
    buf = bytearray(parts.bytes())
    at = len(buf) - 64 - 44
    buf[at + 7] = ord("-")
    assert _rc(lib, kind, buf) == PARSE


def test_chain_marks_unparsable_blocks_before_any_device(lib):
    """hsv_blocks_verify_bincode with nothing that parses never needs a device:
    every block gets HSV_STAGE_PARSE, the count is 0; bad offsets are an
    argument error."""
    from hsverify import wire
    n, results = wire.blocks_verify([b"", b"\x00" * 7, block_parts().bytes()[:-1]])
    assert n == 0 and results == [(wire.STAGE_PARSE, 0)] * 3
    assert wire.blocks_verify([]) == (0, [])
    offsets = np.array([4, 2, 9], np.uint64)
    assert lib.hsv_blocks_verify_bincode(None, b"123456789", ctypes.c_void_p(offsets.ctypes.data), 2, None) == -3


# ---- no device ---------------------------------------------------------------
def test_no_device_fails_loudly(lib):
    """Without a GPU every new verify entry returns HSV_ERR_NO_DEVICE on
    well-formed input: never a rejection, never a fallback."""
    from hsverify import _lib, wire
    if lib.hsv_device_count() > 0:
        pytest.skip("a GPU is visible")
    for kind, parts in (("block", block_parts()), ("block", block_parts(tc=False, payload=[])),
                        ("timeout", timeout_parts()), ("vote", vote_parts())):
        assert _rc(lib, kind, parts.bytes()) == NO_DEVICE
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        wire.proposal_verify(AUTHOR, SIG, ROUND, PAYLOAD, QC_HASH, QC_ROUND, QC_VOTES, TC_ROUND, TC_VOTES)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        wire.blocks_verify([block_parts().bytes(), b"junk", block_parts(tc=False).bytes()])
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        wire.block_verify(block_parts().bytes())
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        wire.timeout_verify(timeout_parts().bytes())
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_NO_DEVICE"):
        wire.vote_verify(vote_parts().bytes())
    # a null proposal is an argument error, before the device as well
    assert lib.hsv_proposal_verify(None, None, None, None) == -3
