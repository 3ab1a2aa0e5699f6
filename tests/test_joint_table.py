"""The joint point pass on the host: 2-bit columns, the 12-line table of
iP + jQ and the Straus loop over it (csrc/hsv_verify_hc.hpp: prep_from_hash
with DW = 2, joint_column, jt_build, straus_joint, the JOINT verify_one_prepped).

tests/native/joint_host.cpp is a stand-alone program over the same headers the
gfx950 kernels are built from (test infrastructure; the product library never
verifies on the CPU).  It is built three ways: plain, with -DHSV_CHECK_BOUNDS
(every field operation asserts its operand classes, so the new sums and
differences prove theirs) and with -fsanitize=address,undefined.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import ed25519_ref as o
from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "joint_host")
NCOL = 70


def _build(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "joint_host.cpp")
    tmp = f"{out}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags,
                    "-I", os.path.join(PKG, "csrc"), src, "-o", tmp], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def joint_host():
    return _build(BIN)


@pytest.fixture(scope="module")
def joint_host_checked():
    return _build(BIN + "_checked", "-DHSV_CHECK_BOUNDS")


@pytest.fixture(scope="module")
def joint_host_san():
    return _build(BIN + "_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _run(binary, args, lines, env=None):
    return subprocess.run([binary] + args, input="\n".join(lines) + "\n", capture_output=True, text=True, check=True,
                          env=dict(os.environ, **(env or {})))


def _triples(rec):
    return [f"{bytes(p).hex()} {bytes(s).hex()} {bytes(m).hex()}" for p, s, m in zip(rec["pk"], rec["sig"], rec["msg"])]


# ---- recoding ---------------------------------------------------------------

def test_two_bit_recoding_sums_to_the_scalar(joint_host):
    """Sum d_t 4^t over the 70 columns equals the scalar, every digit in
    [-2, 1]: the edge scalars and 10^4 seeded random ones below 2^138."""
    top = (1 << 138) - 1
    rnd = random.Random(0x2b17)
    scalars = [0, 1, 2, 3, top, 1 << 137, (1 << 137) - 1, int("a" * 40, 16) & top, int("5" * 40, 16) & top,
               (1 << 136) - 1, (1 << 138) - 2]
    scalars += [rnd.getrandbits(138) for _ in range(10000)]
    out = _run(joint_host, ["--recode"], [f"{s:040x}" for s in scalars]).stdout.strip().split("\n")
    assert len(out) == len(scalars)
    for s, line in zip(scalars, out):
        d = [int(x) for x in line.split()]
        assert len(d) == NCOL and all(-2 <= x <= 1 for x in d), (hex(s), d)
        assert sum(x << (2 * (NCOL - 1 - t)) for t, x in enumerate(d)) == s, hex(s)


# ---- index map --------------------------------------------------------------

def test_index_map_covers_the_twelve_lines(joint_host):
    """All 16 digit pairs under both signs of c0: (0, 0) reads the identity,
    every other pair one of the 12 lines with the fold that makes the line's
    (i, j) the pair or its opposite; no two non-opposite pairs share a line."""
    rows = [tuple(int(x) for x in l.split()) for l in _run(joint_host, ["--indexmap"], []).stdout.strip().split("\n")]
    assert len(rows) == 32
    owner = {}
    for ci, cj, flip, line, neg in rows:
        i, j = ci - 2, (cj - 2) * (-1 if flip else 1)
        assert neg in (0, 1) and 0 <= line <= 12
        if (i, j) == (0, 0):
            assert line == 0
            continue
        assert line >= 1
        fi, fj = (-i, -j) if neg else (i, j)
        assert fi > 0 or (fi == 0 and fj > 0), (i, j, neg)
        assert owner.setdefault(line, (fi, fj)) == (fi, fj), f"line {line} serves {(fi, fj)} and {owner[line]}"
    assert sorted(owner) == list(range(1, 13))
    # the table build's own numbering: 1, 2 = Q, 2Q; 5i + j the lines with P
    assert all(line == 5 * fi + fj for line, (fi, fj) in owner.items())
    assert {l for l, (fi, _) in owner.items() if fi == 0} == {1, 2}  # the lines without R: never flipped


# ---- table build ------------------------------------------------------------

def _enc(e):
    return o.compress(o.to_affine(e))


def _neg_enc(b):
    return _enc(o.ext_neg(o.to_ext(o.decompress(b))))


def _table_cases():
    rnd = random.Random(0x71ab)
    rp = lambda: o.scalar_mult(rnd.getrandbits(252) | 1, o.BASEPOINT)
    cases = [(_enc(rp()), _enc(rp())) for _ in range(12)]
    a = _enc(rp())
    cases += [(a, a), (a, _neg_enc(a))]
    tors = o.torsion_points()
    for t in tors:  # P or Q of small order (the identity among them), and both
        cases += [(_enc(t), _enc(rp())), (_enc(rp()), _enc(t)), (_enc(t), _enc(tors[3]))]
    for t in tors[1:]:  # mixed order: a torsion component on either point
        m = _enc(o.ext_add(rp(), t))
        cases += [(m, _enc(rp())), (_enc(rp()), m), (m, m), (m, _neg_enc(m))]
    return cases


@pytest.mark.parametrize("build", ["plain", "checked"])
def test_table_lines_are_iP_plus_jQ(joint_host, joint_host_checked, build):
    """Each of the 12 lines equals iP + jQ by plain repeated ge_add_cached, as
    affine points (the program's check), and equals the oracle's iP + jQ."""
    cases = _table_cases()
    out = _run(joint_host if build == "plain" else joint_host_checked, ["--table"],
               [f"{p.hex()} {q.hex()}" for p, q in cases]).stdout.strip().split("\n")
    assert len(out) == 12 * len(cases), out[:3]
    for n, (pb, qb) in enumerate(cases):
        pe, qe = o.to_ext(o.decompress(pb)), o.to_ext(o.decompress(qb))
        seen = set()
        for row in out[12 * n:12 * n + 12]:
            l, i, j, ok, xh, yh = row.split()
            l, i, j = int(l), int(i), int(j)
            seen.add(l)
            assert ok == "1", (n, row)
            want = o.ext_add(o.scalar_mult(i, pe), o.scalar_mult(abs(j), qe if j > 0 else o.ext_neg(qe)))
            assert (int(xh, 16), int(yh, 16)) == o.to_affine(want), (n, l, i, j)
        assert seen == set(range(1, 13))


# ---- whole function ---------------------------------------------------------

@pytest.mark.parametrize("build", ["plain", "checked"])
def test_joint_point_pass_matches_golden(joint_host, joint_host_checked, golden, build):
    """The two-pass form with 2-bit records and the joint table, flag for flag
    against the golden records."""
    r = _run(joint_host if build == "plain" else joint_host_checked, [], _triples(golden))
    got = np.array([int(x, 16) for x in r.stdout.split()], np.uint8)
    bad = np.nonzero(got != golden["flags"])[0]
    assert bad.size == 0, [(int(i), golden["cases"][i], hex(got[i]), hex(golden["flags"][i])) for i in bad[:8]]


@pytest.mark.parametrize("build", ["plain", "checked"])
@pytest.mark.parametrize("bits", [133, 138])
def test_joint_point_pass_matches_fallback_fixtures(joint_host, joint_host_checked, fallback_records, build, bits):
    """The fallback fixtures: at 133 bits their challenges take the full-length
    path (its 8-line table in the joint slot), at 138 the joint point pass with
    scalars right below the bound; the oracle's flags either way."""
    fb = fallback_records
    r = _run(joint_host if build == "plain" else joint_host_checked, [], _triples(fb), {"HSV_LAT_BITS": str(bits)})
    got = np.array([int(x, 16) for x in r.stdout.split()], np.uint8)
    assert (got == fb["flags"]).all()
    if bits == 133:
        assert r.stderr.count("fallback") >= 48
    else:
        assert r.stderr.count("fallback") == 0


@pytest.mark.parametrize("mode", [1, 3])
def test_injected_joint_table_corruption_is_a_fault(joint_host, golden, mode):
    """Zeroed lines, or a bit flipped in the lines that involve R: every record
    whose points decode reports the fault; the others keep their flags."""
    idx = list(range(golden["n_edge"])) + list(range(golden["n_edge"], len(golden["flags"]), 5))
    sub = {k: [golden[k][i] for i in idx] for k in ("pk", "sig", "msg")}
    got = _run(joint_host, ["--inject", str(mode)], _triples(sub)).stdout.split()
    for i, g in zip(idx, got):
        f = int(golden["flags"][i])
        if (f & o.A_OK) and (f & o.R_OK):
            assert g == "fault", golden["cases"][i]
        else:
            assert int(g, 16) == f, golden["cases"][i]


def test_sanitizer_build_runs_the_golden_set(joint_host_san, golden, fallback_records):
    """The address and undefined-behaviour sanitizer build of the stand-alone
    program over the golden set (and the fixtures at 133 bits, for the
    full-length path): clean exit, nothing reported, the same flags."""
    r = _run(joint_host_san, [], _triples(golden))
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert (np.array([int(x, 16) for x in r.stdout.split()], np.uint8) == golden["flags"]).all()
    fb = fallback_records
    r = _run(joint_host_san, [], _triples(fb), {"HSV_LAT_BITS": "133"})
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert (np.array([int(x, 16) for x in r.stdout.split()], np.uint8) == fb["flags"]).all()
    r = _run(joint_host_san, ["--table"], [f"{p.hex()} {q.hex()}" for p, q in _table_cases()[:20]])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
