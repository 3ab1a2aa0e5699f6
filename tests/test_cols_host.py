"""The point pass's 2-bit columns with digits in {-1 .. 2} and the column
classes its batches are dealt by, on the host against Python integers
(csrc/hsv_verify_hc.hpp: recode_cols, joint_column<kColOffset>, col_class).

tests/native/cols_host.cpp is a stand-alone program over the same headers the
gfx950 kernels are built from (test infrastructure; the product library never
runs them on the CPU).  It is built plain and with
-fsanitize=address,undefined.
"""
import os
import random
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "cols_host")
NCOL = 70
NEED_MIN, NEED_MAX = 62, 67


def _build(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "cols_host.cpp")
    tmp = f"{out}.{os.getpid()}.tmp"  # parallel test workers build side by side
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags,
                    "-I", os.path.join(PKG, "csrc"), src, "-o", tmp], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def cols_host():
    return _build(BIN)


@pytest.fixture(scope="module")
def cols_host_san():
    return _build(BIN + "_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _run(binary, args, lines):
    return subprocess.run([binary] + args, input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)


def cols(c):
    """Columns the scalar needs: the smallest m with 3c < 2 * 4^m + 1."""
    m = 0
    while 3 * c >= 2 * 4 ** m + 1:
        m += 1
    return m


def _scalars():
    rnd = random.Random(0xc015)
    s = [0, 1, 2, 3, 1 << 126, (1 << 128) - 1, (1 << 138) - 1]
    for m in range(62, 70):
        t = -(-(2 * 4 ** m + 1) // 3)  # the first scalar that needs m + 1 columns
        s += [t - 1, t, t + 1]
    s += [rnd.getrandbits(138) for _ in range(10000)]
    assert all(0 <= x < 1 << 138 for x in s)
    return s


SCALARS = _scalars()


def test_thresholds_are_where_the_column_count_steps():
    """The test's own cols(): it steps at the thresholds the issue names."""
    for m in range(62, 70):
        t = -(-(2 * 4 ** m + 1) // 3)
        assert cols(t - 1) == m and cols(t) == m + 1
    assert cols(0) == 0 and cols(1) == 1 and cols(2) == 1 and cols(3) == 2 and cols((1 << 138) - 1) == 70


def _check_recoding(out):
    assert len(out) == len(SCALARS)
    for s, line in zip(SCALARS, out):
        d = [int(x) for x in line.split()]
        assert len(d) == NCOL and all(-1 <= x <= 2 for x in d), (hex(s), d)
        assert sum(x << (2 * (NCOL - 1 - t)) for t, x in enumerate(d)) == s, hex(s)
        lead = next((t for t, x in enumerate(d) if x), NCOL)
        assert lead == NCOL - cols(s), (hex(s), lead, cols(s))


def test_recoding_digits_sum_and_leading_zeros(cols_host):
    """The 70 digits lie in {-1 .. 2}, sum back to the scalar, and exactly
    70 - cols(c) leading ones are zero: the edge scalars, the thresholds
    ceil((2 * 4^m + 1) / 3) and their neighbours for m = 62 .. 69, and 10^4
    seeded random scalars below 2^138."""
    _check_recoding(_run(cols_host, ["--recode"], [f"{s:040x}" for s in SCALARS]).stdout.strip().split("\n"))


def _check_indexmap(out):
    rows = [tuple(int(x) for x in l.split()) for l in out]
    assert len(rows) == 32 and len({r[:3] for r in rows}) == 32
    lines = set()
    for ci, cj, flip, line, neg in rows:
        i, j = ci - 1, (cj - 1) * (-1 if flip else 1)
        assert i >= -1  # the table has no line for i = -2 with j > 0 folded to i = 2, j < -2
        assert neg in (0, 1) and 0 <= line <= 12, (ci, cj, flip, line, neg)
        assert (-line if neg else line) == 5 * i + j, (ci, cj, flip, line, neg)
        if i == -1:
            assert neg == 1 and 3 <= line <= 7
        lines.add(line)
    assert 0 in lines and lines <= set(range(13))


def test_line_mapping(cols_host):
    """All 16 chunk pairs under both signs of c0: a line <= 12 and a fold whose
    signed value is 5i + j; i = -1 folds onto the lines 3 .. 7."""
    _check_indexmap(_run(cols_host, ["--indexmap"], []).stdout.strip().split("\n"))


def _class_pairs():
    rnd = random.Random(0xc1a5)
    pairs = [(v, rnd.choice(SCALARS)) for v in SCALARS] + [(rnd.choice(SCALARS), v) for v in SCALARS[:31]]
    return pairs + [(v, v) for v in SCALARS[:31]]


def _check_classes(pairs, out):
    assert len(out) == len(pairs)
    for (c0, c1), line in zip(pairs, out):
        need = min(max(cols(c0), cols(c1), NEED_MIN), NEED_MAX)
        assert int(line) == NEED_MAX - need, (hex(c0), hex(c1), line)


def test_class_function(cols_host):
    """col_class(c0, c1) is max(cols(c0), cols(c1)) clamped to 62 .. 67,
    numbered from the longest, on pairs of the same values."""
    pairs = _class_pairs()
    _check_classes(pairs, _run(cols_host, ["--class"], [f"{a:040x} {b:040x}" for a, b in pairs]).stdout.split())


def test_sanitizer_build(cols_host_san):
    """The address and undefined-behaviour sanitizer build of the stand-alone
    program over the same inputs: nothing reported, the same answers."""
    r = _run(cols_host_san, ["--recode"], [f"{s:040x}" for s in SCALARS])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    _check_recoding(r.stdout.strip().split("\n"))
    r = _run(cols_host_san, ["--indexmap"], [])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    _check_indexmap(r.stdout.strip().split("\n"))
    pairs = _class_pairs()
    r = _run(cols_host_san, ["--class"], [f"{a:040x} {b:040x}" for a, b in pairs])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    _check_classes(pairs, r.stdout.split())
