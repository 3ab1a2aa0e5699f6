"""The one-lane field, scalar and lattice primitives against big integers, on
the host build (tests/native/prims_host.cpp: csrc/hsv_test_prims.hpp with g++
and -DHSV_CHECK_BOUNDS).

The vectors (tests/prim_vectors.py) sit where the headers' bounds are tight:
raw limbs at the maxima of the operand classes csrc/hsv_fe26x10.hpp documents
(R, S2, D, g up to fe26_gmax), products scaled to within 1 % of the 64-bit
column limit, loose forms of -1, 0 and 1, structured 512-bit values for the
Barrett reduction, and the structured challenges of the lattice reduction.
tests/test_prims_gpu.py runs the same vectors through the device build of the
same text; the lattice answers of this build reach it as
tests/golden/lattice_prims.bin, which this module keeps current.
"""
import importlib.util
import os
import random
from collections import Counter

import numpy as np
import pytest

import prim_vectors as pv


@pytest.fixture(scope="module")
def prims_host():
    return pv.build_prims_host()


@pytest.fixture(scope="module")
def field_run(prims_host):
    cases, stats = pv.field_cases()
    return cases, stats, pv.run_prims_host(prims_host, "field", pv.field_records(cases))


# what the admissibility filter of prim_vectors keeps and drops: (kept, dropped)
# pairs per (class of f, class of g).  The counts follow from the vectors and
# the rule of fe26_check_columns alone; a D4 operand exceeds fe26_gmax, so it is
# dropped as g and, in fe_mul2(f, g, g, f), as f.
MUL_COUNTS = {("R", "R"): (145, 0), ("S2", "R"): (145, 0), ("D3", "R"): (145, 0), ("D4", "R"): (145, 0),
              ("D3", "S2"): (145, 0), ("D4", "S2"): (145, 0), ("D3", "G"): (139, 0), ("D3", "GMAX"): (139, 0),
              ("D4", "G"): (139, 0), ("D4", "GMAX"): (139, 0), ("G", "G"): (133, 0), ("G", "GMAX"): (133, 0),
              ("GMAX", "G"): (133, 0), ("GMAX", "GMAX"): (133, 0),
              ("R", "D4"): (3, 142), ("S2", "D4"): (3, 142), ("G", "D4"): (3, 136)}
MUL2_COUNTS = {**MUL_COUNTS, ("D4", "R"): (3, 142), ("D4", "S2"): (3, 142), ("D4", "G"): (3, 136),
               ("D4", "GMAX"): (3, 136)}
SQ_COUNTS = {"R": (36, 0), "S2": (36, 0), "D3": (36, 0), "D4": (1, 35), "G": (33, 0), "GMAX": (33, 0)}
NEAR_LIMIT_PAIRS = 29


def check_filter_counts(stats):
    """Shared with the GPU test: the filter can neither empty a class pair
    silently nor let the rule's violations through."""
    assert stats["mul"] == MUL_COUNTS
    assert stats["mul2"] == MUL2_COUNTS
    assert stats["sq"] == SQ_COUNTS
    assert stats["near_limit"] == NEAR_LIMIT_PAIRS
    # every legal class pair keeps the pair built from the class maxima
    assert stats["max_kept"] == set(pv.LEGAL)
    fmax, gmax = pv.class_max("D4"), pv.GMAX
    assert pv.mul_admissible(fmax, gmax) and not pv.mul_admissible(gmax, fmax)
    for (fn, f), (gn, g) in pv.NEAR_LIMIT:
        assert 0.99 * (2**64 - 2**40) <= max(pv.columns(f, g)) < 2**64 - 2**40, (fn, gn)


def test_filter_counts():
    check_filter_counts(pv.field_cases()[1])


def test_field_ops_at_class_maxima(field_run):
    """Every field op of csrc/hsv_test_prims.hpp on raw limbs: the value mod p
    is the integers', fe_canon gives the unique representative, products and
    carries land in class R, flags are the predicate on the integers,
    fe_invert(0) == 0.  The bound-checked build aborts on any operand the
    headers' own rules refuse, so a clean exit also says model and header agree
    on what is admissible."""
    cases, _, out = field_run
    assert Counter(c.op for c in cases)[pv.INVERT] >= 150
    zero_inverts = [i for i, c in enumerate(cases) if c.op == pv.INVERT and pv.value(c.f) % pv.P == 0]
    assert len(zero_inverts) >= 3  # 0, p, 2p as limbs
    for i in zero_inverts:
        assert pv.value(out[i, 1:11]) % pv.P == 0
    errs = pv.check_field(cases, out)
    assert not errs, f"{len(errs)} wrong, first: " + "\n".join(errs[:5])


def test_scalar_ops_on_structured_values(prims_host):
    """sc_reduce512, sc_is_canonical, sc_muladd and sc_mul_small against
    Python's %, on q l + d, 2^e, 2^512 - 2^e, single-limb patterns and the
    scalars around l -- values no SHA-512 caller produces."""
    cases = pv.scalar_cases()
    out = pv.run_prims_host(prims_host, "scalar", pv.scalar_records(cases))
    errs = pv.check_scalar(cases, out)
    assert not errs, f"{len(errs)} wrong, first: " + "\n".join(errs[:5])


def test_barrett_subtraction_counts():
    """How many conditional subtractions of l each sc_reduce512 vector needs
    (the integer model of the routine, q3 from mu): both 0 and 1 occur.

    None needs two, and none can: with q1 = x >> 224,
        x / l - q1 mu / 2^288 = (x mod 2^224) / l + q1 2^224 (2^512 mod l) / (l 2^512)
                              < 2^-28 + (2^512 mod l) / l = 0.2249...,
    so q3 = floor(q1 mu / 2^288) is floor(x / l) or one less.  The directed
    search below (the largest quotients, where the second term peaks, with small
    and large remainders) finds none either.  The routine keeps its second
    pass, the general bound of the method (HAC 14.42: q3 >= q - 2); with it,
    skipping the first pass changes no answer, so no vector can tell."""
    vs, structured = pv.reduce512_values()
    counts = Counter(pv.barrett_subtractions(x) for x in vs)
    assert counts == {0: 3101, 1: 616}
    assert Counter(pv.barrett_subtractions(x) for x in vs[:structured]) == {0: 1341, 1: 376}
    assert (2**512 % pv.L) * 2**28 + pv.L < pv.L * 2**28  # the bound above is below 1
    rnd = random.Random(2604)
    qmax = (2**512 - 1) // pv.L
    for t in range(4000):
        q = qmax - t if t < 2000 else qmax - rnd.randrange(2**200)
        for d in (0, 1, rnd.randrange(pv.L), pv.L - 1):
            x = q * pv.L + d
            if x < 2**512:
                assert pv.barrett_subtractions(x) <= 1, x


def _lattice_generator():
    path = os.path.join(pv.ROOT, "tests", "golden", "make_lattice_prims.py")
    spec = importlib.util.spec_from_file_location("make_lattice_prims", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# challenges of prim_vectors.lattice_ks() without a pair below the bound: all of them structured (N // d and
# the like have a tiny shortest vector with an even cofactor), none of the 2,000 random ones
LATTICE_NOT_OK = {133: 161, 138: 160}


def test_lattice_fixture_is_current_and_sound(prims_host):
    """tests/golden/lattice_prims.bin is what the host build answers now, and
    every recorded answer with ok == 1 satisfies c0 == c1 k (mod 8l), c1 odd,
    0 < c1 < 2^bits, |c0| < 2^bits."""
    fresh = _lattice_generator().generate(prims_host)
    with open(pv.LATTICE_FIXTURE, "rb") as f:
        committed = f.read()
    assert len(committed) < 300 * 1024
    assert committed == fresh, "regenerate with python tests/golden/make_lattice_prims.py"
    ks = pv.lattice_ks()
    rows = pv.lattice_fixture_rows(pv.LATTICE_FIXTURE, len(ks))
    for bits in pv.LATTICE_BOUNDS:
        errs = [e for e in (pv.check_lattice_answer(k, bits, [pv.DONE] + list(rows[bits][i]))
                            for i, k in enumerate(ks)) if e]
        assert not errs, errs[:5]
        assert int((rows[bits][:, 0] == 0).sum()) == LATTICE_NOT_OK[bits]
    assert np.array_equal(rows[133][rows[133][:, 0] == 1], rows[138][rows[133][:, 0] == 1])
