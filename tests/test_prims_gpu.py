"""The device's one-lane field, scalar and lattice primitives against big
integers and against the host build of the same text.

What the device runs is not what tests/test_kernel_host.py compiles: in
csrc/hsv_fe26x10.hpp the products are chains of v_mad_u64_u32 in inline
assembly (early-clobber outputs, a VCC clobber), 2x is v_add_u32 and fe_select
is v_cndmask_b32_e64 on a ballot; in csrc/hsv_lattice.hpp lat_floor_div takes
the hardware reciprocal and the loops run until no lane of the wave is active.
The hooks hsv_test_field_ops / hsv_test_scalar_ops (libhsv_test.so only,
csrc/hsv_test_prims.hip) run csrc/hsv_test_prims.hpp one item per lane, one
launch per family, over the vectors of tests/prim_vectors.py -- the same ones
tests/test_prims_host.py puts through the host build: raw limbs at the class
maxima, columns within 1 % of 2^64, structured 512-bit values, the structured
lattice challenges.  The lattice answers must equal the host build's
(tests/golden/lattice_prims.bin) word for word wherever the challenge sits in
its wave.
"""
import numpy as np
import pytest

import prim_vectors as pv
from test_prims_host import LATTICE_NOT_OK, check_filter_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def field_run():
    from hsverify import _testing
    cases, stats = pv.field_cases()
    with _testing.test_library():
        out = _testing.field_ops(pv.field_records(cases))
    return cases, stats, out


@pytest.fixture(scope="module")
def scalar_run():
    """One launch: the lattice layouts (whole waves), then the mod-l cases; the
    last wave is partial, so the clamped lanes run too."""
    from hsverify import _testing
    ks = pv.lattice_ks()
    k_idx, bits_of, layout = pv.lattice_layouts(len(ks), [ks.index(k) for k in pv.EARLY_FINISHERS])
    cases = pv.scalar_cases()
    rec = np.concatenate([pv.lattice_layout_records(ks, k_idx, bits_of), pv.scalar_records(cases)])
    assert len(rec) % 64 != 0
    with _testing.test_library():
        out = _testing.scalar_ops(rec)
    return {"ks": ks, "k_idx": k_idx, "bits": bits_of, "layout": layout, "lattice": out[:len(k_idx)],
            "cases": cases, "scalar": out[len(k_idx):]}


def test_field_ops_match_integers(field_run):
    """fe_mul, fe_mul2, fe_mul_p, fe_mul2_p, fe_sq, fe_sq2 (fe26_chain in asm),
    fe_add / fe_sub / fe_neg, fe_carry, fe_canon, fe_pack, fe_pack_loose /
    fe_unpack_loose, the verdicts fe_is_zero / fe_eq / fe_canon_low_bit,
    fe_select with the lanes of a wave disagreeing, fe_invert, fe_pow22523,
    fe_pow22523_2 and fe_sqn: value mod p, class R outputs, exact limbs where
    the op defines them, exact flags; an unknown op writes its status only."""
    cases, stats, out = field_run
    check_filter_counts(stats)
    assert len(cases) % 64 != 0  # the last wave has clamped lanes
    errs = pv.check_field(cases, out)
    by_op = sorted({pv.FIELD_OP_NAMES.get(cases[int(e.split()[1])].op, "?") for e in errs})
    assert not errs, f"{len(errs)} wrong in {by_op}, first: " + "\n".join(errs[:5])


def test_scalar_ops_match_integers(scalar_run):
    """sc_reduce512, sc_is_canonical, sc_muladd, sc_mul_small on the device
    against Python's %."""
    errs = pv.check_scalar(scalar_run["cases"], scalar_run["scalar"])
    assert not errs, f"{len(errs)} wrong, first: " + "\n".join(errs[:5])


def _describe(run, i):
    k = run["ks"][int(run["k_idx"][i])]
    return (f"k={k:#x} bound {int(run['bits'][i])} item {i} lane {i % 64} ({pv.LAYOUTS[int(run['layout'][i])]}): "
            f"{[int(x) for x in run['lattice'][i, 1:13]]}")


def test_lattice_answer_does_not_depend_on_the_wave(scalar_run):
    """Each challenge in three placements -- a wave of copies, among 63 others
    in shuffled order, among the earliest finishers (k = 0, 1, 2, 8, 2^31 + 5)
    and other k -- gets one answer.  A step that is not a no-op for a lane whose
    own loop has ended would show here (on the host hsv_any is the identity)."""
    run = scalar_run
    got = run["lattice"]
    assert (got[:, 0] == pv.DONE).all()
    bad = []
    key = run["bits"] * len(run["ks"]) + run["k_idx"]
    order = np.argsort(key, kind="stable")
    srt = key[order]
    starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
    ref = np.repeat(order[starts], np.diff(np.r_[starts, len(order)]))  # first item of each (bound, k)
    differ = np.flatnonzero((got[order] != got[ref]).any(axis=1))
    for j in differ[:5]:
        bad.append(_describe(run, int(order[j])) + "  BUT  " + _describe(run, int(ref[j])))
    assert not bad, f"{len(differ)} items differ from the same k elsewhere: " + "\n".join(bad)
    assert set(np.unique(run["layout"]).tolist()) == {0, 1, 2} and len(starts) == 2 * len(run["ks"])


def test_lattice_matches_host_build(scalar_run):
    """Word for word the host build's ok, c0_neg, c0, c1 (hardware reciprocal
    against IEEE division, wave loops against per-item loops), and for every
    k < l with ok == 1: c0 == c1 k (mod 8l), c1 odd, 0 < c1 < 2^bits,
    |c0| < 2^bits."""
    run = scalar_run
    ks, got = run["ks"], run["lattice"]
    rows = pv.lattice_fixture_rows(pv.LATTICE_FIXTURE, len(ks))
    for bi, bits in enumerate(pv.LATTICE_BOUNDS):
        sel = np.flatnonzero(run["bits"] == bits)
        want = rows[bits][run["k_idx"][sel]]
        differ = sel[(got[sel, 1:13] != want).any(axis=1)]
        msgs = [_describe(run, int(i)) + f"  host: {[int(x) for x in rows[bits][int(run['k_idx'][i])]]}"
                for i in differ[:5]]
        assert differ.size == 0, f"{differ.size} device answers differ from the host build's: " + "\n".join(msgs)
        # one answer per k (the shuffled layout holds every k once before its padding)
        one = sel[run["layout"][sel] == 1][:len(ks)]
        assert sorted(run["k_idx"][one].tolist()) == list(range(len(ks)))
        errs = [e for e in (pv.check_lattice_answer(ks[int(run["k_idx"][i])], bits, got[i]) for i in one) if e]
        assert not errs, errs[:5]
        assert int((got[one, 1] == 0).sum()) == LATTICE_NOT_OK[bits]
