"""ISA-level checks of the seal kernels (no GPU: hipcc -S only, with
tests/test_kernel_isa.py's flags): csrc/hsv_seal.hip holds the expected kernels,
none with scratch.  The test reads structure and resource comments only; it
looks for no particular instruction."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("ILi0EEE", "ILi1EEE")  # offset-addressed and fixed-size transactions
BY_MODE = ("hsv_seal_reduce_kernel", "hsv_seal_apply_kernel", "hsv_seal_copy_kernel", "hsv_seal_pieces_kernel")
SINGLE = ("hsv_seal_blocks_kernelE", "hsv_seal_cut_kernelE", "hsv_seal_digest_kernelE")

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


@pytest.fixture(scope="module")
def kernels():
    from conftest import PKG
    from test_kernel_isa import HIPCC, _compile
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return ic.kernels("\n".join(_compile(os.path.join(PKG, "csrc", "hsv_seal.hip"), "seal_hsv_seal.hip.s")))


def test_seal_kernels_exist_without_scratch(kernels):
    want = [name + mode for name in BY_MODE for mode in MODES] + list(SINGLE)
    assert len(kernels) == len(want), sorted(kernels)
    for frag in want:
        got = [(sym, rsrc) for sym, (_, rsrc) in kernels.items() if frag in sym]
        assert len(got) == 1, (frag, sorted(kernels))
        sym, rsrc = got[0]
        print(sym, len(ic.instructions(ic.normalise(kernels[sym][0]))), rsrc)
        assert set(rsrc) == set(ic.RESOURCES.values()), (sym, rsrc)
        assert rsrc["scratch"] == 0, (sym, rsrc)
        if "digest" not in sym and "reduce" not in sym and "apply" not in sym and "blocks" not in sym:
            assert rsrc["LDS"] == 0, (sym, rsrc)  # only the scans and the digest window use LDS
