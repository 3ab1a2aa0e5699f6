"""ISA-level checks of the sample-index and client-burst kernels (no GPU: hipcc
-S only, with tests/test_kernel_isa.py's flags): csrc/hsv_samples.hip holds the
expected kernels, none with scratch.  The test reads structure and resource
comments only; it looks for no particular instruction."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("hsv_samples_reduce_kernelE", "hsv_samples_blocks_kernelE", "hsv_samples_apply_kernelE",
           "hsv_samples_batches_kernelE", "hsv_client_bursts_kernelE")
SCANS = ("reduce", "blocks", "apply")  # the workgroup scans keep four partial sums in LDS

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


@pytest.fixture(scope="module")
def kernels():
    from conftest import PKG
    from test_kernel_isa import HIPCC, _compile
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return ic.kernels("\n".join(_compile(os.path.join(PKG, "csrc", "hsv_samples.hip"), "samples_hsv_samples.hip.s")))


def test_sample_kernels_exist_without_scratch(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for frag in KERNELS:
        got = [(sym, rsrc) for sym, (_, rsrc) in kernels.items() if frag in sym]
        assert len(got) == 1, (frag, sorted(kernels))
        sym, rsrc = got[0]
        print(sym, len(ic.instructions(ic.normalise(kernels[sym][0]))), rsrc)
        assert set(rsrc) == set(ic.RESOURCES.values()), (sym, rsrc)
        assert rsrc["scratch"] == 0, (sym, rsrc)
        if any(s in sym for s in SCANS):
            assert 0 < rsrc["LDS"] <= 64, (sym, rsrc)
        else:
            assert rsrc["LDS"] == 0, (sym, rsrc)
