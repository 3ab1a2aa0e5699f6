"""ISA-level checks of the signer census kernels (no GPU: hipcc -S only, with
tests/test_kernel_isa.py's flags): csrc/hsv_census.hip holds the count and the
gather kernel in their three input modes, none with scratch or LDS, and
csrc/hsv_mempool.hip still holds exactly the kernels it held -- the census
lives in a file of its own.  The test reads structure and resource comments
only; it looks for no particular instruction."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("ILi0EEE", "ILi1EEE", "ILi2EEE")  # a key array, offset-addressed and fixed-size transactions
# the kernels of csrc/hsv_mempool.hip (tests/test_batch_wire_isa.py pins their bodies)
MEMPOOL = ("hsv_tx_record_kernelILb0ELb0EEE", "hsv_tx_record_kernelILb1ELb0EEE", "hsv_tx_record_kernelILb0ELb1EEE",
           "hsv_tx_mask_kernelILb0EEE", "hsv_tx_mask_kernelILb1EEE", "hsv_ctx_route_kernelILb0EEE",
           "hsv_ctx_route_kernelILb1EEE", "hsv_ctx_comb_kernelE", "hsv_ctx_comb4_kernelE", "hsv_ctx_generic_kernelI",
           "hsv_verify_tx_fused_kernelI")

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


@pytest.fixture(scope="module")
def asm():
    """{file: gfx950 assembly text}"""
    from conftest import PKG
    from test_kernel_isa import HIPCC, _compile
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {f: "\n".join(_compile(os.path.join(PKG, "csrc", f), "census_" + f + ".s"))
            for f in ("hsv_census.hip", "hsv_mempool.hip")}


def test_census_kernels_exist_without_scratch(asm):
    ks = ic.kernels(asm["hsv_census.hip"])
    assert len(ks) == 6, sorted(ks)
    for name in ("hsv_census_count_kernel", "hsv_census_gather_kernel"):
        for mode in MODES:
            got = [(sym, rsrc) for sym, (_, rsrc) in ks.items() if name + mode in sym]
            assert len(got) == 1, (name, mode, sorted(ks))
            sym, rsrc = got[0]
            print(sym, len(ic.instructions(ic.normalise(ks[sym][0]))), rsrc)
            assert set(rsrc) == set(ic.RESOURCES.values()), (sym, rsrc)
            assert rsrc["scratch"] == 0 and rsrc["LDS"] == 0, (sym, rsrc)
            assert rsrc["occupancy"] == 8, (sym, rsrc)  # one lane per item: nothing holds registers for long


def test_mempool_file_holds_the_kernels_it_held(asm):
    ks = ic.kernels(asm["hsv_mempool.hip"])
    for frag in MEMPOOL:
        assert sum(frag in sym for sym in ks) == 1, (frag, sorted(ks))
    assert len(ks) == len(MEMPOOL), sorted(ks)
    assert not any("census" in sym for sym in ks)
