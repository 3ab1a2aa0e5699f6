"""Loop shape of the persistent comb passes of a compact committee
(hsv_ctx_comb4_kernel in csrc/hsv_mempool.hip, hsv_cmsg_comb4_kernel in
csrc/hsv_committee_msgs.hip), as tests/test_kernel_isa.py checks the other
product kernels: each deals batches of 64 hit-list entries from an atomic
counter, and that work loop must compile to a uniform loop (no exec-masked back
edge).  No GPU: hipcc -S only."""
import os

import pytest

from conftest import PKG
from test_kernel_isa import _compile, _kernels, hipcc, work_loops  # noqa: F401  (hipcc: the fixture)

CASES = (("hsv_mempool.hip", "hsv_ctx_comb4_kernel", "hsv_ctx_comb_kernel"),
         ("hsv_committee_msgs.hip", "hsv_cmsg_comb4_kernel", "hsv_cmsg_comb_kernel"))


@pytest.mark.parametrize("src,compact,full", CASES, ids=[c[1] for c in CASES])
def test_compact_comb_pass_is_found_by_name_and_its_work_loop_is_uniform(hipcc, src, compact, full):
    ks = _kernels(_compile(os.path.join(PKG, "csrc", src), "compact_" + src + ".s", []))
    mine = {k: v for k, v in ks.items() if compact in k}
    assert len(mine) == 1, f"{compact}: found {sorted(mine)}"
    loops = work_loops(next(iter(mine.values())))
    assert loops, f"{compact}: work loop not found"
    for h, divergent in loops.items():
        assert not divergent, f"{compact}: work loop {h} compiled as a divergent loop"
    # the full-width pass keeps its own name next to it
    assert any(full in k and work_loops(v) for k, v in ks.items()), f"{full}: work loop not found"
