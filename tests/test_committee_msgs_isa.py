"""Loop shape of the persistent passes of hsv_committee_verify_msgs*
(csrc/hsv_committee_msgs.hip), as tests/test_kernel_isa.py checks the other
product kernels: each pass deals batches from an atomic counter, and that work
loop must compile to a uniform loop (no exec-masked back edge).  No GPU:
hipcc -S only."""
import os

from conftest import PKG
from test_kernel_isa import _compile, _kernels, hipcc, work_loops  # noqa: F401  (hipcc: the fixture)


def test_committee_msgs_work_loops_are_uniform(hipcc):
    ks = _kernels(_compile(os.path.join(PKG, "csrc", "hsv_committee_msgs.hip"), "hsv_committee_msgs.hip.s", []))
    for name, body in ks.items():
        for h, divergent in work_loops(body).items():
            assert not divergent, f"{name}: work loop {h} compiled as a divergent loop"
    for kernel in ("hsv_cmsg_comb_kernel", "hsv_cmsg_generic_kernel"):
        assert any(kernel in k and work_loops(v) for k, v in ks.items()), f"{kernel}: work loop not found"
