"""ISA-level checks of the message instantiations of the four small-batch
kernels (hsv_small.hip; no GPU: hipcc -S only).

Each small form -- quad, joint, row, pair -- is compiled twice: for a 32-byte
digest (the form hsv_verify_device takes) and for whole messages (MSG = true,
hsv_verify_msgs*).  The two differ in the prepass role alone, which runs on a
wave of its own; the point roles are one code.  A message instantiation that
needed more registers than its digest twin, or any more scratch, would have
spilled in the point loop, which is where the time goes: so each is compared
with its twin, both numbers read from the same assembly.
"""
import os
import re

import pytest

from conftest import PKG, ROOT
from test_kernel_isa import HIPCC, OUT, _compile

FORMS = ("hsv_verify_quad_kernel", "hsv_verify_joint_kernel", "hsv_verify_row_kernel",
         "hsv_verify_pair_fused_kernel")


@pytest.fixture(scope="module")
def asm():
    """hsv_small.hip's gfx950 assembly.  tests/test_kernel_isa.py compiles the
    same file with the same flags; when its output is newer than every source
    it is read instead of spending the compile (minutes) a second time."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    done = os.path.join(OUT, "hsv_small.hip.s")
    srcs = [os.path.join(d, f) for d in (os.path.join(PKG, "csrc"), os.path.join(ROOT, "include"))
            for f in os.listdir(d)]
    if os.path.exists(done) and os.path.getmtime(done) > max(os.path.getmtime(s) for s in srcs):
        return open(done).read().split("\n")
    return _compile(os.path.join(PKG, "csrc", "hsv_small.hip"), "hsv_small.hip.s")


def resources(lines):
    """kernel symbol -> {vgprs, scratch bytes, LDS bytes} from the resource
    comments the compiler prints after each kernel ("; NumVgprs: 128",
    "; ScratchSize: 0", "; LDSByteSize: ..."), keyed by the .amdhsa_kernel
    directive before them."""
    res, cur = {}, None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)"),
                         ("lds", r";\s*LDSByteSize:\s*(\d+)")):
            m = re.match(pat, l)
            if m and key not in cur:
                cur[key] = int(m.group(1))
    return res


def twins(res, form):
    """(digest, message) resource records of one small form: the template's
    last argument is MSG, mangled Lb0 / Lb1 before the argument list's E."""
    names = [k for k in res if form in k]
    digest = [k for k in names if re.search(r"Lb0EE", k)]
    message = [k for k in names if re.search(r"Lb1EE", k)]
    assert len(digest) == 1 and len(message) == 1, (form, names)
    return res[digest[0]], res[message[0]]


@pytest.mark.parametrize("form", FORMS)
def test_message_instantiation_exists_and_is_no_heavier_than_its_digest_twin(asm, form):
    res = resources(asm)
    d, m = twins(res, form)
    for r in (d, m):
        assert set(r) == {"vgprs", "scratch", "lds"}, r
    print(f"{form}: digest {d}, message {m}")
    assert m["scratch"] <= d["scratch"], (form, d, m)
    assert m["vgprs"] <= d["vgprs"], (form, d, m)
    # the prepass wave's staging: 64 lanes x 9 chunks of 16 bytes
    assert m["lds"] - d["lds"] == 64 * 9 * 16, (form, d, m)
