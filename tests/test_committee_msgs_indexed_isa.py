"""ISA-level checks of the kernels of hsv_committee_verify_msgs_indexed* (no
GPU: hipcc -S only).

The two new kernels exist by name, and the kernels beside them did not move:
the comb and route passes of hsv_committee_verify_msgs* (hsv_committee_msgs.hip,
where the new kernels live) and the digest latency kernels (hsv_committee.hip,
whose geometry constants and lane helpers moved to hsv_quad.hpp) compile
`identical` (tools/isa_compare.py: equal normalised bodies and equal resource
comments) to the commit before this path was added.  That commit's normalised
bodies are kept as hashes in tests/golden/cmsg_indexed_parent_isa.json, made by
`python tests/test_committee_msgs_indexed_isa.py OLD_committee.s OLD_committee_msgs.s`
from assembly compiled with this file's flags.  The test reads structure and
resource comments only; it looks for no particular instruction.
"""
import hashlib
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cmsg_indexed_parent_isa.json")
NEW = ("hsv_cmsg_quad_kernel", "hsv_cmsg_index_kernel")
UNMOVED = {"hsv_committee_msgs.hip": ("hsv_cmsg_comb_kernel", "hsv_cmsg_comb4_kernel", "hsv_cmsg_route_kernel"),
           "hsv_committee.hip": ("hsv_comb_verify_quad_fused_kernel", "hsv_comb_resident_kernel")}

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


def digests(text, names):
    """{kernel name: {"body": sha256 of the normalised body, "resources": {...}}}
    for the kernels of `text` whose symbol holds one of `names`"""
    out = {}
    for sym, (body, rsrc) in ic.kernels(text).items():
        for n in names:
            if n in sym:
                assert n not in out, (n, sym)
                norm = "\n".join(ic.normalise(body))
                out[n] = {"body": hashlib.sha256(norm.encode()).hexdigest(), "instructions":
                          len(ic.instructions(ic.normalise(body))), "resources": rsrc}
    return out


@pytest.fixture(scope="module")
def asm():
    """{file: gfx950 assembly text}; an output of tests/test_kernel_isa.py's
    flags that is newer than every source is read instead of compiled again"""
    from conftest import PKG
    from test_kernel_isa import HIPCC, OUT, _compile
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    srcs = [os.path.join(d, f) for d in (os.path.join(PKG, "csrc"), os.path.join(ROOT, "include"))
            for f in os.listdir(d)]
    res = {}
    for f in UNMOVED:
        done = os.path.join(OUT, f + ".s")
        if os.path.exists(done) and os.path.getmtime(done) > max(os.path.getmtime(s) for s in srcs):
            res[f] = open(done).read()
        else:
            res[f] = "\n".join(_compile(os.path.join(PKG, "csrc", f), f + ".s"))
    return res


def test_new_kernels_exist_with_their_resources(asm):
    got = digests(asm["hsv_committee_msgs.hip"], NEW)
    assert set(got) == set(NEW), sorted(got)
    for name, d in got.items():
        r = d["resources"]
        print(name, d["instructions"], r)
        assert set(r) == set(ic.RESOURCES.values()), (name, r)
    quad, index = got["hsv_cmsg_quad_kernel"]["resources"], got["hsv_cmsg_index_kernel"]["resources"]
    # the hash wave's staging: 64 lanes x 9 chunks of 16 bytes, one wave in the
    # quad block, four in the index block (which holds nothing else)
    assert index["LDS"] == 4 * 64 * 9 * 16 and quad["LDS"] >= 64 * 9 * 16
    assert index["scratch"] == 0
    assert not any(n in s for s in ic.kernels(asm["hsv_committee.hip"]) for n in NEW)


@pytest.mark.parametrize("src", sorted(UNMOVED))
def test_neighbouring_kernels_are_identical_to_the_parents(asm, src):
    with open(FIXTURE) as f:
        want = json.load(f)[src]
    got = digests(asm[src], UNMOVED[src])
    assert set(got) == set(UNMOVED[src]) == set(want), (sorted(got), sorted(want))
    for name in UNMOVED[src]:
        assert got[name]["resources"] == want[name]["resources"], (name, got[name], want[name])
        assert got[name]["instructions"] == want[name]["instructions"], (name, got[name], want[name])
        assert got[name]["body"] == want[name]["body"], f"{name}: the normalised body differs from the parent's"


if __name__ == "__main__":   # the fixture, from the parent's two assembly files
    old = {"hsv_committee.hip": sys.argv[1], "hsv_committee_msgs.hip": sys.argv[2]}
    json.dump({src: digests(open(path).read(), UNMOVED[src]) for src, path in old.items()}, sys.stdout, indent=1,
              sort_keys=True)
    print()
