"""ISA-level checks of the span-table addressing of the transaction kernels and
of the batch parse kernels (no GPU: hipcc -S only).

The addressing mode is a template parameter of the kernels of
csrc/hsv_mempool.hip, so every kernel that file had before compiles
`identical` (tools/isa_compare.py: equal normalised bodies and equal resource
comments) to the commit before span mode was added -- the offset
instantiations of the record, mask and route kernels under their new symbols,
and the comb, generic and fused kernels, which it does not touch (a body is
hashed with the kernel's own symbol written as KERNEL and without its section
directive, the two places where a new template parameter shows).  That
commit's normalised bodies are kept as hashes in
tests/golden/batch_wire_parent_isa.json, made by
`python tests/test_batch_wire_isa.py OLD_hsv_mempool.hip.s` from assembly
compiled with tests/test_kernel_isa.py's flags.  The span instantiations and
the kernels of csrc/hsv_batchwire.hip exist, the walking kernels without
scratch.  The test reads structure and resource comments only; it looks for no
particular instruction.
"""
import hashlib
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "batch_wire_parent_isa.json")
# label: (fragment of the parent's mangled symbol, fragment of this tree's)
UNMOVED = {
    "hsv_tx_record_kernel<false>": ("hsv_tx_record_kernelILb0EEE", "hsv_tx_record_kernelILb0ELb0EEE"),
    "hsv_tx_record_kernel<true>": ("hsv_tx_record_kernelILb1EEE", "hsv_tx_record_kernelILb1ELb0EEE"),
    "hsv_tx_mask_kernel": ("hsv_tx_mask_kernelE", "hsv_tx_mask_kernelILb0EEE"),
    "hsv_ctx_route_kernel": ("hsv_ctx_route_kernelE", "hsv_ctx_route_kernelILb0EEE"),
    "hsv_ctx_comb_kernel": ("hsv_ctx_comb_kernelE",) * 2,
    "hsv_ctx_comb4_kernel": ("hsv_ctx_comb4_kernelE",) * 2,
    "hsv_ctx_generic_kernel": ("hsv_ctx_generic_kernelI",) * 2,
    "hsv_verify_tx_fused_kernel": ("hsv_verify_tx_fused_kernelI",) * 2,
}
SPANS = {"hsv_tx_record_kernel<false, spans>": "hsv_tx_record_kernelILb0ELb1EEE",
         "hsv_tx_mask_kernel<spans>": "hsv_tx_mask_kernelILb1EEE",
         "hsv_ctx_route_kernel<spans>": "hsv_ctx_route_kernelILb1EEE"}
SCAN = ("hsv_batch_count_kernel", "hsv_batch_index_kernel", "hsv_batch_spans_kernel", "hsv_batch_reduce_kernel")

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


def digests(text, fragments):
    """{label: {"body": sha256 of the normalised body, "instructions", "resources"}}
    for {label: fragment of the kernel's symbol}; a fragment names one kernel"""
    out = {}
    for sym, (body, rsrc) in ic.kernels(text).items():
        for label, frag in fragments.items():
            if frag in sym:
                assert label not in out, (label, sym)
                # a kernel that became a template changes its symbol and moves from .text to a comdat section of
                # its own: the body is compared with the symbol written as KERNEL and without its section line
                norm = [ln.replace(sym, "KERNEL") for ln in ic.normalise(body)
                        if ln != ".text" and not ln.startswith(".section")]
                out[label] = {"body": hashlib.sha256("\n".join(norm).encode()).hexdigest(),
                              "instructions": len(ic.instructions(norm)), "resources": rsrc}
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
    for f in ("hsv_mempool.hip", "hsv_batchwire.hip"):
        done = os.path.join(OUT, f + ".s")
        if os.path.exists(done) and os.path.getmtime(done) > max(os.path.getmtime(s) for s in srcs):
            res[f] = open(done).read()
        else:
            res[f] = "\n".join(_compile(os.path.join(PKG, "csrc", f), f + ".s"))
    return res


def test_earlier_kernels_are_identical_to_the_parents(asm):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = digests(asm["hsv_mempool.hip"], {label: new for label, (_, new) in UNMOVED.items()})
    assert set(got) == set(UNMOVED) == set(want), (sorted(got), sorted(want))
    for label in UNMOVED:
        print(label, got[label]["instructions"], got[label]["resources"])
        assert got[label]["resources"] == want[label]["resources"], (label, got[label], want[label])
        assert got[label]["instructions"] == want[label]["instructions"], (label, got[label], want[label])
        assert got[label]["body"] == want[label]["body"], f"{label}: the normalised body differs from the parent's"
    # the file holds those kernels and the three span instantiations, nothing else
    assert len(ic.kernels(asm["hsv_mempool.hip"])) == len(UNMOVED) + len(SPANS)


def test_span_instantiations_exist(asm):
    got = digests(asm["hsv_mempool.hip"], SPANS)
    assert set(got) == set(SPANS), sorted(got)
    base = digests(asm["hsv_mempool.hip"], {label: new for label, (_, new) in UNMOVED.items()})
    for label, d in got.items():
        print(label, d["instructions"], d["resources"])
        assert set(d["resources"]) == set(ic.RESOURCES.values()), (label, d)
    # no more scratch, registers or LDS than the offset twin (the route kernel's prepass spills 112 bytes in both)
    for label, twin in (("hsv_tx_record_kernel<false, spans>", "hsv_tx_record_kernel<false>"),
                        ("hsv_tx_mask_kernel<spans>", "hsv_tx_mask_kernel"),
                        ("hsv_ctx_route_kernel<spans>", "hsv_ctx_route_kernel")):
        for r in ("scratch", "VGPRs", "LDS"):
            assert got[label]["resources"][r] <= base[twin]["resources"][r], (label, r)
    # the same staging as their offset twins: 4 waves x 64 lanes x 9 chunks of 16 bytes
    assert got["hsv_tx_record_kernel<false, spans>"]["resources"]["LDS"] == \
        base["hsv_tx_record_kernel<false>"]["resources"]["LDS"] == 4 * 64 * 9 * 16
    assert got["hsv_ctx_route_kernel<spans>"]["resources"]["LDS"] == base["hsv_ctx_route_kernel"]["resources"]["LDS"]


def test_scan_and_reduce_kernels_exist_without_scratch(asm):
    got = digests(asm["hsv_batchwire.hip"], {n: n for n in SCAN})
    assert set(got) == set(SCAN), sorted(got)
    for name, d in got.items():
        print(name, d["instructions"], d["resources"])
        assert d["resources"]["scratch"] == 0, (name, d)
    # 16 windows of 1024 bytes and the slack words per walking wave; the reduce kernel holds nothing
    for name in ("hsv_batch_count_kernel", "hsv_batch_spans_kernel"):
        assert got[name]["resources"]["LDS"] == 16 * 1024 + 16, got[name]
    assert got["hsv_batch_reduce_kernel"]["resources"]["LDS"] == 0
    assert not any(n in s for s in ic.kernels(asm["hsv_mempool.hip"]) for n in SCAN)


if __name__ == "__main__":   # the fixture, from the parent's assembly file
    json.dump(digests(open(sys.argv[1]).read(), {label: old for label, (old, _) in UNMOVED.items()}), sys.stdout,
              indent=1, sort_keys=True)
    print()
