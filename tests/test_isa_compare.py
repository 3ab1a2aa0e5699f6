"""tools/isa_compare.py on hand-written assembly snippets (CPU, no compiler)."""
import importlib.util
import os

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


def _kernel(name, body, n, vgprs=12, sgprs=18, scratch=0, lds=0, occ=8):
    return f"""\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
{body}.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
                                        ; -- End function
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
; NumSgprs: {sgprs}
; NumVgprs: {vgprs}
; NumAgprs: 0
; ScratchSize: {scratch}
; Occupancy: {occ}
; LDSByteSize: {lds} bytes/workgroup (compile time only)
"""


LOOP = """; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0                     ; a comment
{l1}:                                ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, 1, v1
\tv_cmp_gt_u32_e32 vcc, 16, v1

\ts_cbranch_vccnz {l1}
; %bb.2:
\tglobal_store_dword v0, v1, s[0:1]
\ts_endpgm
"""

# a role-specialised kernel: one role leaves early, the other at the end
TWO_ENDS = """; %bb.0:
\tv_cmp_eq_u32_e32 vcc, 0, v0
\ts_cbranch_vccz .LBB1_2
; %bb.1:
\tv_mov_b32_e32 v1, 1
\tglobal_store_dword v0, v1, s[0:1]
\ts_endpgm
.LBB1_2:
\tv_mov_b32_e32 v1, 2
\tv_mov_b32_e32 v2, 3
{extra}\tglobal_store_dwordx2 v0, v[1:2], s[0:1]
\ts_endpgm
"""


def _one(old, new, name="k"):
    rows = [r for r in ic.compare(old, new) if r[0] == name]
    assert len(rows) == 1, rows
    return rows[0][1:]


def test_renumbered_label_is_identical():
    old = _kernel("k", LOOP.format(l1=".LBB0_1"), 0)
    new = _kernel("k", LOOP.format(l1=".LBB7_3"), 7)
    assert _one(old, new) == ("identical", 7, 7, 0)


def test_body_runs_to_func_end_not_to_the_first_endpgm():
    old = _kernel("k", TWO_ENDS.format(extra=""), 1)
    body, _ = ic.kernels(old)["k"]
    assert len(ic.instructions(ic.normalise(body))) == 9
    assert sum(l.strip() == "s_endpgm" for l in body) == 2
    # a difference after the first s_endpgm is seen
    new = _kernel("k", TWO_ENDS.format(extra="\tv_mov_b32_e32 v3, 4\n"), 1)
    assert _one(old, new) == ("changed", 9, 10, 1)


def test_register_renamed_lines_are_equivalent():
    old = _kernel("k", TWO_ENDS.format(extra=""), 1)
    new = _kernel("k", TWO_ENDS.format(extra="").replace("v_mov_b32_e32 v1, 2\n\tv_mov_b32_e32 v2, 3",
                                                         "v_mov_b32_e32 v2, 3\n\tv_mov_b32_e32 v1, 2"), 1)
    cls, n_old, n_new, diff = _one(old, new)
    assert (cls, n_old, n_new) == ("equivalent", 9, 9) and diff >= 1
    # the same mnemonics in the same order with v1 and v2 exchanged in the operands of the last
    # two moves: register names are compared as written (two lines differ), yet the pair is equivalent
    renamed = _kernel("k", TWO_ENDS.format(extra="").replace("v_mov_b32_e32 v1, 2\n\tv_mov_b32_e32 v2, 3",
                                                             "v_mov_b32_e32 v2, 2\n\tv_mov_b32_e32 v1, 3"), 1)
    assert _one(old, renamed) == ("equivalent", 9, 9, 2)
    assert _one(old, old)[0] == "identical"  # and only equal register names make a pair identical


def test_scalar_opcode_may_differ_but_resources_may_not():
    old = _kernel("k", LOOP.format(l1=".LBB0_1"), 0)
    flipped = LOOP.format(l1=".LBB0_1").replace("s_cbranch_vccnz", "s_cbranch_vccz")
    assert _one(old, _kernel("k", flipped, 0))[0] == "equivalent"
    assert _one(old, _kernel("k", flipped, 0, vgprs=13))[0] == "changed"
    assert _one(old, _kernel("k", LOOP.format(l1=".LBB0_1"), 0, occ=7))[0] == "changed"
    # the SGPR comment under its other spelling, and a kernel whose comments are missing
    total = lambda text: text.replace("; NumSgprs", "; TotalNumSgprs")
    assert _one(total(old), total(_kernel("k", flipped, 0)))[0] == "equivalent"
    assert _one(total(old), total(_kernel("k", flipped, 0, sgprs=19)))[0] == "changed"
    bare = lambda text: text.replace("; Occupancy", "; Other")
    assert _one(bare(old), bare(_kernel("k", flipped, 0)))[0] == "changed"


def test_one_extra_vector_instruction_is_changed():
    old = _kernel("k", LOOP.format(l1=".LBB0_1"), 0)
    new = _kernel("k", LOOP.format(l1=".LBB0_1").replace("\tglobal_store", "\tv_mov_b32_e32 v2, 0\n\tglobal_store"), 0)
    assert _one(old, new) == ("changed", 7, 8, 1)
    # the same count with another vector mnemonic is changed too
    swapped = _kernel("k", LOOP.format(l1=".LBB0_1").replace("v_add_u32_e32 v1, 1, v1", "v_sub_u32_e32 v1, 1, v1"), 0)
    assert _one(old, swapped)[0] == "changed"


def test_every_kernel_of_either_file_is_listed():
    a = _kernel("ka", LOOP.format(l1=".LBB0_1"), 0) + _kernel("kb", TWO_ENDS.format(extra=""), 1)
    b = _kernel("ka", LOOP.format(l1=".LBB0_1"), 0)
    rows = {r[0]: r[1] for r in ic.compare(a, b)}
    assert rows == {"ka": "identical", "kb": "changed"}
    assert ic.main(["isa_compare", os.devnull, os.devnull]) == 0
