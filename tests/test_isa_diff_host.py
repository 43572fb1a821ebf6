"""tools/isa_diff.py: the splitter and the comparer on hand-written assembly (no compiler)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "isa_diff", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def _kernel(name, body, ordinal, vgpr=5):
    return f"""\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
{body}.LBB{ordinal}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{ordinal}:
\t.size\t{name}, .Lfunc_end{ordinal}-{name}
                                        ; -- End function
\t.set {name}.num_vgpr, {vgpr}
"""


def _meta(name, vgpr=5):
    return f"""  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 0
    .name:           {name}
    .sgpr_count:     14
    .symbol:         {name}.kd
    .vgpr_count:     {vgpr}
"""


BODY = "\tv_mov_b32_e32 v1, 0\n\tv_mov_b32_e32 v2, s2\n\ts_cbranch_execz .LBB{o}_2\n\tv_add_u32_e32 v4, -1, v0\n"
SWAPPED = "\tv_mov_b32_e32 v2, s2\n\tv_mov_b32_e32 v1, 0\n\ts_cbranch_execz .LBB{o}_2\n\tv_add_u32_e32 v4, -1, v0\n"


def _unit(kernels, cuid="7544f37e3fb652e9"):
    """kernels: [(name, body template, vgpr)] in file order."""
    text = "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.text\n"
    for o, (name, body, vgpr) in enumerate(kernels):
        text += _kernel(name, body.format(o=o), o, vgpr)
    text += f"""\t.type\t__hip_cuid_{cuid},@object ; @__hip_cuid_{cuid}
\t.section\t.bss,"aw",@nobits
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.size\t__hip_cuid_{cuid}, 1
\t.addrsig_sym __hip_cuid_{cuid}
\t.amdgpu_metadata
---
amdhsa.kernels:
"""
    for name, _, vgpr in kernels:
        text += _meta(name, vgpr)
    return text + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n\n\t.end_amdgpu_metadata\n"


A, B = "_Z3k_aPi", "_Z3k_bPi"
BASE = _unit([(A, BODY, 5), (B, BODY, 7)])


def _cmp(new):
    return isa_diff.compare(isa_diff.split_functions(BASE), isa_diff.split_functions(new))


def test_split_finds_functions_and_their_three_parts():
    f = isa_diff.split_functions(BASE)
    assert sorted(f) == [A, B]                                   # the data symbol is no function
    assert "\tv_mov_b32_e32 v1, 0" in f[A]["code"] and "\ts_endpgm" in f[A]["code"]
    assert f[B]["desc"] == [".amdhsa_group_segment_fixed_size 0", ".amdhsa_next_free_vgpr 7", ".amdhsa_next_free_sgpr 8"]
    assert any(".vgpr_count:     7" in ln for ln in f[B]["meta"]) and not any(A in ln for ln in f[B]["meta"])
    assert not any(B in ln for ln in f[A]["code"])               # the next symbol's preamble is not A's


def test_identical():
    res = _cmp(BASE)
    assert res["identical"] == [A, B] and isa_diff.all_identical(res)


def test_only_the_cuid_symbol_differs_counts_as_identical():
    res = _cmp(_unit([(A, BODY, 5), (B, BODY, 7)], cuid="0123456789abcdef"))
    assert res["identical"] == [A, B] and isa_diff.all_identical(res)


def test_two_instructions_swapped_differs():
    res = _cmp(_unit([(A, BODY, 5), (B, SWAPPED, 7)]))
    assert res["identical"] == [A] and not isa_diff.all_identical(res)
    assert [(d[0], d[1]) for d in res["differing"]] == [(B, ["code"])]
    assert res["differing"][0][2] == res["differing"][0][3]      # same length, another order


def test_one_descriptor_value_changed_differs():
    new = BASE.replace(".amdhsa_next_free_vgpr 7", ".amdhsa_next_free_vgpr 8")
    res = _cmp(new)
    assert [(d[0], d[1]) for d in res["differing"]] == [(B, ["desc"])] and not isa_diff.all_identical(res)
    res = _cmp(BASE.replace(".vgpr_count:     7", ".vgpr_count:     8"))
    assert [(d[0], d[1]) for d in res["differing"]] == [(B, ["meta"])]


def test_renamed_kernel_is_present_in_one_tree_only():
    C = "_Z3k_cPi"
    res = _cmp(_unit([(A, BODY, 5), (C, BODY, 7)]))
    assert res["only_old"] == [B] and res["only_new"] == [C] and res["identical"] == [A]
    assert not res["differing"] and not isa_diff.all_identical(res)


def test_moving_a_kernel_in_its_file_is_identical():
    res = _cmp(_unit([(B, BODY, 7), (A, BODY, 5)]))
    assert res["identical"] == [A, B] and isa_diff.all_identical(res)
