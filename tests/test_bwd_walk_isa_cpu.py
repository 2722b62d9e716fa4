"""CPU guard on the two window walks of the composite backward (composite_core.h: compn_bwd_wave), read from the gfx950 assembly
hipcc emits without a GPU -- beside tests/test_isa_cpu.py, which holds the fused backward to no spills and its register budget.

The walks are the kernel's inner loops: at cfg3 the fused backward is bound by VALU issue and half of every wave's cycles go
through them.  One accumulator set for both walks and one reach bound per walk took the loop body of the flagship instantiation
from 41 VALU instructions to 38 and the kernel from 120 VGPRs to 112; this test keeps both, for the fused kernel of the frame and
for the stand-alone composite backward that shares the routine, at the figures of the commit before that change:

  fragment_bwd_kernel<0, 3, 2, u32, true, true, false>   120 VGPRs, 9552 bytes of LDS, no scratch, walk loops 41 and 41 VALU
  compositen_kernel<2, 2, true, u32, 0, 0>                79 VGPRs, LDS sized at launch (0 static), no scratch, walk loops 42 and 41

A walk loop is an innermost loop (one basic block that branches back to its own label) with the eight exp2 of two columns'
Gaussian and erfc pairs in it and packed FMAs; each kernel has exactly two, the walk behind the own columns first."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# unit, mangled fragment, VGPRs, static LDS bytes, VALU instructions of the walk behind / in front: the parent's figures
CASES = (("fragment_bwd", "fragment_bwd_kernelILi0ELi3ELi2EjLb1ELb1ELb0E", 120, 9552, (41, 41)),
         ("composite", "compositen_kernelILi2ELi2ELb1EjLi0ELi0E", 79, 0, (42, 41)))


def _asm(unit, tmp_path):
    out = os.path.join(str(tmp_path), unit + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only", "-o", out,
                           os.path.join(CSRC, unit + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(text, mangled_fragment):
    """(body, descriptor) of the one kernel whose mangled name contains the fragment."""
    m = re.search(r"^(_ZN4voge\w*" + re.escape(mangled_fragment) + r"\w*):\s", text, flags=re.M)
    assert m, mangled_fragment
    name = m.group(1)
    body = text[m.start():text.index(".Lfunc_end", m.start())]
    d = text.index(".amdhsa_kernel " + name)
    desc = text[d:text.index(".end_amdhsa_kernel", d)]
    return body, desc


def _field(desc, key):
    return int(re.search(r"\." + key + r"\s+(\d+)", desc).group(1))


def _self_loops(body):
    """Instruction lists of the innermost loops: a label, no other label, a conditional branch back to that label."""
    loops, label, ins = [], None, []
    for raw in body.splitlines():
        line = raw.strip()
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            label, ins = m.group(1), []
            continue
        if not line or line.startswith((";", ".")):
            continue
        ins.append(line)
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", line)
        if m and m.group(1) == label:
            loops.append(list(ins))      # (the block the loop falls through to carries no label: a copy, not the growing list)
    return loops


def _walk_loops(body):
    return [ins for ins in _self_loops(body)
            if sum(i.startswith("v_exp_f32") for i in ins) == 8 and any(i.startswith("v_pk_fma_f32") for i in ins)]


def test_the_loop_finder_on_a_hand_made_body():
    body = "\n".join(["k:", "\tv_mov_b32 v0, 0", ".LBB0_1:", "\tv_add_f32 v0, v0, v1", "\ts_cbranch_execnz .LBB0_1", "\tv_mov_b32 v9, v0",
                      ".LBB0_2:", "; comment"] + ["\tv_exp_f32_e32 v1, v1"] * 8 + ["\tv_pk_fma_f32 v[2:3], v[2:3], v[4:5], v[6:7]", "\ts_nop 0",
                      "\ts_cbranch_execnz .LBB0_2", ".LBB0_3:", "\tv_exp_f32_e32 v1, v1", ".LBB0_4:", "\ts_cbranch_vccnz .LBB0_3"])
    assert [len(x) for x in _self_loops(body)] == [2, 11]
    (w,) = _walk_loops(body)
    assert sum(i.startswith("v_") for i in w) == 9


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("unit,frag,vgprs,lds,valu", CASES, ids=[c[0] for c in CASES])
def test_walk_loops_and_registers_stay_at_or_under_the_parent(tmp_path, unit, frag, vgprs, lds, valu):
    body, desc = _kernel(_asm(unit, tmp_path), frag)
    assert _field(desc, "amdhsa_private_segment_fixed_size") == 0, (frag, "scratch")
    assert "SGPR spill" not in body and "v_writelane_b32" not in body, frag
    assert _field(desc, "amdhsa_next_free_vgpr") <= vgprs, (frag, _field(desc, "amdhsa_next_free_vgpr"))
    assert _field(desc, "amdhsa_group_segment_fixed_size") == lds, (frag, _field(desc, "amdhsa_group_segment_fixed_size"))
    walks = _walk_loops(body)
    assert len(walks) == 2, (frag, len(walks))
    for name, ins, cap in zip(("behind", "in front"), walks, valu):
        n = sum(i.startswith("v_") for i in ins)
        print(f"{frag} walk {name}: {n} VALU of {len(ins)} instructions (parent {cap})")
        assert n <= cap, (frag, name, n, cap)
        # the bound is one compare per row pair: the per-column test it replaced cost two subtractions and two compares
        assert sum(i.startswith("v_cmp") for i in ins) == 1, (frag, name)
        assert not any(i.startswith("v_cndmask") for i in ins), (frag, name)
