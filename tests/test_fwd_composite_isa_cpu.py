"""CPU guard on the frame form of the forward composite (composite.hip: compositen_kernel<..., FRAME = true>), read from the
gfx950 assembly hipcc emits without a GPU -- beside tests/test_isa_cpu.py and tests/test_bwd_walk_isa_cpu.py.

The forward composite is bound by VALU issue and five sixths of its instructions are straight-line code around the window walks.
The frame form makes what the host knows of every launch of the frame path a template fact (counts given, fragments from the
records, K a multiple of four, one-wave workgroups, 32-bit offsets), so the arms the other launches need are not instantiated.
This test holds the flagship instantiation to the figures of the commit before that form (profiles/r20_fwd_composite.txt §1):

  compositen_kernel<0, 4, true, u32, 3, 0>         78 VGPRs, 73 SGPRs, no scratch, 1148 static VALU instructions   (the parent)
  compositen_kernel<0, 4, true, u32, 3, 0, true>   72 VGPRs, 59 SGPRs, 923 static VALU: the parent's count minus the 225 cut (VALU_CAP)

and the unflagged instantiation, which every other launch still takes, to the parent's own count: it is not touched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PARENT = "compositen_kernelILi0ELi4ELb1EjLi3ELi0ELb0E"
FRAME = "compositen_kernelILi0ELi4ELb1EjLi3ELi0ELb1E"
PARENT_VGPRS, PARENT_SGPRS, PARENT_VALU = 78, 73, 1148
VALU_CAP = 923      # profiles/r20_fwd_composite.txt §1: the parent's 1148 minus the 225 cut


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


def _valu(body):
    return sum(1 for raw in body.splitlines() if raw.startswith("\t") and raw.strip().startswith("v_"))


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8 per wave; at most 8 waves."""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


def test_the_counters_on_a_hand_made_body():
    body = "\n".join(["k:", "\tv_mov_b32 v0, 0", ".LBB0_1:", "\ts_nop 0", "\tv_add_f32 v0, v0, v1", "; v_fake", "\tds_read_b32 v1, v0", "\t.p2align 3"])
    assert _valu(body) == 2
    assert [waves_per_simd(v) for v in (40, 64, 65, 78, 80, 96, 128, 129)] == [8, 8, 7, 6, 6, 5, 4, 3]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_frame_form_is_leaner_than_the_parent_and_the_parent_is_untouched(tmp_path):
    text = _asm("composite", tmp_path)
    body, desc = _kernel(text, FRAME)
    assert _field(desc, "amdhsa_private_segment_fixed_size") == 0, "scratch"
    assert "SGPR spill" not in body and "v_writelane_b32" not in body
    vgprs, sgprs, valu = _field(desc, "amdhsa_next_free_vgpr"), _field(desc, "amdhsa_next_free_sgpr"), _valu(body)
    print(f"frame form: {vgprs} VGPRs, {sgprs} SGPRs, {valu} static VALU (parent {PARENT_VGPRS}, {PARENT_SGPRS}, {PARENT_VALU}; cap {VALU_CAP})")
    assert vgprs <= PARENT_VGPRS, vgprs
    assert sgprs <= PARENT_SGPRS, sgprs
    assert waves_per_simd(vgprs) >= waves_per_simd(PARENT_VGPRS), vgprs
    assert valu <= VALU_CAP, valu
    # what the form exists to drop: the act / dsd loader's and the slot-by-slot arms' loads, and 64-bit address arithmetic
    loads = len(re.findall(r"^\s+global_load_dword ", body, flags=re.M))
    pbody, pdesc = _kernel(text, PARENT)
    assert loads < len(re.findall(r"^\s+global_load_dword ", pbody, flags=re.M)), loads
    # every other launch keeps the parent's instantiation
    assert _valu(pbody) <= PARENT_VALU, _valu(pbody)
    assert _field(pdesc, "amdhsa_next_free_vgpr") <= PARENT_VGPRS and _field(pdesc, "amdhsa_next_free_sgpr") <= PARENT_SGPRS
