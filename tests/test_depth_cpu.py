"""CPU tests of Renderer.get_depth (an extension: the reference has no depth output): the import path, the four C-ABI entries
and their host-side argument validation (no GPU in this container: anything that reached HIP would fail differently), the
error on host tensors, the gradient formulas the GPU tests' reference uses against finite differences, and what the compiler
made of the fused backward's depth form (tests/test_isa_cpu.py's limits)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "voge_hip.h")
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = {"voge_depth_fwd": 10, "voge_depth_bwd": 12, "voge_frame_depth_fwd_iso": 18, "voge_frame_depth_bwd_iso": 26}


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_get_depth_is_importable_through_the_alias_package():
    from VoGE.Renderer import get_depth
    from voge_amd import Renderer
    assert get_depth is Renderer.get_depth
    doc = get_depth.__doc__
    assert "cosine" in doc and "background" in doc and "not clamped" in doc


def test_the_four_entries_are_declared_exported_and_typed(lib):
    from voge_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s*" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in voge_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.voge_abi_version() == 7
    text = open(HEADER).read()
    assert text.count("EXTENSION") >= 2 and "vert_weight * frag.vert_hit_length" in text      # which torch expression they replace


def test_entries_validate_before_any_hip_call(lib):
    P = 1234      # (a non-NULL pointer value: nothing is dereferenced before validation is through)
    assert lib.voge_depth_fwd(None, None, None, 10, 8, 1, 0.0, None, None, None) == -1
    assert lib.voge_depth_fwd(P, P, P, -1, 8, 1, 0.0, P, P, None) == -1
    assert lib.voge_depth_fwd(P, P, P, 10, 300, 1, 0.0, P, P, None) == -3
    assert lib.voge_depth_fwd(P, P, P, 0, 8, 1, 0.0, P, P, None) == 0
    assert lib.voge_depth_bwd(P, P, P, P, P, None, 10, 8, 1, P, P, None) == -1
    assert lib.voge_depth_bwd(P, P, P, None, None, P, 10, 8, 1, P, P, None) == -1      # the normalised form needs depth and wsum
    assert lib.voge_depth_bwd(P, P, P, P, P, P, 10, 300, 1, P, P, None) == -3
    assert lib.voge_depth_bwd(P, P, P, P, P, P, 0, 8, 1, P, P, None) == 0
    fw = (P, P, P, P, P, 1.0, 1, 0.0)
    assert lib.voge_frame_depth_fwd_iso(*fw, 100, 129, P, P, P, P, P, None, 0, None) == -3
    assert lib.voge_frame_depth_fwd_iso(P, None, P, P, P, 1.0, 1, 0.0, 100, 16, P, P, P, P, P, None, 0, None) == -1
    assert lib.voge_frame_depth_fwd_iso(*fw, 100, 16, P, P, None, P, P, None, 0, None) == -1
    assert lib.voge_frame_depth_fwd_iso(*fw, 100, 16, P, P, P, P, P, P + 4, 1600, None) == -1      # 16-byte granularity of the accumulator
    assert lib.voge_frame_depth_fwd_iso(*fw, 0, 16, P, P, P, P, P, None, 0, None) == 0
    bw = (P, P, 1, 1, P, P, P, P, P, P, P, P, 1, None, 1, 1.0, 1, 100, 64, 64)
    assert lib.voge_frame_depth_bwd_iso(*bw, 129, P, 1600, P, P, None) == -3
    assert lib.voge_frame_depth_bwd_iso(*bw, 16, P, 100, P, P, None) == -2                          # an accumulator below 16 bytes per Gaussian
    assert lib.voge_frame_depth_bwd_iso(*bw, 16, None, 1600, P, P, None) == -1
    assert lib.voge_frame_depth_bwd_iso(P, P, 1, 1, P, P, P, P, P, P, P, None, 1, None, 1, 1.0, 1, 100, 64, 64, 16, P, 1600, P, P, None) == -1   # neither gradient
    assert lib.voge_frame_depth_bwd_iso(P, P, 1, 1, P, P, P, P, P, P, P, P, 1, None, 1, 1.0, 1, 0, 64, 64, 16, P, 1600, P, P, None) == 0      # no Gaussians


def test_get_depth_on_host_tensors_raises(lib):
    import torch
    from voge_amd import _lib
    from voge_amd.Renderer import Fragments, get_depth
    frag = Fragments(torch.rand(4, 5, 3), torch.zeros(4, 5, 3, dtype=torch.int32), torch.full((4, 5), 3), torch.rand(4, 5, 3))
    with pytest.raises(_lib.VogeHipError, match="no CPU fallback"):
        get_depth(frag)


# ---- the fp64 reference of get_depth and of its gradient, as tests/test_gpu_depth.py states them ---------------------------
def depth_ref(w, ln, vn, normalize, background=0.0):
    w, ln = np.asarray(w, np.float64), np.asarray(ln, np.float64)
    K = w.shape[-1]
    live = np.arange(K) < np.minimum(np.asarray(vn), K)[..., None]
    A = np.where(live, w * np.where(live, ln, 0.0), 0.0).sum(-1)
    S = np.where(live, w, 0.0).sum(-1)
    if not normalize:
        return A, S, live
    hit = S > 0
    return np.where(hit, A / np.where(hit, S, 1.0), background), S, live


def depth_grads_ref(w, ln, vn, g, normalize):
    D, S, live = depth_ref(w, ln, vn, normalize)
    if normalize:
        hit = S > 0
        a = np.where(hit, g / np.where(hit, S, 1.0), 0.0)
        b = np.where(hit, -a * D, 0.0)
    else:
        a, b = np.asarray(g, np.float64), np.zeros_like(S)
    lnl = np.where(live, np.asarray(ln, np.float64), 0.0)
    return (a[..., None] * lnl + b[..., None]) * live, a[..., None] * np.where(live, np.asarray(w, np.float64), 0.0)


@pytest.mark.parametrize("normalize", [True, False])
def test_gradient_formulas_agree_with_finite_differences(normalize):
    """g_w[k] = a len_k + b, g_len[k] = a w_k with a = g_D / S, b = -g_D D / S (normalised) or a = g_D, b = 0: central
    differences of sum(D * g) on a random [6][5] case whose valid_num runs from 0 (nothing hit) to beyond K."""
    rng = np.random.default_rng(0)
    w = rng.uniform(0.02, 0.6, (6, 5))
    ln = np.sort(rng.uniform(1.4, 4.8, (6, 5)), axis=-1)
    vn = np.array([0, 1, 3, 5, 7, 2])
    dead = np.arange(5)[None] >= np.minimum(vn, 5)[:, None]
    ln[dead] = 1e10
    g = rng.normal(size=6)
    g_w, g_h = depth_grads_ref(w, ln, vn, g, normalize)
    assert (g_w[dead] == 0).all() and (g_h[dead] == 0).all()

    def loss(w_, l_):
        return float((depth_ref(w_, l_, vn, normalize, 7.5)[0] * g).sum())
    eps = 1e-6
    for arr, grad in ((w, g_w), (ln, g_h)):
        for i in range(6):
            for k in range(5):
                hi, lo = arr.copy(), arr.copy()
                step = eps * max(1.0, abs(arr[i, k]))
                hi[i, k] += step
                lo[i, k] -= step
                fd = (loss(hi, ln) - loss(lo, ln)) if arr is w else (loss(w, hi) - loss(w, lo))
                fd /= 2 * step
                assert abs(fd - grad[i, k]) <= 1e-6 * max(1.0, abs(grad[i, k])), (i, k, fd, grad[i, k])
    if normalize:      # the background has no gradient, and the value is the background itself
        assert depth_ref(w, ln, vn, True, 7.5)[0][0] == 7.5 and (g_w[0] == 0).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_depth_form_of_the_fused_backward_has_no_register_spills(tmp_path):
    """The SRC = 2 instantiation of fragment_bwd_kernel under the limits tests/test_isa_cpu.py holds the weights-driven form to:
    no scratch, at most 2 scalars parked in VGPR lanes, at most 128 VGPRs and 102 SGPRs -- and the same kernel-argument list as
    every other form (a new SRC value, not a new parameter: the other tests find kernels by mangled-name prefix)."""
    out = os.path.join(str(tmp_path), "fragment_bwd.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only", "-o", out,
                           os.path.join(CSRC, "fragment_bwd.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN4voge\w*fragment_bwd_kernelILi2ELi0ELi2EjLb1ELb1ELb0E\w*):\s", text, flags=re.M)
    assert len(names) == 1, names
    other = re.search(r"^(_ZN4voge\w*fragment_bwd_kernelILi1ELi0ELi2EjLb1ELb1ELb0E\w*):\s", text, flags=re.M).group(1)
    assert names[0].split("ELb0EEEv")[1] == other.split("ELb0EEEv")[1], "the depth form must not change the kernel's argument list"
    start = text.index(names[0] + ":")
    body = text[start:text.index(".Lfunc_end", start)]
    d = text.index(".amdhsa_kernel " + names[0])
    desc = text[d:text.index(".end_amdhsa_kernel", d)]

    def field(key):
        return int(re.search(r"\." + key + r"\s+(\d+)", desc).group(1))
    spills = len(re.findall(r"^\s+v_writelane_b32", body, flags=re.M))
    assert spills <= 2, f"{spills} scalars spilled into VGPR lanes"
    assert field("amdhsa_private_segment_fixed_size") == 0, "scratch"
    assert field("amdhsa_next_free_vgpr") <= 128, field("amdhsa_next_free_vgpr")
    assert field("amdhsa_next_free_sgpr") <= 102, field("amdhsa_next_free_sgpr")
