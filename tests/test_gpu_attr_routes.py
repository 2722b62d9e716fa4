"""GPU tests of every kernel route of merge, blend and the sampler (voge_amd/csrc/merge_blend.hip: voge_shade_fwd's three forward
kernels, voge_merge_bwd's three backward kernels, voge_blend_fwd / _bwd) and of the dense-ray extras (voge_amd/csrc/extras.hip).

References: oracle.torch_ref.merge_final / to_colored_background in fp64 under autograd, oracle/extras_np.py, oracle/coarse_np.py,
on the inputs tests/test_attr_routes_cpu.py builds -- which also guarantees that the fp32 reference alone stays within TOL / 4 and
that no clamp or threshold decision sits within 1e-2 of its switch, so no pixel is ever excluded here.

Values:    util.close at util.TOL (1e-4 relative to max(1, |reference|)).
Gradients summed by float atomics (g_attr, the dense backward, the sampler's features): util.grad_close at TOL of their scale.
Copies, maxima, integers: exactly (bit patterns where a sign of zero could hide)."""
import numpy as np
import pytest
import torch

from oracle import coarse_np, extras_np
from test_attr_routes_cpu import (BLEND_CASES, BLEND_THR, MERGE_CASES, NEAREST_THR_ACT, SAMPLER_CHANNELS, SAMPLER_K, SHADE_DIRECT,
                                  blend_case, blend_reference, case_id, coarse_case, dense_inputs, effective_index, merge_case,
                                  merge_reference, nearest_case, sampler_case)
from util import TOL, close, grad_close, log_line, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def carve(a, dtype, aligned):
    """A contiguous device tensor of `a`; aligned=False: a view that starts one element into a flat buffer (4 bytes past a 16-byte
    boundary), which the 16-byte loads of the four-slot kernel cannot take."""
    a = np.asarray(a)
    if aligned:
        out = t(a, dtype)
        assert out.data_ptr() % 16 == 0
        return out
    flat = torch.zeros(a.size + 1, dtype=dtype, device=DEV)
    view = flat[1:].view(a.shape)
    view.copy_(t(a, dtype))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def fragments_of(case, aligned=True, rg=True):
    from voge_amd.Renderer import Fragments
    w = carve(case["weight"], torch.float32, aligned).requires_grad_(rg)
    idx = carve(case["idx"], torch.int32, aligned)
    return Fragments(vert_weight=w, vert_index=idx, valid_num=t(case["valid_num"], torch.int64), vert_hit_length=torch.zeros_like(w))


def per_channel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    C = want.shape[-1]
    return (np.abs(got - want) / np.maximum(1.0, np.abs(want))).reshape(-1, C).max(0)


def check_values(label, got, want):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    log_line(f"[parity] {label}: max err {max_rel(got, want):.2e} (tolerance {TOL:.1e})")
    assert close(got, want).all(), f"{label}: {max_rel(got, want):.3e}"


def check_image(label, got, want):
    """util.close at TOL, reported per channel: a failure that starts at channel 4 shows as such."""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    e = per_channel(got, want)
    first_bad = int(np.argmax(e > TOL)) if (e > TOL).any() else -1
    log_line(f"[parity] {label}: max err per channel, channels 0-3 {e[:4].max():.2e}, channels 4+ "
             f"{(e[4:].max() if e.size > 4 else 0.0):.2e}, first channel over tolerance {first_bad} (tolerance {TOL:.1e})")
    assert close(got, want).all(), f"{label}: per-channel max err {np.array2string(e, precision=1)}"


# ---- a. merge ------------------------------------------------------------------------------------------------------------------------------
_MERGE_REF = {}


def merge_ref(c):
    key = (c[0], c[1], c[2], c[3])      # (the unaligned cases share the aligned case's numbers when there is one)
    if key not in _MERGE_REF:
        case = merge_case(c)
        _MERGE_REF[key] = (case,) + merge_reference(case)
    return _MERGE_REF[key]


@pytest.mark.parametrize("c", MERGE_CASES, ids=case_id)
def test_merge_forward_and_both_gradients_vs_fp64(hip_lib, c):
    from voge_amd.Renderer import interpolate_attr
    case, want, ga_want, gw_want = merge_ref(c)
    label = f"merge {case_id(c)} [{c[5]}/{c[6]}]"
    frag = fragments_of(case, aligned=c[4])
    attr = t(case["attr"], rg=True)
    out = interpolate_attr(frag, attr)
    assert type(out.grad_fn).__name__ == "_MergeBackward" and out.dtype == torch.float32
    (out * t(case["g"])).sum().backward()
    check_values(label + " out", n(out), want)
    check_values(label + " g_weight", n(frag.vert_weight.grad), gw_want)
    grad_close(label + " g_attr", n(attr.grad), ga_want, TOL)
    # the in-place index fix, exactly, and nothing else of the list touched
    assert np.array_equal(n(frag.vert_index), case["idx"] + (case["idx"] < 0))
    # rows of the attribute table that no live slot reads get exactly zero
    live = np.arange(case["K"]) < case["valid_num"][..., None]
    unread = np.setdiff1d(np.arange(case["Nattr"]), np.maximum(case["idx"], 0)[live])
    assert (n(attr.grad)[unread] == 0).all()
    assert (n(frag.vert_weight.grad)[~live] == 0).all()      # a masked slot's weight has no gradient
    if not c[4]:      # the same numbers through the aligned routes: both within TOL of the reference, so within 2 TOL of each other
        frag2 = fragments_of(case, aligned=True, rg=False)
        out2 = interpolate_attr(frag2, t(case["attr"]))
        assert close(n(out), n(out2), 2 * TOL).all()


# ---- b. blend with a constant colour ---------------------------------------------------------------------------------------------------------
_BLEND_REF = {}


def blend_ref(c, thr):
    key = (c, thr)
    if key not in _BLEND_REF:
        case = _BLEND_REF[(c, "case")] = _BLEND_REF.get((c, "case")) or blend_case(c)
        full = blend_reference(case, thr)
        rgb32 = full[1].astype(np.float32)
        _BLEND_REF[key] = (case, full, rgb32, blend_reference(case, thr, rgb=rgb32))
    return _BLEND_REF[key]


@pytest.mark.parametrize("c", BLEND_CASES, ids=case_id)
@pytest.mark.parametrize("thr", BLEND_THR)
def test_ops_blend_vs_fp64(hip_lib, c, thr):
    """voge_blend_fwd / voge_blend_bwd from a given rgb: image, g_rgb and the silhouette term of g_weight.  (While shade_fwd_kernel
    cleared the pixel's weight sum with every channel pass, the image's channels 4 and up came out as min(rgb + bg, 1): off by
    0.25 to 0.90 on these cases, with channels 0-3 within 1e-7.)"""
    from voge_amd import ops
    case, _, rgb32, (img_want, _, grgb_want, gw_want) = blend_ref(c, thr)
    label = f"ops.blend {case_id(c)} thr={thr}"
    rgb, w = t(rgb32, rg=True), t(case["weight"], rg=True)
    img = ops.blend(rgb, w, t(case["bg"]), thr)
    assert type(img.grad_fn).__name__ == "_BlendBackward"
    (img * t(case["g"])).sum().backward()
    check_image(label + " image", n(img), img_want)
    check_image(label + " g_rgb", n(rgb.grad), grgb_want)
    check_values(label + " g_weight", n(w.grad), gw_want)
    if thr > 0:
        assert (n(w.grad) == 0).all()      # ([sil > thr] has no gradient)
    else:
        assert float(np.abs(gw_want).max()) > 0


@pytest.mark.parametrize("c", BLEND_CASES, ids=case_id)
@pytest.mark.parametrize("thr", BLEND_THR)
def test_to_colored_background_constant_colour_vs_fp64(hip_lib, c, thr):
    """The public route: fused shade for <= 4 channels, merge + voge_blend_fwd / _bwd above (Renderer.to_colored_background)."""
    from voge_amd.Renderer import to_colored_background
    case, (img_want, _, ga_want, gw_want), _, _ = blend_ref(c, thr)
    label = f"to_colored_background {case_id(c)} thr={thr}"
    frag = fragments_of(case)
    attr = t(case["attr"], rg=True)
    bg = tuple(float(v) for v in case["bg"])
    img = to_colored_background(frag, attr, background_color=bg, thr=thr)
    assert type(img.grad_fn).__name__ == ("_ShadeBackward" if case["C"] <= 4 else "_BlendBackward"), type(img.grad_fn).__name__
    (img * t(case["g"])).sum().backward()
    check_image(label + " image", n(img), img_want)
    check_values(label + " g_weight", n(frag.vert_weight.grad), gw_want)
    grad_close(label + " g_attr", n(attr.grad), ga_want, TOL)


@pytest.mark.parametrize("thr", BLEND_THR)
def test_shade_entry_with_merge_and_image_in_the_general_kernel(hip_lib, thr):
    """voge_shade_fwd itself with attr, out_rgb, out_img, out_sil and out_wsum at C = 6, K = 5: six channels take two passes of the
    general kernel, and the second must still see the pixel's weight sum."""
    from voge_amd import ops
    case, (img_want, rgb_want, _, _), _, _ = blend_ref(SHADE_DIRECT, thr)
    K, C, Nattr = case["K"], case["C"], case["Nattr"]
    idx, w, vn = t(case["idx"], torch.int32), t(case["weight"]), t(case["valid_num"], torch.int64)
    attr, bg = t(case["attr"]), t(case["bg"])
    npix = idx.numel() // K
    rgb = torch.full(idx.shape[:-1] + (C,), float("nan"), device=DEV)
    img = torch.full_like(rgb, float("nan"))
    sil = torch.full(idx.shape[:-1], float("nan"), device=DEV)
    wsum = torch.full_like(sil, float("nan"))
    rc = hip_lib.voge_shade_fwd(attr.data_ptr(), idx.data_ptr(), w.data_ptr(), vn.data_ptr(), bg.data_ptr(), float(thr), npix, K, C,
                                Nattr, 1, rgb.data_ptr(), img.data_ptr(), sil.data_ptr(), wsum.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    label = f"voge_shade_fwd {case_id(SHADE_DIRECT)} thr={thr}"
    check_image(label + " rgb", n(rgb), rgb_want)
    check_image(label + " image", n(img), img_want)
    s = case["weight"].astype(np.float64).sum(-1)
    check_values(label + " wsum", n(wsum), s)
    check_values(label + " sil", n(sil), np.minimum(s, 1.0))
    assert np.array_equal(n(idx), case["idx"] + (case["idx"] < 0))


# ---- c. sampler ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", SAMPLER_CHANNELS)
@pytest.mark.parametrize("K", SAMPLER_K)
def test_sample_features_and_both_gradients_vs_oracle(hip_lib, C, K):
    from voge_amd.Sampler import sample_features
    case = sampler_case(C, K)
    eff = effective_index(case["idx"], case["valid_num"])
    frag = fragments_of(case)
    image = t(case["image"], rg=True)
    feat, wsum = sample_features(frag, image, n_vert=case["Nattr"])
    ((feat * t(case["g_feat"])).sum() + (wsum * t(case["g_wsum"])).sum()).backward()
    rf, rw = extras_np.sample_voge(case["image"], case["weight"], eff, case["Nattr"])
    g_img, g_w = extras_np.sample_voge_bwd(case["image"], case["weight"], eff, case["g_feat"], case["g_wsum"])
    label = f"sampler C={C} (kernels see {C + 1}) K={K}"
    grad_close(label + " features", n(feat), rf, TOL)      # (sums by float atomics, as g_attr)
    grad_close(label + " weight sums", n(wsum), rw, TOL)
    check_values(label + " g_image", n(image.grad), g_img)
    check_values(label + " g_weight", n(frag.vert_weight.grad), g_w)
    assert np.array_equal(n(frag.vert_index), case["idx"])      # the sampler leaves the index list alone


def test_scatter_max_is_the_exact_maximum_under_heavy_collisions(hip_lib):
    """70 000 slots onto 3 vertices through the C ABI, with -1, indices >= Nv (the kernel's own guard), negative weights and exact
    zeros: a maximum does not depend on the order, so the result is the fp32 maximum bit for bit."""
    from voge_amd import ops
    rng = np.random.default_rng(41)
    cnt, Nv = 70000, 3
    idx = rng.integers(-1, Nv + 3, cnt).astype(np.int32)
    w = rng.normal(size=cnt).astype(np.float32)
    w[rng.random(cnt) < 0.1] = 0.0
    want = np.zeros(Nv, np.float32)
    for v in range(Nv):
        want[v] = max(np.float32(0), w[idx == v].max())
    ti, tw = t(idx, torch.int32), t(w)
    out = torch.full((Nv + 2,), float("nan"), device=DEV)      # two guard elements behind the table
    rc = hip_lib.voge_scatter_max(tw.data_ptr(), ti.data_ptr(), cnt, Nv, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = n(out)
    assert got[:Nv].view(np.int32).tolist() == want.view(np.int32).tolist() and (want > 0).all()
    assert np.isnan(got[Nv:]).all()      # nothing written behind the table
    # all weights of a vertex negative or zero: its maximum stays 0
    w2 = np.where(idx == 1, -np.abs(w), w).astype(np.float32)
    rc = hip_lib.voge_scatter_max(t(w2).data_ptr(), ti.data_ptr(), cnt, Nv, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and n(out)[1] == 0 and n(out)[0] == want[0] and n(out)[2] == want[2]
    # the public wrapper on in-range indices, and the empty calls
    inr = np.where(idx >= Nv, -1, idx).astype(np.int32)
    assert n(ops.scatter_max(tw, t(inr, torch.int32), Nv)).view(np.int32).tolist() == want.view(np.int32).tolist()
    assert n(ops.scatter_max(tw[:0], ti[:0], Nv)).tolist() == [0.0, 0.0, 0.0]
    assert ops.scatter_max(tw, ti, 0).shape == (0,)


# ---- d. dense ray API ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 1), (64, 64), (65, 129), (1100, 2000)])
def test_dense_forward_vs_oracle(hip_lib, M, N):
    """(1100, 2000): 2.2 M pairs, more than the 8192 x 256 items of the capped grid -- the grid-stride loop runs."""
    from voge_amd.RayTracing import ray_trace_voge_ray
    assert (M, N) != (1100, 2000) or M * N > 8192 * 256
    mus, isg, rays = dense_inputs(M, N, seed=M + N)
    got = ray_trace_voge_ray(t(mus), t(isg), t(rays))
    ref = extras_np.ray_dense_fwd(mus, isg, rays)
    for name, g, r in zip(("len", "act", "dsd"), got, ref):
        assert g.shape == (N, M)
        check_values(f"dense forward M={M} N={N} {name}", n(g), r)


@pytest.mark.parametrize("M,N", [(130, 200), (65, 129)])
def test_dense_backward_across_workgroups_vs_oracle(hip_lib, M, N):
    """Several workgroups in x add into the same g_ray rows, several in y into the same g_mus / g_isg rows."""
    from voge_amd.RayTracing import ray_trace_voge_ray
    assert M > 64 and N > 64
    mus, isg, rays = dense_inputs(M, N, seed=M + N)
    tm, tA, tr = t(mus, rg=True), t(isg, rg=True), t(rays, rg=True)
    ln, act, dsd = ray_trace_voge_ray(tm, tA, tr)
    rng = np.random.default_rng(M)
    gl, ga, gd = (rng.normal(size=(N, M)).astype(np.float32) for _ in range(3))
    (ln * t(gl) + act * t(ga) + dsd * t(gd)).sum().backward()
    g_ray, g_mu, g_A = extras_np.ray_dense_bwd(mus, isg, rays, gl, ga, gd)
    for name, got, ref in (("g_ray", tr.grad, g_ray), ("g_mus", tm.grad, g_mu), ("g_isg", tA.grad, g_A)):
        grad_close(f"dense backward M={M} N={N} {name}", n(got), ref, TOL)


@pytest.mark.parametrize("M,N", [(0, 7), (7, 0)])
def test_dense_backward_of_an_empty_side_zero_fills(hip_lib, M, N):
    from voge_amd import ops
    bufs = [torch.full((max(N, 1), 3), float("nan"), device=DEV), torch.full((max(M, 1), 3), float("nan"), device=DEV),
            torch.full((max(M, 1), 3, 3), float("nan"), device=DEV)]
    mus, isg, rays = torch.zeros((max(M, 1), 3), device=DEV), torch.zeros((max(M, 1), 3, 3), device=DEV), torch.zeros((max(N, 1), 3), device=DEV)
    g = torch.zeros((1,), device=DEV)
    rc = hip_lib.voge_ray_dense_bwd(mus.data_ptr(), isg.data_ptr(), rays.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), M, N,
                                    bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    g_ray, g_mus, g_isg = (n(b) for b in bufs)
    if N > 0:
        assert (g_ray == 0).all() and np.isnan(g_mus).all() and np.isnan(g_isg).all()
    else:
        assert (g_mus == 0).all() and (g_isg == 0).all() and np.isnan(g_ray).all()
    out = [torch.full((1,), float("nan"), device=DEV) for _ in range(3)]
    rc = hip_lib.voge_ray_dense_fwd(mus.data_ptr(), isg.data_ptr(), rays.data_ptr(), M, N, out[0].data_ptr(), out[1].data_ptr(),
                                    out[2].data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(np.isnan(n(o)).all() for o in out)      # nothing to do, nothing written


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def nearest_k_raw(ln, act, dsd, K, farthest=False):
    """_FindNearestK at NEAREST_THR_ACT through the public functions' autograd node (find_nearest_k / find_farest_k take the
    activation threshold as thr = exp(-thr_act): the same number after one rounding, so the node is called directly)."""
    from voge_amd import ops
    tl, ta, td = t(ln, rg=True), t(act, rg=True), t(dsd, rg=True)
    idx, ol, oa, od = ops._FindNearestK.apply(-tl if farthest else tl, ta, td, NEAREST_THR_ACT, K)
    return (tl, ta, td), idx, (-ol if farthest else ol), oa, od


@pytest.mark.parametrize("N,M,K", [(5, 3, 5), (129, 9, 4), (70, 300, 256), (66, 40, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("farthest", [False, True])
def test_nearest_and_farthest_k_are_exact_copies_in_oracle_order(hip_lib, N, M, K, farthest):
    """K > M, a row with nothing under the threshold (-1, 1e10, 0, 0), lengths of both signs with -0.0, bit-equal lengths (ascending
    index), N = 129 (three workgroups, the last with one ray), K = 256 (128 KiB of LDS).  What is selected is a COPY of the input:
    compared bit for bit; the backward is the scatter of the upstream gradients, exactly."""
    ln, act, dsd = nearest_case(N, M, seed=N + M + K)
    (tl, ta, td), idx, ol, oa, od = nearest_k_raw(ln, act, dsd, K, farthest)
    sign = -1.0 if farthest else 1.0
    ri, rl, ra, rd = extras_np.find_nearest_k(np.float32(sign) * ln, act, dsd, K, NEAREST_THR_ACT)
    rl = np.where(ri >= 0, sign * rl, sign * 1e10)
    assert np.array_equal(n(idx), ri)
    assert (ri[0] == -1).all() and (n(ol)[0] == np.float32(sign * 1e10)).all() and (n(oa)[0] == 0).all() and (n(od)[0] == 0).all()
    assert ri[2].tolist() == [M // 2] + [-1] * (K - 1)
    sel = ri >= 0
    for name, got, ref in (("len", ol, rl), ("act", oa, ra), ("dsd", od, rd)):
        assert np.array_equal(bits(n(got))[sel], bits(ref)[sel]), name      # copies: the very bits, the sign of zero included
        assert np.array_equal(n(got)[~sel], np.asarray(ref, np.float32)[~sel]), name
    if K >= 4:      # the tied pairs, ascending in index either way round
        zeros, pair = ([1, M - 1] if M >= 5 else [1]), [0, 2]
        head = zeros + pair if farthest else pair + zeros
        assert n(idx)[1].tolist() == head + [-1] * (K - len(head))
    rng = np.random.default_rng(K)
    g = rng.normal(size=(3, N, K)).astype(np.float32)
    (ol * t(g[0]) + oa * t(g[1]) + od * t(g[2])).sum().backward()
    rows, ks = np.nonzero(sel)
    for name, got, gi in (("len", tl.grad, g[0]), ("act", ta.grad, g[1]), ("dsd", td.grad, g[2])):
        ref = np.zeros((N, M), np.float32)
        ref[rows, ri[rows, ks]] = gi[rows, ks]
        assert np.array_equal(n(got), ref), name


def test_public_nearest_k_entry_points_and_k_above_the_limit(hip_lib):
    from voge_amd._lib import VogeHipError
    from voge_amd.RayTracing import find_farest_k, find_nearest_k
    import math
    ln, act, dsd = nearest_case(70, 300, seed=5)
    thr = 0.1
    thr_act = -math.log(thr + 1 / 1e8)
    for fn, sign in ((find_nearest_k, 1.0), (find_farest_k, -1.0)):
        idx, ol, oa, od = fn(t(ln), t(act), t(dsd), 7, thr)
        ri, rl, ra, rd = extras_np.find_nearest_k(np.float32(sign) * ln, act, dsd, 7, thr_act)
        assert np.array_equal(n(idx), ri)
        assert np.array_equal(n(ol), (sign * rl).astype(np.float32)) and np.array_equal(n(oa), ra.astype(np.float32))
        assert np.array_equal(n(od), rd.astype(np.float32))
    with pytest.raises(VogeHipError, match="VOGE_MAX_K"):
        find_nearest_k(t(ln), t(act), t(dsd), 257, thr)
    out = torch.zeros((70, 257), device=DEV)
    rc = hip_lib.voge_find_nearest_k(t(ln).data_ptr(), t(act).data_ptr(), t(dsd).data_ptr(), 1.0, 300, 257, 70, out.data_ptr(),
                                     out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
    assert rc == -3      # VOGE_ERR_K_TOO_LARGE, before anything is launched


# ---- e. coarse bins ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size", [(40, 72), (72, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", [1033, 40])
def test_coarse_bins_two_clouds_non_square_vs_oracle(hip_lib, image_size, M):
    from voge_amd import ops
    pts, rad, first, num = coarse_case(image_size)
    want = coarse_np.rasterize_points_coarse(pts, first, num, image_size, rad, 16, M)
    got = n(ops.rasterize_points_coarse(t(pts), t(first, torch.int64), t(num, torch.int64), image_size, t(rad), 16, M))
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} of {want[..., 0].size} bins differ"
    if M == 40:      # the small capacity drops chunks in at least one bin
        full = coarse_np.rasterize_points_coarse(pts, first, num, image_size, rad, 16, 1033)
        assert ((want >= 0).sum(-1) < (full >= 0).sum(-1)).any()
    for b in range(2):
        e = got[b][got[b] >= 0]
        assert e.min() >= first[b] and e.max() < first[b] + num[b]
