"""Every per-Gaussian accumulation table past its entries and past its probe limit: the straight-to-memory arm behind the
wave-private LDS tables of trace_bwd_kernel, trace_bwd_iso_kernel (trace_bwd.hip), shade_bwd_tile_kernel (merge_blend.hip) and
fragment_bwd_kernel with four and with two slots per lane (fragment_bwd.hip), on the index lists of tests/table_cases.py.
tests/test_table_cases_cpu.py proves, with a model of the tables and under both extreme lane orders, which keys of every case take
that arm and why (table full, probes run out with slots free, the & (NE - 1) wrap, a planted id on each path, one Gaussian tabled
in one tile and refused in another), that the fp32 reference alone stays within TOL / 4, and that every memory-path slot's own
term is at least 10 TOL of scale: a lost or doubled term fails here.

All comparisons: util.grad_close at TOL = 1e-4 of scale (values that are not sums: util.close at TOL), against fp64, over every
element; rows no live slot names must be exactly zero.

Measured on MI355X (largest error of scale; measurements, nothing is asserted below TOL):
  kernel / kind                capacity K=40   capacity K=13   probe_runout   hot       mixed
  trace 3x3   g_mus            1.4e-07         9.6e-08         1.1e-07        1.6e-07   2.5e-07
              g_isigmas        1.9e-07         1.7e-07         7.4e-08        1.2e-07   1.5e-07
              g_rays           1.4e-07         1.1e-07         1.5e-07        1.5e-07   1.3e-07
  trace scalar g_mus           7.2e-08         1.1e-07         1.4e-07        7.9e-08   9.9e-08
              g_a              1.3e-07         1.2e-07         5.7e-08        8.5e-08   1.5e-07
              two views (K=40) g_mus 6.6e-08, g_sigmas 1.1e-07, g_rays 1.6e-07
  merge g_attr  C=1 / 3 / 4    1.8e-08 / 7.8e-08 / 2.9e-08;  6.6e-08 / 6.0e-08 / 2.1e-08;  4.9e-08 / 7.4e-08 / 5.0e-08;  6.2e-08 / 9.5e-08 / 7.1e-08
  shade g_attr  C=3 / 4        3.4e-08 / 2.8e-08;  6.0e-08 / 2.1e-08;  7.6e-08 / 5.9e-08;  6.5e-08 / 5.5e-08   (g_weight up to 6.8e-07, image 1.7e-07)
  scatter_attr C=3 (K=40)      7.8e-08
  fused g_mus / g_isigmas      entries 6.5e-07 / 5.9e-08, directory 5.2e-07 / 1.8e-07 (K=40); capacity 8.2e-07 / 1.0e-07, probe_runout 6.0e-07 / 9.2e-08 (K=130)
With the straight-to-memory block cut out of a scratch build (never committed) the matching tests fail with g_mus off by 0.63-1.05 of
scale (trace_bwd_kernel, all five kinds) and g_attr off by 0.07-0.76 of scale (shade_bwd_tile_kernel, all 21 cases):
profiles/r23_accumulation_tables.txt."""
import numpy as np
import pytest
import torch

import oracle
import table_cases as T
import test_attr_routes_cpu as A
from test_table_cases_cpu import SHADE_CASES, TRACE_CASES, shade_id, trace_id
from util import TOL, close, grad_close, log_line, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def check_values(label, got, want):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    log_line(f"[parity] {label}: max err {max_rel(got, want):.2e} (tolerance {TOL:.1e})")
    assert close(got, want).all(), f"{label}: {max_rel(got, want):.3e}"


# ---- trace backward -----------------------------------------------------------------------------------------------------------------------
_TRACE_REF = {}


def trace_ref(c):
    """-> case, (g_rays, g_mus [B * N, 3], g_isigmas [B * N, 3, 3]) fp64, rows of Gaussians no live slot names"""
    if c not in _TRACE_REF:
        case = T.trace_case(*c)
        mus, isg, idx = T.trace_reference_inputs(case)
        ref = oracle.trace_bwd(mus, isg, case["rays"], idx, case["g_len"], case["g_act"], case["g_dsd"])
        _TRACE_REF[c] = (case, ref, np.setdiff1d(np.arange(mus.shape[0]), idx[idx >= 0]))
    return _TRACE_REF[c]


def trace_gpu(case, mode, need_rays):
    from voge_amd import ops
    cnt = None if case["cnt"] is None else t(case["cnt"], torch.int32)
    lists = (t(case["rays"]), t(case["idx"], torch.int32), cnt, t(case["g_len"]), t(case["g_act"]), t(case["g_dsd"]), need_rays)
    if mode == 0:
        out = ops._trace_bwd(0, t(case["mus"]), t(case["isg"]), None, False, 0, *lists)
    elif mode == 1:
        out = ops._trace_bwd(1, t(case["mus"]), t(case["isg"]), None, False, 0, *lists)
    else:      # one set of Gaussians shared by the views, sigma_mode 1: a = 2 sigma
        out = ops._trace_bwd(2, t(case["mus"]), t(case["isg"] / 2), t(case["origin"]), True, 1, *lists)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", [c for c in TRACE_CASES if not c[1]], ids=trace_id)
def test_trace_bwd_3x3_vs_fp64(hip_lib, c):
    case, (r_ray, r_mu, r_A), unread = trace_ref(c)
    label = f"tables trace {trace_id(c)}"
    g_mu, g_A, g_ray = trace_gpu(case, 0, True)
    grad_close(label + " g_mus", n(g_mu), r_mu, TOL)
    grad_close(label + " g_isigmas", n(g_A), r_A, TOL)
    grad_close(label + " g_rays", n(g_ray), r_ray, TOL)
    assert unread.size and (n(g_mu)[unread] == 0).all() and (n(g_A)[unread] == 0).all()
    g_mu, g_A, g_ray = trace_gpu(case, 0, False)      # the g_ray == nullptr arm
    assert g_ray is None
    grad_close(label + " g_mus, no g_rays", n(g_mu), r_mu, TOL)
    grad_close(label + " g_isigmas, no g_rays", n(g_A), r_A, TOL)
    assert (n(g_mu)[unread] == 0).all() and (n(g_A)[unread] == 0).all()


@pytest.mark.parametrize("c", [c for c in TRACE_CASES if c[1]], ids=trace_id)
def test_trace_bwd_scalar_vs_fp64(hip_lib, c):
    """A = a I: the gradient of the scalar is trace(g_A) (tests/test_gpu_parity.py: test_trace_iso_scalar_form_vs_oracle).  B = 2:
    voge_trace_bwd_iso_view on one set shared by two views -- the views' sums added, g_sigma = 2 g_a."""
    case, (r_ray, r_mu, r_A), unread = trace_ref(c)
    label = f"tables trace {trace_id(c)}"
    B, N = case["B"], case["N"]
    r_a = np.einsum("nii->n", r_A)
    g_mu, g_a, g_ray = trace_gpu(case, 1 if B == 1 else 2, True)
    if B > 1:
        r_mu, r_a = r_mu.reshape(B, N, 3).sum(0), 2.0 * r_a.reshape(B, N).sum(0)
        unread = np.setdiff1d(np.arange(N), np.setdiff1d(np.arange(B * N), unread) % N)
    grad_close(label + " g_mus", n(g_mu), r_mu, TOL)
    grad_close(label + " g_a", n(g_a), r_a, TOL)
    grad_close(label + " g_rays", n(g_ray), r_ray, TOL)
    assert unread.size and (n(g_mu)[unread] == 0).all() and (n(g_a)[unread] == 0).all()


# ---- shade / merge backward, C <= 4 ---------------------------------------------------------------------------------------------------------
_SHADE_REF = {}


def shade_ref(c):
    if c not in _SHADE_REF:
        case = T.shade_case(*c)
        _SHADE_REF[c] = (case, A.blend_reference(case, -1.0) if c[2] else A.merge_reference(case))
    return _SHADE_REF[c]


def fragments_of(case):
    from voge_amd.Renderer import Fragments
    w = t(case["weight"], rg=True)
    return Fragments(vert_weight=w, vert_index=t(case["idx"], torch.int32), valid_num=t(case["valid_num"], torch.int64),
                     vert_hit_length=torch.zeros_like(w))


def unread_rows(case):
    live = np.arange(case["K"]) < case["valid_num"][..., None]
    return np.setdiff1d(np.arange(case["Nattr"]), np.maximum(case["idx"], 0)[live])


@pytest.mark.parametrize("c", [c for c in SHADE_CASES if not c[2]], ids=shade_id)
def test_interpolate_attr_vs_fp64(hip_lib, c):
    from voge_amd.Renderer import interpolate_attr
    case, (want, ga_want, gw_want) = shade_ref(c)
    label = f"tables merge {shade_id(c)}"
    frag, attr = fragments_of(case), t(case["attr"], rg=True)
    out = interpolate_attr(frag, attr)
    assert type(out.grad_fn).__name__ == "_MergeBackward"
    (out * t(case["g"])).sum().backward()
    check_values(label + " out", n(out), want)
    check_values(label + " g_weight", n(frag.vert_weight.grad), gw_want)
    grad_close(label + " g_attr", n(attr.grad), ga_want, TOL)
    unread = unread_rows(case)
    assert unread.size and (n(attr.grad)[unread] == 0).all()


@pytest.mark.parametrize("c", [c for c in SHADE_CASES if c[2]], ids=shade_id)
def test_to_colored_background_vs_fp64(hip_lib, c):
    """the bg != NULL arm of shade_bwd_tile_kernel, through the public entry and, once per kind, through ops.shade"""
    from voge_amd import ops
    from voge_amd.Renderer import to_colored_background
    case, (img_want, _, ga_want, gw_want) = shade_ref(c)
    label = f"tables shade {shade_id(c)}"
    frag, attr = fragments_of(case), t(case["attr"], rg=True)
    bg = tuple(float(v) for v in case["bg"])
    if case["C"] == 3:
        img = to_colored_background(frag, attr, background_color=bg, thr=-1.0)
    else:
        img = ops.shade(attr, frag.vert_weight, frag.vert_index, frag.valid_num, t(case["bg"]), -1.0)
    assert type(img.grad_fn).__name__ == "_ShadeBackward", type(img.grad_fn).__name__
    (img * t(case["g"])).sum().backward()
    check_values(label + " image", n(img), img_want)
    check_values(label + " g_weight", n(frag.vert_weight.grad), gw_want)
    grad_close(label + " g_attr", n(attr.grad), ga_want, TOL)
    unread = unread_rows(case)
    assert unread.size and (n(attr.grad)[unread] == 0).all()


def test_scatter_attr_vs_fp64(hip_lib):
    """attr == NULL: the sampler's scatter of weight * image is the merge's attribute gradient for that image as upstream gradient"""
    from voge_amd import ops
    c = ("capacity40", 3, False)
    case, (_, ga_want, _) = shade_ref(c)
    out = ops.scatter_attr(t(case["g"]), t(case["weight"]), t(case["idx"], torch.int32), t(case["valid_num"], torch.int64), case["Nattr"])
    torch.cuda.synchronize()
    grad_close(f"tables scatter {shade_id(c)} features", n(out), ga_want, TOL)
    unread = unread_rows(case)
    assert unread.size and (n(out)[unread] == 0).all()


# ---- fused backward, weights form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(T.FUSED_KINDS))
def test_fused_backward_vs_fp64(hip_lib, kind):
    from voge_amd import ops
    case = T.fused_case(kind)
    K, P, H, W, g = case["K"], case["P"], case["H"], case["W"], case["g"]
    _, r_mu, r_A = T.fused_reference(case)
    tm, ts = t(g["mus"]), t(g["isg"])
    g_mu, g_A = ops._fragment_bwd(0, tm, ts, None, False, 0, t(g["rays"]).reshape(1, H, W, 3), t(case["idx"], torch.int32).reshape(1, H, W, K),
                                  t(case["nv"], torch.int32), 1, P, (tm, ts), t(T.fused_weights(case)), t(case["act"]), t(case["ln"]),
                                  t(case["dsd"]), t(case["gw"]), None, case["occ"])
    torch.cuda.synchronize()
    label = f"tables fused {kind} K={K}"
    grad_close(label + " g_mus", n(g_mu), r_mu, TOL)
    grad_close(label + " g_isigmas", n(g_A).reshape(P, 3, 3), r_A, TOL)
    unread = np.setdiff1d(np.arange(P), case["idx"][case["idx"] >= 0])
    if kind != "entries":      # (256 ids in all: every one is named)
        assert unread.size
    assert (n(g_mu)[unread] == 0).all() and (n(g_A)[unread] == 0).all()
