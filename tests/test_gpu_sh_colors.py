"""GPU tests of the view-dependent colours (Renderer.sh_to_colors, ops._ShColors: voge_sh_colors_fwd / _bwd; an extension, the
reference and the oracle have no spherical-harmonic code).

The reference is the DEFINITION, Aggregation.sh_colors, evaluated in fp64 on the host from the fp32-rounded inputs
(tests/test_sh_colors_cpu.py pins it against an independent numpy restatement and central differences).

Colours:   |got - ref| <= 16 * 2^-23 * (sum_m |Y_m| |sh_m| + 0.5) per element -- at most 16 products and sums, each a few roundings
           of terms no larger than that magnitude.  Derived, not tuned.
Gradients: util.grad_close at 1e-5 of the gradient's scale (the fp32 torch definition itself is at 2.5e-7 on the large case; the
           rest is for summing the views in another order).  The clamp is a discontinuity of the gradient: a Gaussian whose fp64
           |pre| is below 1e-5 in any view and channel is left out of the GRADIENT comparison (never of the colour comparison),
           and at most 0.1 % of the Gaussians may be left out: floor(N / 1000), which is none at all in the small cases."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from util import TOL, grad_close, log_line, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23


def basis_np(d):
    """The sixteen Y_m of the issue's table at [..., 3] unit vectors -> [..., 16], fp64 (restated here: the bound's magnitude)."""
    x, y, z = (np.asarray(d, np.float64)[..., i] for i in range(3))
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
        1.0925484305920792 * x * y,
        -1.0925484305920792 * y * z,
        0.31539156525252005 * (2 * zz - xx - yy),
        -1.0925484305920792 * x * z,
        0.5462742152960396 * (xx - yy),
        -0.5900435899266435 * y * (3 * xx - yy),
        2.890611442640554 * x * y * z,
        -0.4570457994644658 * y * (4 * zz - xx - yy),
        0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
        -0.4570457994644658 * x * (4 * zz - xx - yy),
        1.445305721320277 * z * (xx - yy),
        -0.5900435899266435 * x * (xx - 3 * yy)], axis=-1)


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def inputs(N, B, M, C, seed, per_view=False):
    """verts ~ U(-1, 1)^3, camera centres on the sphere of radius 3, sh ~ N(0, 0.5^2), upstream gradient ~ N(0, 1); fp32."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (B, N, 3) if per_view else (N, 3)).astype(np.float32)
    c = rng.normal(size=(B, 3))
    centres = (3 * c / np.linalg.norm(c, axis=-1, keepdims=True)).astype(np.float32)
    sh = rng.normal(0, 0.5, (N, M, C)).astype(np.float32)
    g = rng.normal(size=(B * N, C)).astype(np.float32)
    return sh, verts, centres, g


def reference(sh, verts, centres, g, degree, clamp):
    """fp64 definition on the host -> colours, the bound's magnitude, g_sh, g_verts, and the Gaussians kept in the gradient
    comparison."""
    from voge_amd.Aggregation import sh_colors
    a, v = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (sh, verts))
    c = torch.tensor(centres, dtype=torch.float64)
    out = sh_colors(a, v, c, degree=degree, clamp=clamp)
    if out.numel():
        (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    g_sh = np.zeros(sh.shape) if a.grad is None else a.grad.numpy()
    g_v = np.zeros(verts.shape) if v.grad is None else v.grad.numpy()
    N, M, C = sh.shape
    B = centres.shape[0]
    active = M if degree is None else (degree + 1) ** 2
    delta = (verts if verts.ndim == 3 else verts[None]).astype(np.float64) - centres.astype(np.float64)[:, None]
    d = delta / np.linalg.norm(delta, axis=-1, keepdims=True)
    Y = basis_np(d)[..., :active]
    sh64 = sh.astype(np.float64)[:, :active]
    mag = np.einsum("bnm,nmc->bnc", np.abs(Y), np.abs(sh64)) + 0.5
    pre = np.einsum("bnm,nmc->bnc", Y, sh64) + 0.5
    keep = ~(np.abs(pre) < 1e-5).any(axis=(0, 2)) if clamp else np.ones(N, bool)
    return out.detach().numpy(), mag.reshape(B * N, C), g_sh, g_v, keep, pre


def run_kernel(sh, verts, centres, g, degree, clamp):
    from voge_amd.Renderer import sh_to_colors
    a, v = t(sh, rg=True), t(verts, rg=True)
    out = sh_to_colors(a, v, t(centres), degree=degree, clamp=clamp)
    assert type(out.grad_fn).__name__ == "_ShColorsBackward", type(out.grad_fn).__name__      # the kernel, not the fallback
    if out.numel():
        (out * t(g)).sum().backward()
    return out, a, v


def compare(label, sh, verts, centres, g, degree, clamp):
    out, a, v = run_kernel(sh, verts, centres, g, degree, clamp)
    want, mag, g_sh, g_v, keep, pre = reference(sh, verts, centres, g, degree, clamp)
    N = sh.shape[0]
    assert out.shape == want.shape and out.dtype == torch.float32
    if N == 0:
        assert a.grad is None or a.grad.numel() == 0
        return
    ratio = float((np.abs(n(out).astype(np.float64) - want) / (EPS * mag)).max())
    log_line(f"[parity] {label}: colours at most {ratio:.2f} x 2^-23 of their magnitude (bound 16); {int((~keep).sum())} of {N} "
             f"Gaussians near the clamp left out of the gradient comparison; {100 * float((pre < 0).mean()) if clamp else 0.0:.1f} % "
             "of the elements clamped")
    assert ratio <= 16.0, ratio
    assert (~keep).sum() <= N // 1000, ((~keep).sum(), N)      # at most 0.1 % of the Gaussians
    assert keep.any()                                          # (the gradient comparison is never empty)
    grad_close(f"{label} g_sh", n(a.grad)[keep], g_sh[keep], 1e-5)
    gv, wv = (n(v.grad), g_v) if verts.ndim == 2 else (n(v.grad).transpose(1, 0, 2), g_v.transpose(1, 0, 2))
    grad_close(f"{label} g_verts", gv[keep], wv[keep], 1e-5)
    active = sh.shape[1] if degree is None else (degree + 1) ** 2
    assert (n(a.grad)[:, active:] == 0).all()      # written, and exactly zero, above the active degree
    return a, v


# ---- 5. the kernel against the fp64 definition ---------------------------------------------------------------------------------
def test_kernel_vs_fp64_definition_50k_gaussians_8_views(hip_lib):
    """N = 50 000, B = 8, C = 3, M = 16, seed 1: 16 Gaussians (0.032 %) sit near the clamp and 18.7 % of the elements are clamped,
    so the mask is exercised; the fp32 torch definition on these inputs is at 2.5 x 2^-23 and 2.6e-7."""
    sh, verts, centres, g = inputs(50000, 8, 16, 3, seed=1)
    compare("sh 50k x 8 views, degree 3", sh, verts, centres, g, None, True)
    # two backward runs on the same inputs: the same bits
    _, a1, v1 = run_kernel(sh, verts, centres, g, None, True)
    _, a2, v2 = run_kernel(sh, verts, centres, g, None, True)
    assert torch.equal(a1.grad, a2.grad) and torch.equal(v1.grad, v2.grad)
    assert float(a1.grad.abs().max()) > 0 and float(v1.grad.abs().max()) > 0
    # the same with a set of verts per view (g_verts [B, N, 3] is then written view by view)
    shp, vp, cp, gp = inputs(5000, 4, 16, 3, seed=2, per_view=True)
    _, a1, v1 = run_kernel(shp, vp, cp, gp, None, True)
    _, a2, v2 = run_kernel(shp, vp, cp, gp, None, True)
    assert torch.equal(a1.grad, a2.grad) and torch.equal(v1.grad, v2.grad) and v1.grad.shape == (4, 5000, 3)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("M,degree", [(1, 0), (4, 0), (4, 1), (9, 0), (9, 1), (9, 2), (16, 0), (16, 1), (16, 2), (16, 3)])
def test_every_instantiation_and_active_degree(hip_lib, M, C, degree):
    sh, verts, centres, g = inputs(333, 3, M, C, seed=100 * M + 10 * C + degree)
    sh[:, (degree + 1) ** 2:] = np.nan      # the coefficients above the active degree are not read
    compare(f"sh M={M} C={C} degree={degree}", sh, verts, centres, g, degree, True)


@pytest.mark.parametrize("N,B,per_view,clamp", [(700, 1, False, True), (450, 4, True, True), (450, 1, True, True), (1, 5, False, True),
                                                (1, 1, True, False), (0, 3, False, True), (64, 2, False, False), (65, 3, True, False)])
def test_one_view_per_view_verts_tiny_and_empty_inputs_no_clamp(hip_lib, N, B, per_view, clamp):
    sh, verts, centres, g = inputs(N, B, 16, 3, seed=7 + N + B, per_view=per_view)
    compare(f"sh N={N} B={B} per_view={per_view} clamp={clamp}", sh, verts, centres, g, None, clamp)


def test_gaussian_at_a_camera_centre_and_unaligned_coefficients(hip_lib):
    """|delta| = 0: the constant term alone, a finite and zero vertex gradient from that view.  And a coefficient tensor that
    starts in the middle of a 16-byte group (a view into a flat buffer) is copied, not misread."""
    from voge_amd.Renderer import sh_to_colors
    sh, verts, centres, g = inputs(40, 2, 16, 3, seed=5)
    verts[3] = centres[0]
    out, a, v = run_kernel(sh, verts, centres[:1], g[:40], None, False)
    assert torch.equal(out[3], (0.28209479177387814 * a[3, 0] + 0.5).detach())
    assert bool(torch.isfinite(v.grad).all()) and bool((v.grad[3] == 0).all()) and float(v.grad[2].abs().max()) > 0
    flat = torch.zeros(40 * 48 + 1, device=DEV)
    flat[1:] = t(sh).reshape(-1)
    odd = flat[1:].view(40, 16, 3)
    assert odd.data_ptr() % 16 != 0
    assert torch.equal(sh_to_colors(odd, t(verts), t(centres)), sh_to_colors(t(sh), t(verts), t(centres)))


# ---- 6. through the frame ----------------------------------------------------------------------------------------------------------
K = 40
SIZE = (128, 128)


def frame_scene(B=3, N=5000, seed=11):
    from voge_amd import scenes
    from voge_amd.cameras import look_at_view_transform
    verts, sig, _ = scenes.random_gaussians(N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    sh = rng.normal(0, 0.5, (N, 16, 3)).astype(np.float32)
    R, T = look_at_view_transform(dist=[2.7, 3.0, 3.3][:B], elev=[0.0, 25.0, -30.0][:B], azim=[0.0, 120.0, 230.0][:B], device=DEV)
    g = rng.normal(size=(B,) + SIZE + (3,)).astype(np.float32)
    return verts, sig, sh, R, T, g


def frame_renderer(R, T):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    cams = PerspectiveCameras(focal_length=126.0, principal_point=((64.0, 64.0),), image_size=(SIZE,), device=DEV, R=R, T=T)
    return GaussianRenderer(cams, GaussianRenderSettings(image_size=SIZE, max_assign=K, max_point_per_bin=-1)).to(DEV), cams


def white(frag, colors):
    from voge_amd.Renderer import to_white_background
    return to_white_background(frag, colors)


def attr_and_silhouette(frag, colors):
    from voge_amd.Renderer import get_silhouette, interpolate_attr
    rgb = interpolate_attr(frag, colors)
    return rgb * 0.5 + get_silhouette(frag)[..., None]


@pytest.mark.parametrize("form,consumer", [("scalar", white), ("scalar", attr_and_silhouette), ("oriented", white)])
def test_through_the_frame_against_the_torch_definition(hip_lib, form, consumer):
    """to_white_background(renderer(...), sh_to_colors(...)) against the same call with Aggregation.sh_colors (fp32 torch on the
    device) in its place: image and the gradients of sh, verts and the sigmas / scales at util.TOL -- and the [B*N, 3] table
    leaves the fragments on their one-pass route (their composite is still pending when the blend gets them)."""
    from voge_amd.Aggregation import sh_colors
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes
    from voge_amd.Renderer import sh_to_colors
    verts, sig, sh, R, T, g = frame_scene()
    renderer, cams = frame_renderer(R, T)
    centres = cams.get_camera_center()
    got = []
    for colour_fn in (sh_to_colors, sh_colors):
        if form == "oriented":
            rng = np.random.default_rng(3)
            scales = (sig[:, None] * rng.uniform(0.5, 1.5, (len(sig), 3))).astype(np.float32)
            quats = rng.normal(size=(len(sig), 4)).astype(np.float32)
            gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
            shape_param = gm.scales
        else:
            gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
            shape_param = gm.sigmas
        a = t(sh, rg=True)
        frag = renderer(gm, R=R, T=T)
        colors = colour_fn(a, gm.verts, centres)
        assert colors.shape == (3 * len(verts), 3)
        assert frag._lazy is not None      # still deferred: the per-view table did not push the frame off its one-pass route
        img = consumer(frag, colors)
        assert frag._lazy is None
        (img * t(g)).sum().backward()
        got.append((n(img), n(a.grad), n(gm.verts.grad), n(shape_param.grad)))
    (img_k, *grads_k), (img_t, *grads_t) = got
    err = max_rel(img_k, img_t)
    log_line(f"[parity] sh through the frame ({form}, {consumer.__name__}): image max rel err {err:.2e} (tolerance {TOL:.1e})")
    assert err <= TOL and float(np.abs(img_t - 1.0).max()) > 0.3
    for name, gk, gt in zip(("g_sh", "g_verts", "g_sigmas"), grads_k, grads_t):
        assert np.abs(gt).max() > 0
        grad_close(f"sh through the frame ({form}, {consumer.__name__}) {name}", gk, gt, TOL)


# ---- 7. the routes the kernel does not take ------------------------------------------------------------------------------------------
def test_fallback_routes_give_the_same_values(hip_lib):
    from voge_amd.Renderer import sh_to_colors
    # C = 5: the torch definition on the device, against the fp64 definition under the kernel's own bounds
    sh, verts, centres, g = inputs(500, 3, 16, 5, seed=21)
    a, v = t(sh, rg=True), t(verts, rg=True)
    out = sh_to_colors(a, v, t(centres))
    assert type(out.grad_fn).__name__ != "_ShColorsBackward"
    (out * t(g)).sum().backward()
    want, mag, g_sh, g_v, keep, _ = reference(sh, verts, centres, g, None, True)
    assert float((np.abs(n(out).astype(np.float64) - want) / (EPS * mag)).max()) <= 16.0
    assert keep.all()      # (500 Gaussians: 0.1 % is none)
    grad_close("sh fallback C=5 g_sh", n(a.grad)[keep], g_sh[keep], 1e-5)
    grad_close("sh fallback C=5 g_verts", n(v.grad)[keep], g_v[keep], 1e-5)
    # a camera centre that requires grad: the definition's values and gradients, the centre's being minus the sum over the
    # Gaussians of the per-view vertex gradient -- which the KERNEL delivers from per-view verts
    sh, verts, centres, g = inputs(400, 3, 9, 3, seed=22)
    a, v, c = t(sh, rg=True), t(verts, rg=True), t(centres, rg=True)
    out = sh_to_colors(a, v, c)
    assert type(out.grad_fn).__name__ != "_ShColorsBackward"
    (out * t(g)).sum().backward()
    per_view = np.ascontiguousarray(np.broadcast_to(verts[None], (3,) + verts.shape))
    out_k, a_k, v_k = run_kernel(sh, per_view, centres, g, None, True)
    want, mag, *_ = reference(sh, verts, centres, g, None, True)
    for o in (out, out_k):
        assert float((np.abs(n(o).astype(np.float64) - want) / (EPS * mag)).max()) <= 16.0
    grad_close("sh fallback cam_center g_sh", n(a.grad), n(a_k.grad), 1e-5)
    grad_close("sh fallback cam_center g_verts", n(v.grad), n(v_k.grad).sum(0), 1e-5)
    grad_close("sh fallback cam_center g_cam_center", n(c.grad), -n(v_k.grad).sum(1), 1e-5)
    # no channels at all: an empty table from the definition, not an error from the kernel entry
    empty = sh_to_colors(torch.zeros((5, 4, 0), device=DEV), t(verts[:5]), t(centres))
    assert empty.shape == (15, 0)
    # a cameras object in place of the centres
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    R, T = look_at_view_transform(dist=[3.0, 4.0, 5.0], elev=[10.0, -20.0, 40.0], azim=[30.0, 200.0, 300.0], device=DEV)
    cams = PerspectiveCameras(focal_length=100.0, principal_point=((32.0, 32.0),), image_size=((64, 64),), device=DEV, R=R, T=T)
    assert torch.equal(sh_to_colors(t(sh), t(verts), cams), sh_to_colors(t(sh), t(verts), cams.get_camera_center()))


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------------------
def test_ten_captured_steps_replay_to_the_eager_gradients(hip_lib):
    """Ten steps of the frame test's loss + backward in ONE HIP graph (which refuses a host synchronisation, a host-to-device
    copy or a stray allocation inside sh_to_colors), replayed: the gradients of an eager step, as bench.py checks its replay."""
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import sh_to_colors
    verts, sig, sh, R, T, g = frame_scene()
    renderer, cams = frame_renderer(R, T)
    centres = cams.get_camera_center()
    gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
    a, gt = t(sh, rg=True), t(g)
    params = [a, gm.verts, gm.sigmas]

    def step():
        for p in params:
            p.grad = None
        img = white(renderer(gm, R=R, T=T), sh_to_colors(a, gm.verts, centres))
        (img * gt).sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = [p.grad.detach().clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(10):
            step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for name, p, w in zip(("sh", "verts", "sigmas"), params, want):
        assert float(w.abs().max()) > 0
        grad_close(f"sh graph replay {name}", n(p.grad), n(w), 1e-4)


# ---- 9. the demo ---------------------------------------------------------------------------------------------------------------------
def test_view_dependent_colors_demo_converges(hip_lib):
    spec = importlib.util.spec_from_file_location("demo_ViewDependentColors", os.path.join(ROOT, "demo", "ViewDependentColors.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = demo.run(iters=300, log=lambda s: log_line("[demo] ViewDependentColors: " + s))
    assert np.isfinite(out["loss"]).all()
    assert out["loss"][-1] < 5e-2 * out["loss"][0], (out["loss"][0], out["loss"][-1])
