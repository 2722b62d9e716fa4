"""GPU tests of the normals-from-depth extension (Renderer.get_normals, ops._DepthNormals: voge_depth_normals_fwd / _bwd; the
reference and the oracle have neither depth nor normals).

The reference is the DEFINITION, Aggregation.depth_normals, evaluated in fp64 on the host from the SAME fp32 depth values and fp64
rays of the same fp32 camera (tests/test_normals_cpu.py pins it on planes, holes and steps and by gradcheck, builds the inputs used
here, and guarantees that the fp32 evaluation of the definition alone stays within TOL / 4 on every one of them, that the
defined-masks do not depend on the precision and that no sign or edge decision sits near its switch).

Normals:   util.close at util.TOL (1e-4), the defined-mask identical.
Gradients: util.grad_close at util.TOL of the gradient's scale, for an upstream gradient ~ N(0, 1).
High focal length: no constant -- at most 4 x the error the fp32 torch definition shows on the same input."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_normals_cpu import GPU_BAND, GPU_EDGES, GPU_SHAPES, evaluate, gpu_case, high_focal_case, rays_torch
from util import TOL, close, grad_close, log_line, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def cameras_of(case, rg=False):
    from voge_amd.cameras import PerspectiveCameras
    cams = PerspectiveCameras(focal_length=t(case["focal"]), principal_point=t(case["pp"]), T=torch.zeros((2, 3), device=DEV),
                              image_size=((case["H"], case["W"]),), device=DEV)
    cams.R = t(case["R"], rg=rg)      # (a leaf: the constructor would keep a reshaped view of it)
    return cams


def run_kernel(case, edge, view_space=False, rows=None):
    from voge_amd.Renderer import get_normals
    r0, r1 = (0, case["H"]) if rows is None else rows
    d = t(case["depth"][:, r0:r1], rg=True)
    out = get_normals(d, cameras_of(case), rows=rows, edge=edge, view_space=view_space)
    assert type(out.grad_fn).__name__ == "_DepthNormalsBackward", type(out.grad_fn).__name__      # the kernels, not the fallback
    (out * t(case["g"][:, r0:r1])).sum().backward()
    return out, d


_REF = {}


def reference(shape, edge, view_space, rows=None):
    """(case, fp64 normals, fp64 g_depth, defined mask): computed once per case and shared."""
    key = (shape, edge, view_space, rows)
    if key not in _REF:
        case = gpu_case(*shape)
        _REF[key] = (case,) + evaluate(case, edge, torch.float64, rows, view_space)[:3]
    return _REF[key]


def compare(label, out, d, want, g_want, defined):
    got = n(out)
    assert got.shape == want.shape and out.dtype == torch.float32
    assert ((got != 0).any(-1) == defined).all(), f"{label}: the defined-masks differ"
    assert (got[~defined] == 0).all()
    log_line(f"[parity] {label}: normals max err {max_rel(got, want):.2e} (tolerance {TOL:.1e}), {int(defined.sum())} of {defined.size} "
             "pixels defined")
    assert close(got, want).all(), max_rel(got, want)
    grad_close(f"{label} g_depth", n(d.grad), g_want, TOL)
    holes = ~(np.isfinite(n(d)) & (n(d) > 0))
    assert np.isfinite(n(d.grad)).all() and (n(d.grad)[holes] == 0).all()


# ---- 1. the kernels against the fp64 definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("edge", GPU_EDGES)
@pytest.mark.parametrize("view_space", [False, True])
def test_kernels_vs_fp64_definition(hip_lib, shape, edge, view_space):
    case, want, g_want, defined = reference(shape, edge, view_space)
    out, d = run_kernel(case, edge, view_space)
    compare(f"normals {shape[0]}x{shape[1]} edge={edge} view_space={view_space}", out, d, want, g_want, defined)
    if min(shape[:2]) > 2:
        assert defined.mean() > 0.5 and float(d.grad.abs().max()) > 0
    if min(shape[:2]) == 1:
        assert not defined.any() and bool((d.grad == 0).all())


@pytest.mark.parametrize("edge", GPU_EDGES)
@pytest.mark.parametrize("view_space", [False, True])
def test_band_of_rows_vs_definition_and_bitwise_equal_to_the_frame_inside(hip_lib, edge, view_space):
    """rows=(5, 14) of the 19-row image: the definition on the band's own rays (rows outside the band do not exist: its first and
    last row use one-sided differences), and on the band's interior rows 6..12 the very bits of the full frame."""
    shape = GPU_SHAPES[0]
    case, want, g_want, defined = reference(shape, edge, view_space, GPU_BAND)
    out, d = run_kernel(case, edge, view_space, rows=GPU_BAND)
    compare(f"normals band {GPU_BAND} edge={edge} view_space={view_space}", out, d, want, g_want, defined)
    full, _ = run_kernel(case, edge, view_space)
    r0, r1 = GPU_BAND
    assert torch.equal(out[:, 1:-1], full[:, r0 + 1:r1 - 1])
    assert not torch.equal(out[:, 0], full[:, r0])


def test_backward_is_bitwise_reproducible_and_writes_every_element(hip_lib):
    """Two backward runs give the same bits; and the entry itself, handed a g_depth buffer full of NaN, leaves none behind: every
    element is written, zeros at the holes."""
    from voge_amd import ops
    shape = GPU_SHAPES[2]
    case = gpu_case(*shape)
    for edge in GPU_EDGES:
        (_, d1), (_, d2) = run_kernel(case, edge, True), run_kernel(case, edge, True)
        assert torch.equal(d1.grad, d2.grad) and float(d1.grad.abs().max()) > 0
        d, g = t(case["depth"]), t(case["g"])
        R, focal, pp = t(case["R"]), t(case["focal"]), t(case["pp"])
        B, H, W = d.shape
        poisoned = torch.full_like(d, float("nan"))
        rc = hip_lib.voge_depth_normals_bwd(d.data_ptr(), R.data_ptr(), focal.data_ptr(), pp.data_ptr(), g.data_ptr(), B, 0, H, W,
                                            -1.0 if edge is None else edge, 1, poisoned.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isfinite(poisoned).all()) and torch.equal(poisoned, d1.grad)
        holes = ~(torch.isfinite(d) & (d > 0))
        assert int(holes.sum()) > 0 and bool((poisoned[holes] == 0).all())
        out = torch.full((B, H, W, 3), float("nan"), device=DEV)
        rc = hip_lib.voge_depth_normals_fwd(d.data_ptr(), R.data_ptr(), focal.data_ptr(), pp.data_ptr(), B, 0, H, W,
                                            -1.0 if edge is None else edge, 0, out.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isfinite(out).all()) and bool((out[holes] == 0).all())


def test_high_focal_length_against_the_fp32_definitions_own_error(hip_lib):
    """64 x 64, focal length 2000, distance 6, no holes: the tolerance is not a constant.  The kernel's error against the fp64
    definition may be at most 4 x the error of the fp32 torch definition (fp32 rays, fp32 arithmetic, on the host) on the same
    input -- the 4 x allows for a different order of operations; both numbers are logged."""
    case = high_focal_case()
    want, g_want, defined, _ = evaluate(case, None, torch.float64)
    n32, g32, _, _ = evaluate(case, None, torch.float32)
    out, d = run_kernel(case, None)
    assert defined.all() and bool((out != 0).any(-1).all())
    err_k, err_t = float(np.abs(n(out) - want).max()), float(np.abs(n32 - want).max())
    scale = float(np.abs(g_want).max())
    gerr_k, gerr_t = float(np.abs(n(d.grad) - g_want).max()) / scale, float(np.abs(g32 - g_want).max()) / scale
    log_line(f"[parity] normals high focal (2000, 64x64, distance 6): kernel {err_k:.2e} / fp32 torch definition {err_t:.2e} against fp64; "
             f"g_depth {gerr_k:.2e} / {gerr_t:.2e} of scale")
    assert err_t > 0 and err_k <= 4 * err_t, (err_k, err_t)
    assert gerr_k <= 4 * gerr_t, (gerr_k, gerr_t)


# ---- 2. the routes the kernels do not take ---------------------------------------------------------------------------------------
def test_fallbacks_give_the_same_values_and_reach_the_camera(hip_lib):
    from voge_amd.Renderer import get_normals
    from voge_amd.cameras import pixel_rays
    shape = GPU_SHAPES[1]
    for edge in GPU_EDGES:
        for view_space in (False, True):
            case, want, g_want, defined = reference(shape, edge, view_space)
            # a camera whose rotation wants a gradient: pixel_rays + the definition
            cams = cameras_of(case, rg=True)
            d = t(case["depth"], rg=True)
            out = get_normals(d, cams, edge=edge, view_space=view_space)
            assert type(out.grad_fn).__name__ != "_DepthNormalsBackward"
            (out * t(case["g"])).sum().backward()
            compare(f"normals fallback (R requires grad) edge={edge} view_space={view_space}", out, d, want, g_want, defined)
            assert bool(torch.isfinite(cams.R.grad).all()) and float(cams.R.grad.abs().max()) > 0
    # a tensor of rays in place of the cameras: the same values as the camera route
    case, want, g_want, defined = reference(shape, 0.1, False)
    rays = pixel_rays(cameras_of(case), (case["H"], case["W"]))[0]
    d = t(case["depth"], rg=True)
    out = get_normals(d, rays, edge=0.1)
    (out * t(case["g"])).sum().backward()
    compare("normals fallback (ray tensor)", out, d, want, g_want, defined)
    kernel, _ = run_kernel(case, 0.1)
    assert close(n(out), n(kernel)).all()
    with pytest.raises(ValueError, match="view_space"):
        get_normals(d, rays, view_space=True)
    # fp64 depth on the device, and a single [h, W] map with a one-camera object
    out64 = get_normals(t(case["depth"], torch.float64), cameras_of(case), edge=0.1)
    assert out64.dtype == torch.float64 and close(n(out64), want).all()
    from voge_amd.cameras import PerspectiveCameras
    one = PerspectiveCameras(focal_length=t(case["focal"][:1]), principal_point=t(case["pp"][:1]), R=t(case["R"][:1]),
                             T=torch.zeros((1, 3), device=DEV), device=DEV)
    single = get_normals(t(case["depth"][0]), one, edge=0.1)
    assert single.shape == (case["H"], case["W"], 3) and torch.equal(single, kernel[0])


# ---- 3. through the renderer -----------------------------------------------------------------------------------------------------
def render_scene():
    from voge_amd import scenes
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    verts, sig, _ = scenes.random_gaussians(500, seed=4, r_lo=0.1, r_hi=0.2)
    R, T = look_at_view_transform(dist=3.2, elev=15.0, azim=40.0, device=DEV)
    cams = PerspectiveCameras(focal_length=44.0, principal_point=((24.0, 24.0),), image_size=((48, 48),), device=DEV, R=R, T=T)
    renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(48, 48), max_assign=16, max_point_per_bin=-1)).to(DEV)
    gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
    g = torch.randn((1, 48, 48, 3), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    return renderer, cams, gm, R, T, g


def test_end_to_end_gradients_reach_the_gaussians(hip_lib):
    """renderer -> get_depth -> get_normals -> loss.backward() on 500 Gaussians at 48 x 48: finite, non-zero gradients on verts and
    sigmas."""
    from voge_amd.Renderer import get_depth, get_normals
    renderer, cams, gm, R, T, g = render_scene()
    depth = get_depth(renderer(gm, R=R, T=T), background=0.0)
    normals = get_normals(depth, cams, edge=0.1)
    assert type(normals.grad_fn).__name__ == "_DepthNormalsBackward"
    assert float((normals != 0).any(-1).float().mean()) > 0.1
    (normals * g).sum().backward()
    for p in (gm.verts, gm.sigmas):
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


def test_captured_step_replays_to_the_eager_result(hip_lib):
    """The same step captured into a HIP graph (which refuses a host synchronisation, a host-to-device copy or a stray allocation
    inside get_normals) and replayed: the eager run's normals, bit for bit, and its gradients."""
    from voge_amd.Renderer import get_depth, get_normals
    renderer, cams, gm, R, T, g = render_scene()
    params = [gm.verts, gm.sigmas]

    def step():
        for p in params:
            p.grad = None
        normals = get_normals(get_depth(renderer(gm, R=R, T=T), background=0.0), cams, edge=0.1, view_space=True)
        (normals * g).sum().backward()
        return normals
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_n, want = eager.detach().clone(), [p.grad.detach().clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, want_n) and float(want_n.abs().max()) > 0
    for name, p, w in zip(("verts", "sigmas"), params, want):
        assert float(w.abs().max()) > 0
        grad_close(f"normals graph replay {name}", n(p.grad), n(w), 2e-4)      # (the trace's atomics: order of the sums)


# ---- 4. the demo --------------------------------------------------------------------------------------------------------------------
def test_normals_from_depth_demo_runs_and_writes_its_files(hip_lib, tmp_path):
    spec = importlib.util.spec_from_file_location("demo_NormalsFromDepth", os.path.join(ROOT, "demo", "NormalsFromDepth.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    prefix = os.path.join(str(tmp_path), "bunny_normals")
    out = demo.run(out=prefix, log=lambda s: log_line("[demo] NormalsFromDepth: " + s))
    img = np.load(prefix + ".npy")
    assert img.shape == (256, 256, 3) and np.isfinite(img).all() and img.max() > 0.3
    assert out["defined"] > 5000 and np.isfinite(out["median_angle_deg"])      # (the angle is recorded, not judged)
    norms = out["normals"].norm(dim=-1)
    assert bool(((norms == 0) | ((norms - 1).abs() < 1e-5)).all())
    try:
        import PIL      # noqa: F401
        assert os.path.exists(prefix + ".png")
    except ImportError:
        pass
