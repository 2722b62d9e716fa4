"""GPU tests of the per-view normals of oriented Gaussians (Renderer.gaussian_normals, ops._GaussNormals:
voge_gauss_normals_fwd / _bwd; an extension, the reference and the oracle have none) and of get_rendered_normals.

The reference is the DEFINITION, Aggregation.gaussian_normals, evaluated in fp64 on the host from the fp32-rounded inputs
(tests/test_gauss_normals_cpu.py pins it against an independent numpy restatement and central differences).

Values:    |got - ref| <= 16 * 2^-23 per component, absolute (the components of a unit vector are <= 1): the unit quaternion's
           components carry about 3 roundings each and a matrix entry adds about 6 roundings of terms <= 2.  Derived, not tuned.
Gradients: util.grad_close at 1e-5 of the gradient's scale (the bar of sh_to_colors: an fp64 chain on fp32 inputs, the views
           summed in another order).
Sign mask: the facing sign is a discontinuity.  A Gaussian whose fp64 |n0 . delta| / |delta| is below 1e-5 in any view is left
           out of the value AND the gradient comparison (the fp32 dot product is good to about 1e-6 there); at most
           floor(N / 1000) Gaussians may be left out -- none at all in the small cases -- and the comparison is never empty.
Per-view orientations: the shared (scales, quats) set tiled B times, the quaternions of view b then multiplied by 1 + b / 2 (the
           same rotation, another |q|: the gradient differs by view, as does the upstream gradient) and perturbed by
           0.3 * N(0, 1) drawn AFTER the five draws the shared cases make."""
import numpy as np
import pytest
import torch

from test_gauss_normals_cpu import edge_cases
from util import TOL, grad_close, log_line, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
NODE = "_GaussNormalsBackward"


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def inputs(N, B, seed, per_view_verts=False, per_view_orient=False):
    """verts ~ U(-1, 1), centres on the sphere of radius 3, scales ~ U(0.5, 2), quats = N(0, I) * U(0.1, 10), upstream gradient
    ~ N(0, 1), drawn in that order; fp32."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (B, N, 3) if per_view_verts else (N, 3)).astype(np.float32)
    c = rng.normal(size=(B, 3))
    centres = (3 * c / np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), 1e-300)).astype(np.float32)
    scales = rng.uniform(0.5, 2, (N, 3)).astype(np.float32)
    quats = (rng.normal(size=(N, 4)) * rng.uniform(0.1, 10, (N, 1))).astype(np.float32)
    g = rng.normal(size=(B * N, 3)).astype(np.float32)
    if per_view_orient:
        scales = np.ascontiguousarray(np.broadcast_to(scales, (B, N, 3)))
        quats = (quats[None] * (1 + 0.5 * np.arange(B))[:, None, None] + 0.3 * rng.normal(size=(B, N, 4))).astype(np.float32)
    return scales, quats, verts, centres, g


REFS = {}


def reference(key, scales, quats, verts, centres, g, inverse):
    """fp64 definition on the host -> (out [B*N,3], g_quats, keep [N]); computed once per case and left unchanged."""
    if key in REFS:
        return REFS[key]
    from voge_amd.Aggregation import gaussian_normals
    q = torch.tensor(quats, dtype=torch.float64, requires_grad=True)
    s, v, c = (torch.tensor(x, dtype=torch.float64) for x in (scales, verts, centres))
    out = gaussian_normals(s, q, v, c, inverse_sigma=inverse)
    if out.numel():
        (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    g_q = np.zeros(quats.shape) if q.grad is None else q.grad.numpy()
    B, N = centres.shape[0], scales.shape[-2]
    want = out.detach().numpy()
    delta = (verts if verts.ndim == 3 else verts[None]).astype(np.float64) - centres.astype(np.float64)[:, None]
    cos = np.abs((want.reshape(B, N, 3) * delta).sum(-1)) / np.linalg.norm(delta, axis=-1)
    keep = ~(cos < 1e-5).any(axis=0) if B * N else np.ones(N, bool)
    REFS[key] = (want, g_q, keep, float(cos.min()) if B * N else float("nan"))
    return REFS[key]


def run_kernel(scales, quats, verts, centres, g, inverse):
    from voge_amd.Renderer import gaussian_normals
    q = t(quats, rg=True)
    s, v, c = t(scales, rg=True), t(verts, rg=True), t(centres, rg=True)      # (requires_grad on them is fine: they get none)
    out = gaussian_normals(s, q, v, c, inverse_sigma=inverse)
    assert type(out.grad_fn).__name__ == NODE, type(out.grad_fn).__name__      # the kernel, not the fallback
    if out.numel():
        (out * t(g)).sum().backward()
        assert s.grad is None and v.grad is None and c.grad is None
    return out, q


def compare(label, N, B, seed, inverse=False, per_view_verts=False, per_view_orient=False):
    scales, quats, verts, centres, g = inputs(N, B, seed, per_view_verts, per_view_orient)
    out, q = run_kernel(scales, quats, verts, centres, g, inverse)
    want, g_q, keep, cos_min = reference((N, B, seed, inverse, per_view_verts, per_view_orient), scales, quats, verts, centres, g,
                                         inverse)
    assert out.shape == want.shape == (B * N, 3) and out.dtype == torch.float32
    if B * N == 0:
        assert q.grad is None or not q.grad.any()
        return
    got = n(out).astype(np.float64).reshape(B, N, 3)
    ref = want.reshape(B, N, 3)
    ratio = float((np.abs(got - ref)[:, keep] / EPS).max())
    log_line(f"[parity] {label}: normals at most {ratio:.2f} x 2^-23 off (bound 16); {int((~keep).sum())} of {N} Gaussians near "
             f"the sign's discontinuity left out (cap {N // 1000}); smallest |cos| {cos_min:.1e}")
    assert (~keep).sum() <= N // 1000, ((~keep).sum(), N)
    assert keep.any()
    assert ratio <= 16.0, ratio
    gq, wq = n(q.grad), g_q
    assert gq.shape == quats.shape
    if per_view_orient:
        gq, wq = gq.transpose(1, 0, 2), wq.transpose(1, 0, 2)
    grad_close(f"{label} g_quats", gq[keep], wq[keep], 1e-5)
    assert np.isfinite(n(q.grad)).all() and np.abs(n(q.grad)).max() > 0
    # orthogonal to quats: |g . q| against |g| |q| at fp32
    dot = np.abs((n(q.grad).astype(np.float64) * quats).sum(-1))
    assert (dot <= 1e-5 * np.linalg.norm(n(q.grad), axis=-1) * np.linalg.norm(quats, axis=-1) + 1e-30).all()
    return q


# ---- 1. the kernel against the fp64 definition ---------------------------------------------------------------------------------
def test_kernel_vs_fp64_definition_50k_gaussians_8_views(hip_lib):
    """N = 50 000, B = 8, seed 1: 9 Gaussians sit within 1e-5 of the sign's discontinuity (cap 50); about half of the (view,
    Gaussian) pairs are flipped.  Two backward runs give the same bits."""
    q1 = compare("normals 50k x 8 views", 50000, 8, 1)
    scales, quats, verts, centres, g = inputs(50000, 8, 1)
    out, q2 = run_kernel(scales, quats, verts, centres, g, False)
    assert torch.equal(q1.grad, q2.grad)
    rows = n(out).reshape(8, 50000, 3)
    differs = float((np.abs(rows - rows[:1]).max(-1) > 0.5).any(0).mean())      # Gaussians seen from both sides by the 8 views
    log_line(f"[parity] normals 50k x 8 views: {100 * differs:.1f} % of the Gaussians are seen from both sides")
    assert differs > 0.3


@pytest.mark.parametrize("N,B,seed,inverse,per_view_verts,per_view_orient", [
    (1, 1, 3, False, False, False),          # one thread
    (67, 3, 2, False, True, False),          # a partial wave, per-view verts
    (257, 5, 5, False, False, False),        # one thread past a workgroup
    (1031, 2, 4, True, False, False),        # inverse_sigma
    (67, 3, 2, False, False, True),          # per-view orientations: g_quats per view, not summed
    (67, 3, 6, True, True, True),            # everything per view, inverse_sigma, 201 threads
    (0, 3, 7, False, False, False), (5, 0, 7, False, False, False), (0, 2, 7, False, True, True)])      # empty: no launch
def test_smallest_shapes(hip_lib, N, B, seed, inverse, per_view_verts, per_view_orient):
    compare(f"normals N={N} B={B} inverse={inverse} verts/view={per_view_verts} orient/view={per_view_orient}", N, B, seed, inverse,
            per_view_verts, per_view_orient)


def test_two_backward_runs_per_view_give_the_same_bits(hip_lib):
    args = inputs(300, 4, 12, True, True)
    _, q1 = run_kernel(*args, False)
    _, q2 = run_kernel(*args, False)
    assert torch.equal(q1.grad, q2.grad) and q1.grad.shape == (4, 300, 4)


# ---- 2. the named edge cases through the kernel --------------------------------------------------------------------------------
def test_named_edge_cases_through_the_kernel(hip_lib):
    """tests/test_gauss_normals_cpu.py's table, one call each: the expected normal exactly, the definition's (fp32, host) values
    exactly, its gradient at 1e-6, an exactly zero gradient for a quaternion without a usable fp32 norm."""
    from voge_amd.Aggregation import gaussian_normals as definition
    from voge_amd.Renderer import gaussian_normals
    up = [[0.3, -0.7, 1.1]]
    for name, s, q, v, c, inverse, want, zero_grad in edge_cases():
        qk = t([q], rg=True)
        out = gaussian_normals(t([s]), qk, t([v]), t([c]), inverse_sigma=inverse)
        assert type(out.grad_fn).__name__ == NODE
        (out * t(up)).sum().backward()
        qd = torch.tensor([q], dtype=torch.float32, requires_grad=True)
        ref = definition(torch.tensor([s]), qd, torch.tensor([v]), torch.tensor([c]), inverse_sigma=inverse)
        (ref * torch.tensor(up)).sum().backward()
        assert n(out).tolist() == [[float(x) for x in want]], (name, n(out))
        assert np.array_equal(n(out), ref.detach().numpy()), name
        g = n(qk.grad)
        assert np.isfinite(g).all(), (name, g)
        if zero_grad:
            assert (g == 0).all(), (name, g)
        else:
            assert np.abs(g - qd.grad.numpy()).max() <= 1e-6 and np.abs(g).max() > 0, (name, g, qd.grad)


def test_every_element_of_g_quats_is_written(hip_lib):
    """The ABI called directly on a NaN-filled g_quats: shared and per-view orientations, bad quaternions among good ones."""
    from voge_amd import _lib, ops
    lib = _lib.load()
    for per_view in (False, True):
        scales, quats, verts, centres, g = inputs(70, 3, 15, False, per_view)
        bad = np.array([[0, 0, 0, 0], [np.nan, 1, 0, 0], [1, np.inf, 0, 0], [1e20, 1e20, 0, 0], [1e-30, 0, 1e-30, 0]], np.float32)
        quats.reshape(-1, 4)[3:8] = bad
        s, q, v, c, go = t(scales), t(quats), t(verts), t(centres), t(g)
        gq = torch.full_like(q, float("nan"))
        out = torch.full((3 * 70, 3), float("nan"), device=DEV)
        flags = (int(not per_view), 1, 0)
        assert lib.voge_gauss_normals_fwd(s.data_ptr(), q.data_ptr(), v.data_ptr(), c.data_ptr(), 3, 70, *flags, out.data_ptr(),
                                          ops._stream()) == 0
        assert lib.voge_gauss_normals_bwd(s.data_ptr(), q.data_ptr(), v.data_ptr(), c.data_ptr(), go.data_ptr(), 3, 70, *flags,
                                          gq.data_ptr(), ops._stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gq).all())
        assert not n(gq).reshape(-1, 4)[3:8].any() and np.abs(n(gq).reshape(-1, 4)[8:]).min(-1).max() > 0
        # the bad rows: the identity's column, exactly
        k = np.argmax(scales.reshape(-1, 3)[3:8], axis=-1)
        assert np.array_equal(np.abs(n(out))[3:8], np.eye(3, dtype=np.float32)[k])
        # nothing is launched or written for an empty batch
        gq.fill_(float("nan"))
        assert lib.voge_gauss_normals_bwd(s.data_ptr(), q.data_ptr(), v.data_ptr(), c.data_ptr(), go.data_ptr(), 0, 70, *flags,
                                          gq.data_ptr(), ops._stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(gq).all())


def test_quats_at_a_4_byte_odd_offset(hip_lib):
    """A quats view that starts 4 bytes into a flat buffer is off the 16-byte boundary of the kernels' vector access: they read
    it (and write its gradient, when that is unaligned too) element by element -- no copy -- and give the same bits."""
    from voge_amd import _lib, ops
    from voge_amd.Renderer import gaussian_normals
    scales, quats, verts, centres, g = inputs(333, 3, 8)
    flat = torch.zeros(333 * 4 + 1, device=DEV)
    flat[1:] = t(quats).reshape(-1)
    odd = flat[1:].view(333, 4).requires_grad_(True)
    assert odd.data_ptr() % 16 == 4
    q = t(quats, rg=True)
    a = gaussian_normals(t(scales), odd, t(verts), t(centres))
    b = gaussian_normals(t(scales), q, t(verts), t(centres))
    assert type(a.grad_fn).__name__ == NODE and torch.equal(a, b)
    (a * t(g)).sum().backward()
    (b * t(g)).sum().backward()
    assert torch.equal(odd.grad, q.grad)
    # the ABI with an unaligned g_quats as well
    lib = _lib.load()
    gflat = torch.full((333 * 4 + 1,), float("nan"), device=DEV)
    s, v, c, go = t(scales), t(verts), t(centres), t(g)
    assert lib.voge_gauss_normals_bwd(s.data_ptr(), odd.data_ptr(), v.data_ptr(), c.data_ptr(), go.data_ptr(), 3, 333, 1, 1, 0,
                                      gflat[1:].data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gflat[1:].view(333, 4), q.grad) and bool(torch.isnan(gflat[0]))


# ---- 3. the routes the kernel does not take ------------------------------------------------------------------------------------
def test_fp64_and_mixed_devices_take_the_definition(hip_lib):
    from voge_amd import _lib
    from voge_amd.Renderer import gaussian_normals
    scales, quats, verts, centres, g = inputs(200, 3, 21)
    q = t(quats, torch.float64, rg=True)
    out = gaussian_normals(t(scales, torch.float64), q, t(verts, torch.float64), t(centres, torch.float64))
    assert out.dtype == torch.float64 and type(out.grad_fn).__name__ != NODE
    want, g_q, keep, _ = reference((200, 3, 21, False, False, False), scales, quats, verts, centres, g, False)
    assert keep.all() and np.abs(n(out) - want).max() <= 1e-13
    (out * t(g, torch.float64)).sum().backward()
    grad_close("normals fp64 route g_quats", n(q.grad), g_q, 1e-12)
    # one fp64 tensor among fp32 ones: still the definition
    mixed = gaussian_normals(t(scales), t(quats, rg=True), t(verts, torch.float64), t(centres))
    assert type(mixed.grad_fn).__name__ != NODE
    # tensors on different devices: the definition, whose torch arithmetic refuses them -- not an error of the HIP entry
    with pytest.raises(RuntimeError) as e:
        gaussian_normals(t(scales), t(quats), torch.tensor(verts), t(centres))
    assert not isinstance(e.value, _lib.VogeHipError)
    # a cameras object in place of the centres
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    R, T = look_at_view_transform(dist=[3.0, 4.0, 5.0], elev=[10.0, -20.0, 40.0], azim=[30.0, 200.0, 300.0], device=DEV)
    cams = PerspectiveCameras(focal_length=100.0, principal_point=((32.0, 32.0),), image_size=((64, 64),), device=DEV, R=R, T=T)
    assert torch.equal(gaussian_normals(t(scales), t(quats), t(verts), cams),
                       gaussian_normals(t(scales), t(quats), t(verts), cams.get_camera_center()))


# ---- 4. through the renderer ---------------------------------------------------------------------------------------------------
K = 8
SIZE = (64, 64)


def frame_scene(N=200, B=2, seed=31):
    """~200 discs in the unit cube, five times thinner along their largest scale, two views."""
    from voge_amd.cameras import look_at_view_transform
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-0.8, 0.8, (N, 3)).astype(np.float32)
    r = rng.uniform(0.12, 0.2, N)
    s = 2 * np.log(1 / 0.6) / (r * r)
    scales = (s[:, None] * np.array([25.0, 1.0, 1.0]) * rng.uniform(0.8, 1.25, (N, 3))).astype(np.float32)
    quats = (rng.normal(size=(N, 4)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    R, T = look_at_view_transform(dist=[3.0, 3.4][:B], elev=[10.0, -25.0][:B], azim=[20.0, 160.0][:B], device=DEV)
    g = rng.normal(size=(B,) + SIZE + (3,)).astype(np.float32)
    return verts, scales, quats, R, T, g


def frame_renderer(R, T):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    cams = PerspectiveCameras(focal_length=80.0, principal_point=((32.0, 32.0),), image_size=(SIZE,), device=DEV, R=R, T=T)
    return GaussianRenderer(cams, GaussianRenderSettings(image_size=SIZE, max_assign=K, max_point_per_bin=-1)).to(DEV), cams


def test_through_the_frame_against_the_torch_definition(hip_lib):
    """interpolate_attr(renderer(...), gaussian_normals(...)) against the same call with Aggregation.gaussian_normals (fp32 torch
    on the device) in its place: the map and the gradient at quats -- through the table AND through the trace -- at util.TOL; the
    [B*N, 3] table leaves the fragments on their one-pass route."""
    from voge_amd.Aggregation import gaussian_normals as definition
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import gaussian_normals, interpolate_attr
    verts, scales, quats, R, T, g = frame_scene()
    renderer, cams = frame_renderer(R, T)
    centres = cams.get_camera_center()
    got = []
    for fn in (gaussian_normals, definition):
        gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
        frag = renderer(gm, R=R, T=T)
        table = fn(gm.scales, gm.quats, gm.verts, centres)
        assert table.shape == (2 * len(verts), 3) and (type(table.grad_fn).__name__ == NODE) == (fn is gaussian_normals)
        assert frag._lazy is not None
        img = interpolate_attr(frag, table)
        assert frag._lazy is None and img.shape == (2,) + SIZE + (3,)
        (img * t(g)).sum().backward()
        got.append((n(img), n(gm.quats.grad), n(table)))
    (img_k, gq_k, tab_k), (img_t, gq_t, tab_t) = got
    assert np.abs(tab_k - tab_t).max() <= 16 * EPS      # (no sign disagreement between the fp32 definition and the kernel here)
    err = max_rel(img_k, img_t)
    log_line(f"[parity] normals through the frame: map max rel err {err:.2e} (tolerance {TOL:.1e})")
    assert err <= TOL and float(np.abs(img_t).max()) > 0.3
    assert np.abs(gq_t).max() > 0
    grad_close("normals through the frame g_quats", gq_k, gq_t, TOL)


def test_one_shared_orientation_renders_as_that_normal(hip_lib):
    """Every Gaussian with the SAME scales and quaternion: sum_k w_k n / |sum_k w_k n| = n whatever the weights, so
    get_rendered_normals gives the facing normal of the view at 1e-5 on every pixel with a hit, zeros elsewhere."""
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import gaussian_normals, get_rendered_normals, get_silhouette
    verts, scales, quats, R, T, g = frame_scene()
    # axis 2 the thin one, turned 15 degrees about x: n0 = (0, -sin 15, cos 15), within 35 degrees of both view axes and
    # |n0 . c| > 2.4 against |n0 . v| < 1 -- every Gaussian shows a view the same side
    scales[:] = scales[0, 1] * np.array([1.0, 1.0, 25.0], np.float32)
    quats[:] = 2.5 * np.array([np.cos(np.deg2rad(7.5)), np.sin(np.deg2rad(7.5)), 0.0, 0.0], np.float32)
    renderer, cams = frame_renderer(R, T)
    centres = cams.get_camera_center()
    gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
    table = gaussian_normals(gm.scales, gm.quats, gm.verts, centres)
    tab = n(table).reshape(2, -1, 3)
    frag = renderer(gm, R=R, T=T)
    out = n(get_rendered_normals(frag, table, normalize=True))
    hit = n(frag.valid_num) > 0
    assert hit.any() and not out[~hit].any()
    for b in range(2):
        assert np.abs(tab[b] - tab[b, :1]).max() == 0      # one orientation, one side
        lit = hit[b] & (out[b] != 0).any(-1)               # (a hit whose every weight underflowed has |M| = 0 and gives zeros)
        assert lit.sum() > 500 and lit.sum() >= 0.99 * hit[b].sum() and np.abs(out[b][lit] - tab[b, 0]).max() <= 1e-5
    assert np.abs(tab[0, 0] + tab[1, 0]).max() == 0        # the two views look at opposite sides
    assert float(get_silhouette(frag).max()) > 0.5


def test_the_consistency_step_captures_into_a_hip_graph(hip_lib):
    """table + render + depth + depth normals + rendered normals + the consistency term + backward in ONE HIP graph (which refuses
    a host synchronisation, a host-to-device copy or a stray allocation inside gaussian_normals), replayed: the eager image and
    gradient."""
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import gaussian_normals, get_depth, get_normals, get_rendered_normals
    verts, scales, quats, R, T, g = frame_scene()
    renderer, cams = frame_renderer(R, T)
    centres = cams.get_camera_center()
    gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
    gt = t(g)

    def step():
        gm.quats.grad = None
        table = gaussian_normals(gm.scales, gm.quats, gm.verts, centres)
        frag = renderer(gm, R=R, T=T)
        n_depth = get_normals(get_depth(frag), cams)
        n_hat = get_rendered_normals(frag, table)
        both = ((n_hat != 0).any(-1) & (n_depth != 0).any(-1)).float()      # (a mask product, not a boolean gather: static shapes)
        ((1 - (n_hat * n_depth).sum(-1)) * both).sum().backward()
        return n_hat
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            img_e = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_img, want = img_e.detach().clone(), gm.quats.grad.detach().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img_g = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(img_g, want_img) and float(want_img.abs().max()) > 0.5
    assert float(want.abs().max()) > 0
    grad_close("normals graph replay g_quats", n(gm.quats.grad), n(want), TOL)
