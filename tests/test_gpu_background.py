"""to_colored_background with any background that broadcasts to the image (Renderer.py:162-171 under torch broadcasting):
a background image [B,H,W,C] or [H,W,C] (a permuted CHW photograph included), a colour per view [B,1,1,C], a grey level, odd
broadcasts such as [W,C], and a background that requires grad -- through interpolate_attr + get_silhouette and the blend
node of voge_blend_bg_fwd / _bwd.

What is asserted:
  * against the fp64 oracle chain (oracle.torch_ref: trace_dense -> aggregation -> merge_final -> to_colored_background with the
    SAME broadcast background, differentiated by autograd): image and the gradients of colours, verts, sigmas and background;
  * against the port's own composed route (interpolate_attr + get_silhouette + the reference's expression in torch) on larger
    frames, over background shapes, channel counts, thr, sigma forms, K above the fused merge, aggregation()-built fragments
    and a row band;
  * a learnable colour starting at white: the reference's gradient (half of it at uncovered pixels), the same bits on every
    backward, and an Adam loop that recovers an unknown colour;
  * the route replayed from a captured graph equals eager; plain colours keep their routes and bits; enlarging backgrounds
    raise ValueError.
"""
import math

import numpy as np
import pytest
import torch

from oracle import camera_np
from util import TOL, grad_close, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def _scene(N, seed, kind=0):
    from voge_amd import scenes
    verts, sig, cols = scenes.random_gaussians(N, seed=seed, anisotropic={0: False, 1: "diag", 2: True}[kind], r_lo=0.04, r_hi=0.09)
    return verts, sig, cols


def _views(B, seed):
    rng = np.random.default_rng(seed)
    return camera_np.look_at_view_transform(list(rng.uniform(3.0, 3.6, B)), list(rng.uniform(-30, 30, B)), list(rng.uniform(-180, 180, B)))


def _camera(size):
    H, W = size
    return float(1.1 * max(H, W)), (W / 2.0 + 0.25, H / 2.0 - 0.5)


def _renderer(size, K):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    focal, pp = _camera(size)
    cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=(size,), device=DEV)
    return GaussianRenderer(cams, GaussianRenderSettings(image_size=size, max_assign=K, max_point_per_bin=-1)).to(DEV)


def _frag(scene, R, T, size, K, rows=None, route="renderer", grad=True):
    """Fragments of the scene through the public API, and the leaves to differentiate (verts, sigmas, colours)."""
    from voge_amd.Meshes import GaussianMeshes
    verts, sig, cols = scene
    gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
    if grad:
        gm.verts.requires_grad_(True)
        gm.sigmas.requires_grad_(True)
    B = np.asarray(R).reshape(-1, 3, 3).shape[0]
    colors = t(np.tile(cols, (B, 1)) if B > 1 else cols, rg=grad)
    if route == "aggregation":      # the reference's own split: ray_tracing + aggregation (RayTracing.py:12-30, Aggregation.py:82-107)
        from voge_amd import RayTracing
        from voge_amd.Aggregation import aggregation
        from voge_amd.Renderer import Fragments
        from voge_amd.cameras import pixel_rays
        renderer = _renderer(size, K)
        cams = renderer.cameras
        cams.R, cams.T = t(R), t(T)
        rays, origin = pixel_rays(cams, size)
        isg = (2 * gm.sigmas)[:, None, None] * torch.eye(3, device=DEV)[None]
        isg = isg[None].expand(B, -1, -1, -1).contiguous()
        sel = RayTracing.ray_tracing(cams, gm.verts[None] - origin[:, None], isg, rays, size, thr=0.01, n_assign=K, max_points_per_bin=-1)
        w, idx, vn, hl = aggregation(sel[0], sel[2], sel[1], sel[3], 1.0)
        return Fragments(w, idx, vn, hl), gm, colors
    frag = _renderer(size, K)(gm, R=t(R), T=t(T), **({} if rows is None else dict(rows=rows)))
    return frag, gm, colors


def _composed(frag, colors, bg, thr=-1.0):
    """The port's own composed route: interpolate_attr + get_silhouette + Renderer.py:167-171 in torch."""
    from voge_amd.Renderer import get_silhouette, interpolate_attr
    masks = get_silhouette(frag).unsqueeze(-1)
    if thr > 0:
        masks = (masks > thr).type_as(masks)
    rgb = interpolate_attr(frag, colors)
    return torch.min(rgb + torch.ones_like(rgb) * (1 - masks) * bg, torch.ones_like(rgb))


def _off_tie(rgb_and_mask, bg, g):
    """g with the elements whose x = rgb + (1 - m) bg lies within 1e-6 of 1 but not on it zeroed: there one rounding more
    or less (an fma against a multiply and an add, fp32 against fp64) moves min's gradient between 1, 1/2 and 0."""
    rgb, m = rgb_and_mask
    x = (rgb + (1 - m)[..., None] * bg).detach().to(g.dtype)
    return g * ~(((x - 1).abs() <= 1e-6) & (x != 1))


# ---------------------------------------------------------------------------------------------------- 1. the fp64 oracle
def _oracle(scene, R, T, size, K, bg):
    """oracle.torch_ref's chain in fp64 on the CPU, per view, with the broadcast background bg (a float64 leaf)."""
    from oracle import torch_ref
    verts, sig, cols = (torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in scene)
    focal, pp = _camera(size)
    rays, origin = camera_np.pixel_rays(R, T, focal, pp, size)
    B = rays.shape[0]
    thr_act = -math.log(0.01 + 1 / 1e10)
    isg = (2 * sig)[:, None, None] * torch.eye(3, dtype=torch.float64)[None]
    rgbs, ws, idxs = [], [], []
    for b in range(B):
        mus = verts - torch.tensor(origin[b], dtype=torch.float64)[None]
        idx, ln, act, dsd = torch_ref.trace_dense(mus, isg, torch.tensor(rays[b].reshape(-1, 3), dtype=torch.float64), K, thr_act)
        w, vn = torch_ref.aggregation(idx, act, ln, dsd)
        rgbs.append(torch_ref.merge_final(cols, w, vn, idx).reshape(size + (3,)))
        ws.append(w.reshape(size + (K,)))
        idx = idx.reshape(size + (K,)).numpy()
        idxs.append(np.where(idx >= 0, idx + b * verts.shape[0], idx))      # (view b's rows of the tiled colour table)
    rgb, w = torch.stack(rgbs), torch.stack(ws)
    img = torch_ref.to_colored_background(rgb, w, bg)
    return img, np.stack(idxs), (cols, verts, sig), (rgb.detach(), w.detach().sum(-1))


@pytest.mark.parametrize("bg_kind,B", [("image", 2), ("hw1", 2), ("colour", 1), ("per_view", 2), ("grey", 1)])
def test_against_the_fp64_oracle(hip_lib, bg_kind, B):
    from voge_amd.Renderer import to_colored_background
    size, K = (40, 48), 14
    scene = _scene(900, seed=11)
    R, T = _views(B, seed=3)
    rng = np.random.default_rng(5)
    shape = {"image": (B,) + size + (3,), "hw1": size + (1,), "colour": (3,), "per_view": (B, 1, 1, 3), "grey": (1,)}[bg_kind]
    bg_np = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    bg = t(bg_np, rg=True)
    frag, gm, colors = _frag(scene, R, T, size, K)
    img = to_colored_background(frag, colors, bg)
    bg64 = torch.tensor(bg_np, dtype=torch.float64, requires_grad=True)
    ref, ref_idx, leaves, (rgb64, wsum64) = _oracle(scene, R, T, size, K, bg64)
    idx = n(frag.vert_index)
    same = (idx == np.where(ref_idx < 0, 0, ref_idx)).all(-1) | (idx == ref_idx).all(-1)
    log_line(f"[parity] background {bg_kind}: {(~same).sum()} of {same.size} pixels have a different index list")
    assert (~same).sum() <= 4
    err = np.abs(n(img) - ref.detach().numpy())[same].max()
    assert err < TOL, err
    g_img = torch.tensor(rng.normal(size=ref.shape) * same[..., None] * (np.abs(wsum64.numpy() - 1) > 1e-5)[..., None])
    g_img = _off_tie((rgb64, wsum64.clamp(max=1)), bg64.detach(), g_img).numpy()
    (img * t(g_img)).sum().backward()
    (ref * torch.tensor(g_img)).sum().backward()
    want_cols = leaves[0].grad.numpy()
    got_cols = n(colors.grad).reshape(B, -1, 3).sum(0)
    for name, got, want in (("colors", got_cols, want_cols), ("verts", n(gm.verts.grad), leaves[1].grad.numpy()),
                            ("sigmas", n(gm.sigmas.grad), leaves[2].grad.numpy()), ("background", n(bg.grad), bg64.grad.numpy())):
        grad_close(f"background {bg_kind} vs oracle: {name}", got, want, TOL)


# ---------------------------------------------------------------------------------- 2. the port's own composed route
CASES = {
    # name: (B, background shape (H, W, C substituted), C, thr, sigma kind, K, fragments route, rows)
    "image BHWC": (2, ("B", "H", "W", "C"), 3, -1.0, 0, 20, "renderer", None),
    "image HWC behind two views": (2, ("H", "W", "C"), 3, -1.0, 0, 20, "renderer", None),
    "image HWC, one view": (1, ("H", "W", "C"), 3, -1.0, 0, 20, "renderer", None),
    "colour per view": (2, ("B", 1, 1, "C"), 3, -1.0, 0, 20, "renderer", None),
    "grey [1]": (2, (1,), 3, -1.0, 0, 20, "renderer", None),
    "HW1": (2, ("H", "W", 1), 3, -1.0, 0, 20, "renderer", None),
    "HW1, one view": (1, ("H", "W", 1), 3, -1.0, 0, 20, "renderer", None),
    "W C": (2, ("W", "C"), 3, -1.0, 0, 20, "renderer", None),
    "permuted CHW": (2, "chw", 3, -1.0, 0, 20, "renderer", None),
    "permuted CHW, one view": (1, "chw", 3, -1.0, 0, 20, "renderer", None),
    "C = 4": (2, ("B", "H", "W", "C"), 4, -1.0, 0, 20, "renderer", None),
    "C = 4 colour": (1, ("C",), 4, -1.0, 0, 20, "renderer", None),
    "C = 8 features": (2, ("H", "W", "C"), 8, -1.0, 0, 20, "renderer", None),
    "C = 8 per view": (2, ("B", 1, 1, "C"), 8, -1.0, 0, 20, "renderer", None),
    "thr > 0": (2, ("B", "H", "W", "C"), 3, 0.3, 0, 20, "renderer", None),
    "thr > 0 colour": (1, ("C",), 3, 0.5, 0, 20, "renderer", None),
    "(N,3) sigmas": (2, ("H", "W", "C"), 3, -1.0, 1, 20, "renderer", None),
    "(N,3,3) sigmas": (1, ("B", "H", "W", "C"), 3, -1.0, 2, 20, "renderer", None),
    "K = 200": (1, ("H", "W", "C"), 3, -1.0, 0, 200, "renderer", None),
    "aggregation() fragments": (2, ("H", "W", "C"), 3, -1.0, 0, 20, "aggregation", None),
    "row band": (1, "band", 3, -1.0, 0, 20, "renderer", (37, 101)),
}


def _background(spec, B, size, rows, C, rng):
    """A background of the case's shape that requires grad: permuted CHW photographs and row bands are strided views."""
    H, W = size
    if spec == "chw":
        return t(rng.uniform(0, 1, (C, H, W))).permute(1, 2, 0).requires_grad_(True)
    if spec == "band":      # (a banded render takes the band of the frame's background)
        return t(rng.uniform(0, 1, (B, H, W, C)))[:, rows[0]:rows[1]].requires_grad_(True)
    dims = {"B": B, "H": H, "W": W, "C": C}
    return t(rng.uniform(0, 1, tuple(dims.get(d, d) for d in spec)), rg=True)


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_composed_route(hip_lib, case):
    from voge_amd.Renderer import to_colored_background
    B, spec, C, thr, kind, K, route, rows = CASES[case]
    size = (128, 160)
    H = size[0] if rows is None else rows[1] - rows[0]
    verts, sig, cols = _scene(3000, seed=21 + kind, kind=kind)
    rng = np.random.default_rng(7)
    if C != 3:
        cols = rng.uniform(0, 1, (cols.shape[0], C)).astype(np.float32)
    scene = (verts, sig, cols)
    R, T = _views(B, seed=4)
    bg0 = _background(spec, B, size, rows, C, rng)
    assert spec not in ("chw", "band") or not bg0.is_contiguous() or bg0.storage_offset() > 0
    runs = []
    for which in ("kernel", "composed"):
        frag, gm, colors = _frag(scene, R, T, size, K, rows=rows, route=route)
        bg = bg0.detach().requires_grad_(True)      # (the same strides and storage, a leaf of its own)
        img = (to_colored_background if which == "kernel" else _composed)(frag, colors, bg, thr=thr)
        assert img.shape == (B, H, size[1], C), img.shape
        runs.append((frag, img, gm, colors, bg))
    from voge_amd.Renderer import get_silhouette, interpolate_attr
    frag, colors = runs[1][0], runs[1][3]
    with torch.no_grad():
        m = get_silhouette(frag) if thr <= 0 else (get_silhouette(frag) > thr).float()
        g_img = _off_tie((interpolate_attr(frag, colors), m), bg0, t(rng.normal(size=(B, H, size[1], C))))
    out = []
    for frag, img, gm, colors, bg in runs:
        (img * g_img).sum().backward()
        out.append((img.detach(), colors.grad, gm.verts.grad, gm.sigmas.grad, bg.grad))
    (a, *ga), (b, *gb) = out
    assert float((b < 1).float().mean()) > 0.05 and float((1 - b).abs().max()) > 0.1      # (an image, not a blank)
    err = float((a - b).abs().max())
    assert err <= 1e-6, (case, err)
    for name, x, y in zip(("colors", "verts", "sigmas", "background"), ga, gb):
        assert x is not None and x.shape == y.shape, (case, name)
        grad_close(f"background '{case}' vs composed: {name}", n(x), n(y), 1e-5)


# ------------------------------------------------------------------------------------- 3. a learnable background colour
def _object(size=(96, 112), K=16, N=1500, seed=31):
    scene = _scene(N, seed=seed)
    R, T = camera_np.look_at_view_transform(3.6, 15.0, 40.0)
    return scene, R, T, size, K


def test_learnable_colour_gets_the_reference_gradient(hip_lib):
    from voge_amd.Renderer import get_silhouette, to_colored_background
    scene, R, T, size, K = _object()
    grads = []
    for _ in range(2):
        frag, gm, colors = _frag(scene, R, T, size, K, grad=False)
        bg = torch.ones(3, device=DEV, requires_grad=True)
        to_colored_background(frag, colors, bg).sum().backward()      # (autograd's stride-0 gradient, read in place)
        grads.append(bg.grad.clone())
        sil = get_silhouette(frag)
    assert torch.equal(grads[0], grads[1]), "two backward passes differ"
    frag, gm, colors = _frag(scene, R, T, size, K, grad=False)
    bg = torch.ones(3, device=DEV, requires_grad=True)
    _composed(frag, colors, bg).sum().backward()
    grad_close("learnable colour vs composed", n(grads[0]), n(bg.grad), 1e-5)
    # uncovered pixels sit on min's tie (x = 0 + 1 * 1): half of their gradient, as the reference's autograd gives
    uncovered = int((sil == 0).sum())
    assert uncovered > 100
    frag, gm, colors = _frag(scene, R, T, size, K, grad=False)
    bg = torch.ones(3, device=DEV, requires_grad=True)
    img = to_colored_background(frag, colors, bg)
    (img * (sil == 0)[..., None]).sum().backward()
    assert torch.equal(bg.grad, torch.full((3,), 0.5 * uncovered, device=DEV)), (bg.grad, uncovered)


def test_adam_recovers_an_unknown_background_colour(hip_lib):
    from voge_amd.Renderer import to_colored_background
    scene, R, T, size, K = _object()
    truth = (0.2, 0.55, 0.8)
    with torch.no_grad():
        frag, _, colors = _frag(scene, R, T, size, K, grad=False)
        target = to_colored_background(frag, colors, truth)
    bg = torch.ones(3, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([bg], lr=0.1, betas=(0.5, 0.9))
    decay = torch.optim.lr_scheduler.ExponentialLR(opt, 0.95)
    for _ in range(100):
        opt.zero_grad()
        frag, _, colors = _frag(scene, R, T, size, K, grad=False)
        loss = ((to_colored_background(frag, colors, bg) - target) ** 2).mean()
        loss.backward()
        assert bg.grad is not None, "the background got no gradient"
        opt.step()
        decay.step()
    err = float((bg.detach() - t(truth)).abs().max())
    log_line(f"[parity] Adam background recovery: max error {err:.2e} after 100 steps")
    assert err < 1e-3, bg.detach()


# --------------------------------------------------------------------------------------------------- 4. graph replay
def test_captured_graph_equals_eager(hip_lib):
    """A photograph behind the object and a learnable per-view colour (the per-pixel and the slab form of the background's
    gradient), forward and backward captured in one graph and replayed."""
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import to_colored_background
    scene, R, T, size, K = _object(size=(80, 96))
    gm = GaussianMeshes(t(scene[0]), t(scene[1])).to(DEV)
    gm.verts.requires_grad_(True)
    colors = t(scene[2], rg=True)
    photo = t(np.random.default_rng(2).uniform(0, 1, (3,) + size)).permute(1, 2, 0).requires_grad_(True)
    tint = torch.full((1, 1, 1, 3), 0.7, device=DEV, requires_grad=True)
    renderer = _renderer(size, K)
    Rt, Tt = t(R), t(T)
    params = [gm.verts, colors, photo, tint]

    def step():
        for p in params:
            p.grad = None
        frag = renderer(gm, R=Rt, T=Tt)
        img = to_colored_background(frag, colors, photo)
        ((img * img).sum() + to_colored_background(frag, colors, tint).sum()).backward()
        return img
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            img_e = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_img = img_e.detach().clone()
    want = [p.grad.detach().clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img_g = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert float((img_g - want_img).abs().max()) < 1e-6
    for p, w in zip(params, want):
        assert float((p.grad - w).abs().max()) <= 2e-4 * max(1.0, float(w.abs().max()))      # (atomics upstream: order of the sums)
    assert float(tint.grad.abs().min()) > 0 and float(photo.grad.abs().max()) > 0


# ----------------------------------------------------------------------------------------- 5. plain colours, 6. refusals
def test_plain_colours_keep_their_route_and_bits(hip_lib):
    from voge_amd.Renderer import to_colored_background
    scene, R, T, size, K = _object(size=(64, 72))
    imgs = {}
    for name, bg in (("tuple", (0.3, 0.6, 0.9)), ("list", [0.3, 0.6, 0.9]), ("[3]", t((0.3, 0.6, 0.9))),
                     ("[1,1,1,3]", t(((((0.3, 0.6, 0.9),),),))), ("grey tuple", (0.5,)), ("grey triple", (0.5, 0.5, 0.5)),
                     ("grey tensor", torch.tensor(0.5)), ("grey cuda [1]", t((0.5,)))):
        frag, gm, colors = _frag(scene, R, T, size, K)
        img = to_colored_background(frag, colors, bg)
        assert img.grad_fn is not None and "BlendBackground" not in type(img.grad_fn).__name__, (name, img.grad_fn)
        img.sum().backward()
        imgs[name] = (img.detach(), colors.grad)
    for name in ("list", "[3]", "[1,1,1,3]"):
        assert torch.equal(imgs[name][0], imgs["tuple"][0]), name
        g, want = imgs[name][1], imgs["tuple"][1]      # (the fused backward adds with atomics: the order of the sums)
        assert float((g - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max())), name
    for name in ("grey tuple", "grey tensor", "grey cuda [1]"):
        assert torch.equal(imgs[name][0], imgs["grey triple"][0]), name


def test_enlarging_backgrounds_are_refused(hip_lib):
    from voge_amd.Renderer import to_colored_background
    scene, R, T, size, K = _object(size=(48, 56))
    for shape in ((2,) + size + (3,), size + (4,), (1, 1) + size + (3,), (7, 3)):
        frag, gm, colors = _frag(scene, R, T, size, K)
        with pytest.raises(ValueError, match=r"does not broadcast"):
            to_colored_background(frag, colors, torch.rand(shape, device=DEV))
    frag, gm, colors = _frag(scene, R, T, size, K)
    img = to_colored_background(frag, colors, t(np.full(size + (3,), 0.25)))
    img.sum().backward()
    torch.cuda.synchronize()
    assert float(img.min()) < 0.25 and torch.isfinite(gm.verts.grad).all()
