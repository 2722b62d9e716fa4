"""Oriented Gaussians on the frame path (voge_frame_trace_fwd_ori / voge_frame_bwd_ori): three scales and a quaternion per
Gaussian go into the renderer as they are.

What is asserted:
  * the records' A against fp64 R diag(d) R^T of the same fp32 inputs, 64 * 2^-24 * max_k d_k per Gaussian, bitwise symmetric;
  * fragments and images == the existing [N,3,3] frame path fed with A_records / 2, bit for bit, every pixel, for every consumer;
  * gradients: verts against that run's, (scales, quats) against fp64 autograd of Aggregation.oriented_sigma fed with that run's
    sigmas.grad, on every backward route; quats.grad is orthogonal to quats; quaternions whose fp32 norm is unusable render the
    identity and get a zero gradient;
  * the torch fallbacks, HIP-graph capture, and a 50-step fit against the composed route.
"""
import numpy as np
import pytest
import torch

from oracle import camera_np
from util import TOL, close, grad_close, log_line, random_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def oriented_scene(N, seed, B=None, lo=0.04, hi=0.09):
    """util.random_scene's centres; scales = s * U(0.3, 1.5) per axis, quats ~ N(0, I) * U(0.5, 2) (not unit).  B: one (scales,
    quats) set per view, [B,N,..]; None: one shared set."""
    verts, s, cols = random_scene(N, seed=seed, lo=lo, hi=hi)
    rng = np.random.default_rng(seed + 1000)
    lead = (N,) if B is None else (B, N)
    scales = (s[:, None] * rng.uniform(0.3, 1.5, lead + (3,))).astype(np.float32)
    quats = (rng.normal(size=lead + (4,)) * rng.uniform(0.5, 2.0, lead + (1,))).astype(np.float32)
    return verts, scales, quats, cols


def views(B, seed):
    rng = np.random.default_rng(seed)
    return camera_np.look_at_view_transform(list(rng.uniform(3.0, 4.0, B)), list(rng.uniform(-30, 30, B)), list(rng.uniform(-180, 180, B)))


def renderer_for(size, K, inverse=False):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    H, W = size
    cams = PerspectiveCameras(focal_length=float(1.2 * max(H, W)), principal_point=((W / 2.0 + 0.25, H / 2.0 - 0.5),),
                              image_size=(size,), device=DEV)
    st = GaussianRenderSettings(image_size=size, max_assign=K, max_point_per_bin=-1, inverse_sigma=inverse)
    return GaussianRenderer(cams, st).to(DEV)


def render_ori(renderer, verts, scales, quats, R, T, rows=None):
    from voge_amd.Meshes import OrientedGaussianMeshes
    gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
    frag = renderer(gm, R=t(R), T=t(T), **({} if rows is None else dict(rows=rows)))
    lz = frag._lazy
    assert lz is not None and lz.frame and lz.gen[0] == 3 and lz.p1 is gm.scales and lz.p2 is gm.quats
    return frag, gm


def render_k2(renderer, verts, sigmas, R, T, rows=None):
    from voge_amd.Meshes import GaussianMeshes
    gm = GaussianMeshes(t(verts), sigmas.detach().clone()).to(DEV)
    frag = renderer(gm, R=t(R), T=t(T), **({} if rows is None else dict(rows=rows)))
    assert frag._lazy is not None and frag._lazy.frame and frag._lazy.gen[0] == 2
    return frag, gm


def records_A(frag, B, lead):
    """A [B,N,3,3] of the packed (centred mu, A) records, read before anything composites; -> the [N,3,3] | [B,N,3,3] `sigmas`
    (= A / 2, exact) that reproduce them on the kind-2 path."""
    rec = frag._lazy.records
    N = rec.shape[0] // B
    A = rec[:, 3:12].reshape(B, N, 3, 3).clone()
    if len(lead) == 1:      # a shared set: every view's record pass made the same A
        for b in range(1, B):
            assert torch.equal(A[b], A[0])
        return A, (A[0] / 2)
    return A, A / 2


def exact_A(scales, quats, inverse):
    """fp64 R diag(d) R^T of the fp32 inputs (numpy: the definition, independent of the package)."""
    s, q = scales.astype(np.float64), quats.astype(np.float64)
    qh = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = (qh[..., i] for i in range(4))
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))
    d = 2.0 / s if inverse else 2.0 * s
    return np.einsum("...ik,...k,...jk->...ij", Rm, d, Rm), d


CASES = [
    # N, B, per-view (scales, quats), size, rows, inverse_sigma
    (3000, 1, False, (64, 64), None, False),
    (3000, 2, True, (64, 96), None, True),
    (6000, 2, False, (96, 128), None, False),
    (6000, 2, True, (128, 128), (30, 100), False),
    (6000, 1, False, (128, 96), None, True),
]
K = 20


def case_scene(N, B, per_view, inverse):
    verts, scales, quats, cols = oriented_scene(N, seed=N // 100 + B + 7 * per_view, B=B if per_view else None)
    if inverse:      # (d = 2 / s: hand in the reciprocals, so that the Gaussians have the same extent)
        scales = (1.0 / scales).astype(np.float32)
    return verts, scales, quats, cols


@pytest.mark.parametrize("N,B,per_view,size,rows,inverse", CASES)
def test_records_hold_R_diag_d_Rt(hip_lib, N, B, per_view, size, rows, inverse):
    verts, scales, quats, cols = case_scene(N, B, per_view, inverse)
    R, T = views(B, seed=N + B)
    frag, gm = render_ori(renderer_for(size, K, inverse), verts, scales, quats, R, T, rows)
    A, _ = records_A(frag, B, scales.shape[:-1])
    assert torch.equal(A, A.transpose(-1, -2)), "A must be bitwise symmetric"
    want, d = exact_A(scales, quats, inverse)
    err = np.abs(n(A).astype(np.float64) - want).reshape(B, N, 9).max(-1) / d.max(-1)      # ([N] broadcasts over the views)
    log_line(f"[oriented] records N={N} B={B} per_view={per_view} inverse={inverse}: max |A - exact| / max_k d_k = "
             f"{err.max() / 2.0 ** -24:.2f} x 2^-24 (bound 64)")
    assert (err <= 64 * 2.0 ** -24).all()


def consumers():
    from voge_amd.Renderer import get_silhouette, interpolate_attr, to_white_background

    def white(frag, colors):
        return (to_white_background(frag, colors),)

    def merge_sil(frag, colors):
        return interpolate_attr(frag, colors), get_silhouette(frag)

    def weights(frag, colors):
        return (frag.vert_weight,)
    return dict(white=white, merge_sil=merge_sil, weights=weights)


@pytest.mark.parametrize("N,B,per_view,size,rows,inverse", CASES)
def test_forward_equals_the_3x3_frame_path_bit_for_bit(hip_lib, N, B, per_view, size, rows, inverse):
    verts, scales, quats, cols = case_scene(N, B, per_view, inverse)
    R, T = views(B, seed=N + B)
    colors = t(np.tile(cols, (B, 1)))
    for name, use in consumers().items():
        fa, _ = render_ori(renderer_for(size, K, inverse), verts, scales, quats, R, T, rows)
        _, sig = records_A(fa, B, scales.shape[:-1])
        fb, _ = render_k2(renderer_for(size, K, False), verts, sig, R, T, rows)
        assert torch.equal(fa._lazy.records, fb._lazy.records), name
        outs_a, outs_b = use(fa, colors), use(fb, colors)
        for a, b in zip(outs_a, outs_b):
            assert a.shape == b.shape and torch.equal(a, b), name
        for field in ("vert_index", "vert_hit_length", "vert_weight", "valid_num"):
            assert torch.equal(getattr(fa, field), getattr(fb, field)), (name, field)
        assert int(fa.valid_num.max()) > 0


def test_identity_quaternions_equal_diag_embed(hip_lib):
    verts, scales, quats, cols = oriented_scene(3000, seed=3)
    quats = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (3000, 1))
    R, T = views(2, seed=5)
    colors = t(np.tile(cols, (2, 1)))
    for name, use in consumers().items():
        fa, _ = render_ori(renderer_for((64, 80), K), verts, scales, quats, R, T)
        fb, _ = render_k2(renderer_for((64, 80), K), verts, torch.diag_embed(t(scales)), R, T)
        assert torch.equal(fa._lazy.records, fb._lazy.records), name
        for a, b in zip(use(fa, colors), use(fb, colors)):
            assert torch.equal(a, b), name
        for field in ("vert_index", "vert_hit_length", "vert_weight", "valid_num"):
            assert torch.equal(getattr(fa, field), getattr(fb, field)), (name, field)


def losses():
    """The backward routes -- image, merge + silhouette, hit length, the weights read directly, and the nodes that receive a
    gradient of their weights beside their own output's -- each with a fixed random upstream gradient."""
    from voge_amd.Renderer import get_silhouette, interpolate_attr, to_white_background

    def image(frag, colors, rng):
        img = to_white_background(frag, colors)
        return (img * t(rng.normal(size=tuple(img.shape)))).sum()

    def merge_sil(frag, colors, rng):
        rgb, sil = interpolate_attr(frag, colors), get_silhouette(frag)
        return (rgb * t(rng.normal(size=tuple(rgb.shape)))).sum() + (sil * t(rng.normal(size=tuple(sil.shape)))).sum()

    def hit_length(frag, colors, rng):
        hl = frag.vert_hit_length
        g = t(rng.normal(size=tuple(hl.shape))) * (hl.detach() < 1e9)
        return (torch.where(hl.detach() < 1e9, hl, torch.zeros_like(hl)) * g).sum()

    def weights(frag, colors, rng):      # (the weights read first: _CompositeLean)
        w = frag.vert_weight
        return (w * t(rng.normal(size=tuple(w.shape)))).sum()

    def image_and_weights(frag, colors, rng):      # (_CompositeShade with a gradient of its weights beside the image's)
        img = to_white_background(frag, colors)
        w = frag.vert_weight
        return (img * t(rng.normal(size=tuple(img.shape)))).sum() + (w * t(rng.normal(size=tuple(w.shape)))).sum()

    def merge_and_weights(frag, colors, rng):      # (_CompositeMerge likewise)
        rgb = interpolate_attr(frag, colors)
        w = frag.vert_weight
        return (rgb * t(rng.normal(size=tuple(rgb.shape)))).sum() + (w * t(rng.normal(size=tuple(w.shape)))).sum()
    return dict(image=image, merge_sil=merge_sil, hit_length=hit_length, weights=weights, image_and_weights=image_and_weights,
                merge_and_weights=merge_and_weights)


@pytest.mark.parametrize("N,B,per_view,size,rows,inverse", CASES)
def test_backward_against_the_3x3_run_and_fp64_autograd(hip_lib, N, B, per_view, size, rows, inverse):
    from voge_amd.Aggregation import oriented_sigma
    verts, scales, quats, cols = case_scene(N, B, per_view, inverse)
    R, T = views(B, seed=N + B)
    for name, loss in losses().items():
        label = f"oriented N={N} B={B} per_view={per_view} inverse={inverse} {name}"
        colors = t(np.tile(cols, (B, 1)))
        fa, ga = render_ori(renderer_for(size, K, inverse), verts, scales, quats, R, T, rows)
        _, sig = records_A(fa, B, scales.shape[:-1])
        loss(fa, colors, np.random.default_rng(N)).backward()
        fb, gb = render_k2(renderer_for(size, K, False), verts, sig, R, T, rows)
        loss(fb, colors, np.random.default_rng(N)).backward()
        assert ga.verts.grad is not None and gb.sigmas.grad is not None and float(gb.sigmas.grad.abs().max()) > 0
        grad_close(label + " verts", n(ga.verts.grad), n(gb.verts.grad), TOL)
        # the reference chain: fp64 autograd through the definition, fed with the 3x3 run's gradient
        s64, q64 = t(scales, torch.float64, rg=True), t(quats, torch.float64, rg=True)
        S = oriented_sigma(1.0 / s64 if inverse else s64, q64)
        (S * gb.sigmas.grad.double()).sum().backward()
        grad_close(label + " scales", n(ga.scales.grad), n(s64.grad), TOL)
        grad_close(label + " quats", n(ga.quats.grad), n(q64.grad), TOL)
        # (the dot product's rounding grows with the gradient's size: judged on grad_close's own scale, taken from the reference)
        along = (ga.quats.grad.double() * t(quats, torch.float64)).sum(-1) / max(1.0, float(q64.grad.abs().max()))
        grad_close(label + " quats.grad . quats", n(along), np.zeros(tuple(along.shape)), TOL)


def test_quaternions_without_a_usable_fp32_norm(hip_lib):
    """Zero, NaN, and quaternions whose squared norm overflows or underflows in fp32 (finite and positive in fp64): the record pass
    renders the identity rotation, so the backward must hand them a zero gradient -- the forward's own decision, not fp64's --
    while scales and vertices get the gradients of the diagonal form; the usable quaternions around them are untouched by it."""
    from voge_amd.Renderer import to_white_background
    Ng = 3000
    verts, scales, quats, cols = oriented_scene(Ng, seed=17)
    odd = np.array([[0, 0, 0, 0], [np.nan, 1, 0, 0], [3e19, 1e19, 0, -2e19], [1e-24, -2e-24, 1e-24, 0], [np.inf, 0, 0, 1]], np.float32)
    bad = np.arange(0, Ng, 7)
    quats[bad] = odd[np.arange(bad.size) % len(odd)]
    q64 = quats[bad].astype(np.float64)
    assert (np.isfinite((q64 * q64).sum(-1)) & ((q64 * q64).sum(-1) > 0)).sum() >= 2 * (bad.size // len(odd))      # fp64 would accept those
    R, T = views(2, seed=6)
    colors = t(np.tile(cols, (2, 1)))
    rng = np.random.default_rng(3)
    fa, ga = render_ori(renderer_for((64, 80), K), verts, scales, quats, R, T)
    A, _ = records_A(fa, 2, scales.shape[:-1])
    assert torch.equal(A[0][bad], torch.diag_embed(2.0 * t(scales[bad])))
    img = to_white_background(fa, colors)
    g = t(rng.normal(size=tuple(img.shape)))
    (img * g).sum().backward()
    assert torch.isfinite(img).all() and torch.isfinite(ga.scales.grad).all() and torch.isfinite(ga.verts.grad).all()
    assert torch.equal(ga.quats.grad[bad], torch.zeros((bad.size, 4), device=DEV))
    assert float(ga.scales.grad[bad].abs().max()) > 0
    # the same frame with identity quaternions in their place: the same image, the same gradients elsewhere
    quats_id = quats.copy()
    quats_id[bad] = [1, 0, 0, 0]
    fb, gb = render_ori(renderer_for((64, 80), K), verts, scales, quats_id, R, T)
    img_b = to_white_background(fb, colors)
    assert torch.equal(img, img_b)
    (img_b * g).sum().backward()
    grad_close("oriented unusable norms: scales", n(ga.scales.grad), n(gb.scales.grad), TOL)
    keep = np.setdiff1d(np.arange(Ng), bad)
    grad_close("oriented unusable norms: quats elsewhere", n(ga.quats.grad)[keep], n(gb.quats.grad)[keep], TOL)


def test_fallbacks_give_the_frame_paths_image(hip_lib):
    from voge_amd import ops
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import to_white_background
    verts, scales, quats, cols = oriented_scene(3000, seed=21)
    R, T = views(1, seed=4)
    for inverse in (False, True):
        sc = (1.0 / scales).astype(np.float32) if inverse else scales
        renderer = renderer_for((64, 64), K, inverse)
        colors = t(cols)
        fa, _ = render_ori(renderer, verts, sc, quats, R, T)
        want = n(to_white_background(fa, colors))
        # a camera that wants a gradient
        gm = OrientedGaussianMeshes(t(verts), t(sc), t(quats)).to(DEV)
        Rg = t(R, rg=True)
        fb = renderer_for((64, 64), K, inverse)(gm, R=Rg, T=t(T))
        assert fb._lazy is None or not fb._lazy.frame
        img = to_white_background(fb, colors)
        bad = ~close(n(img), want, TOL)
        log_line(f"[oriented] fallback R.requires_grad inverse={inverse}: {int(bad.sum())} of {bad.size} values beyond TOL")
        assert not bad.any()
        img.sum().backward()
        assert Rg.grad is not None and gm.scales.grad is not None and gm.quats.grad is not None
        # the frame path switched off
        old = ops.FRAME_PATH
        ops.FRAME_PATH = False
        try:
            gm2 = OrientedGaussianMeshes(t(verts), t(sc), t(quats)).to(DEV)
            fc = renderer_for((64, 64), K, inverse)(gm2, R=t(R), T=t(T))
            assert fc._lazy is None or not fc._lazy.frame
            img2 = to_white_background(fc, colors)
        finally:
            ops.FRAME_PATH = old
        bad = ~close(n(img2), want, TOL)
        log_line(f"[oriented] fallback FRAME_PATH off inverse={inverse}: {int(bad.sum())} of {bad.size} values beyond TOL")
        assert not bad.any()


def test_graph_capture_of_a_training_step(hip_lib):
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import to_white_background
    verts, scales, quats, cols = oriented_scene(6000, seed=31)
    R, T = views(1, seed=9)
    renderer = renderer_for((96, 96), K)
    gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
    colors = t(cols, rg=True)
    Rt, Tt = t(R), t(T)
    params = [gm.verts, gm.scales, gm.quats, colors]

    def step():
        for p in params:
            p.grad = None
        img = to_white_background(renderer(gm, R=Rt, T=Tt), colors)
        img.sum().backward()
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
    assert torch.equal(img_g, want_img)
    for name, p, w in zip(("verts", "scales", "quats", "colors"), params, want):
        grad_close(f"oriented graph replay {name}", n(p.grad), n(w), TOL)
    assert float(want_img.min()) < 0.9 and float(want[2].abs().max()) > 0


def test_it_optimises(hip_lib):
    """50 Adam steps on (verts, scales, quats) of 64 oriented Gaussians towards a target rendered from a perturbed copy: through
    the oriented frame path and through oriented_sigma composed in torch + the [N,3,3] route, from the same start."""
    from voge_amd.Aggregation import oriented_sigma
    from voge_amd.Meshes import GaussianMeshesNaive, OrientedGaussianMeshes, OrientedGaussianMeshesNaive
    from voge_amd.Renderer import to_white_background
    rng = np.random.default_rng(41)
    Ng = 64
    verts = rng.uniform(-0.6, 0.6, (Ng, 3)).astype(np.float32)
    r = rng.uniform(0.12, 0.25, Ng)
    s = 1.0 / (r * r / (2 * np.log(1 / 0.6)))
    scales = (s[:, None] * rng.uniform(0.3, 1.5, (Ng, 3))).astype(np.float32)
    quats = (rng.normal(size=(Ng, 4)) * rng.uniform(0.5, 2.0, (Ng, 1))).astype(np.float32)
    cols = t(rng.uniform(0, 1, (Ng, 3)))
    R, T = views(1, seed=2)
    Rt, Tt = t(R), t(T)
    renderer = renderer_for((64, 64), K)
    with torch.no_grad():
        tgt = OrientedGaussianMeshesNaive(t(verts + rng.normal(size=verts.shape) * 0.05),
                                          t(scales * rng.uniform(0.7, 1.4, scales.shape)),
                                          t(quats + rng.normal(size=quats.shape) * 0.3))
        target = to_white_background(renderer(tgt, R=Rt, T=Tt), cols).clone()

    def fit(composed):
        gm = OrientedGaussianMeshes(t(verts), t(scales), t(quats)).to(DEV)
        # (50 steps of 0.05 move a scale by 2.5 at the most; the smallest one starts at 4.9: they stay positive)
        opt = torch.optim.Adam([{"params": [gm.verts], "lr": 2e-3}, {"params": [gm.scales], "lr": 0.05}, {"params": [gm.quats], "lr": 5e-3}])
        hist = []
        for _ in range(50):
            opt.zero_grad()
            if composed:
                frag = renderer(GaussianMeshesNaive(gm.verts, oriented_sigma(gm.scales, gm.quats)), R=Rt, T=Tt)
                assert frag._lazy.gen[0] == 2
            else:
                frag = renderer(gm, R=Rt, T=Tt)
                assert frag._lazy.gen[0] == 3
            loss = ((to_white_background(frag, cols) - target) ** 2).mean()
            loss.backward()
            hist.append(float(loss.detach()))
            opt.step()
        with torch.no_grad():
            final = float(((to_white_background(renderer(gm, R=Rt, T=Tt), cols) - target) ** 2).mean())
            S = oriented_sigma(gm.scales.double(), gm.quats.double())
        assert torch.equal(S, S.transpose(-1, -2)) and float(torch.linalg.eigvalsh(S).min()) > 0
        return hist[0], final
    first_new, final_new = fit(False)
    first_ref, final_ref = fit(True)
    log_line(f"[oriented] 50 Adam steps: loss {first_new:.4e} -> {final_new:.4e} (oriented path), {first_ref:.4e} -> {final_ref:.4e} "
             f"(composed in torch); ratio {final_new / final_ref:.4f}")
    assert final_new < first_new and final_ref < first_ref
    assert final_new <= 1.10 * final_ref
