"""GPU tests of Renderer.get_depth (an extension: the reference and the oracle have no depth function).

The reference values are formed in fp64 numpy from the ORACLE's weight, len and valid_num of the same frame:
    A = sum_{k<n} w_k len_k,  S = sum_{k<n} w_k,  D = A / S (S > 0, else the background) | A,
and the reference gradients by handing g_w[k] = a len_k + b, g_len[k] = a w_k (a = g_D / S, b = -g_D D / S | a = g_D, b = 0; the
formulas tests/test_depth_cpu.py checks against finite differences) to the oracle's composite + trace backward.  The scenes are
those of test_gpu_training_path.test_fragment_backward_from_a_weight_gradient_vs_oracle (12 flipped pixels at most); comparisons
run on the pixels whose index lists match.  Tolerances: util.TOL forward (what the merged attributes get: both are K-term
weighted sums), 0.25 * TOL of the gradient scale backward (that test's own: the same kernel fed the same kind of input)."""
import numpy as np
import pytest
import torch

import oracle
from oracle import camera_np
from util import TOL, close, grad_close, log_line, max_rel, random_scene, _report_flips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = 7.5


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


# ---- helpers restated from tests/test_gpu_training_path.py -----------------------------------------------------------
def oracle_frame(verts, sigmas, R, T, focal, pp, size, K, thr=0.01, occ=1.0, inverse=False):
    rays, origin = camera_np.pixel_rays(R, T, focal, pp, size)
    B = rays.shape[0]
    mus = (np.asarray(verts, np.float32)[None] - origin[:, None].astype(np.float32)).astype(np.float32)
    sig3 = camera_np.expand_sigma(np.asarray(sigmas, np.float32))
    isg = (2 * np.linalg.inv(sig3.astype(np.float64))).astype(np.float32) if inverse else (2 * sig3).astype(np.float32)
    isg = np.ascontiguousarray(np.broadcast_to(isg[None], (B,) + isg.shape))
    idx, ln, act, dsd = oracle.trace_fwd(mus, isg, rays, K, oracle.thr_act_of(thr))
    w, vn = oracle.composite_fwd(idx, act, ln, dsd, occ)
    return dict(rays=rays, mus=mus, isg=isg, idx=idx, len=ln, act=act, dsd=dsd, weight=w, valid_num=vn, occ=occ)


def oracle_param_grads(ref, sigmas, g_w, g_hitlen=None):
    g_act, g_len, g_dsd = oracle.composite_bwd(ref["act"], ref["len"], ref["dsd"], g_w, ref["occ"])
    if g_hitlen is not None:
        g_len = g_len + g_hitlen
    _, g_mu, g_A = oracle.trace_bwd(ref["mus"], ref["isg"], ref["rays"], ref["idx"], g_len, g_act, g_dsd)
    B, N = ref["rays"].shape[0], ref["mus"].shape[1]
    g_mu = g_mu.reshape(B, N, 3).sum(0)
    g_A = g_A.reshape(B, N, 3, 3).sum(0)
    sigmas = np.asarray(sigmas)
    if sigmas.ndim == 1:
        return g_mu, 2 * np.einsum("nii->n", g_A)
    if sigmas.ndim == 2:
        return g_mu, 2 * np.einsum("nii->ni", g_A)
    return g_mu, 2 * g_A


def same_lists(frag, ref, label, max_flips):
    idx = n(frag.vert_index)
    same = (idx == np.where(ref["idx"] < 0, 0, ref["idx"])).all(-1) | (idx == ref["idx"]).all(-1)
    _report_flips(label, (~same).sum(), same.size)
    assert (~same).sum() <= max_flips, f"{label}: {(~same).sum()} of {same.size} pixels flipped (ceiling {max_flips})"
    assert np.abs(n(frag.vert_weight)[same] - ref["weight"][same]).max(initial=0.0) < TOL
    return same


def renderer_for(H, W, K, focal, thr=0.01, occ=1.0, inverse=False, mppb=-1):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    cams = PerspectiveCameras(focal_length=focal, principal_point=((W / 2.0, H / 2.0),), image_size=((H, W),), device=DEV)
    st = GaussianRenderSettings(image_size=(H, W), max_assign=K, thr_activation=thr, absorptivity=occ, inverse_sigma=inverse,
                                max_point_per_bin=mppb)
    return GaussianRenderer(cams, st).to(DEV)


# ---- the fp64 reference of get_depth and of its gradient (tests/test_depth_cpu.py pins these against finite differences) -------
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
    """g = d loss / d depth [..] -> (g_weight, g_len) [.., K], zero in the dead slots."""
    D, S, live = depth_ref(w, ln, vn, normalize)
    if normalize:
        hit = S > 0
        a = np.where(hit, g / np.where(hit, S, 1.0), 0.0)
        b = np.where(hit, -a * D, 0.0)
    else:
        a, b = np.asarray(g, np.float64), np.zeros_like(S)
    lnl = np.where(live, np.asarray(ln, np.float64), 0.0)
    return (a[..., None] * lnl + b[..., None]) * live, a[..., None] * np.where(live, np.asarray(w, np.float64), 0.0)


# ---- the scenes of test_fragment_backward_from_a_weight_gradient_vs_oracle --------------------------------------------------
def scene(K, B, form, inverse):
    N, H, W = (900, 40, 56) if K > 64 else (2000, 56, 72)
    lo, hi = (0.15, 0.3) if K > 64 else (0.05, 0.12)
    verts, sig, cols = random_scene(N, seed=300 + K, lo=lo, hi=hi, aniso=(form == "full"))
    if form == "diag":
        sig = (sig[:, None] * np.random.default_rng(K).uniform(0.6, 1.6, (N, 3))).astype(np.float32)
    if inverse:
        sig = (1.0 / sig).astype(np.float32)
    R, T = camera_np.look_at_view_transform([3.0, 3.3][:B], [10.0, -20.0][:B], [30.0, 200.0][:B])
    return dict(N=N, H=H, W=W, K=K, B=B, verts=verts, sig=sig, cols=cols, R=R, T=T, occ=1.1, focal=80.0, inverse=inverse)


def render(sc, rows=None):
    from voge_amd.Meshes import GaussianMeshes
    renderer = renderer_for(sc["H"], sc["W"], sc["K"], sc["focal"], occ=sc["occ"], inverse=sc["inverse"])
    gm = GaussianMeshes(t(sc["verts"]), t(sc["sig"])).to(DEV)
    kw = {} if rows is None else {"rows": rows}
    return gm, renderer(gm, R=t(sc["R"]), T=t(sc["T"]), **kw)


def reference(sc):
    return oracle_frame(sc["verts"], sc["sig"], sc["R"], sc["T"], sc["focal"], (sc["W"] / 2.0, sc["H"] / 2.0), (sc["H"], sc["W"]),
                        sc["K"], occ=sc["occ"], inverse=sc["inverse"])


def sigma_grad(sc, g_sig):
    """the oracle's gradient of A = 2 sigma, turned into the gradient of what the user holds (inverse_sigma: A = 2 / s)."""
    return -g_sig / (np.asarray(sc["sig"], np.float64) ** 2) if sc["inverse"] else g_sig


def forbid_chain(monkeypatch):
    """Make every backward but the depth form's unreachable: a test that passes took ONE voge_frame_depth_bwd_iso."""
    from voge_amd import _lib
    lib = _lib.load()

    def boom(*a):
        raise AssertionError("a backward other than voge_frame_depth_bwd_iso was taken")
    for name in ("voge_fragment_bwd_iso", "voge_composite_bwd", "voge_trace_bwd", "voge_trace_bwd_iso", "voge_trace_bwd_iso_view",
                 "voge_fragment_act_dsd_iso"):
        monkeypatch.setattr(lib, name, boom, raising=True)


def count_calls(monkeypatch, names):
    from voge_amd import _lib
    lib = _lib.load()
    calls = {k: 0 for k in names}
    for name in names:
        def wrap(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, wrap, raising=True)
    return calls


ONE_PASS = ("voge_frame_depth_fwd_iso", "voge_frame_depth_bwd_iso")
ROWS = [(25, 1, "scalar", False, True), (40, 2, "scalar", False, True), (7, 1, "scalar", True, True), (1, 1, "scalar", False, True),
        (130, 1, "scalar", False, False), (25, 1, "full", False, False), (9, 1, "diag", False, False)]


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("K,B,form,inverse,one_pass", ROWS)
def test_depth_and_its_gradient_vs_oracle(hip_lib, monkeypatch, K, B, form, inverse, one_pass, normalize):
    """Forward at TOL on the matched pixels, empty pixels EXACTLY the background (normalised) or 0, the gradients of verts and
    sigmas of (D * g).sum() at 0.25 * TOL of their scale -- on the route the fragments are expected to take: scalar sigmas with
    K <= 128 one voge_frame_depth_fwd_iso and one voge_frame_depth_bwd_iso per step and no other backward kernel, everything
    else ops._Depth on the fragments' tensors."""
    from voge_amd.Renderer import get_depth
    sc = scene(K, B, form, inverse)
    calls = count_calls(monkeypatch, ONE_PASS)
    if one_pass:
        forbid_chain(monkeypatch)
    gm, frag = render(sc)
    D = get_depth(frag, normalize=normalize, background=BG)
    assert type(D.grad_fn).__name__ == ("_CompositeDepthBackward" if one_pass else "_DepthBackward")
    assert frag._lazy is None and D.shape == frag.vert_index.shape[:-1] and D.dtype == torch.float32
    assert int(n(frag.vert_index).min()) == -1 or (n(frag.valid_num) == K).all()      # (-1 stays -1: no merge_final rewrite)
    ref = reference(sc)
    label = f"get_depth K={K} B={B} {form} normalize={normalize}"
    same = same_lists(frag, ref, label, max_flips=12)
    D_ref, S_ref, live = depth_ref(ref["weight"], ref["len"], ref["valid_num"], normalize, BG)
    log_line(f"[parity] {label}: forward max rel err {max_rel(n(D)[same], D_ref[same]):.2e} (tolerance {TOL:.1e}), "
             f"{int((ref['valid_num'] == 0).sum())} empty pixels, max sum w {S_ref.max():.3f}, min lit sum w {S_ref[S_ref > 0].min():.3e}")
    assert close(n(D)[same], D_ref[same]).all(), max_rel(n(D)[same], D_ref[same])
    empty = (ref["valid_num"] == 0) & same
    assert (n(D)[empty] == np.float32(BG if normalize else 0.0)).all()
    g = np.random.default_rng(7).normal(size=D_ref.shape) * same
    (D * t(g)).sum().backward()
    g_w, g_h = depth_grads_ref(ref["weight"], ref["len"], ref["valid_num"], g, normalize)
    g_mu, g_sig = oracle_param_grads(ref, sc["sig"], g_w, g_h)
    grad_close(f"{label} verts", n(gm.verts.grad), g_mu, 0.25 * TOL)
    grad_close(f"{label} sigmas", n(gm.sigmas.grad), sigma_grad(sc, g_sig), 0.25 * TOL)
    assert np.abs(g_mu).max() > 0 and np.abs(g_sig).max() > 0
    assert calls == dict.fromkeys(ONE_PASS, 1 if one_pass else 0), calls


def test_forward_is_bitwise_reproducible(hip_lib):
    from voge_amd.Renderer import get_depth
    sc = scene(25, 1, "scalar", False)
    for force_depth_node in (False, True):
        outs = []
        for _ in range(3):
            _, frag = render(sc)
            if force_depth_node:
                _ = frag.vert_weight
            outs.append(get_depth(frag).detach().clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ behaviour
def test_silhouette_after_depth_is_free_and_one_backward_launch_serves_both(hip_lib, monkeypatch):
    """get_silhouette after get_depth launches nothing (the composite wrote min(S, 1) with the sum it had in hand) and a loss on
    depth plus silhouette still makes ONE fused backward launch, whose gradients are the sum of the two oracle gradients."""
    from voge_amd import _lib
    from voge_amd.Renderer import get_depth, get_silhouette
    sc = scene(25, 1, "scalar", False)
    calls = count_calls(monkeypatch, ONE_PASS)
    forbid_chain(monkeypatch)

    def boom(*a):
        raise AssertionError("get_silhouette launched a kernel")
    monkeypatch.setattr(_lib.load(), "voge_silhouette_fwd", boom, raising=True)
    gm, frag = render(sc)
    D = get_depth(frag)
    sil = get_silhouette(frag)
    ref = reference(sc)
    same = same_lists(frag, ref, "get_depth + get_silhouette", max_flips=12)
    D_ref, S_ref, live = depth_ref(ref["weight"], ref["len"], ref["valid_num"], True)
    assert close(n(sil)[same], np.minimum(S_ref, 1)[same]).all() and float(sil.detach().max()) <= 1.0
    rng = np.random.default_rng(3)
    g = rng.normal(size=D_ref.shape) * same
    tgt = rng.uniform(0, 1, S_ref.shape)
    ((D * t(g)).sum() + (((sil - t(tgt)) ** 2) * t(same.astype(np.float32))).sum()).backward()
    assert calls == dict.fromkeys(ONE_PASS, 1), calls
    g_w, g_h = depth_grads_ref(ref["weight"], ref["len"], ref["valid_num"], g, True)
    g_pix = 2 * (np.minimum(S_ref, 1) - tgt) * (S_ref < 1) * same
    g_mu, g_sig = oracle_param_grads(ref, sc["sig"], g_w + g_pix[..., None] * live, g_h)
    grad_close("depth + silhouette verts", n(gm.verts.grad), g_mu, 0.25 * TOL)
    grad_close("depth + silhouette sigmas", n(gm.sigmas.grad), g_sig, 0.25 * TOL)
    # the silhouette alone, behind a get_depth nobody differentiates: still that one launch
    gm, frag = render(sc)
    get_depth(frag, normalize=False)
    (((get_silhouette(frag) - t(tgt)) ** 2) * t(same.astype(np.float32))).sum().backward()
    assert calls == dict.fromkeys(ONE_PASS, 2), calls
    g_mu, g_sig = oracle_param_grads(ref, sc["sig"], g_pix[..., None] * live)
    grad_close("silhouette behind get_depth verts", n(gm.verts.grad), g_mu, 0.25 * TOL)
    grad_close("silhouette behind get_depth sigmas", n(gm.sigmas.grad), g_sig, 0.25 * TOL)


@pytest.mark.parametrize("K,B,inverse", [(25, 1, False), (40, 2, False), (7, 1, True)])
@pytest.mark.parametrize("normalize", [True, False])
def test_one_pass_and_depth_node_agree(hip_lib, monkeypatch, K, B, inverse, normalize):
    """The same scene through ops._CompositeDepth and -- vert_weight read first -- through ops._Depth: TOL forward, 0.25 * TOL
    of the gradient scale backward.  The weights are the same bits where both composites give a lane four slots (K % 4 == 0; the
    composite alone gives it two for any other K, the one-pass forms always four: within TOL there, as for the other one-pass forms)."""
    from voge_amd.Renderer import get_depth
    sc = scene(K, B, "scalar", inverse)
    g = torch.randn((B, sc["H"], sc["W"]), device=DEV, generator=torch.Generator(DEV).manual_seed(11))
    out = {}
    for forced in (False, True):
        gm, frag = render(sc)
        if forced:
            _ = frag.vert_weight
        D = get_depth(frag, normalize=normalize, background=BG)
        assert type(D.grad_fn).__name__ == ("_DepthBackward" if forced else "_CompositeDepthBackward")
        (D * g).sum().backward()
        out[forced] = [n(x) for x in (D, frag.vert_weight, gm.verts.grad, gm.sigmas.grad)]
    label = f"one-pass vs _Depth K={K} B={B} normalize={normalize}"
    log_line(f"[parity] {label}: forward max rel difference {max_rel(out[False][0], out[True][0]):.2e} (tolerance {TOL:.1e})")
    assert close(out[False][0], out[True][0]).all()
    assert np.array_equal(out[False][1], out[True][1]) if K % 4 == 0 else close(out[False][1], out[True][1]).all()
    grad_close(f"{label} verts", out[False][2], out[True][2], 0.25 * TOL)
    grad_close(f"{label} sigmas", out[False][3], out[True][3], 0.25 * TOL)


def test_rgbd_step_in_both_orders(hip_lib):
    """get_depth then to_white_background (the fast order: the colours take _ShadeThrough on the finished weights) and the
    reverse, on fresh fragments: gradients of verts, sigmas and colours equal the oracle's sum; vert_weight is the same bits in
    both orders and without get_depth (every route composites with the same core); the colour image behind get_depth comes from
    another kernel than the one-pass shade, so it is compared at TOL."""
    from voge_amd.Renderer import get_depth, to_white_background
    sc = scene(25, 1, "scalar", False)
    ref = reference(sc)
    K = sc["K"]
    rgb = oracle.merge_fwd(sc["cols"], ref["idx"], ref["weight"], ref["valid_num"])
    img_ref, sil = oracle.blend_fwd(rgb, ref["weight"])
    D_ref, S_ref, live = depth_ref(ref["weight"], ref["len"], ref["valid_num"], True)
    rng = np.random.default_rng(5)
    g_img0, g_d0 = rng.normal(size=img_ref.shape), rng.normal(size=D_ref.shape)
    weights = {}
    for order in ("depth first", "colour first", "colour only"):
        gm, frag = render(sc)
        colors = t(sc["cols"], rg=True)
        if order == "depth first":
            D = get_depth(frag)
            img = to_white_background(frag, colors)
            assert type(D.grad_fn).__name__ == "_CompositeDepthBackward" and type(img.grad_fn).__name__ == "_ShadeThroughBackward"
        elif order == "colour first":
            img = to_white_background(frag, colors)
            D = get_depth(frag)
            assert type(img.grad_fn).__name__ == "_CompositeShadeBackward" and type(D.grad_fn).__name__ == "_DepthBackward"
        else:
            img, D = to_white_background(frag, colors), None
        same = same_lists(frag, ref, f"RGB-D step, {order}", max_flips=12)
        weights[order] = n(frag.vert_weight)
        assert close(n(img)[same], img_ref[same]).all(), order
        if D is None:
            continue
        assert close(n(D)[same], D_ref[same]).all(), order
        g_img, g_d = g_img0 * same[..., None], g_d0 * same
        ((img * t(g_img)).sum() + (D * t(g_d)).sum()).backward()
        g_rgb = g_img * ((rgb + (1 - sil)[..., None]) < 1)
        g_sumw = -g_rgb.sum(-1) * (ref["weight"].sum(-1) < 1)
        g_attr, g_wc = oracle.merge_bwd(sc["cols"], ref["idx"], ref["weight"], ref["valid_num"], g_rgb)
        g_wd, g_h = depth_grads_ref(ref["weight"], ref["len"], ref["valid_num"], g_d, True)
        g_mu, g_sig = oracle_param_grads(ref, sc["sig"], g_wc + g_sumw[..., None] * live + g_wd, g_h)
        grad_close(f"RGB-D {order} colors", n(colors.grad), g_attr, 0.25 * TOL)
        grad_close(f"RGB-D {order} verts", n(gm.verts.grad), g_mu, 0.25 * TOL)
        grad_close(f"RGB-D {order} sigmas", n(gm.sigmas.grad), g_sig, 0.25 * TOL)
    assert np.array_equal(weights["depth first"], weights["colour first"])
    assert np.array_equal(weights["depth first"], weights["colour only"])


def test_views_of_the_fragments_and_row_bands_keep_the_one_pass_route(hip_lib, monkeypatch):
    """frag.squeeze(), frag.copy() and rows=(r0, r1) still take ops._CompositeDepth, with the full frame's values."""
    from voge_amd.Renderer import get_depth
    sc = scene(25, 1, "scalar", False)
    _, frag = render(sc)
    base = get_depth(frag, background=BG)
    calls = count_calls(monkeypatch, ONE_PASS)
    forbid_chain(monkeypatch)
    for name, fn in (("squeeze", lambda f: f.squeeze()), ("copy", lambda f: f.copy()), ("squeeze.unsqueeze", lambda f: f.squeeze().unsqueeze())):
        gm, frag = render(sc)
        D = get_depth(fn(frag), background=BG)
        node = D.grad_fn if name == "copy" else D.grad_fn.next_functions[0][0]      # (a reshaped view of the node's output)
        assert type(node).__name__ == "_CompositeDepthBackward" and D.shape == fn(frag).vert_index.shape[:-1], name
        assert torch.equal(D.reshape(base.shape), base), name
        D.sum().backward()
        assert gm.verts.grad.abs().max().item() > 0, name
    r0, r1 = 16, 40
    gm, frag = render(sc, rows=(r0, r1))
    D = get_depth(frag, background=BG)
    assert type(D.grad_fn).__name__ == "_CompositeDepthBackward" and D.shape == (1, r1 - r0, sc["W"])
    assert (D - base[:, r0:r1]).abs().max().item() <= 1e-6
    D.sum().backward()
    assert calls == dict.fromkeys(ONE_PASS, 4), calls


def test_autograd_mode_follows_the_render_call(hip_lib):
    """As test_deferred_composite_keeps_the_render_calls_autograd_mode: fragments rendered under no_grad give a depth without a
    grad_fn whoever asks; a first read under no_grad after a render WITH grad leaves a later get_depth differentiable, with the
    gradient of the untouched frame."""
    from voge_amd.Renderer import get_depth
    sc = scene(25, 1, "scalar", False)
    with torch.no_grad():
        _, frag = render(sc)
    D = get_depth(frag)
    assert D.grad_fn is None and not D.requires_grad
    grads = {}
    for touched in (False, True, "depth under no_grad"):
        gm, frag = render(sc)
        if touched is True:
            with torch.no_grad():
                _ = frag.vert_weight, frag.valid_num
        elif touched:
            with torch.no_grad():
                assert get_depth(frag).grad_fn is not None      # (the render call's mode, not the reader's)
        D = get_depth(frag)
        assert D.grad_fn is not None
        (D * t(np.linspace(0.5, 1.5, sc["W"]))).sum().backward()
        grads[touched] = (n(gm.verts.grad), n(gm.sigmas.grad))
    for key in (True, "depth under no_grad"):
        for a, b in zip(grads[False], grads[key]):
            assert np.abs(a).max() > 0
            assert np.abs(a - b).max() <= 0.25 * TOL * max(1.0, np.abs(a).max()), key


def test_captured_depth_step_replays_to_the_eager_gradients(hip_lib):
    """render -> get_depth -> backward captured into a HIP graph (which refuses a host synchronisation or a host-to-device copy
    inside get_depth) and replayed back to back reproduces the eager step's depth and gradients."""
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import get_depth, get_silhouette
    sc = scene(25, 1, "scalar", False)
    renderer = renderer_for(sc["H"], sc["W"], sc["K"], sc["focal"], occ=sc["occ"])
    gm = GaussianMeshes(t(sc["verts"]), t(sc["sig"])).to(DEV)
    Rt, Tt = t(sc["R"]), t(sc["T"])
    g = torch.randn((1, sc["H"], sc["W"]), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    params = [gm.verts, gm.sigmas]

    def step():
        for p in params:
            p.grad = None
        frag = renderer(gm, R=Rt, T=Tt)
        D = get_depth(frag, background=BG)
        ((D * g).sum() + get_silhouette(frag).sum()).backward()
        return D
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            D_e = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_D = D_e.detach().clone()
    want = [p.grad.detach().clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        D_g = step()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(D_g, want_D)
    for p, w in zip(params, want):
        assert w.abs().max().item() > 0
        assert (p.grad - w).abs().max().item() <= 2e-4 * max(1.0, w.abs().max().item())      # (atomics: order of the sums)


def test_edited_fragments_and_existing_weights_take_the_depth_node(hip_lib):
    """Whatever is not an untouched scalar-sigma frame goes through ops._Depth with the same semantics: slots beyond valid_num
    never contribute (their len is 1e10), a user-made Fragments works, and valid_num above K is read as K."""
    from voge_amd.Renderer import Fragments, get_depth
    rng = np.random.default_rng(1)
    for K in (5, 8, 64, 130):
        P = 37
        w = rng.uniform(0, 0.6, (P, K))
        ln = np.sort(rng.uniform(1.4, 4.8, (P, K)), axis=-1)
        vn = rng.integers(0, K + 3, P)
        vn[:3] = 0
        dead = np.arange(K)[None] >= np.minimum(vn, K)[:, None]
        ln[dead] = 1e10
        w[dead & (rng.uniform(size=dead.shape) < 0.5)] = 0.25      # (garbage in dead slots must not count)
        idx = np.where(dead, -1, 1).astype(np.int32)
        for normalize in (True, False):
            wt, lt = t(w, rg=True), t(ln, rg=True)
            frag = Fragments(wt, t(idx, dtype=torch.int32), t(vn, dtype=torch.int64), lt)
            D = get_depth(frag, normalize=normalize, background=BG)
            w32, l32 = n(wt).astype(np.float64), n(lt).astype(np.float64)
            D_ref, S_ref, live = depth_ref(w32, l32, vn, normalize, BG)
            assert close(n(D), D_ref).all(), (K, normalize, max_rel(n(D), D_ref))
            assert (n(D)[vn == 0] == np.float32(BG if normalize else 0.0)).all()
            g = rng.normal(size=P)
            (D * t(g)).sum().backward()
            g_w, g_h = depth_grads_ref(w32, l32, vn, g, normalize)
            grad_close(f"_Depth K={K} normalize={normalize} g_weight", n(wt.grad), g_w, 0.25 * TOL)
            grad_close(f"_Depth K={K} normalize={normalize} g_len", n(lt.grad), g_h, 0.25 * TOL)
            assert (n(wt.grad)[dead] == 0).all() and (n(lt.grad)[dead] == 0).all()
