"""The composite backward's two window walks with ONE accumulator set and ONE reach bound per walk (composite_core.h:
compn_bwd_wave), fused (voge_fragment_bwd*, the frame path's kernels) and stand-alone (voge_composite_bwd), against the fp64
oracle (oracle.composite_bwd, then oracle.trace_bwd) at the project's TOL = 1e-4 of scale -- the bound
tests/test_gpu_composite_routes.py holds the same gradients to.

Synthetic lists, a frame of 12 x 16 pixels over 60 Gaussians (140 at K = 130: a list names a Gaussian once), per K:
  K = 1 no walk; K = 2 the diagonal block alone; K = 3, 5 odd, slot by slot; K = 40 the flagship forms; K = 130 four slots per lane.
Pixels built for what the walks and their bound can get wrong (KINDS below): no hit and one hit; every Gaussian at ONE depth (all
gaps 0: every window covers the list); a very flat Gaussian first / last in its list (its window runs into the sentinel pair at the
far end, through every row); a very sharp one (s = 300: no row inside its window); an odd count (a lane with one live and one empty
column, whose sentinel len must not widen the bound); the rest random sorted lists of every count.  Five of them are repeated
at other places of the frame: a pixel's bits do not depend on where it sits, and a band of rows launched alone has the bits of
those rows in the frame (the stand-alone kernel writes per-pixel gradients, so this is exact; the fused kernel sums per Gaussian
with atomics, whose order differs from run to run by 1e-7 .. 2e-6 of scale -- its band is held to 2e-5, the figure
tests/test_gpu_frame.py allows two backward passes over one graph).

An unsorted list goes through the public entry (ops.composite): the cold K x K scan is not part of the change and must give the bits
the golden file of tests/test_gpu_erfc_walks.py holds for it.  Real frames of the same size through the renderer: scalar sigmas
(the kernel bench.py times, act / dsd re-derived from the records), per-axis and 3 x 3 sigmas, against the oracle's whole chain.

Measured on MI355X (largest error of scale over the arrays; the commit before the change gives the same figures to two digits):
  K     stand-alone   fused     fused band against the masked frame
  1     8.1e-07       8.1e-07   2.0e-08
  2     1.0e-06       1.2e-06   8.7e-08
  3     1.2e-06       1.4e-06   9.7e-08
  5     1.4e-06       2.0e-06   4.4e-08
  40    1.1e-06       7.1e-07   1.6e-07
  130   1.7e-06       1.0e-06   8.4e-08
  real frames (colours / verts / sigmas): scalar K = 40 6.9e-07 / 1.4e-06 / 4.1e-07, per-axis 3.3e-07 / 1.0e-06 / 3.4e-07,
  3 x 3 1.1e-06 / 1.2e-06 / 1.4e-06; their bands 3e-08 .. 2.6e-07.  (With the sharp Gaussian at s = 1e4 the same lists gave
  9.9e-05 in g_len at K = 2, before and after the change: see build_lists.)"""
import numpy as np
import pytest
import torch

import oracle
from oracle import camera_np
from util import TOL, grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 12, 16
NPIX = H * W
OCC = 0.9
K_LIST = (1, 2, 3, 5, 40, 130)
BAND = (4, 9)
KINDS = ("empty", "one", "one_depth", "flat_first", "flat_last", "sharp", "odd")
COPIES = {150 + i: 2 + i for i in range(5)}      # destination: source (one_depth .. odd)
ORDER_TOL = 2e-5


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def n_gauss(K):
    return max(60, K + 10)


def build_lists(K):
    """-> idx [NPIX,K] int32, act, ln, dsd fp32 (empty slots: -1, 1e10, 1e10, 0 -- what the trace leaves), nv [NPIX]."""
    rng = np.random.default_rng(1900 + K)
    P = n_gauss(K)
    idx, act = np.full((NPIX, K), -1, np.int32), np.full((NPIX, K), 1e10, np.float32)
    ln, dsd = np.full((NPIX, K), 1e10, np.float32), np.zeros((NPIX, K), np.float32)
    nv = np.zeros(NPIX, np.int64)
    for p in range(NPIX):
        if p in COPIES:
            continue
        kind = KINDS[p] if p < len(KINDS) else "random"
        c = {"empty": 0, "one": 1, "odd": K - 1 if K % 2 == 0 else K - 2,
             "random": int(rng.integers(1, (min(K, 8) if p % 2 else K) + 1))}.get(kind, K)      # (every second list short: every small count)
        c = int(np.clip(c, 0 if kind == "empty" else 1, K))
        s = rng.uniform(0.5, 8.0) * rng.uniform(0.7, 1.4, c)
        steps = rng.uniform(0.05, 2.0, c) / s      # (a fraction of a window, or a window and a half, of the list's ordinary Gaussians)
        if kind == "one_depth":
            steps[:] = 0.0
        if kind == "flat_first" and c:
            s[0] = 1e-3
        if kind == "flat_last" and c:
            s[c - 1] = 1e-3
        if kind == "sharp" and c:      # (300, not more: g_len's two self terms u E s phi(0) cancel, and what fp32 leaves of them grows with s)
            steps = rng.uniform(0.5, 2.0, c) / s
            s[c // 2] = 300.0
        ln[p, :c] = (rng.uniform(1.0, 2.0) + np.cumsum(steps) - steps[:1].sum()).astype(np.float32) if c else 0
        ln[p, :c] = np.maximum.accumulate(ln[p, :c])      # (fp32 rounding of a cumulative sum never unsorts)
        dsd[p, :c] = (s * s).astype(np.float32)
        act[p, :c] = rng.uniform(0.0, 4.0, c)
        idx[p, :c] = rng.permutation(P)[:c]
        nv[p] = c
    for d, s_ in COPIES.items():
        idx[d], act[d], ln[d], dsd[d], nv[d] = idx[s_], act[s_], ln[s_], dsd[s_], nv[s_]
    return idx, act, ln, dsd, nv


def composite_gpu(K, idx, act, ln, dsd, gw):
    """voge_composite_fwd, then voge_composite_bwd with its weights -> w, (g_act, g_len, g_dsd), each [pixels, K]."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    npix = idx.shape[0]
    ti, ta, tl, td, tg = t(idx, torch.int32), t(act), t(ln), t(dsd), t(gw)
    w = torch.full_like(ta, -7.0)
    vn = torch.full((npix,), -7, dtype=torch.int64, device=DEV)
    assert lib.voge_composite_fwd(ti.data_ptr(), None, ta.data_ptr(), tl.data_ptr(), td.data_ptr(), OCC, npix, K, w.data_ptr(), vn.data_ptr(), st) == 0
    outs = [torch.full_like(ta, -7.0) for _ in range(3)]
    assert lib.voge_composite_bwd(ta.data_ptr(), tl.data_ptr(), td.data_ptr(), w.data_ptr(), None, tg.data_ptr(), OCC, npix, K,
                                  *[o.data_ptr() for o in outs], st) == 0
    torch.cuda.synchronize()
    return n(w), np.stack([n(o) for o in outs])


def fused_gpu(K, g, idx, act, ln, dsd, nv, w, gw, rows):
    """voge_fragment_bwd (3 x 3 Sigma^-1, act / dsd given) on the rows [rows[0], rows[1]) of the frame -> g_mus, g_isigmas."""
    from voge_amd import ops
    sl = slice(rows[0] * W, rows[1] * W)
    h = rows[1] - rows[0]
    tm, ts = t(g["mus"]), t(g["isg"])
    P = g["mus"].shape[0]
    g_mus, g_isg = ops._fragment_bwd(0, tm, ts, None, False, 0, t(g["rays"][sl]).reshape(1, h, W, 3), t(idx[sl], torch.int32).reshape(1, h, W, K),
                                     t(nv[sl], torch.int32), 1, P, (tm, ts), t(w[sl]), t(act[sl]), t(ln[sl]), t(dsd[sl]), t(gw[sl]), None, OCC)
    torch.cuda.synchronize()
    return n(g_mus), n(g_isg).reshape(P, 3, 3)


def gaussians(K):
    rng = np.random.default_rng(5 + K)
    P = n_gauss(K)
    mus = rng.uniform(-1, 1, (P, 3)).astype(np.float32) + np.array([0, 0, 4], np.float32)
    L = np.tril(rng.uniform(-1, 1, (P, 3, 3)))
    L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
    rays = rng.normal(size=(NPIX, 3)) * 0.2 + np.array([0, 0, 1.0])
    return dict(mus=mus, isg=(L @ L.transpose(0, 2, 1)).astype(np.float32), rays=(rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32))


@pytest.fixture(scope="module", params=K_LIST)
def case(request, hip_lib):
    K = request.param
    idx, act, ln, dsd, nv = build_lists(K)
    gw = np.random.default_rng(77 + K).normal(size=(NPIX, K)).astype(np.float32)
    gw[list(COPIES)] = gw[list(COPIES.values())]
    w, got = composite_gpu(K, idx, act, ln, dsd, gw)
    gr = np.stack(oracle.composite_bwd(act, ln, dsd, gw, OCC))
    return dict(K=K, idx=idx, act=act, ln=ln, dsd=dsd, nv=nv, gw=gw, w=w, got=got, gr=gr, g=gaussians(K))


def test_lists_hold_every_kind(case):
    """The inputs alone: sorted, the kinds present with the counts they are meant to have."""
    K, nv, ln, dsd = case["K"], case["nv"], case["ln"], case["dsd"]
    for p in range(NPIX):
        assert (np.diff(ln[p, :nv[p]]) >= 0).all() and (case["idx"][p, nv[p]:] == -1).all() and (ln[p, nv[p]:] == np.float32(1e10)).all()
        assert len(set(case["idx"][p, :nv[p]].tolist())) == nv[p]
    assert nv[0] == 0 and nv[1] == 1 and nv[2] == K and (np.diff(ln[2]) == 0).all()
    if K >= 3:
        assert nv[6] % 2 == 1 and nv[6] >= 1 and np.isclose(dsd[3, 0], 1e-6) and np.isclose(dsd[4, K - 1], 1e-6) and dsd[5, K // 2] == np.float32(9e4)
        # the flat Gaussian's window holds the whole list and both sentinel pairs stop it; nothing lies inside the sharp one's
        assert (ln[3, K - 1] - ln[3, 0]) * 1e-3 < 3.5 and (ln[4, K - 1] - ln[4, 0]) * 1e-3 < 3.5
        assert min(ln[5, K // 2 + 1] - ln[5, K // 2], ln[5, K // 2] - ln[5, K // 2 - 1]) * 300.0 > 3.5
    assert set(nv.tolist()) >= set(range(0, min(K, 6) + 1))


def test_stand_alone_gradients_within_tol(case):
    got = case["got"]
    assert np.isfinite(got).all() and (got[:, case["idx"] < 0] == 0).all()
    for name, g, ref in zip(("g_act", "g_len", "g_dsd"), got, case["gr"]):
        grad_close(f"bwd walks K={case['K']} stand-alone {name}", g, ref, TOL)
        grad_close(f"bwd walks K={case['K']} stand-alone {name} (the built pixels)", g[:len(KINDS)], ref[:len(KINDS)], TOL)


def test_a_pixel_has_the_same_bits_anywhere_and_in_a_band(case):
    K, got = case["K"], case["got"]
    dst, src = list(COPIES), list(COPIES.values())
    assert np.array_equal(np.ascontiguousarray(got[:, dst]).view(np.uint32), np.ascontiguousarray(got[:, src]).view(np.uint32))
    sl = slice(BAND[0] * W, BAND[1] * W)
    wb, gb = composite_gpu(K, *(case[k][sl] for k in ("idx", "act", "ln", "dsd", "gw")))
    assert np.array_equal(wb.view(np.uint32), np.ascontiguousarray(case["w"][sl]).view(np.uint32))
    assert np.array_equal(gb.view(np.uint32), np.ascontiguousarray(got[:, sl]).view(np.uint32))


def test_fused_gradients_within_tol_and_band(case):
    K = case["K"]
    lists = tuple(case[k] for k in ("idx", "act", "ln", "dsd", "nv", "w", "gw"))
    g_mus, g_isg = fused_gpu(K, case["g"], *lists, rows=(0, H))
    ga, gl, gd = case["gr"]
    _, rm, rs = oracle.trace_bwd(case["g"]["mus"], case["g"]["isg"], case["g"]["rays"], case["idx"], gl, ga, gd)
    assert np.abs(rm).max() > 0 and np.abs(rs).max() > 0
    grad_close(f"bwd walks K={K} fused g_mus", g_mus, rm, TOL)
    grad_close(f"bwd walks K={K} fused g_isigmas", g_isg, rs, TOL)
    # the band alone against the frame with the loss masked to the band (an unlit gradient of the weights gives a pixel no term)
    masked = case["gw"].copy()
    masked[:BAND[0] * W] = 0
    masked[BAND[1] * W:] = 0
    fm, fs = fused_gpu(K, case["g"], *lists[:6], masked, rows=(0, H))
    bm, bs = fused_gpu(K, case["g"], *lists, rows=BAND)
    grad_close(f"bwd walks K={K} fused band g_mus", bm, fm, ORDER_TOL)
    grad_close(f"bwd walks K={K} fused band g_isigmas", bs, fs, ORDER_TOL)


def test_unsorted_list_keeps_the_cold_scan_through_the_public_entry(hip_lib):
    import test_gpu_erfc_walks as E
    from voge_amd import ops
    K = 40
    cold = np.load(E.COLD_FILE)
    idx, act, ln, dsd, _ = build_lists(K)
    rows = [7, 8, 0, 2, 9]
    idx, act, ln, dsd = (np.concatenate([a[rows], cold[f"in_{k}_k{K}"]]) for a, k in ((idx, "idx"), (act, "act"), (ln, "len"), (dsd, "dsd")))
    gw = np.random.default_rng(77 + K).normal(size=(E.NPIX, K)).astype(np.float32)      # (what the golden file's gradients were taken with)
    gw = np.concatenate([gw[:len(rows)], gw[[E.UNSORTED, E.NAN_LEN]]])
    ta, tl, td = (t(a, rg=True) for a in (act, ln, dsd))
    w, _ = ops.composite(t(idx, torch.int32), ta, tl, td, E.OCC)
    w.backward(t(gw))
    torch.cuda.synchronize()
    got = np.stack([n(ta.grad), n(tl.grad), n(td.grad)])
    assert np.array_equal(np.ascontiguousarray(got[:, len(rows):]).view(np.uint32), cold[f"g_given_k{K}"]), "the cold scan's bits moved"
    gr = np.stack(oracle.composite_bwd(act[:-1], ln[:-1], dsd[:-1], gw[:-1], E.OCC))      # (all but the NaN len)
    for name, g, ref in zip(("g_act", "g_len", "g_dsd"), got[:, :-1], gr):
        grad_close(f"bwd walks public entry, sorted and unsorted lists, {name}", g, ref, TOL)


@pytest.mark.parametrize("kind,K", [("scalar", 40), ("diag", 14), ("full", 14)])
def test_real_frames_against_the_oracle_chain(hip_lib, kind, K):
    """12 x 16 pixels, 60 wide Gaussians, through the renderer's frame path: scalar sigmas run the kernel bench.py times."""
    import test_gpu_configs as C
    from voge_amd import scenes
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, to_white_background
    from voge_amd.cameras import PerspectiveCameras
    verts, sig, cols = scenes.random_gaussians(60, seed=19, anisotropic={"scalar": False, "diag": "diag", "full": True}[kind], r_lo=0.25, r_hi=0.6)
    R, T = camera_np.look_at_view_transform(3.5, 12.0, 40.0)
    size = (H, W)
    sc = dict(verts=verts, sigmas=sig, colors=cols, focal=20.0, principal=(8.25, 5.5), image_size=size, K=K)
    cams = PerspectiveCameras(focal_length=20.0, principal_point=((8.25, 5.5),), image_size=(size,), device=DEV)
    renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=size, max_assign=K, max_point_per_bin=-1)).to(DEV)
    ref = C._oracle_frame(sc, R, T)
    g_rng = np.random.default_rng(6).normal(size=ref["image"].shape)
    grads = {}
    for rows in (None, BAND):
        gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
        colors = t(cols, rg=True)
        frag = renderer(gm, R=t(R), T=t(T), **({} if rows is None else dict(rows=rows)))
        assert frag._lazy is not None and frag._lazy.frame
        img = to_white_background(frag, colors)
        if rows is None:
            same = C._check_frame(f"bwd walks {kind} frame K={K}", frag, img, ref, max_flips=8)
            assert same.mean() > 0.9 and ref["valid_num"].max() >= min(K, 12) and (ref["valid_num"] % 2 == 1).any()
            g_img = g_rng * same[..., None]
            whole = n(img)
            (img * t(g_img)).sum().backward()
            C._check_grads(f"bwd walks {kind} frame K={K}", (colors.grad, gm.verts.grad, gm.sigmas.grad), C._oracle_grads(sc, ref, g_img), mult=1)
            g_band = g_img.copy()
            g_band[:, :BAND[0]] = 0
            g_band[:, BAND[1]:] = 0
            gm2, colors2 = GaussianMeshes(t(verts), t(sig)).to(DEV), t(cols, rg=True)
            (to_white_background(renderer(gm2, R=t(R), T=t(T)), colors2) * t(g_band)).sum().backward()
            grads["masked"] = (colors2.grad, gm2.verts.grad, gm2.sigmas.grad)
        else:
            assert np.array_equal(n(img).view(np.uint32), np.ascontiguousarray(whole[:, rows[0]:rows[1]]).view(np.uint32))      # the forward is untouched
            (img * t(g_img[:, rows[0]:rows[1]])).sum().backward()
            grads["band"] = (colors.grad, gm.verts.grad, gm.sigmas.grad)
    for name, a, b in zip(("colors", "verts", "sigmas"), grads["band"], grads["masked"]):
        grad_close(f"bwd walks {kind} frame K={K} band against the masked frame, {name}", n(a), n(b), ORDER_TOL)
