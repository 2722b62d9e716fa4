"""The fused backward's accumulation table (voge_common.h: WaveDirTable -- a directory of 256 keys probed by double hashing
over 96 dense value entries per wave, 512 keys in the kernel of scalar sigmas and three colour channels; fragment_bwd.hip) at the smallest shapes where it can go wrong: a 4x3 group with more
distinct Gaussians than the table has entries (the straight-to-memory path), keys that all hash to one directory slot, the
ordinary forms (K = 40, odd K, per-axis and full 3x3 sigmas), the repeatability of the atomics, and the other instantiations over
capacity through the renderer (3x3 with colours, per-axis with attributes and silhouette, oriented, the weights' own gradient at
K = 128, the depth form: groups of 289-457 distinct Gaussians over 256 keys, measured errors 2e-8 .. 7e-6 of scale; the frame's own
kernel with 664 over its 512 keys: 9e-6).  Synthetic lists for the same arms: tests/test_gpu_accumulation_tables.py.  Gradients are compared
with the fp64 oracle chain at the tolerance the whole-frame tests of test_gpu_configs.py use (1e-4 of max(1, largest entry))."""
import numpy as np
import pytest
import torch

from oracle import camera_np
import test_gpu_configs as cfg
from util import log_line

pytestmark = pytest.mark.gpu

ND, NEV, GW, GH = 512, 96, 4, 3      # fragment_bwd.hip: kFbNDFrame (the kernel these scenes run; 256 elsewhere), kFbNEV, kFbGW, kFbGH
MUL = 2654435761


def dir_slot(ids):
    """the directory slot a Gaussian id starts its probe sequence at (wd_find2: the top 9 bits of id * 2654435761 for 512 keys;
    ids that share it share the slot of a 256-key directory too)"""
    return ((np.asarray(ids, np.uint64) * MUL) & 0xFFFFFFFF) >> 23


def _radius_to_sigma(r):
    return (1.0 / (r * r / (2 * np.log(1 / 0.6)))).astype(np.float32)


def _scene(verts, sig, cols, H, W, K, focal, dist=3.0):
    return dict(verts=verts, sigmas=sig, colors=cols, focal=focal, principal=(W / 2.0, H / 2.0), image_size=(H, W), dist=dist,
                elev=10.0, azim=70.0, K=K)


def _group_distinct(idx):
    """distinct Gaussians of every 4x3 group of an [H, W, K] index array (-1: empty)"""
    H, W, _ = idx.shape
    out = []
    for y0 in range(0, H, GH):
        for x0 in range(0, W, GW):
            g = idx[y0:y0 + GH, x0:x0 + GW].ravel()
            out.append(len(np.unique(g[g >= 0])))
    return np.array(out)


def _grads_vs_oracle(label, sc, seed, min_same=0.9):
    frag, img, gm, colors, (R, T) = cfg._render(sc)
    ref = cfg._oracle_frame(sc, R, T)
    idx = cfg.n(frag.vert_index)
    same = (idx == np.where(ref["idx"] < 0, 0, ref["idx"])).all(-1) | (idx == ref["idx"]).all(-1)
    assert same.mean() >= min_same, f"{label}: only {same.mean():.3f} of the pixels have the oracle's index list"
    # (pixels whose member set differs from the oracle's leave the loss, as in test_gpu_configs.py: what remains is arithmetic)
    g_img = np.random.default_rng(seed).normal(size=ref["image"].shape) * same[..., None]
    (img * cfg.t(g_img)).sum().backward()
    want = cfg._oracle_grads(sc, ref, g_img)
    out = cfg._check_grads(label, (colors.grad, gm.verts.grad, gm.sigmas.grad), want, mult=1)
    return ref, out


def test_group_with_more_gaussians_than_table_entries(hip_lib):
    """16 x 12 pixels, K = 128 (the largest list the two-slots-per-lane kernel takes), 4000 Gaussians two to three pixels wide in a
    cube behind the image: a 4x3 group sees several hundred distinct ids, the table has 96 entries -- the rest goes straight
    to memory, key by key and whole."""
    H, W, K, N = 12, 16, 128, 4000
    rng = np.random.default_rng(11)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.8).astype(np.float32)
    sig = _radius_to_sigma(rng.uniform(0.07, 0.11, N))
    cols = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    sc = _scene(verts, sig, cols, H, W, K, focal=40.0, dist=4.0)
    ref, _ = _grads_vs_oracle("table over capacity 16x12 K=128", sc, seed=1)
    distinct = _group_distinct(ref["idx"][0])
    log_line(f"[table] over capacity: distinct Gaussians per 4x3 group min {distinct.min()} max {distinct.max()} ({NEV} entries); "
             f"hits per pixel max {(ref['idx'][0] >= 0).sum(-1).max()}")
    assert distinct.max() > NEV, "no group exceeds the table's entries: the scene does not test the straight-to-memory path"
    assert (ref["idx"][0] >= 0).sum(-1).max() > 64      # lists beyond one wave's 64 slots per pixel


def test_keys_that_share_one_directory_slot(hip_lib):
    """32 x 24, K = 40, 144 000 Gaussians of which only those whose id hashes to ONE directory slot stand in front of the camera
    (about 280; the others lie far off to the side): every look-up of the frame starts at the same slot and walks its
    double-hash sequence."""
    H, W, K, N = 24, 32, 40, 144000
    rng = np.random.default_rng(12)
    ids = np.arange(N)
    chosen = ids[dir_slot(ids) == 75]
    assert 200 < len(chosen) < 400
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.5 + np.array([0.0, 60.0, 0.0])).astype(np.float32)      # out of view
    verts[chosen] = rng.uniform(-0.6, 0.6, (len(chosen), 3)).astype(np.float32)
    sig = _radius_to_sigma(rng.uniform(0.08, 0.16, N))
    cols = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    sc = _scene(verts, sig, cols, H, W, K, focal=35.0)
    ref, _ = _grads_vs_oracle("table colliding keys 32x24 K=40", sc, seed=2)
    seen = np.unique(ref["idx"][ref["idx"] >= 0])
    assert len(seen) > 100 and (dir_slot(seen) == 75).all(), "the frame must see the chosen Gaussians and only them"
    distinct = _group_distinct(ref["idx"][0])
    log_line(f"[table] colliding keys: {len(seen)} Gaussians in view, all in directory slot 75; distinct per group max {distinct.max()}")
    assert distinct.max() > 16      # (more keys in one group than the probe limit: sequences must part after the first slot)


@pytest.mark.parametrize("K,form", [(40, "scalar"), (25, "scalar"), (40, "diag"), (40, "full")])
def test_ordinary_scenes(hip_lib, K, form):
    """64 x 48, 3000 Gaussians: K = 40, K = 25 (odd: the slot-by-slot loads), (N,3) per-axis and [N,3,3] sigmas."""
    from voge_amd import scenes
    H, W, N = 48, 64, 3000
    verts, sig, cols = scenes.random_gaussians(N, seed=5, anisotropic={"scalar": False, "diag": "diag", "full": True}[form],
                                               r_lo=0.04, r_hi=0.11)
    sc = _scene(verts, sig, cols, H, W, K, focal=70.0)
    ref, _ = _grads_vs_oracle(f"table ordinary 64x48 K={K} {form}", sc, seed=3)
    assert (ref["idx"] >= 0).sum(-1).max() == K and _group_distinct(ref["idx"][0]).max() > 20


def test_two_backwards_agree_within_the_atomics_noise(hip_lib):
    """The table's sums per Gaussian and wave are bit-identical from run to run; only the order of the waves' global atomics
    differs.  bench.py bounds that at 1e-4 of the largest entry (measured 2e-6)."""
    from voge_amd import scenes
    verts, sig, cols = scenes.random_gaussians(3000, seed=5, r_lo=0.04, r_hi=0.11)
    sc = _scene(verts, sig, cols, 48, 64, 40, focal=70.0)
    g_img = np.random.default_rng(4).normal(size=(1, 48, 64, 3))
    runs = []
    for _ in range(2):
        frag, img, gm, colors, _ = cfg._render(sc)
        (img * cfg.t(g_img)).sum().backward()
        runs.append([cfg.n(x).astype(np.float64) for x in (colors.grad, gm.verts.grad, gm.sigmas.grad)])
    for name, a, b in zip(("colors", "verts", "sigmas"), *runs):
        d = np.abs(a - b).max() / np.abs(a).max()
        log_line(f"[table] repeatability {name}: {d:.2e} of the largest entry (bound 1e-4)")
        assert np.abs(a).max() > 0 and d <= 1e-4


# ---- the other instantiations over capacity, through the renderer ------------------------------------------------------------------
# Scenes of the size class above (16 x 12 pixels, K = 64 .. 128, thousands of Gaussians two to three pixels wide) through the routes
# tests/test_gpu_fragment_bwd_entries.py knows (its consume / reference_outputs and fp64 torch_ref autograd), one per table
# instantiation the frame's own kernel does not cover.  (name, entry, Gaussians' form, consumer, K, C, Gaussians, radii, the
# distinct ids the fullest 4x3 group must exceed: the 256 directory keys, so that look-ups also end with their probes run out)
OVER_H, OVER_W, OVER_FOCAL, OVER_VIEW = 12, 16, 40.0, {1: ([4.0], [10.0], [70.0])}
OVER_CAPACITY = [
    ("full-white", "voge_frame_bwd_gen", "full", "white", 64, 3, 6000, (0.05, 0.08), 256),                # NV4 = 4
    ("diag-attr-sil", "voge_frame_bwd_gen", "diag", "attr_sil", 64, 4, 6000, (0.05, 0.08), 256),          # DIAG, NV4 = 3
    ("oriented-white", "voge_frame_bwd_ori", "ori", "white", 64, 3, 6000, (0.05, 0.08), 256),
    ("scalar-weight-K128", "voge_fragment_bwd_iso", "scalar", "weight", 128, 3, 4000, (0.07, 0.11), 256),  # NV4 = 1
    ("scalar-depth", "voge_frame_depth_bwd_iso", "scalar", "depth_norm", 64, 3, 6000, (0.05, 0.08), 256),  # the depth form
]


def dense_gaussians(form, N, radii, seed=11):
    """N Gaussians in a cube of side 1.6 around the origin (the scene of test_group_with_more_gaussians_than_table_entries), their
    sigmas in one of the forms of test_gpu_fragment_bwd_entries.scene -> verts, sigmas | scales, quats | None, colours [N, 4]"""
    rng = np.random.default_rng(seed)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.8).astype(np.float32)
    s = _radius_to_sigma(rng.uniform(radii[0], radii[1], N))
    quats = None
    if form == "scalar":
        sig = s
    elif form in ("diag", "ori"):
        sig = (s[:, None] * rng.uniform(0.6, 1.6, (N, 3))).astype(np.float32)
        if form == "ori":
            quats = (rng.normal(size=(N, 4)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    else:
        L = np.tril(rng.uniform(-1, 1, (N, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
        L = L * np.sqrt(s)[:, None, None] * 0.8
        sig = (L @ L.transpose(0, 2, 1)).astype(np.float32)
    return verts, sig, quats, rng.uniform(0, 1, (N, 4)).astype(np.float32)


@pytest.mark.parametrize("c", OVER_CAPACITY, ids=lambda c: c[0])
def test_other_instantiations_over_capacity(hip_lib, monkeypatch, c):
    import test_gpu_depth as dpt
    import test_gpu_fragment_bwd_entries as E
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes
    from util import TOL, grad_close
    name, entry, form, consumer, K, C, N, radii, need = c
    H, W = OVER_H, OVER_W
    for k, v in dict(H=H, W=W, FOCAL=OVER_FOCAL, VIEWS=OVER_VIEW).items():      # (E.reference renders E's own frame: give it this one)
        monkeypatch.setattr(E, k, v)
    verts, sig, quats, cols = dense_gaussians(form, N, radii)
    ref = E.reference(form, 1, K, verts, sig, quats)
    calls = E.spy_on(monkeypatch)
    gm = (OrientedGaussianMeshes(cfg.t(verts), cfg.t(sig), cfg.t(quats)) if form == "ori" else GaussianMeshes(cfg.t(verts), cfg.t(sig))).to(cfg.DEV)
    frag = dpt.renderer_for(H, W, K, OVER_FOCAL)(gm, R=cfg.t(ref["R"]), T=cfg.t(ref["T"]))
    colors = cfg.t(cols[:, :C], rg=True)
    got = E.consume(consumer, frag, colors, C)
    idx, ridx = cfg.n(frag.vert_index).reshape(H * W, K), cfg.n(ref["idx"][0])
    same = (idx == np.where(ridx < 0, 0, ridx)).all(-1) | (idx == ridx).all(-1)
    distinct = _group_distinct(ridx.reshape(H, W, K))
    log_line(f"[table] {name}: distinct Gaussians per 4x3 group min {distinct.min()} max {distinct.max()}; hits per pixel max "
             f"{(ridx >= 0).sum(-1).max()}; {same.mean():.3f} of the pixels have the reference's index list")
    assert distinct.max() > need, f"{name}: no group exceeds {need} distinct Gaussians"
    assert same.mean() >= 0.9, f"{name}: only {same.mean():.3f} of the pixels have the reference's index list"
    rng = np.random.default_rng(17)
    colors64 = torch.tensor(cols[:, :C], dtype=torch.float64, requires_grad=True)
    loss_gpu, loss_ref = 0.0, 0.0
    for out, r in zip(got, E.reference_outputs(consumer, ref, 0, colors64)):
        shape = (H * W,) + tuple(out.shape[3:])
        G = rng.normal(size=shape) * same.reshape((H * W,) + (1,) * (len(shape) - 1))      # (a flipped pixel leaves the loss: the selection is discrete)
        loss_gpu = loss_gpu + (out.reshape(shape) * cfg.t(G)).sum()
        loss_ref = loss_ref + (r * torch.tensor(G)).sum()
    loss_gpu.backward()
    torch.cuda.synchronize()
    loss_ref.backward()
    assert [nm for nm, _ in calls] == [entry], (name, [nm for nm, _ in calls])
    assert calls[0][1]["K"] == K
    pairs = [("verts", gm.verts.grad, ref["verts"].grad), ("scales" if form == "ori" else "sigmas", (gm.scales if form == "ori" else gm.sigmas).grad,
                                                            ref["p1"].grad)]
    if form == "ori":
        pairs.append(("quats", gm.quats.grad, ref["quats"].grad))
    if consumer in ("white", "attr_sil"):
        pairs.append(("colors", colors.grad, colors64.grad))
    for what, g, want in pairs:
        assert g is not None and want is not None and float(want.abs().max()) > 0, (name, what)
        grad_close(f"[table] {name} over capacity {what}", cfg.n(g), cfg.n(want), TOL)


def test_frame_kernel_group_with_more_gaussians_than_directory_keys(hip_lib):
    """The frame's own kernel (scalar sigmas, three colour channels: 512 directory keys) on 8000 Gaussians one to two pixels wide at
    K = 128: a 4x3 group names more distinct ids than the directory has keys, so keys end with their probes run out in a full
    directory, on top of those that find the 96 entries handed out."""
    H, W, K, N = 12, 16, 128, 8000
    rng = np.random.default_rng(11)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.8).astype(np.float32)
    sig = _radius_to_sigma(rng.uniform(0.05, 0.08, N))
    cols = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    sc = _scene(verts, sig, cols, H, W, K, focal=40.0, dist=4.0)
    ref, _ = _grads_vs_oracle("table over the directory 16x12 K=128", sc, seed=6)
    distinct = _group_distinct(ref["idx"][0])
    log_line(f"[table] over the directory: distinct Gaussians per 4x3 group min {distinct.min()} max {distinct.max()} ({ND} keys)")
    assert distinct.max() > ND, "no group exceeds the directory's keys"
