"""CPU side of the attribute-route tests: the inputs tests/test_gpu_attr_routes.py feeds to every kernel route of merge, blend and
the sampler (voge_amd/csrc/merge_blend.hip) and to the dense-ray extras (voge_amd/csrc/extras.hip) are BUILT here, so that both
files see the same numbers, and their CONDITIONING is asserted here.  Nothing in this file measures a kernel.

Tolerance rules the GPU file applies (none is invented there): values at util.close / util.TOL (1e-4 relative to max(1, |ref|));
gradients summed by float atomics at util.grad_close / TOL of the gradient's scale; a copy, a maximum or an integer exactly.
What this file guarantees for that: every decision of a blend case (min(x, 1), sil > thr, min(sum w, 1)) sits at least 1e-2 away
from its switch -- no pixel is ever excluded from a comparison --, and the fp32 evaluation of the reference alone stays within
TOL / 4 of its fp64 value on every case, so the reference cannot use up the tolerance."""
import numpy as np
import pytest
import torch

from oracle import extras_np, torch_ref
from util import TOL

GRID_A, GRID_B = (1, 11, 13), (2, 5, 9)      # 143 and 90 pixels: no multiple of 4, 8, 16 or 32 -- ragged last wave, ragged last tile
MARGIN = 1e-2
THR = 0.3
MPC_SLOTS = 1024      # kMpcSlots of merge_blend.hip


# ---- the dispatch of voge_shade_fwd / voge_merge_bwd, restated ----------------------------------------------------------------------
def fwd_route(K, C, aligned=True, Nattr=50):
    return "fwd4" if (K % 4 == 0 and K <= 64 and aligned) else "pc" if (1 <= C <= 64 and K <= MPC_SLOTS and Nattr > 0) else "general"


def bwd_route(C):
    return "tile" if C <= 4 else "slot" if C <= 64 else "chan"


# ---- the synthetic fragments ----------------------------------------------------------------------------------------------------------------
def _draw_target(rng, n):
    u = rng.random(n)
    t = np.where(rng.random(n) < 0.5, 0.2 + 0.75 * u, 1.05 + 0.75 * u)      # [0.2, 0.95] u [1.05, 1.8]
    near = np.abs(t - THR) < 2 * MARGIN
    return np.where(near, t + 4 * MARGIN, t)      # (the silhouette mask's switch: sil > 0.3)


def _blend_x(w32, rgb64, bg32):
    """x = rgb + (1 - mask(sil)) bg for both thresholds the tests use, in fp64 from the fp32 inputs -> [2, P, C]."""
    s = w32.astype(np.float64).sum(-1)
    sil = np.minimum(s, 1.0)
    return np.stack([rgb64 + (1 - sil)[:, None] * bg32[None].astype(np.float64),
                     rgb64 + (1 - (sil > THR))[:, None] * bg32[None].astype(np.float64)])


def _merge_np(attr, w, vn, idx):
    K = idx.shape[-1]
    live = np.arange(K)[None] < vn[:, None]
    return (attr.astype(np.float64)[np.maximum(idx, 0)] * (w.astype(np.float64) * live)[..., None]).sum(1)


def attr_case(npix_shape, K, C, Nattr=50, seed=0, blend=False):
    """Fragments + attributes by the recipe of the module docstring's tests -> dict of numpy arrays:
      idx [.., K] int32       uniform in [0, Nattr), -1 from a random per-pixel count on
      valid_num [..] int64    that count + an offset in [-2, 2], clipped to [0, K]: live slots hold -1 (they read row 0), masked slots
                              hold real indices; pixel 1 has valid_num = 0 and the last but one valid_num = K
      weight [.., K] fp32     positive, ~5 % exact zeros, each pixel's sum at a target drawn from [0.2, 0.95] u [1.05, 1.8]
      attr [Nattr, C] fp32    ~ N(0, 1) (blend: times max(1, 0.8 sqrt(K)));   bg [C] fp32 in [0.1, 0.9];   g [.., C] fp32 ~ N(0, 1), the upstream gradient
    blend=True also keeps every rgb + (1 - mask) bg (mask = min(sum w, 1), or [that > 0.3]) at least MARGIN from 1: a pixel that
    comes closer has its target redrawn (nothing else of it changes), so no pixel needs to be left out of a comparison."""
    rng = np.random.default_rng(seed)
    P = int(np.prod(npix_shape))
    cnt = rng.integers(0, K + 1, P)
    idx = rng.integers(0, Nattr, (P, K)).astype(np.int32)
    idx[np.arange(K)[None] >= cnt[:, None]] = -1
    vn = np.clip(cnt + rng.integers(-2, 3, P), 0, K).astype(np.int64)
    vn[1], vn[-2] = 0, K
    w0 = rng.uniform(0.05, 1.0, (P, K))
    w0[rng.random((P, K)) < 0.05] = 0.0
    w0[w0.sum(-1) == 0, 0] = 0.5
    w0 /= w0.sum(-1, keepdims=True)
    # (blend: rgb is a sum of K weighted rows, ~ N(0, 1 / K); scaled so that it stays of order 1 and crosses the clamp at any K)
    attr = (rng.normal(size=(Nattr, C)) * (max(1.0, 0.8 * np.sqrt(K)) if blend else 1.0)).astype(np.float32)
    bg = rng.uniform(0.1, 0.9, C).astype(np.float32)
    g = rng.normal(size=(P, C)).astype(np.float32)
    target = _draw_target(rng, P)
    w = (w0 * target[:, None]).astype(np.float32)
    raw_gap = float(np.abs(w.astype(np.float64).sum(-1) - 1).min())      # smallest |sum w - 1| before any margin is enforced
    if blend:
        for _ in range(400):
            x = _blend_x(w, _merge_np(attr, w, vn, idx), bg)
            bad = (np.abs(x - 1) < 1.2 * MARGIN).any(axis=(0, 2))
            if not bad.any():
                break
            target[bad] = _draw_target(rng, int(bad.sum()))
            w[bad] = (w0[bad] * target[bad, None]).astype(np.float32)
        else:
            raise AssertionError("no target keeps every channel of some pixel away from the clamp")
    sh = tuple(npix_shape)
    return dict(idx=idx.reshape(sh + (K,)), valid_num=vn.reshape(sh), weight=w.reshape(sh + (K,)), attr=attr, bg=bg,
                g=g.reshape(sh + (C,)), K=K, C=C, Nattr=Nattr, raw_gap=raw_gap)


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------
# merge: (grid, K, C, Nattr, aligned, forward route, backward route)
MERGE_CASES = [
    (GRID_A, 1, 1, 50, True, "pc", "tile"),
    (GRID_B, 3, 2, 50, True, "pc", "tile"),
    (GRID_A, 4, 3, 50, True, "fwd4", "tile"),
    (GRID_B, 12, 4, 50, True, "fwd4", "tile"),
    (GRID_A, 40, 3, 50, True, "fwd4", "tile"),
    (GRID_B, 65, 4, 50, True, "pc", "tile"),
    (GRID_A, 100, 3, 50, True, "pc", "tile"),
    (GRID_B, 600, 2, 50, True, "pc", "tile"),          # pixels per wave limited by K: 1024 // 600 = 1
    (GRID_B, 1028, 3, 50, True, "general", "tile"),
    (GRID_B, 12, 5, 50, True, "fwd4", "slot"),
    (GRID_A, 13, 5, 50, True, "pc", "slot"),           # 12 pixels x 5 channels = 60 lanes: four idle
    (GRID_B, 3, 7, 50, True, "pc", "slot"),            # 9 x 7 = 63 lanes: one idle
    (GRID_B, 12, 7, 1, True, "fwd4", "slot"),          # one attribute row
    (GRID_A, 64, 16, 50, True, "fwd4", "slot"),
    (GRID_B, 65, 16, 50, True, "pc", "slot"),
    (GRID_A, 68, 63, 50, True, "pc", "slot"),
    (GRID_B, 100, 64, 50, True, "pc", "slot"),
    (GRID_A, 102, 6, 50, True, "pc", "slot"),          # the cuboid-optimisation demo's shape
    (GRID_A, 1028, 5, 50, True, "general", "slot"),    # leaves the per-channel kernel because of K
    (GRID_A, 12, 65, 50, True, "fwd4", "chan"),
    (GRID_B, 13, 65, 50, True, "general", "chan"),
    (GRID_A, 12, 100, 50, True, "fwd4", "chan"),       # 25 channel passes
    (GRID_B, 13, 100, 50, True, "general", "chan"),
    (GRID_A, 12, 3, 50, False, "pc", "tile"),          # unaligned views: the same values from the other routes
    (GRID_B, 12, 7, 50, False, "pc", "slot"),
    (GRID_A, 12, 100, 50, False, "general", "chan"),
]
MERGE_C = {1, 2, 3, 4, 5, 7, 16, 63, 64, 65, 100}
MERGE_K = {1, 3, 4, 12, 40, 64, 65, 68, 100, 1028}

# blend with a constant colour: (grid, K, C), each at thr = -1 and thr = 0.3
BLEND_CASES = [(GRID_A, 1, 1), (GRID_B, 5, 3), (GRID_A, 12, 4), (GRID_B, 64, 5), (GRID_A, 100, 8), (GRID_B, 5, 9), (GRID_A, 12, 65),
               (GRID_B, 1, 8), (GRID_A, 64, 3), (GRID_B, 100, 4), (GRID_A, 5, 5)]
BLEND_THR = [-1.0, THR]
SHADE_DIRECT = (GRID_A, 5, 6)      # voge_shade_fwd with attr, out_rgb and out_img at once: merge + image in the general kernel

# sampler: image channels (the kernels see one more: [image | 1]) x an odd and an even K
SAMPLER_CHANNELS = [1, 3, 4, 7, 63, 64, 99]
SAMPLER_K = [5, 12]


def case_id(c):
    return f"{'x'.join(map(str, c[0]))}-K{c[1]}-C{c[2]}" + ("" if len(c) < 5 else ("-N1" if c[3] == 1 else "") + ("" if c[4] else "-unaligned"))


def merge_case(c):
    return attr_case(c[0], c[1], c[2], Nattr=c[3], seed=1000 + 7 * c[1] + c[2])


def blend_case(c):
    return attr_case(c[0], c[1], c[2], seed=2000 + 7 * c[1] + c[2], blend=True)


def sampler_case(C, K):
    """Fragments of attr_case on GRID_B and an image [2, 5, 9, C] in [0, 1]; upstream gradients for features and weight sums."""
    case = attr_case(GRID_B, K, 1, seed=3000 + 7 * K + C)
    rng = np.random.default_rng(3500 + 7 * K + C)
    case.update(image=rng.uniform(0, 1, GRID_B + (C,)).astype(np.float32), g_feat=rng.normal(size=(case["Nattr"], C)),
                g_wsum=rng.normal(size=case["Nattr"]))
    return case


def effective_index(idx, valid_num):
    """The index list as merge_final reads it (Aggregation.py:111-141): slots from valid_num on do not exist, a negative index
    in a live slot reads row 0.  oracle.extras_np.sample_voge masks by `idx != -1` alone, so it is given this list."""
    K = idx.shape[-1]
    live = np.arange(K) < np.asarray(valid_num)[..., None]
    return np.where(live, np.maximum(idx, 0), -1).astype(np.int32)


# ---- fp64 / fp32 evaluation of the references -----------------------------------------------------------------------------------------------
def merge_reference(case, dtype=torch.float64):
    """torch_ref.merge_final and its autograd gradients for the case's upstream gradient -> (out, g_attr, g_weight) numpy."""
    attr = torch.tensor(case["attr"], dtype=dtype, requires_grad=True)
    w = torch.tensor(case["weight"], dtype=dtype, requires_grad=True)
    out = torch_ref.merge_final(attr, w, torch.tensor(case["valid_num"]), torch.tensor(case["idx"]))
    (out * torch.tensor(case["g"], dtype=dtype)).sum().backward()
    return out.detach().numpy(), attr.grad.numpy(), w.grad.numpy()


def blend_reference(case, thr, dtype=torch.float64, rgb=None):
    """torch_ref.to_colored_background under autograd.  rgb=None: of the merged attributes -> (img, rgb, g_attr, g_weight);
    rgb given (fp32 values, a leaf): -> (img, rgb, g_rgb, g_weight)."""
    w = torch.tensor(case["weight"], dtype=dtype, requires_grad=True)
    if rgb is None:
        leaf = torch.tensor(case["attr"], dtype=dtype, requires_grad=True)
        mid = torch_ref.merge_final(leaf, w, torch.tensor(case["valid_num"]), torch.tensor(case["idx"]))
    else:
        leaf = mid = torch.tensor(rgb, dtype=dtype, requires_grad=True)
    img = torch_ref.to_colored_background(mid, w, torch.tensor(case["bg"], dtype=dtype), thr)
    (img * torch.tensor(case["g"], dtype=dtype)).sum().backward()
    g_w = w.grad if w.grad is not None else torch.zeros_like(w)      # ([sil > thr] of a given rgb: the weights are not reached)
    return img.detach().numpy(), mid.detach().numpy(), leaf.grad.numpy(), g_w.numpy()


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if b.size else 0.0


def _scaled(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())) if b.size else 0.0


# ---- the dense-ray extras' inputs -----------------------------------------------------------------------------------------------------------
def dense_inputs(M, N, seed=0):
    """Gaussians in front of the origin, well-conditioned 3x3 forms, a narrow bundle of unit rays.  The forms are of order 1, so
    that act = mu'A mu - (mu'A d)^2 / d'A d cancels two numbers of order 30, not 300: what is tested with these is the kernels'
    indexing, grid-stride loop and cross-workgroup sums at util.TOL, element by element, not the conditioning of the formula."""
    rng = np.random.default_rng(seed)
    mus = (rng.normal(size=(M, 3)) * 0.3 + [0, 0, 3]).astype(np.float32)
    L = np.tril(rng.uniform(0.5, 1.5, (M, 3, 3)))
    isg = (L @ L.transpose(0, 2, 1) + rng.normal(size=(M, 3, 3)) * 0.01).astype(np.float32)
    rays = rng.normal(size=(N, 3)) * 0.1 + [0, 0, 1]
    rays = (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    return mus, isg, rays


NEAREST_THR_ACT = 2.5


def nearest_case(N, M, seed=0, ties=True):
    """Dense rows for find_nearest_k, fp32: len ~ N(0, 2) of mixed sign, act uniform in [0, 5] (threshold 2.5), dsd positive.
    ties: row 0 has every act above the threshold (all its slots stay empty); row 1 passes only columns 0 and 2, which share one
    bit pattern (-0.75), column 1 (-0.0) and, where M >= 5, column M - 1 (+0.0, equal to -0.0 as a number); row 2 passes a single
    column."""
    rng = np.random.default_rng(seed)
    ln = rng.normal(size=(N, M)).astype(np.float32) * 2
    act = rng.uniform(0, 5, (N, M)).astype(np.float32)
    dsd = rng.uniform(0.5, 2, (N, M)).astype(np.float32)
    if ties:
        assert N >= 3 and M >= 3
        act[0] = NEAREST_THR_ACT + 0.5 + act[0]
        act[1] = NEAREST_THR_ACT + 0.5 + act[1]
        ln[1, 0] = ln[1, 2] = np.float32(-0.75)
        ln[1, 1] = -0.0
        act[1, :3] = 0.5
        if M >= 5:
            ln[1, M - 1], act[1, M - 1] = 0.0, 0.5
        act[2] = NEAREST_THR_ACT + 1.0
        act[2, M // 2] = 0.25
    return ln, act, dsd


def coarse_case(image_size, seed=0):
    """Two clouds packed into one array -- num_points (700, 333), first_idx (0, 700): 1033 points, no multiple of the 512-point
    chunk -- in NDC over the (possibly non-square) image, ~8 % behind the camera (z < 0), ~5 % NaN radii."""
    rng = np.random.default_rng(seed)
    H, W = image_size
    P = 1033
    rx, ry = max(W / H, 1.0), max(H / W, 1.0)      # half the NDC range per axis
    pts = np.stack([rng.uniform(-1.1 * rx, 1.1 * rx, P), rng.uniform(-1.1 * ry, 1.1 * ry, P), rng.uniform(0.5, 5, P)], 1).astype(np.float32)
    pts[rng.random(P) < 0.08, 2] *= -1
    rad = rng.uniform(0.02, 0.5, (P, 2)).astype(np.float32)
    rad[rng.random(P) < 0.05] = np.nan
    return pts, rad, np.array([0, 700], np.int64), np.array([700, 333], np.int64)


# ---- assertions on the inputs -----------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_route_and_every_required_size():
    fwd, bwd = set(), set()
    for c in MERGE_CASES:
        grid, K, C, Nattr, aligned, f, b = c
        assert f == fwd_route(K, C, aligned, Nattr) and b == bwd_route(C), case_id(c)
        fwd.add(f)
        bwd.add(b)
    assert fwd == {"fwd4", "pc", "general"} and bwd == {"tile", "slot", "chan"}
    assert MERGE_C <= {c[2] for c in MERGE_CASES} and MERGE_K <= {c[1] for c in MERGE_CASES}
    assert len(MERGE_CASES) == len({case_id(c) for c in MERGE_CASES})
    have = {(c[1], c[2], c[4]) for c in MERGE_CASES}
    assert {(102, 6, True), (600, 2, True), (1028, 5, True), (12, 100, True), (13, 100, True), (12, 3, False), (12, 7, False),
            (12, 100, False)} <= have
    assert any(c[3] == 1 for c in MERGE_CASES)
    # every backward route is reached from an aligned and from an unaligned case, every forward route with C > 64 and with C <= 4
    assert {bwd_route(c[2]) for c in MERGE_CASES if not c[4]} == {"tile", "slot", "chan"}
    assert {1, 3, 4, 5, 8, 9, 65} <= {c[2] for c in BLEND_CASES} and {1, 5, 12, 64, 100} <= {c[1] for c in BLEND_CASES}
    assert {bwd_route(C + 1) for C in SAMPLER_CHANNELS} == {"tile", "slot", "chan"}
    assert {C + 1 for C in SAMPLER_CHANNELS} == {2, 4, 5, 8, 64, 65, 100} and {k % 2 for k in SAMPLER_K} == {0, 1}
    for grid in (GRID_A, GRID_B):
        assert all(int(np.prod(grid)) % m for m in (4, 8, 16, 32))
    # "attribute rows that no live slot reads get a zero gradient" is not vacuous: the small-K cases leave rows unread
    unread = 0
    for c in MERGE_CASES:
        if c[1] <= 3:
            case = merge_case(c)
            live = np.arange(case["K"]) < case["valid_num"][..., None]
            unread += np.setdiff1d(np.arange(case["Nattr"]), np.maximum(case["idx"], 0)[live]).size
    assert unread > 0


def _check_fragments(case):
    idx, vn, w = case["idx"].reshape(-1, case["K"]), case["valid_num"].reshape(-1), case["weight"].reshape(-1, case["K"])
    K = case["K"]
    assert idx.dtype == np.int32 and vn.dtype == np.int64 and w.dtype == np.float32
    assert (vn == 0).any() and (vn == K).any() and vn.min() >= 0 and vn.max() <= K
    assert idx.min() >= -1 and idx.max() < case["Nattr"]
    assert (w >= 0).all() and (w.sum(-1) > 0).all()
    s = w.astype(np.float64).sum(-1)
    assert np.abs(s - 1).min() >= MARGIN and np.abs(np.minimum(s, 1) - THR).min() >= MARGIN
    assert s.min() > 0.15 and s.max() < 1.85 and (s < 1).any() and (s > 1).any()
    return idx, vn, w


@pytest.mark.parametrize("c", MERGE_CASES, ids=case_id)
def test_merge_inputs_keep_the_fp32_reference_inside_a_quarter_of_the_tolerance(c):
    case = merge_case(c)
    idx, vn, w = _check_fragments(case)
    K = case["K"]
    if K >= 12:      # live slots that hold -1, masked slots that hold real indices, exact zeros among the weights
        live = np.arange(K)[None] < vn[:, None]
        assert (idx[live] < 0).any() and (idx[~live] >= 0).any() and (w == 0).any()
    assert case["raw_gap"] >= 2e-3
    ref64, ref32 = merge_reference(case), merge_reference(case, torch.float32)
    errs = (_rel(ref32[0], ref64[0]), _scaled(ref32[1], ref64[1]), _rel(ref32[2], ref64[2]))
    print(f"[conditioning] merge {case_id(c)}: fp32 reference out {errs[0]:.2e}, g_attr {errs[1]:.2e} of scale, g_weight {errs[2]:.2e}")
    assert max(errs) <= TOL / 4, errs


@pytest.mark.parametrize("c", BLEND_CASES + [SHADE_DIRECT], ids=case_id)
def test_blend_inputs_keep_their_margins_and_the_fp32_reference_inside_a_quarter_of_the_tolerance(c):
    case = blend_case(c)
    _, _, w = _check_fragments(case)
    P = w.shape[0]
    for thr in BLEND_THR:
        img64, rgb64, ga64, gw64 = blend_reference(case, thr)
        s = w.astype(np.float64).sum(-1)
        sil = np.minimum(s, 1.0)
        mask = (sil > thr).astype(np.float64) if thr > 0 else sil
        x = rgb64.reshape(P, -1) + (1 - mask)[:, None] * case["bg"][None].astype(np.float64)
        assert np.abs(x - 1).min() >= MARGIN, np.abs(x - 1).min()      # EVERY pixel and channel: nothing is left out later
        assert (x > 1).any() and (x < 1).any()                         # both sides of the clamp are there
        img32, _, ga32, gw32 = blend_reference(case, thr, torch.float32)
        rgb32 = rgb64.astype(np.float32)
        d64, d32 = blend_reference(case, thr, rgb=rgb32), blend_reference(case, thr, torch.float32, rgb=rgb32)
        x = rgb32.reshape(P, -1).astype(np.float64) + (1 - mask)[:, None] * case["bg"][None].astype(np.float64)
        assert np.abs(x - 1).min() >= MARGIN
        errs = (_rel(img32, img64), _scaled(ga32, ga64), _rel(gw32, gw64), _rel(d32[0], d64[0]), _rel(d32[2], d64[2]), _rel(d32[3], d64[3]))
        print(f"[conditioning] blend {case_id(c)} thr={thr}: fp32 reference image {errs[0]:.2e}, g_attr {errs[1]:.2e} of scale, "
              f"g_weight {errs[2]:.2e}; from a given rgb: image {errs[3]:.2e}, g_rgb {errs[4]:.2e}, g_weight {errs[5]:.2e}")
        assert max(errs) <= TOL / 4, errs


@pytest.mark.parametrize("C", SAMPLER_CHANNELS)
@pytest.mark.parametrize("K", SAMPLER_K)
def test_sampler_inputs_and_the_reading_of_the_index_list(C, K):
    """The sampler is the transpose of merge_final: extras_np.sample_voge on effective_index() is merge_final's transpose on the raw
    fragments (checked here against torch_ref.merge_final's gradient), and its fp32 evaluation stays within TOL / 4."""
    case = sampler_case(C, K)
    _check_fragments(case)
    eff = effective_index(case["idx"], case["valid_num"])
    feat, wsum = extras_np.sample_voge(case["image"], case["weight"], eff, case["Nattr"])
    # <merge_final(attr), image> differentiated by attr IS the scatter of weight * image
    attr = torch.zeros((case["Nattr"], C), dtype=torch.float64, requires_grad=True)
    out = torch_ref.merge_final(attr, torch.tensor(case["weight"], dtype=torch.float64), torch.tensor(case["valid_num"]), torch.tensor(case["idx"]))
    (out * torch.tensor(case["image"], dtype=torch.float64)).sum().backward()
    assert np.abs(attr.grad.numpy() - feat).max() < 1e-12
    f32 = np.zeros((case["Nattr"], C), np.float32)
    np.add.at(f32, eff[eff >= 0], (case["weight"][..., None] * case["image"][..., None, :])[eff >= 0])
    assert _scaled(f32, feat) <= TOL / 4 and wsum.max() > 0


def test_oracle_orders_equal_lengths_by_ascending_index_on_the_tie_case():
    ln, act, dsd = nearest_case(5, 9, seed=11)
    idx, ol, oa, od = extras_np.find_nearest_k(ln, act, dsd, 5, NEAREST_THR_ACT)
    assert (idx[0] == -1).all() and (ol[0] == 1e10).all() and (oa[0] == 0).all() and (od[0] == 0).all()
    assert idx[1].tolist() == [0, 2, 1, 8, -1]      # the bit-equal pair, then -0.0 before +0.0: by index
    assert np.signbit(ol[1][2]) and not np.signbit(ol[1][3])
    assert idx[2].tolist() == [4, -1, -1, -1, -1]
    assert (ln < 0).any() and (ln > 0).any()
    # farthest-K negates the lengths: the same pairs stay tied, still in ascending index
    assert extras_np.find_nearest_k(-ln, act, dsd, 4, NEAREST_THR_ACT)[0][1].tolist() == [1, 8, 0, 2]
    # K > M on three columns
    ln, act, dsd = nearest_case(5, 3, seed=12)
    assert extras_np.find_nearest_k(ln, act, dsd, 5, NEAREST_THR_ACT)[0][1].tolist() == [0, 2, 1, -1, -1]


@pytest.mark.parametrize("image_size", [(40, 72), (72, 40)])
def test_coarse_inputs_overflow_the_small_capacity_and_use_both_windows(image_size):
    from oracle import coarse_np
    pts, rad, first, num = coarse_case(image_size)
    assert pts.shape[0] == 1033 and pts.shape[0] % 512 and (pts[:, 2] < 0).any() and np.isnan(rad).any()
    full = coarse_np.rasterize_points_coarse(pts, first, num, image_size, rad, 16, 1033)
    small = coarse_np.rasterize_points_coarse(pts, first, num, image_size, rad, 16, 40)
    assert full.shape[:3] == (2, 1 + (image_size[0] - 1) // 16, 1 + (image_size[1] - 1) // 16) and image_size[0] % 16 and image_size[1] % 16
    n_full, n_small = (full >= 0).sum(-1), (small >= 0).sum(-1)
    assert (n_small < n_full).any() and (n_full > 40).any()      # a chunk is dropped in at least one bin
    assert (n_full < 1033).all()                                 # ... and the large capacity drops nothing
    for b in range(2):      # each cloud lists its own window only, and never a point behind the camera or with a NaN radius
        e = full[b][full[b] >= 0]
        assert e.size and e.min() >= first[b] and e.max() < first[b] + num[b]
        assert (pts[e, 2] >= 0).all() and not np.isnan(rad[e]).any()
