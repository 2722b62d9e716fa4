"""Seeded inputs for the tests that run the reference's own kernels (tests/test_gpu_reference_kernels.py), for the CPU checks of
those inputs (tests/test_reference_kernels_cpu.py) and for the recorded fixture (tests/golden/make_ref_kernel_golden.py).  numpy only.

Conditioning.  The reference evaluates act = m'Am - (m'Ad)^2 / d'Ad in fp32, so its error is a few ulps of m'Am.  The scenes here
keep m'Am of order 10..100 (forms of order 1..10, Gaussians 1..2.5 units from the camera): the fp32 reference-order oracle then
stays within TOL / 4 of the fp64 oracle, which test_reference_kernels_cpu.py asserts for every scene, and the reference kernel can
be held to util.TOL.

Sums by float atomics.  fp32 addition of m terms in ANY order is within (m - 1) 2^-24 sum|terms| of the exact sum (to first
order; every partial sum is bounded by sum|terms| and each of the m - 1 additions rounds once by at most 2^-24 relative).  The
terms themselves carry a few roundings each, which the TOL-of-the-scale part covers.  `*_terms` below return, per output element
and in fp64, the sum, the sum of |terms| and the number of terms, and atomic_bound() turns them into the bound."""
import functools

import numpy as np

import oracle
from util import TOL

BIN_SIZE = 10
EPS32 = 2.0 ** -24


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def rays_of(B, H, W, focal):
    """Unit pixel rays of a pinhole at the origin looking along +z; view b is turned by 0.2 b rad about y."""
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs + 0.5 - W / 2.0) / focal, (ys + 0.5 - H / 2.0) / focal, np.ones((H, W))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    out = np.empty((B, H, W, 3), np.float32)
    for b in range(B):
        c, s = np.cos(0.2 * b), np.sin(0.2 * b)
        out[b] = d @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
    return out


def gaussians_of(rng, n, form, a_lo=1.5, a_hi=12.0, behind=False):
    """n Gaussians in the camera's frame: centres in x, y in [-1.2, 1.2], z in [1, 2.5] (behind: every other one mirrored to -z);
    form "iso": A = a I, a log-uniform in [a_lo, a_hi]; "sym": A = a L L' with a unit-scale lower-triangular L; "skew": "sym"
    plus a non-symmetric part of 2 % of a."""
    mus = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(1.0, 2.5, n)], 1)
    if behind:
        mus[1::2, 2] *= -1
    a = np.exp(rng.uniform(np.log(a_lo), np.log(a_hi), n))
    if form == "iso":
        A = a[:, None, None] * np.eye(3)
    else:
        L = np.tril(rng.uniform(-0.4, 0.4, (n, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = rng.uniform(0.7, 1.0, (n, 3))
        A = a[:, None, None] * (L @ L.transpose(0, 2, 1))
        if form == "skew":
            nz = rng.normal(size=(n, 3, 3))
            A = A + 0.02 * a[:, None, None] * (nz - nz.transpose(0, 2, 1))
    return mus.astype(np.float32), A.astype(np.float32)


def full_lists(B, H, W, N):
    """RayTracing.py:22-26's list for max_points_per_bin == -1, in the shape the kernel's indexing expects: [B,BH,BW,N]."""
    BH, BW = (H - 1) // BIN_SIZE + 1, (W - 1) // BIN_SIZE + 1
    lst = np.arange(B * N, dtype=np.int32).reshape(B, 1, 1, N)
    return np.ascontiguousarray(np.broadcast_to(lst, (B, BH, BW, N)))


def holed_lists(rng, B, H, W, N, M):
    """Per bin a random number of distinct Gaussians of the bin's own view at random positions of an M-long list, -1 elsewhere."""
    BH, BW = (H - 1) // BIN_SIZE + 1, (W - 1) // BIN_SIZE + 1
    bins = np.full((B, BH, BW, M), -1, np.int32)
    for b in range(B):
        for y in range(BH):
            for x in range(BW):
                m = rng.integers(0, min(M, N) + 1)
                bins[b, y, x, rng.choice(M, size=m, replace=False)] = rng.choice(N, size=m, replace=False) + N * b
    return bins


#            name            H   W  B    N   K  form    thr   lists    a_lo  a_hi  behind
FINE_CASES = [("full_ragged", 45, 61, 1, 400, 9, "iso", 0.01, "full", 1.5, 12.0, False),
              ("full_b2", 32, 32, 2, 300, 9, "iso", 0.01, "full", 1.5, 12.0, False),
              ("holes_ragged", 45, 61, 1, 400, 9, "sym", 0.01, "holes", 1.5, 12.0, False),
              ("holes_b2", 32, 32, 2, 300, 9, "iso", 0.01, "holes", 1.5, 12.0, False),
              ("k1", 45, 61, 1, 200, 1, "iso", 0.01, "full", 1.5, 12.0, False),
              ("tails_k40", 32, 32, 1, 30, 40, "iso", 0.01, "full", 6.0, 12.0, False),
              ("displace_k40", 45, 61, 1, 2000, 40, "iso", 0.01, "full", 1.5, 12.0, False),
              ("thr0", 32, 32, 2, 120, 9, "sym", 0.0, "full", 1.5, 12.0, False),
              ("skew", 45, 61, 1, 300, 9, "skew", 0.01, "full", 1.5, 12.0, False),
              ("behind", 32, 32, 1, 200, 9, "skew", 0.01, "full", 1.5, 8.0, True)]
FINE_NAMES = [c[0] for c in FINE_CASES]


@functools.lru_cache(maxsize=None)
def fine_case(name):
    """-> dict(mus [B*N,3], isg [B*N,3,3], a [B*N] | None, rays [B,H,W,3], bins [B,BH,BW,M] int32, full, K, thr_act, B, N, H, W)."""
    i = FINE_NAMES.index(name)
    _, H, W, B, N, K, form, thr, lists, a_lo, a_hi, behind = FINE_CASES[i]
    rng = np.random.default_rng(9100 + i)
    mus, isg = gaussians_of(rng, B * N, form, a_lo, a_hi, behind)
    rays = rays_of(B, H, W, 0.8 * max(H, W))
    bins = full_lists(B, H, W, N) if lists == "full" else holed_lists(rng, B, H, W, N, 150)
    a = np.ascontiguousarray(isg[:, 0, 0]) if form == "iso" else None
    return dict(name=name, mus=mus, isg=isg, a=a, rays=rays, bins=bins, full=lists == "full", K=K, thr_act=oracle.thr_act_of(thr),
                B=B, N=N, H=H, W=W)


@functools.lru_cache(maxsize=None)
def fine_oracle(name, precision="f64"):
    c = fine_case(name)
    return oracle.trace_fwd(c["mus"], c["isg"], c["rays"], c["K"], c["thr_act"], bin_points=c["bins"], bin_size=BIN_SIZE,
                            precision=precision)


def flips_between(a, b):
    K = a[0].shape[-1]
    return int((np.asarray(a[0]).reshape(-1, K) != np.asarray(b[0]).reshape(-1, K)).any(1).sum())


@functools.lru_cache(maxsize=None)
def fine_flip_ceiling(name):
    """The ceiling on pixels whose index lists may differ between two evaluations of a scene: what the scene shows between the fp32
    reference-order oracle and the fp64 oracle, plus 2."""
    return flips_between(fine_oracle(name, "f32"), fine_oracle(name, "f64")) + 2


@functools.lru_cache(maxsize=None)
def twin_case(descending):
    """The construction of test_gpu_parity.test_explicit_bin_lists_tie_break_deviation -- 60 Gaussians listed twice (i and i + 60 are
    bit-identical, so their len are exactly tied in any implementation), one list for every bin, in ascending or descending index
    order, 32 x 40 pixels, K = 12 -- on Gaussians of this module: that test's own scene (forms of ~300 at distance 3) puts the fp32
    reference-order oracle 8e-4 from the fp64 one, eight times TOL, so the reference kernel's values could not be held to TOL on it."""
    n0, H, W, K = 60, 32, 40, 12
    mus, isg = gaussians_of(np.random.default_rng(9200), n0, "iso", 6.0, 12.0)
    mus, isg = np.concatenate([mus, mus]), np.concatenate([isg, isg])
    BH, BW = (H - 1) // BIN_SIZE + 1, (W - 1) // BIN_SIZE + 1
    order = np.arange(2 * n0, dtype=np.int32)
    if descending:
        order = order[::-1]
    bins = np.ascontiguousarray(np.broadcast_to(order[None, None, None], (1, BH, BW, 2 * n0)))
    return dict(name="twins_desc" if descending else "twins_asc", mus=mus, isg=isg, a=np.ascontiguousarray(isg[:, 0, 0]),
                rays=rays_of(1, H, W, 0.8 * W), bins=bins, full=False, K=K, thr_act=oracle.thr_act_of(0.01), B=1, N=2 * n0, H=H, W=W, n0=n0)


# ---- fp64 term sums: the trace backward (fine and dense) ----------------------------------------------------------------------------
def atomic_bound(abs_sum, count, ref):
    """Per element: (m - 1) 2^-24 sum|terms| + TOL max(1, max|ref|)."""
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    return np.maximum(count - 1, 0) * EPS32 * abs_sum + TOL * scale


def trace_bwd_terms(mus, isg, rays, idx, g_len, g_act, g_dsd):
    """The reference's backward (ray_trace_voge.cu:283-332, Innerdot3dBackward :41-91) with every atomicAdd as one term, fp64.
    mus [P,3], isg [P,3,3], rays [R,3], idx / g_* [R,K] (-1 = empty).  -> {"ray" | "mus" | "isg": (sum, sum|terms|, count)} with
    shapes [R,3], [P,3], [P,3,3]."""
    mu_all, A_all, d_all = (np.asarray(x, np.float64) for x in (mus, isg, rays))
    idx = np.asarray(idx)
    R, K = idx.shape
    P = mu_all.shape[0]
    r_of, k_of = np.nonzero(idx != -1)
    p_of = idx[r_of, k_of]
    d, mu, A = d_all[r_of], mu_all[p_of], A_all[p_of]
    gl, ga, gd = (np.asarray(g, np.float64)[r_of, k_of] for g in (g_len, g_act, g_dsd))
    ksk = np.einsum("si,sij,sj->s", d, A, d)
    msk = np.einsum("si,sij,sj->s", mu, A, d)
    g_ksk = (ga * msk - gl) * msk / (ksk * ksk) + gd
    g_msk = (gl - 2 * ga * msk) / ksk
    g_msm = ga
    out = {"ray": [np.zeros((R, 3)) for _ in range(2)] + [np.zeros((R, 3), np.int64)],
           "mus": [np.zeros((P, 3)) for _ in range(2)] + [np.zeros((P, 3), np.int64)],
           "isg": [np.zeros((P, 3, 3)) for _ in range(2)] + [np.zeros((P, 3, 3), np.int64)]}

    def add(key, rows, term):
        s, a, c = out[key]
        np.add.at(s, rows, term)
        np.add.at(a, rows, np.abs(term))
        np.add.at(c, rows, 1)

    # (grad, a, c, key and rows of a's gradient, key and rows of c's gradient), :328-330
    for g, av, cv, (ka, ra), (kc, rc) in ((g_ksk, d, d, ("ray", r_of), ("ray", r_of)), (g_msk, mu, d, ("mus", p_of), ("ray", r_of)),
                                          (g_msm, mu, mu, ("mus", p_of), ("mus", p_of))):
        add(ka, ra, np.einsum("sij,sj->si", A, cv) * g[:, None])
        add("isg", p_of, av[:, :, None] * cv[:, None, :] * g[:, None, None])
        add(kc, rc, np.einsum("sji,sj->si", A, av) * g[:, None])
    return {k: tuple(v) for k, v in out.items()}


#           name         H   W  B   N   K  form    lists
BWD_CASES = [("bwd_iso_b2", 32, 32, 2, 60, 9, "iso", "holes"),
             ("bwd_skew_ragged", 45, 61, 1, 80, 9, "skew", "holes"),
             ("bwd_sym_b2_full", 32, 32, 2, 40, 12, "sym", "full")]
BWD_NAMES = [c[0] for c in BWD_CASES]


@functools.lru_cache(maxsize=None)
def bwd_case(name):
    """A forward case (narrower Gaussians, so that many slots stay -1) plus upstream gradients [B,H,W,K] for len, act and dsd."""
    i = BWD_NAMES.index(name)
    _, H, W, B, N, K, form, lists = BWD_CASES[i]
    rng = np.random.default_rng(9300 + i)
    mus, isg = gaussians_of(rng, B * N, form, 6.0, 12.0)
    rays = rays_of(B, H, W, 0.8 * max(H, W))
    bins = full_lists(B, H, W, N) if lists == "full" else holed_lists(rng, B, H, W, N, 50)
    g = rng.normal(size=(3, B, H, W, K)).astype(np.float32)
    g[2] *= 0.1
    return dict(name=name, mus=mus, isg=isg, a=np.ascontiguousarray(isg[:, 0, 0]) if form == "iso" else None, rays=rays, bins=bins,
                full=lists == "full", K=K, thr_act=oracle.thr_act_of(0.01), B=B, N=N, H=H, W=W, g_len=g[0], g_act=g[1], g_dsd=g[2])


# ---- dense extras ------------------------------------------------------------------------------------------------------------------
DENSE_RAYS, DENSE_GAUSSIANS, DENSE_K = 130, 70, [1, 8, 70, 90]


@functools.lru_cache(maxsize=None)
def dense_case():
    """130 rays (no multiple of 64), 70 Gaussians with full 3x3 forms.  Two pairs of Gaussians are bit-identical, so their len
    columns are exactly equal in any implementation: the two Gaussians that are most often among a ray's four nearest passing ones
    (threshold: the median act) are copied over their upper neighbours.  Upstream gradients [130,70] for the dense backward."""
    from oracle import extras_np
    rng = np.random.default_rng(9400)
    mus, isg = gaussians_of(rng, DENSE_GAUSSIANS, "skew")
    rays = np.ascontiguousarray(rays_of(1, 10, 13, 10.0).reshape(-1, 3))
    assert rays.shape[0] == DENSE_RAYS
    ln, act, _ = extras_np.ray_dense_fwd(mus, isg, rays)
    rank = np.argsort(np.argsort(np.where(act < np.median(act), ln, np.inf), axis=1), axis=1)
    often = np.argsort(-(rank < 4).sum(0), kind="stable")
    i1 = int(often[0])
    i2 = int(next(i for i in often[1:] if abs(int(i) - i1) > 1))
    ties = tuple((i, (i + 1) % DENSE_GAUSSIANS) for i in (i1, i2))
    for i, j in ties:
        mus[j], isg[j] = mus[i], isg[i]
    g = rng.normal(size=(3, DENSE_RAYS, DENSE_GAUSSIANS)).astype(np.float32)
    g[2] *= 0.1
    return dict(mus=mus, isg=isg, rays=rays, g_len=g[0], g_act=g[1], g_dsd=g[2], ties=ties)


# ---- sampler -----------------------------------------------------------------------------------------------------------------------
SAMPLER_C, SAMPLER_K, SAMPLER_VERTS = [1, 3, 5], 5, 40


@functools.lru_cache(maxsize=None)
def sampler_case(C):
    """image [2,9,13,C], weights >= 0 and index lists [2,9,13,5]: slot 0 of every pixel holds vertex 0, the others vertices of
    1..37 up to a random count, then -1; vertices 38 and 39 are referenced by nobody."""
    rng = np.random.default_rng(9500 + C)
    B, H, W, K, Nv = 2, 9, 13, SAMPLER_K, SAMPLER_VERTS
    cnt = rng.integers(1, K + 1, (B, H, W))
    cnt.reshape(-1)[:3] = (1, K, 1)
    idx = rng.integers(1, Nv - 2, (B, H, W, K)).astype(np.int32)
    idx[..., 0] = 0
    idx[np.arange(K) >= cnt[..., None]] = -1
    w = rng.uniform(0.0, 1.0, (B, H, W, K)).astype(np.float32)
    w[rng.random(w.shape) < 0.05] = 0.0
    return dict(image=rng.uniform(0, 1, (B, H, W, C)).astype(np.float32), weight=w, idx=idx, valid_num=cnt.astype(np.int64), n_vert=Nv,
                g_feat=rng.normal(size=(Nv, C)).astype(np.float32), g_wsum=rng.normal(size=Nv).astype(np.float32), C=C, K=K)


def sampler_terms(case):
    """sample_voge (sample_voge.cu:35-66) and its backward (:173-209) term by term in fp64 ->
    {"feat" [Nv,C] | "wsum" [Nv] | "g_image" [B,H,W,C] | "g_weight" [B,H,W,K]: (sum, sum|terms|, count)}.  g_weight is one
    atomicAdd of a sum the thread forms itself from C + 1 terms in order; it is bounded the same way with m = C + 1."""
    img, w, idx = case["image"].astype(np.float64), case["weight"].astype(np.float64), case["idx"]
    gf, gw = case["g_feat"].astype(np.float64), case["g_wsum"].astype(np.float64)
    C, K, Nv = case["C"], case["K"], case["n_vert"]
    pix = img.reshape(-1, C)
    w2, ix = w.reshape(-1, K), idx.reshape(-1, K)
    r_of, k_of = np.nonzero(ix != -1)
    v_of, ws = ix[r_of, k_of], w2[r_of, k_of]
    feat = [np.zeros((Nv, C)), np.zeros((Nv, C)), np.zeros((Nv, C), np.int64)]
    wsum = [np.zeros(Nv), np.zeros(Nv), np.zeros(Nv, np.int64)]
    g_img = [np.zeros(pix.shape), np.zeros(pix.shape), np.zeros(pix.shape, np.int64)]
    g_w = [np.zeros(w2.shape), np.zeros(w2.shape), np.zeros(w2.shape, np.int64)]
    for acc, rows, term in ((feat, v_of, ws[:, None] * pix[r_of]), (wsum, v_of, ws), (g_img, r_of, ws[:, None] * gf[v_of])):
        np.add.at(acc[0], rows, term)
        np.add.at(acc[1], rows, np.abs(term))
        np.add.at(acc[2], rows, 1)
    inner = np.concatenate([gw[v_of][:, None], gf[v_of] * pix[r_of]], 1)
    g_w[0][r_of, k_of], g_w[1][r_of, k_of], g_w[2][r_of, k_of] = inner.sum(1), np.abs(inner).sum(1), C + 1
    return {"feat": tuple(feat), "wsum": tuple(wsum), "g_image": tuple(a.reshape(img.shape) for a in g_img),
            "g_weight": tuple(a.reshape(w.shape) for a in g_w)}


# ---- coarse rasteriser ---------------------------------------------------------------------------------------------------------------
COARSE_SIZE, COARSE_FIRST, COARSE_NUM = (45, 61), (0, 700), (700, 333)
COARSE_MARGIN = 1e-4


def coarse_bin_edges(image_size, bin_size=BIN_SIZE):
    """The NDC positions of every bin edge (rasterize_coarse.cu:116-128, rasterization_utils.cuh:15-42) in fp64 -> (x edges, y edges)."""
    H, W = image_size
    rx, ry = max(W / H, 1.0), max(H / W, 1.0)      # half the NDC range per axis
    ex = sorted({-rx + 2 * rx * b * bin_size / W for b in range((W - 1) // bin_size + 2)})
    ey = sorted({-ry + 2 * ry * b * bin_size / H for b in range((H - 1) // bin_size + 2)})
    return np.array(ex), np.array(ey)


def coarse_edge_gap(pts, rad, image_size=COARSE_SIZE):
    """Per point, the smallest fp64 distance of any of its four box edges to any bin edge of its axis."""
    ex, ey = coarse_bin_edges(image_size)
    p, r = pts.astype(np.float64), rad.astype(np.float64)
    gx = np.minimum(np.abs((p[:, 0] - r[:, 0])[:, None] - ex).min(1), np.abs((p[:, 0] + r[:, 0])[:, None] - ex).min(1))
    gy = np.minimum(np.abs((p[:, 1] - r[:, 1])[:, None] - ey).min(1), np.abs((p[:, 1] + r[:, 1])[:, None] - ey).min(1))
    return np.minimum(gx, gy)


def coarse_points(rng, P, image_size, r_hi):
    """P points in NDC over the (possibly non-square) image with z in [0.5, 5] and radii in [0.02, r_hi]; a point with a box edge
    within 2e-4 NDC of a bin edge (fp64) is moved by 1e-3 until none is, so membership is no rounding question."""
    H, W = image_size
    rx, ry = max(W / H, 1.0), max(H / W, 1.0)
    pts = np.stack([rng.uniform(-1.1 * rx, 1.1 * rx, P), rng.uniform(-1.1 * ry, 1.1 * ry, P), rng.uniform(0.5, 5, P)], 1).astype(np.float32)
    rad = rng.uniform(0.02, r_hi, (P, 2)).astype(np.float32)
    for _ in range(50):
        near = coarse_edge_gap(pts, rad, image_size) < 2 * COARSE_MARGIN
        if not near.any():
            break
        pts[near, :2] += np.float32(1e-3)
    assert coarse_edge_gap(pts, rad, image_size).min() >= 2 * COARSE_MARGIN
    return pts, rad


@functools.lru_cache(maxsize=None)
def coarse_case():
    """Two clouds (700 and 333 points, 1033 in all: three 512-point chunks) over a 45 x 61 image, ~8 % at z < 0."""
    rng = np.random.default_rng(9600)
    pts, rad = coarse_points(rng, sum(COARSE_NUM), COARSE_SIZE, 0.5)
    pts[rng.random(pts.shape[0]) < 0.08, 2] *= -1
    return pts, rad, np.array(COARSE_FIRST, np.int64), np.array(COARSE_NUM, np.int64)


def sorted_bins(bins):
    """Each bin's list as a sorted row (-1 padding first): the order inside a bin is the scheduler's."""
    return np.sort(np.asarray(bins), axis=-1)


# ---- the recorded fixture (tests/golden/ref_kernels.npz) ----------------------------------------------------------------------------
def decision_margins(c):
    """How far a fine-trace scene is from every decision the selection makes, in fp64 and relative to max(1, |value|):
    (the smallest |act - thr_act| over every listed candidate of every pixel, the smallest gap between the len of two candidates
    that pass the threshold at one pixel).  Both above TOL / 2, an evaluation within TOL / 4 of fp64 -- the fp32 reference on the
    scenes here -- makes every decision as fp64 does: the index lists are reproduced exactly."""
    from oracle import extras_np
    B, H, W, N, bins = c["B"], c["H"], c["W"], c["N"], c["bins"]
    m_act, m_len = np.inf, np.inf
    for b in range(B):
        ln, act, _ = extras_np.ray_dense_fwd(c["mus"], c["isg"], c["rays"][b].reshape(-1, 3))      # [H W, B N]
        ys, xs = np.divmod(np.arange(H * W), W)
        listed = np.zeros(ln.shape, bool)
        for by in range(bins.shape[1]):
            for bx in range(bins.shape[2]):
                e = bins[b, by, bx]
                rows = np.nonzero((ys // BIN_SIZE == by) & (xs // BIN_SIZE == bx))[0]
                listed[np.ix_(rows, e[e >= 0])] = True
        m_act = min(m_act, float((np.abs(act - c["thr_act"]) / max(1.0, abs(c["thr_act"])))[listed].min()))
        l = np.where(listed & (act < c["thr_act"]), ln, np.inf)
        l.sort(axis=1)
        with np.errstate(invalid="ignore"):
            gap = (l[:, 1:] - l[:, :-1]) / np.maximum(1.0, np.abs(l[:, :-1]))
        m_len = min(m_len, float(np.where(np.isfinite(l[:, 1:]), gap, np.inf).min()))
    return m_act, m_len
