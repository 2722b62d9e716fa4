"""Ray bundles and Gaussian sets that drive the forward trace (csrc/trace_fwd.hip, trace_bin.h, sweep_iso.h) through the arms of
its culls and of its early exit that pinhole rays in front of a unit cube never reach (plain numpy, seeded, no GPU), and the
forward error bound of the sweep's evaluation that the strict comparison (util.compare_trace_strict) holds the kernels to.

A case is (mus [N,3], a [N] | A [N,3,3], rays [1,H,W,3], K, thr_act, what it is for), built at two sizes: "small" (N <= 4096: the
small-set form, binA skipped) and "binned" (N >= 4097: binA -> binB -> sweep).  The camera sits at the origin: `mus` are the
centres as the entry points take them.  tests/test_trace_bound_cases_cpu.py proves in fp64 that each case is what it claims;
tests/test_gpu_trace_bounds.py runs the kernels on the same arrays.

The error bound (u = 2^-24; every operation below is one correctly rounded fp32 operation or a hardware reciprocal of <= 1 ulp = 2 u;
the library is built with -ffp-contract=off, so the chains are exactly the ones written in sweep_iso.h / voge_common.h)
----------------------------------------------------------------------------------------------------------------------------
len.  pair_eval_gen: ksk = s00 qxx + s11 qyy + ... + s12 qyz, a chain of one product and five fmas over the features q = d d^T
(one rounding each) and the coefficients sXY = A_XY + A_YX (one rounding): every term carries at most (1 + 1 + 6) u, hence
|d ksk| <= 8 u |d|^T |A| |d|  (|.| entry by entry).  msk = b . d with b = A^T mu (three products, two sums, one final rounding each
in the record pass) and a three-term chain: |d msk| <= 6 u |d|^T |A| |mu|.  t = msk * rcp(ksk): 3 u more.  To first order
    |d len| <= (6 u |d|^T|A||mu| + 8 u |len| |d|^T|A||d|) / |ksk| + 3 u |len|  =  2^-23 * k_len ,
    k_len = (3 |d|^T|A||mu| + 4 |len| |d|^T|A||d|) / |d^T A d| + 1.5 |len| .
The scalar-sigma form (md = mu . d: a three-term chain, 3 u sum |mu_i d_i|; rdn2 = rcp((dx dx + dy dy) + dz dz): 3 u and 2 u;
t = md rdn2: u) has the same shape with A = I:  k_len = 1.5 sum |mu_i d_i| / |d|^2 + 3 |len|  <=  4.5 |mu| / |d|.
act.  v = mu - t d, one fma per component: the computed v differs from the exact one by
    e_i = u |v_i| + |d_i| |d len| + u |len| |d_i| ,
and act = v^T A v (a six-term chain over rounded products, 8 u |v|^T|A||v|; symmetric A: the k . d term is exactly zero):
    |d act| <= 2 |v|^T|A| e + e^T|A| e + 8 u |v|^T|A||v|  =  2^-23 * k_act .
The reference's own formula, mu^T A mu - (mu^T A d)^2 / ksk, cancels: its error scales with a |mu|^2, not with a |mu| |v|; the
fp32 oracle's share of this bound is therefore above one where |v| << |mu| and is logged only.
dsd.  |d dsd| <= 8 u |d|^T|A||d| = 4 * 2^-23 * k_dsd.

delta.  A case's delta is what its DECISIONS need, from every (pixel, Gaussian) pair in fp64 (pair_terms over all pairs):
    delta_len = max 2 |d len| / max(1, |len|) over the pairs with act < 2 thr          (two lens this far apart cannot swap)
    delta_act = max |d act| / thr            over the pairs with thr / 2 < act < 2 thr  (a pair this far from thr cannot cross it)
and every pair outside that band must have |d act| < |act - thr| / 2 (asserted).  delta = max of the two, and at least 2^-20.
The cases are built so that delta <= 1e-4.  Pairs whose fp64 values are not finite (invalid forms, degenerate rays) are no hits in
the oracle, and the kernels' tests on them are exact compares of NaN / inf, not roundings: they carry no bound.
"""
import functools

import numpy as np

THR = 0.01
THR_ACT = float(-np.log(THR + 1 / 1e10))
CAP = 0.05
U23 = 2.0 ** -23
N_SIZE = dict(small=3000, binned=4200)
SIZES = ("small", "binned")


class Case:
    def __init__(self, name, size, mus, rays, K, what, a=None, A=None, exit_case=False, diag=False, empty_pixels=(), notes=None):
        self.name, self.size, self.K, self.what = name, size, int(K), what
        self.mus = np.ascontiguousarray(mus, np.float32)
        self.a = None if a is None else np.ascontiguousarray(a, np.float32)
        self.A = None if A is None else np.ascontiguousarray(A, np.float32)
        self.rays = np.ascontiguousarray(rays, np.float32)
        assert self.rays.ndim == 4 and self.rays.shape[0] == 1 and max(self.rays.shape[1:3]) <= 96 and 4 <= self.K <= 24
        assert (self.a is None) != (self.A is None) and self.mus.shape[0] == (self.a if self.A is None else self.A).shape[0]
        self.thr_act = THR_ACT
        self.exit_case = exit_case          # the case is about the early exit: lists must be full on most pixels
        self.diag = diag                    # every form is per-axis (diagonal): the fragments entry runs it too
        self.empty_pixels = tuple(empty_pixels)      # (y, x) of the degenerate rays: empty in the oracle
        self.notes = notes or {}

    @property
    def N(self):
        return self.mus.shape[0]

    def isigmas(self):
        """The forms as the general entry takes them, [N,3,3]."""
        if self.A is not None:
            return self.A
        return (self.a[:, None, None] * np.eye(3, dtype=np.float32)[None]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# rays and clouds
# ---------------------------------------------------------------------------------------------------------------------------
def pinhole(H, W, focal, pp=None):
    """Unit rays of a pinhole camera at the origin looking down +z, [1,H,W,3] fp32 (pixel centres at +0.5)."""
    cx, cy = (W / 2.0, H / 2.0) if pp is None else pp
    x = (np.arange(W) + 0.5 - cx) / focal
    y = (np.arange(H) + 0.5 - cy) / focal
    d = np.stack(np.broadcast_arrays(x[None, :], y[:, None], np.ones((H, W))), -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d[None].astype(np.float32)


def a_of(r):
    """The scalar form whose hits are the rays passing within r of the centre: act = a dist^2 < thr_act."""
    return THR_ACT / np.square(np.asarray(r, np.float64))


def around(rng, n, lo, hi):
    """n centres with uniform directions and distances in [lo, hi] from the camera."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * rng.uniform(lo, hi, (n, 1))


def in_front(rng, n, z_lo, z_hi, half_tan):
    z = rng.uniform(z_lo, z_hi, n)
    xy = rng.uniform(-half_tan, half_tan, (n, 2)) * z[:, None]
    return np.concatenate([xy, z[:, None]], 1)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.diag(r))[None]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _front_cloud(rng, N, r_lo=0.08, r_hi=0.16):
    """An ordinary cloud in front of a 64-pixel camera of focal length 64: ~a dozen hits per pixel."""
    mus = in_front(rng, N, 2.0, 6.0, 0.6)
    return mus, a_of(rng.uniform(r_lo, r_hi, N) * mus[:, 2] / 4.0)


def _around_cloud(rng, N, r_lo=0.06, r_hi=0.14):
    mus = around(rng, N, 1.0, 3.0)
    return mus, a_of(rng.uniform(r_lo, r_hi, N))


# ---------------------------------------------------------------------------------------------------------------------------
# the ray-bundle cases
# ---------------------------------------------------------------------------------------------------------------------------
NEAR_UNIT_S = 4e-5
NEAR_UNIT_EDGE = 4.9e-5        # |dn2 - 1| = 9.8e-5: just inside the 1e-4 that ray_dir's `unit` allowed before these tests
NEAR_UNIT_INSIDE = 1.9e-5      # |dn2 - 1| = 3.8e-5: inside the 4e-5 it allows now
NEAR_UNIT_REL_REACH = 1e-6
NEAR_UNIT_D = 100.0
NEAR_UNIT_FAR = 1.01           # one Gaussian per 8x8 tile at 1.01 D: the quad's span is 0.01 D, a bucket (span / 510) 1.96e-5 D


def _near_unit(rng, N, size, s1):
    """Every ray scaled by 1 + s1.  Five Gaussians of reach 1e-6 of their distance ON every pixel's ray, at D (1 + e) with e
    rising from [0, 1e-7] in four gaps of 1.25e-6 .. 1.35e-6 (2e-6 .. 3e-6 at s1 = 4.9e-5): apart by more than delta,
    yet all of a quad's in ONE depth bucket -- the quad's nearest key is the bucket's lower edge, and one far Gaussian per tile
    stretches its span.  Inside a bucket binB's order is whatever its LDS atomics made (the indices are shuffled), every entry
    carries the bucket's edge as its bound, K = 4: a tile that exits as soon as its 64 lists are full loses, on every ray whose
    last arrival is not its farthest candidate, a member."""
    H, W = (32, 32) if size == "binned" else (24, 32)
    unit = pinhole(H, W, 40.0).astype(np.float64)
    per = 5
    g_lo, g_hi = (2e-6, 3e-6) if abs(s1) > 4.5e-5 else (1.25e-6, 1.35e-6)
    eps = np.concatenate([rng.uniform(0, 1e-7, (H * W, 1)), rng.uniform(g_lo, g_hi, (H * W, per - 1))], 1).cumsum(1)
    dist = NEAR_UNIT_D * (1.0 + eps)
    mus = (unit.reshape(-1, 1, 3) * dist[..., None]).reshape(-1, 3)
    far = unit[0, 4::8, 4::8].reshape(-1, 3) * (NEAR_UNIT_D * NEAR_UNIT_FAR)
    mus = np.concatenate([mus, far])
    dist = np.concatenate([dist.reshape(-1), np.full(far.shape[0], NEAR_UNIT_D * NEAR_UNIT_FAR)])
    order = rng.permutation(mus.shape[0])
    return dict(mus=mus[order], a=a_of(NEAR_UNIT_REL_REACH * dist[order]), rays=unit * (1.0 + s1), K=4, exit_case=True)


def _nonunit_random(rng, N, size):
    mus, a = _front_cloud(rng, N)
    rays = pinhole(64, 64, 64.0) * rng.uniform(0.25, 4.0, (1, 64, 64, 1))
    return dict(mus=mus, a=a, rays=rays, K=8)


def one_pixel_scaled_mask(H, W):
    """Pixel (3, 5) of every second 8x8 tile (tiles counted row by row)."""
    m = np.zeros((H, W), bool)
    for t in range(0, (H // 8) * (W // 8), 2):
        m[(t // (W // 8)) * 8 + 3, (t % (W // 8)) * 8 + 5] = True
    return m


def _nonunit_one_pixel(rng, N, size):
    mus, a = _front_cloud(rng, N, 0.08, 0.16)
    rays = pinhole(64, 64, 64.0).copy()
    rays[0][one_pixel_scaled_mask(64, 64)] *= np.float32(1.7)
    return dict(mus=mus, a=a, rays=rays, K=6, exit_case=True)


def _nonunit_const(rng, N, size, factor):
    """len = mu . u / factor: at 1e-9 the cloud's 2 .. 11 units of depth straddle the 1e10 sentinel; at 1e-12 all lie beyond."""
    mus = in_front(rng, N, 2.0, 11.0, 0.6)
    a = a_of(rng.uniform(0.08, 0.16, N) * mus[:, 2] / 4.0)
    return dict(mus=mus, a=a, rays=pinhole(64, 64, 64.0) * np.float32(factor), K=8)


def _wide(rng, N, size, focal):
    """Camera inside the cloud, 64x64 pixels at a focal length of a few pixels."""
    mus, a = _around_cloud(rng, N, 0.05, 0.11)
    return dict(mus=mus, a=a, rays=pinhole(64, 64, focal), K=12)


def _scrambled(rng, N, size):
    v = rng.normal(size=(64 * 64, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    n = 1400
    return dict(mus=around(rng, n, 1.0, 2.5), a=a_of(rng.uniform(0.15, 0.4, n)), rays=v.reshape(1, 64, 64, 3), K=6)


def _scrambled_supertiles(rng, N, size):
    """Every 32x32 super-tile keeps its pinhole rays but gets a rotation of its own."""
    H, W = 96, 64
    rays = pinhole(H, W, 80.0).astype(np.float64)
    for y0 in range(0, H, 32):
        for x0 in range(0, W, 32):
            rays[0, y0:y0 + 32, x0:x0 + 32] = rays[0, y0:y0 + 32, x0:x0 + 32] @ random_rotation(rng).T
    mus, a = _around_cloud(rng, N, 0.08, 0.2)
    return dict(mus=mus, a=a, rays=rays, K=6)


DEGENERATE = (((3, 4), "zero"), ((12, 21), "nan"), ((37, 50), "inf"), ((58, 9), "tiny"))


def _degenerate(rng, N, size):
    mus, a = _front_cloud(rng, N)
    rays = pinhole(64, 64, 64.0).copy()
    for (y, x), kind in DEGENERATE:
        if kind == "zero":
            rays[0, y, x] = 0.0
        elif kind == "nan":
            rays[0, y, x, 1] = np.nan
        elif kind == "inf":
            rays[0, y, x, 2] = np.inf
        else:
            rays[0, y, x] *= np.float32(1e-30)
    return dict(mus=mus, a=a, rays=rays, K=8, empty_pixels=[p for p, _ in DEGENERATE])


# ---------------------------------------------------------------------------------------------------------------------------
# the Gaussian cases (unit pinhole rays)
# ---------------------------------------------------------------------------------------------------------------------------
def _front_4r(rng, N, size):
    """An ordinary cloud all around the camera (hits behind it: negative lens come first), plus centres at (4 +- 1e-3) R, the
    camera inside (|mu| < R) and on the surface (|mu| ~ R).  notes: which is which."""
    n_edge, n_in, n_on = 240, 30, 30
    n_cloud = N - n_edge - n_in - n_on
    mus, a = _around_cloud(rng, n_cloud, 0.06, 0.12)
    d_edge = rng.uniform(0.02, 0.2, n_edge)
    rel = 4.0 + rng.choice([-1e-3, 1e-3], n_edge)
    d_in, d_on = rng.uniform(0.01, 0.05, n_in), rng.uniform(0.02, 0.08, n_on)
    extra = np.concatenate([around(rng, n_edge, 1, 1) * d_edge[:, None], around(rng, n_in, 1, 1) * d_in[:, None],
                            around(rng, n_on, 1, 1) * d_on[:, None]])
    r = np.concatenate([d_edge / rel, d_in * rng.uniform(1.5, 4.0, n_in), d_on * (1 + rng.uniform(-1e-3, 1e-3, n_on))])
    kind = np.concatenate([np.zeros(n_cloud, int), np.ones(n_edge, int), np.full(n_in, 2), np.full(n_on, 3)])
    order = rng.permutation(N)
    return dict(mus=np.concatenate([mus, extra])[order], a=np.concatenate([a, a_of(r)])[order], rays=pinhole(64, 64, 64.0), K=16,
                exit_case=True, notes=dict(kind=kind[order], reach=np.concatenate([np.sqrt(THR_ACT / a), r])[order]))


def _mixed_reach(rng, N, size, big_in_front):
    """Thousands of tiny Gaussians at depth 3 .. 5 and a dozen whose reach, 20, is ten times the scene."""
    n_big = 12
    mus = in_front(rng, N - n_big, 3.0, 5.0, 0.6)
    a = a_of(rng.uniform(0.084, 0.116, N - n_big) * mus[:, 2] / 4.0)
    zb = rng.uniform(0.5, 1.5, n_big) if big_in_front else rng.uniform(30.0, 40.0, n_big)
    big = np.concatenate([rng.uniform(-1, 1, (n_big, 2)), zb[:, None]], 1)
    where = np.sort(rng.choice(N, n_big, replace=False))
    mus_all, a_all = np.empty((N, 3)), np.empty(N)
    mask = np.zeros(N, bool)
    mask[where] = True
    mus_all[mask], a_all[mask] = big, a_of(np.full(n_big, 20.0))
    mus_all[~mask], a_all[~mask] = mus, a
    return dict(mus=mus_all, a=a_all, rays=pinhole(64, 64, 64.0), K=12 if not big_in_front else 16, notes=dict(big=where))


def fp32_norm(m):
    """|mu| as depth_key computes it: sqrt(fma(z, z, fma(y, y, x * x))), every step rounded to fp32."""
    m = np.asarray(m, np.float32).astype(np.float64)
    s = (m[:, 0] * m[:, 0]).astype(np.float32).astype(np.float64)
    s = (m[:, 1] * m[:, 1] + s).astype(np.float32).astype(np.float64)
    s = (m[:, 2] * m[:, 2] + s).astype(np.float32).astype(np.float64)
    return np.sqrt(s).astype(np.float32)


def _on_shell(rng, n, D, polar_lo, polar_hi):
    """n fp32 centres whose fp32 norm is the same number, D, at polar angles (from +z, degrees) in [polar_lo, polar_hi]."""
    out = []
    want = np.float32(D)
    c_lo, c_hi = np.cos(np.radians(polar_hi)), np.cos(np.radians(polar_lo))
    while sum(len(o) for o in out) < n:
        z = rng.uniform(c_lo, c_hi, 4 * n)
        ph = rng.uniform(0, 2 * np.pi, 4 * n)
        s_ = np.sqrt(1 - z * z)
        v = (np.stack([s_ * np.cos(ph), s_ * np.sin(ph), z], 1) * D).astype(np.float32)
        out.append(v[fp32_norm(v) == want])
    return np.concatenate(out)[:n].astype(np.float64)


SHELL_VIEW = 50.0      # the camera's corner rays are 35.3 degrees off axis, a reach of 0.24 D subtends 13.9


def _shell_one(rng, N, size):
    """Every centre at fp32 distance 5 exactly, reach 0.2 .. 0.24 of it ('front' needs |mu| > 4 R): 500 towards the image, the
    others beside it (a shell's lens crowd into D (R / D)^2 / 2: the density in view is what keeps lens apart)."""
    mus = np.concatenate([_on_shell(rng, 500, 5.0, 0.0, SHELL_VIEW), _on_shell(rng, N - 500, 5.0, SHELL_VIEW + 2, 90.0)])
    order = rng.permutation(N)
    return dict(mus=mus[order], a=a_of(rng.uniform(1.0, 1.2, N)), rays=pinhole(64, 64, 64.0), K=6, exit_case=True)


def _shell_two(rng, N, size):
    """Shells at 1e-2 (30 towards the image: about two hits per pixel) and 1e3 (500), the others beside the image on either."""
    h = (N - 530) // 2
    mus = np.concatenate([_on_shell(rng, 30, 1e-2, 0.0, SHELL_VIEW), _on_shell(rng, 500, 1e3, 0.0, SHELL_VIEW),
                          _on_shell(rng, h, 1e-2, SHELL_VIEW + 2, 90.0), _on_shell(rng, N - 530 - h, 1e3, SHELL_VIEW + 2, 90.0)])
    r = rng.uniform(0.2, 0.24, N) * np.linalg.norm(mus, axis=1)
    order = rng.permutation(N)
    return dict(mus=mus[order], a=a_of(r)[order], rays=pinhole(64, 64, 64.0), K=8, exit_case=True)


INVALID_A = (0.0, -1.0, np.inf, np.nan)


def _invalid_scalar(rng, N, size):
    """a in {0, -1, +inf, NaN} (three of each) and three NaN centres inside an ordinary cloud."""
    mus, a = _front_cloud(rng, N)
    where = np.sort(rng.choice(N, 15, replace=False))
    for j, g in enumerate(where[:12]):
        a[g] = INVALID_A[j % 4]
    for j, g in enumerate(where[12:]):
        mus[g, j] = np.nan
    return dict(mus=mus, a=a, rays=pinhole(64, 64, 64.0), K=10, notes=dict(where=where))


def _sym(A):
    A = np.asarray(A, np.float64).astype(np.float32)
    iu = np.triu_indices(3, 1)
    A[:, iu[1], iu[0]] = A[:, iu[0], iu[1]]
    return A


def _aniso_forms(rng, n, a, ratio):
    """Symmetric positive forms R diag(a, a k1, a k2) R^T, k in [1, ratio]."""
    A = np.empty((n, 3, 3))
    for i in range(n):
        Rm = random_rotation(rng)
        A[i] = Rm @ np.diag(a[i] * np.array([1.0, rng.uniform(1, ratio), rng.uniform(1, ratio)])) @ Rm.T
    return A


def _invalid_general(rng, N, size):
    """Mildly anisotropic forms, three indefinite ones (diag(a, a, -a): d^T A d < 0 inside this camera's 35 degrees) and three with
    a zero eigenvalue (diag(a, 0, a): a slab of unbounded reach).  Their a is thr_act / |mu|^2 times 0.5 .. 2: an unbounded form
    is hit at |v| ~ |mu|, where act rounds by a |mu|^2 2^-22 -- a larger a would make the threshold itself undecidable in fp32."""
    mus, a = _front_cloud(rng, N, 0.36, 0.52)
    A = _aniso_forms(rng, N, a, 2.0)
    where = np.sort(rng.choice(N, 6, replace=False))
    for j, g in enumerate(where):
        aw = THR_ACT / (mus[g] ** 2).sum() * rng.uniform(0.5, 2.0)
        A[g] = np.diag([aw, aw, -aw]) if j % 2 == 0 else np.diag([aw, 0.0, aw])
    return dict(mus=mus, A=_sym(A), rays=pinhole(64, 64, 64.0), K=12, notes=dict(where=where))


NEEDLE_Q = 0.08


def _needles(rng, N, size):
    """40 needles along their own view direction m, A = a (I - (1 - q) m m^T), q = 0.08, among ordinary anisotropic forms: the
    ellipsoid {x : (x - mu)^T A (x - mu) < thr_act} has half-width r = 0.35 |mu| and half-length r / sqrt(q) = 1.24 |mu| along mu,
    so it contains the camera.  (q is the conditioning of len along the needle: d^T A d = a q there.)"""
    mus, a = _front_cloud(rng, N, 0.32, 0.48)
    A = _aniso_forms(rng, N, a, 2.0)
    where = np.sort(rng.choice(N, 40, replace=False))
    for g in where:
        nm = np.linalg.norm(mus[g])
        m = mus[g] / nm
        A[g] = a_of(0.35 * nm) * (np.eye(3) - (1.0 - NEEDLE_Q) * np.outer(m, m))
    return dict(mus=mus, A=_sym(A), rays=pinhole(64, 64, 64.0), K=12, exit_case=True, notes=dict(where=where))


def _per_axis(rng, N, size):
    """Per-axis (diagonal) forms of an ordinary cloud: the launch form the fragments entry has for them."""
    mus, a = _front_cloud(rng, N, 0.32, 0.48)
    A = a[:, None, None] * np.eye(3)[None] * rng.uniform(1.0, 2.0, (N, 1, 3))
    return dict(mus=mus, A=_sym(A), rays=pinhole(72, 88, 90.0), K=8, diag=True)


def _twins(rng, N, size):
    """Every Gaussian twice, at i and i + N / 2: bit-equal lens, which the result orders by ascending index."""
    h = N // 2
    mus, a = _front_cloud(rng, h, 0.08, 0.15)
    return dict(mus=np.concatenate([mus, mus]), a=np.concatenate([a, a]), rays=pinhole(64, 64, 64.0), K=4, exit_case=True)


BUILDERS = {
    "near_unit_plus": (lambda r, n, s: _near_unit(r, n, s, +NEAR_UNIT_S), "rays scaled by 1 + 4e-5, tiny Gaussians in one depth bucket: the exit's unit-ray bound"),
    "near_unit_minus": (lambda r, n, s: _near_unit(r, n, s, -NEAR_UNIT_S), "rays scaled by 1 - 4e-5"),
    "near_unit_edge": (lambda r, n, s: _near_unit(r, n, s, +NEAR_UNIT_EDGE), "rays scaled by 1 + 4.9e-5: the edge of the former tolerance"),
    "near_unit_inside": (lambda r, n, s: _near_unit(r, n, s, +NEAR_UNIT_INSIDE), "rays scaled by 1 + 1.9e-5: inside the tolerance, where the exit still runs"),
    "nonunit_random": (_nonunit_random, "per-pixel factors in [0.25, 4]: no tile may exit early"),
    "nonunit_one_pixel": (_nonunit_one_pixel, "one scaled pixel in every second tile: the exit is off for those tiles only"),
    "nonunit_1e-9": (lambda r, n, s: _nonunit_const(r, n, s, 1e-9), "len near 6e9: hits up to the 1e10 sentinel"),
    "nonunit_1e-12": (lambda r, n, s: _nonunit_const(r, n, s, 1e-12), "every len beyond 1e10: every pixel empty"),
    "wide_6px": (lambda r, n, s: _wide(r, n, s, 6.0), "focal length 6 px: super-tile cones with cs < 0.5, keys not 'front'"),
    "wide_2px": (lambda r, n, s: _wide(r, n, s, 2.0), "focal length 2 px: the region cone fails cmin > 0.05, the tiles' hold"),
    "scrambled": (_scrambled, "directions all over the sphere in random order: no cone usable, nothing culled"),
    "scrambled_supertiles": (_scrambled_supertiles, "coherent inside a super-tile, unrelated across the region: binA's !ok / use_rows arm"),
    "degenerate_rays": (_degenerate, "a zero, a NaN, an infinite and a 1e-30 ray inside ordinary tiles"),
    "front_4r": (_front_4r, "centres at (4 +- 1e-3) R, camera inside / on Gaussians, hits behind the camera"),
    "mixed_reach_behind": (lambda r, n, s: _mixed_reach(r, n, s, False), "a dozen of reach 20 behind thousands of tiny ones"),
    "mixed_reach_front": (lambda r, n, s: _mixed_reach(r, n, s, True), "the dozen in front"),
    "shell_one": (_shell_one, "every centre at the same fp32 distance: span at its 1e-20 floor"),
    "shell_two": (_shell_two, "shells at 1e-2 and 1e3: one bucket spans most of the scene"),
    "invalid_scalar": (_invalid_scalar, "a in {0, -1, inf, NaN} and NaN centres in an ordinary cloud"),
    "invalid_general": (_invalid_general, "indefinite forms and forms with a zero eigenvalue"),
    "needles": (_needles, "needles along the view direction that contain the camera: bin_own_bound's t < 0 arm"),
    "per_axis": (_per_axis, "per-axis forms (the fragments entry's diagonal launch)"),
    "twins": (_twins, "every Gaussian twice: ties in ascending index order on the binned path"),
}
NAMES = tuple(BUILDERS)
ONLY_SIZE = {"scrambled": "small", "scrambled_supertiles": "binned"}      # (N <= 1 500; binA's arm needs binA)


def case_ids():
    return [(n, s) for n in NAMES for s in SIZES if ONLY_SIZE.get(n, s) == s]


@functools.lru_cache(maxsize=None)
def build(name, size):
    import zlib
    fn, what = BUILDERS[name]
    rng = np.random.default_rng(zlib.crc32(f"{name}/{size}".encode()))
    return Case(name, size, what=what, **fn(rng, N_SIZE[size], size))


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 evaluation of (pixel, Gaussian) pairs and the error bound's terms
# ---------------------------------------------------------------------------------------------------------------------------
def pair_terms(case, d, g):
    """d [..., 3] ray directions (fp64 of the fp32 bundle), g [...] Gaussian indices (broadcastable against d's leading shape)
    -> dict of fp64 arrays: len, act, dsd and the bounds b_len, b_act, b_dsd of the module docstring."""
    mu = case.mus.astype(np.float64)[g]
    d = np.asarray(d, np.float64)
    ad, am = np.abs(d), np.abs(mu)
    with np.errstate(all="ignore"):
        if case.A is None:
            a = case.a.astype(np.float64)[g]
            aa = np.abs(a)
            dn2 = (d * d).sum(-1)
            ksk = a * dn2
            t = (a * (mu * d).sum(-1)) / ksk      # (as the oracle: 0 / 0 and inf / inf are no hits)
            v = mu - t[..., None] * d
            act = a * (v * v).sum(-1)
            dAm, dAd = aa * (ad * am).sum(-1), aa * dn2
            b_len = U23 / 2 * ((3 * dAm + 3 * np.abs(t) * dAd) / np.abs(ksk) + 3 * np.abs(t))
            e = U23 / 2 * (np.abs(v) + np.abs(t)[..., None] * ad) + ad * b_len[..., None]
            av = np.abs(v)
            vAv, vAe, eAe = aa * (av * av).sum(-1), aa * (av * e).sum(-1), aa * (e * e).sum(-1)
        else:
            A = case.A.astype(np.float64)[g]
            aA = np.abs(A)
            Ad = np.einsum("...ij,...j->...i", A, d)
            ksk = (d * Ad).sum(-1)
            t = (mu * Ad).sum(-1) / ksk
            v = mu - t[..., None] * d
            act = (v * np.einsum("...ij,...j->...i", A, v)).sum(-1)
            aAd = np.einsum("...ij,...j->...i", aA, ad)
            dAm, dAd = (am * aAd).sum(-1), (ad * aAd).sum(-1)
            b_len = U23 / 2 * ((6 * dAm + 8 * np.abs(t) * dAd) / np.abs(ksk) + 3 * np.abs(t))
            e = U23 / 2 * (np.abs(v) + np.abs(t)[..., None] * ad) + ad * b_len[..., None]
            av = np.abs(v)
            aAv, aAe = np.einsum("...ij,...j->...i", aA, av), np.einsum("...ij,...j->...i", aA, e)
            vAv, vAe, eAe = (av * aAv).sum(-1), (av * aAe).sum(-1), (e * aAe).sum(-1)
        b_act = 2 * vAe + eAe + 4 * U23 * vAv
        b_dsd = 4 * U23 * dAd
    return dict(len=t, act=act, dsd=ksk, b_len=b_len, b_act=b_act, b_dsd=b_dsd)


@functools.lru_cache(maxsize=None)
def case_delta(name, size):
    """-> (delta, delta_len, delta_act, worst outside-band ratio |d act| / (|act - thr| / 2)) over ALL pairs of the case."""
    case = build(name, size)
    d = case.rays.astype(np.float64).reshape(-1, 3)
    thr = case.thr_act
    g = np.arange(case.N)[None, :]
    d_len = d_act = outside = 0.0
    step = max(1, (1 << 21) // case.N)
    for p0 in range(0, d.shape[0], step):
        T = pair_terms(case, d[p0:p0 + step, None, :], g)
        with np.errstate(all="ignore"):
            hit = np.isfinite(T["len"]) & np.isfinite(T["act"]) & (np.abs(T["len"]) < 2e10)
            near = hit & (T["act"] < 2 * thr)
            band = near & (T["act"] > thr / 2)
            if near.any():
                d_len = max(d_len, float((2 * T["b_len"][near] / np.maximum(1.0, np.abs(T["len"][near]))).max()))
            if band.any():
                d_act = max(d_act, float((T["b_act"][band] / thr).max()))
            out = hit & ~band
            if out.any():
                outside = max(outside, float((T["b_act"][out] / (np.abs(T["act"][out] - thr) / 2)).max()))
    return max(d_len, d_act, 2.0 ** -20), d_len, d_act, outside


def bounds_fn(case):
    """What util.compare_trace_strict takes as `bounds`: (pixel numbers [M], Gaussian indices [M]) -> (b_len, b_act, b_dsd)."""
    d = case.rays.astype(np.float64).reshape(-1, 3)

    def fn(pix, idx):
        T = pair_terms(case, d[pix], idx)
        return T["b_len"], T["b_act"], T["b_dsd"]
    return fn


def oracle_fn(case):
    """(K', thr') -> oracle.trace_fwd in fp64 on the case; results are kept (the three runs of a case are shared by its tests)."""
    import oracle
    cache = {}

    def fn(Kp, thr, precision="f64"):
        key = (int(Kp), float(thr), precision)
        if key not in cache:
            out = oracle.trace_fwd(case.mus, case.isigmas(), case.rays, int(Kp), float(thr), precision=precision)
            for x in out:
                x.setflags(write=False)
            cache[key] = out
        return cache[key]
    return fn


@functools.lru_cache(maxsize=None)
def case_oracle(name, size):
    return oracle_fn(build(name, size))
