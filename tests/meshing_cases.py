"""Fields, views, mesh checks and derived bounds shared by tests/test_meshing_cpu.py and tests/test_gpu_meshing.py.

Every bound here is derived from the arithmetic the kernels are documented to do (voge_amd/csrc/meshing.hip's header,
Aggregation.marching_tets and Aggregation.tsdf_integrate), never fitted to what they return; eps = 2^-24 below.

vertices   VERT_BOUND.  The kernel evaluates p_a + t (p_b - p_a), t = (level - v_a) / (v_b - v_a), p = lo + i h, in fp32 from
           the fp32 numbers the fp64 definition starts from.  t: three roundings, 0 <= t <= 1 (rounding is monotone), so
           |dt| <= 3.01 eps.  A grid coordinate: the product i h and the sum, each eps of a number below M = max |lo| +
           (n - 1) h over the axes: |dp| <= 2 eps M.  The vertex: (1 - t) dp_a + t dp_b <= 2 eps M; |p_b - p_a| dt <= 3.01 eps D
           with D the cell's diagonal (a component of an edge is at most h <= D); the difference and the product round by
           eps D each, the last sum by eps M.  Together eps (3 M + 5.01 D) < 4 * 2^-23 (M + D), the bound used.
tsdf       TSDF_BOUND, for a grid point that takes the same decisions (the definition's own marks exclude the others; the
           depth, a pixel's fp32 number, is exact in both).  x: 2 eps X per component, X = max |coordinate| of the grid;
           c: eps C / 2, C = max |centre component|; dx = x - c: eps (2 X + C / 2) + eps (X + C) <= eps (3 X + 1.5 C) = e1 per
           component.  dist = sqrt(dx^2 + dy^2 + dz^2): the input errors move it by at most sqrt(3) e1, the three squares, two
           sums and the root by at most 3 eps dist (each step is 0.5 relative in the root's argument or 1 in the root; 3 covers
           them with the second-order terms).  sdf = d - dist rounds by eps |sdf| <= eps (d + dist).  t = sdf / trunc: one
           more rounding of |t| <= ~1 (beyond 1 the minimum clamps both).  So |dt| <= (sqrt(3) e1 + eps (4 dist + d)) / trunc
           + eps =: e_t.  A running-average step (tsdf w + t) / (w + 1) with |tsdf|, |t| <= 1: the incoming errors average
           (w e_prev + e_t) / (w + 1) <= max(e_prev, e_t); the product, the sum and the quotient round by eps (w + (w + 1)) /
           (w + 1) + eps <= 3 eps.  After B steps: e_t + 3 B eps, with dist and d at their maxima over the views."""
import functools
import math

import numpy as np
import torch

from voge_amd import Aggregation

EPS = 2.0 ** -24


# ---- fields -------------------------------------------------------------------------------------------------------------------

def grid_xyz(shape):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return x, y, z


def sphere_field(shape=(12, 12, 12), centre=(5.3, 5.6, 5.45), r=3.7):
    x, y, z = grid_xyz(shape)
    return torch.from_numpy((np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32))


def sphere_gradient(centre):
    return lambda p: p - np.asarray(centre)


def torus_field(shape=(12, 12, 12), centre=(5.3, 5.6, 5.45), R=3.1, r=1.3):
    x, y, z = grid_xyz(shape)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return torch.from_numpy((np.sqrt(q ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32))


def torus_gradient(centre, R):
    def grad(p):
        d = p - np.asarray(centre)
        rho = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        q = rho - R
        return np.stack([q * d[:, 0] / rho, q * d[:, 1] / rho, d[:, 2]], -1)
    return grad


TWO_CENTRES = ((3.3, 3.6, 3.45), (8.2, 7.9, 8.35))


def two_spheres_field(shape=(12, 12, 12), r=2.2):
    x, y, z = grid_xyz(shape)
    d = [np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r for c in TWO_CENTRES]
    return torch.from_numpy(np.minimum(d[0], d[1]).astype(np.float32))


def two_spheres_gradient(p):
    d = [p - np.asarray(c) for c in TWO_CENTRES]
    near = (np.linalg.norm(d[0], axis=-1) < np.linalg.norm(d[1], axis=-1))[:, None]
    return np.where(near, d[0], d[1])


def random_field(shape=(9, 8, 7), seed=0, border=3.0):
    """Random normal values on nx x ny x nz = 7 x 8 x 9 (shape is [nz,ny,nx]) with an outside value on the border"""
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    for ax in range(3):
        idx = [slice(None)] * 3
        for k in (0, -1):
            idx[ax] = k
            v[tuple(idx)] = border
    return torch.from_numpy(v)


def holes_field(shape=(9, 8, 7), seed=0):
    """(values, weight) of the random field with 10 % of the points unobserved: half of them as NaN, half as weight == 0"""
    v = random_field(shape, seed).clone()
    rng = np.random.default_rng(seed + 100)
    n = v.numel()
    pick = rng.permutation(n)[:n // 10]
    w = torch.ones(n)
    flat = v.reshape(-1)
    flat[torch.from_numpy(pick[:len(pick) // 2])] = float("nan")
    w[torch.from_numpy(pick[len(pick) // 2:])] = 0.0
    return v, w.reshape(shape)


# ---- mesh checks --------------------------------------------------------------------------------------------------------------

def edge_stats(verts, faces):
    """dict of: counts (the number of faces on every undirected edge), directed_once (no directed edge twice), opposite (every
    directed edge is met by its opposite), chi (used vertices - edges + faces), used (bool [V])"""
    f = faces.cpu().numpy().astype(np.int64)
    V = int(verts.shape[0])
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    dkey = de[:, 0] * V + de[:, 1]
    rkey = de[:, 1] * V + de[:, 0]
    ukey = np.minimum(de[:, 0], de[:, 1]) * V + np.maximum(de[:, 0], de[:, 1])
    _, counts = np.unique(ukey, return_counts=True)
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    return {"counts": counts, "directed_once": len(np.unique(dkey)) == len(dkey), "opposite": set(dkey.tolist()) == set(rkey.tolist()),
            "chi": int(used.sum()) - len(counts) + len(f), "used": used}


def assert_closed(verts, faces, chi=None, all_used=True):
    s = edge_stats(verts, faces)
    assert len(faces) > 0
    assert (s["counts"] == 2).all(), np.unique(s["counts"], return_counts=True)
    assert s["directed_once"] and s["opposite"]
    if chi is not None:
        assert s["chi"] == chi, s["chi"]
    if all_used:
        assert s["used"].all()
    return s


def face_normals(verts, faces):
    v, f = verts.double().cpu().numpy(), faces.cpu().numpy().astype(np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3


def assert_on_grid_edges(verts, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), tol=1e-5):
    """Every vertex lies on a grid edge of Kuhn's split with t in [0, 1]: in grid units, frac(coordinate) is 0 or ONE common t on
    every axis."""
    g = (verts.double().cpu().numpy() - np.asarray(lo)) / np.asarray(h)
    fr = g - np.floor(g + tol)
    fr[np.abs(fr) < tol] = 0.0
    assert (fr >= 0).all() and (fr <= 1).all()
    t = fr.max(-1, keepdims=True)
    assert (np.minimum(np.abs(fr - t), np.abs(fr)) < 10 * tol).all()


def vert_bound(shape, lo, h):
    nz, ny, nx = shape
    M = max(abs(l) + (n - 1) * s for l, n, s in zip(lo, (nx, ny, nz), h))
    D = math.sqrt(sum(s * s for s in h))
    return 4 * 2.0 ** -23 * (M + D)


# ---- views of a sphere --------------------------------------------------------------------------------------------------------

SPHERE_R = 0.6
GRID_N = 24
GRID_LO = -1.013
GRID_H = 2.0 / 23
IMAGE = 96
FOCAL = 150.0
PP = (47.63, 48.29)


def look_at(eye):
    """(R [3,3], T [3]) fp32 of a camera at `eye` that looks at the origin, in cameras.pixel_rays' convention"""
    from oracle import camera_np
    eye = np.asarray(eye, np.float64)
    up = (0, 1, 0) if abs(eye[1]) < 0.9 * np.linalg.norm(eye) else (0, 0, 1)
    R = camera_np.look_at_rotation(eye[None], up=up)[0]
    T = -eye @ R
    return R.astype(np.float32), T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_views():
    """The 14 views of the end-to-end check: 6 axis + 8 diagonal directions at distance 3, each eye offset by
    (0.137, -0.071, 0.093); 96^2 images, f = 150, pp = (47.63, 48.29) -> (depth [14,96,96], R, T, focal [14,2], pp [14,2]) fp32
    tensors; depth is the analytic ray-sphere distance along the unit pixel ray (r = 0.6 about the origin), inf off the sphere."""
    from oracle import camera_np
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    Rs, Ts = [], []
    for d in dirs:
        d = np.asarray(d, np.float64)
        R, T = look_at(3.0 * d / np.linalg.norm(d) + np.array([0.137, -0.071, 0.093]))
        Rs.append(R)
        Ts.append(T)
    R, T = np.stack(Rs), np.stack(Ts)
    B = len(dirs)
    focal = np.full((B, 2), FOCAL, np.float32)
    pp = np.tile(np.asarray(PP, np.float32), (B, 1))
    rays, cen = camera_np.pixel_rays(R, T, focal, pp, (IMAGE, IMAGE))
    rays = rays.astype(np.float64)
    b = np.einsum("bhwk,bk->bhw", rays, cen)
    disc = b * b - ((cen * cen).sum(-1)[:, None, None] - SPHERE_R ** 2)
    depth = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (depth, R, T, focal, pp))


def three_views():
    """Views 0, 2 and 6 (+x, +y and the (1,1,1) diagonal): three views that overlap, so weights reach 3"""
    return tuple(t[[0, 2, 6]] for t in sphere_views())


class Cams:
    """What TSDFVolume.integrate reads of a camera object"""

    def __init__(self, R, T, focal, pp):
        self.R, self.T, self.focal_length, self.principal_point = R, T, focal, pp


def radial_error(verts):
    return float((verts.double().norm(dim=-1) - SPHERE_R).abs().max())


def tsdf_bound_of(X, C, trunc, B, depth_max):
    """TSDF_BOUND of the header for any grid: X bounds the numbers a coordinate lo + i h passes through, C = max |centre component|"""
    e1 = EPS * (3 * X + 1.5 * C)
    dist = math.sqrt(3) * (X + C)
    return (math.sqrt(3) * e1 + EPS * (4 * dist + depth_max)) / trunc + EPS + 3 * B * EPS


def tsdf_bound(centre, trunc, B, depth_max):
    """TSDF_BOUND of the header for the end-to-end grid"""
    return tsdf_bound_of(abs(GRID_LO) + (GRID_N - 1) * GRID_H, float(centre.abs().max()), trunc, B, depth_max)


def definition_fp64(depth, R, T, focal, pp, trunc, mark=None, max_weight=None, n=GRID_N):
    """Aggregation.tsdf_integrate in fp64 on the fp32 inputs (lo, h and trunc as the fp32 numbers the kernel gets)"""
    f32 = lambda x: float(np.float32(x))
    z = torch.zeros((n, n, n), dtype=torch.float64)
    centre = Aggregation.camera_centres(R.double(), T.double()).to(torch.float32)
    return Aggregation.tsdf_integrate(z, z.clone(), depth, R, T, focal, pp, [f32(GRID_LO)] * 3, f32(GRID_H), f32(trunc),
                                      max_weight=max_weight, centre=centre, mark=mark)
