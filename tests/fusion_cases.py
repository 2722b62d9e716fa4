"""One asymmetric scene for the two fusion kernels (tsdf_integrate_kernel, tsdf_integrate_attr_kernel<C>), the generalised fp64
definition, single grid points on any device and the derived bounds, shared by tests/test_fusion_cases_cpu.py and
tests/test_gpu_fusion.py.

Nothing here is equal to anything else: nx, ny, nz = 19, 13, 11 (2 717 grid points: ten full workgroups of 256 and one of 157),
three different lo and three different voxel sizes, H, W = 40, 56, fx != fy in four of the five views and a principal point off
the image centre in every one.  A kernel that swaps H and W, hy and hz, ny and nz or fx and fy, or that strides the depth rows by H,
computes another volume on it.  The surface is the sphere r = 0.45 about (0.05, 0.03, -0.05); a depth is the analytic distance along
oracle.camera_np.pixel_rays' unit ray (the near root, or the far one where the near one is not positive), +inf off the sphere.

  view 0, 1   ordinary cameras outside the grid;
  view 2      a camera INSIDE the grid: grid points behind it (p_z <= 0) and in front of it in the same launch;
  view 3      looks away from the grid: every grid point is behind it, whole waves skip the view;
  view 4      15 % of its pixels (seeded) are overwritten with NaN, +inf, -inf, 0.0 and -1.5: step 3 of the rule.

Bounds, derived and never fitted (eps = 2^-24):
  tsdf_bound    meshing_cases.TSDF_BOUND (that module's header) with this grid's X and these views' C.  X bounds every number the
                coordinate x = lo + i h passes through -- the product i h <= (n - 1) h and the sum --, so X = max over the axes of
                |lo| + (n - 1) h, the form meshing_cases uses for its own grid; C = max |centre component|.  The derivation needs
                only |tsdf| <= 1 and integer weights, which prior() keeps, so it holds from a prior state and under a weight cap.
  attributes    meshing_attr_cases.fuse_bound(B, M) with M = max(|attr_image|, |prior attr|): an average of numbers below M stays
                below M, whichever of the two it started from."""
import functools
import types

import numpy as np
import torch

import meshing_attr_cases as ac
import meshing_cases as mc
from voge_amd import Aggregation

RES = (19, 13, 11)                       # nx, ny, nz
SHAPE = (RES[2], RES[1], RES[0])         # [nz,ny,nx]
LO = (-0.93, -0.71, -0.52)
VOXEL = (0.11, 0.13, 0.09)
IMAGE_H, IMAGE_W = 40, 56
TRUNC = 0.25
SPHERE_C = (0.05, 0.03, -0.05)
SPHERE_R = 0.45
MARK = ac.MARK                           # (2^-10, 2^-18): the marks of the existing fusion tests
MAX_WEIGHT = 3                           # the cap the prior state is used with
POISON = (float("nan"), float("inf"), float("-inf"), 0.0, -1.5)
POISON_SHARE = 0.15
# (eye, target, (fx, fy), (px, py))
VIEWS = (((2.4, 0.3, 0.2), SPHERE_C, (70.0, 55.0), (27.4, 19.7)),
         ((0.2, -2.2, 0.5), SPHERE_C, (60.0, 80.0), (30.2, 22.1)),
         ((0.95, 0.1, 0.02), SPHERE_C, (30.0, 26.0), (28.0, 20.0)),
         ((0.3, 0.2, 2.6), (0.3, 0.2, 6.0), (64.0, 64.0), (28.5, 20.5)),
         ((-1.9, 1.1, -0.8), SPHERE_C, (90.0, 75.0), (25.3, 17.9)))
B = len(VIEWS)

F32 = lambda xs: tuple(float(np.float32(x)) for x in xs)


def look_at(eye, target):
    """(R [3,3], T [3]) fp32 of a camera at `eye` that looks at `target`: mc.look_at(eye - target) with T shifted by -target @ R"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    R, T = mc.look_at(eye - target)
    return R, (T.astype(np.float64) - target @ R.astype(np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene():
    """The scene, made once: depth [5,40,56] (view 4 poisoned), depth_clean (the same before the poison), poisoned (bool [40,56] of
    view 4), R, T, focal [5,2], pp [5,2]: fp32 tensors on the host.  Nobody writes into them."""
    from oracle import camera_np
    cams = [look_at(eye, target) for eye, target, _, _ in VIEWS]
    R, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    focal = np.asarray([v[2] for v in VIEWS], np.float32)
    pp = np.asarray([v[3] for v in VIEWS], np.float32)
    rays, cen = camera_np.pixel_rays(R, T, focal, pp, (IMAGE_H, IMAGE_W))
    rays = rays.astype(np.float64)
    o = cen - np.asarray(SPHERE_C)
    b = np.einsum("bhwk,bk->bhw", rays, o)
    disc = b * b - ((o * o).sum(-1)[:, None, None] - SPHERE_R ** 2)
    root = np.sqrt(np.maximum(disc, 0))
    near, far = -b - root, -b + root
    d = np.where(near > 0, near, far)
    clean = np.where((disc > 0) & (d > 0), d, np.inf).astype(np.float32)
    rng = np.random.default_rng(4)
    poisoned = rng.uniform(size=(IMAGE_H, IMAGE_W)) < POISON_SHARE
    depth = clean.copy()
    depth[4][poisoned] = np.asarray(POISON, np.float32)[rng.integers(0, len(POISON), int(poisoned.sum()))]
    t = torch.from_numpy
    return types.SimpleNamespace(depth=t(depth), depth_clean=t(clean), poisoned=t(poisoned), R=t(R), T=t(T), focal=t(focal), pp=t(pp))


def centres(s):
    """[B,3] fp32: the centres in fp64, rounded once, as TSDFVolume.integrate makes them"""
    return Aggregation.camera_centres(s.R.double(), s.T.double()).to(torch.float32)


def cams(s, device="cpu", views=slice(None)):
    return mc.Cams(s.R[views].to(device), s.T[views].to(device), s.focal[views].to(device), s.pp[views].to(device))


def volume(device="cpu", channels=0, prior=None):
    """The scene's TSDFVolume, empty or holding a copy of prior = (tsdf, weight[, attr]); a prior attr of more channels is cut"""
    from voge_amd.Meshing import TSDFVolume
    vol = TSDFVolume(LO, voxel_size=VOXEL, resolution=RES, device=device, channels=channels)
    assert vol.tsdf.shape == SHAPE and vol.lo == F32(LO) and vol.voxel_size == F32(VOXEL)
    if prior is not None:
        vol.tsdf.copy_(prior[0])
        vol.weight.copy_(prior[1])
        if channels:
            vol.attr.copy_(prior[2][..., :channels])
    return vol


@functools.lru_cache(maxsize=None)
def prior(seed=7):
    """(tsdf uniform in [-1, 1], integer weights 0 .. 4, attr [nz,ny,nx,8] uniform in [-1, 1]) fp32, seeded: a volume some earlier
    calls left.  Used with max_weight = MAX_WEIGHT, below the largest prior weight: min(w + 1, max_weight) LOWERS such a weight, and
    that is the rule (step 7)."""
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1.0, 1.0, SHAPE).astype(np.float32)
    weight = rng.integers(0, 5, SHAPE).astype(np.float32)
    attr = rng.uniform(-1.0, 1.0, SHAPE + (8,)).astype(np.float32)
    return torch.from_numpy(tsdf), torch.from_numpy(weight), torch.from_numpy(attr)


@functools.lru_cache(maxsize=None)
def images(seed=11):
    """[5,40,56,8] fp32 noise in [-1, 1]: a different image per view AND per channel"""
    return ac.noise_images(B, 8, seed, IMAGE_H, IMAGE_W)


def definition(s, dtype, prior=None, max_weight=None, attr_image=None, mark=None, depth=None):
    """Aggregation.tsdf_integrate in `dtype` on the fp32 inputs of the scene (lo, h and trunc as the fp32 numbers the kernel gets, the
    centre rounded once to fp32) from an empty volume or from prior = (tsdf, weight[, attr]) -> (tsdf, weight[, marked][, attr])"""
    z = torch.zeros(SHAPE, dtype=dtype)
    tsdf, weight = (z, z.clone()) if prior is None else (prior[0].to(dtype), prior[1].to(dtype))
    kw = {}
    if attr_image is not None:
        C = attr_image.shape[-1]
        kw = {"attr": torch.zeros(SHAPE + (C,), dtype=dtype) if prior is None else prior[2][..., :C].to(dtype), "attr_image": attr_image}
    return Aggregation.tsdf_integrate(tsdf, weight, s.depth if depth is None else depth, s.R, s.T, s.focal, s.pp, list(F32(LO)), list(F32(VOXEL)),
                                      float(np.float32(TRUNC)), max_weight=max_weight, centre=centres(s), mark=mark, **kw)


def definition_fp64(s, prior=None, max_weight=None, attr_image=None, mark=MARK):
    return definition(s, torch.float64, prior, max_weight, attr_image, mark)


@functools.lru_cache(maxsize=None)
def reference(with_prior):
    """(tsdf, weight, marked, attr [..,8]) of the fp64 definition with images() -- from an empty volume, or from prior() under
    MAX_WEIGHT -- computed once and left unchanged.  The channels of the definition are independent: [..., :C] is the C-channel answer."""
    if with_prior:
        return definition_fp64(scene(), prior(), MAX_WEIGHT, images())
    return definition_fp64(scene(), attr_image=images())


def tsdf_bound(s):
    X = max(abs(l) + (n - 1) * h for l, n, h in zip(F32(LO), RES, F32(VOXEL)))
    d = s.depth[torch.isfinite(s.depth) & (s.depth > 0)]
    return mc.tsdf_bound_of(X, float(centres(s).abs().max()), float(np.float32(TRUNC)), B, float(d.max()))


def attr_bound(image, prior_attr=None):
    M = float(image.abs().max())
    if prior_attr is not None:
        M = max(M, float(prior_attr.abs().max()))
    return ac.fuse_bound(B, M)


def branch_counts(s):
    """Per view, how many grid points take each branch of the rule, in fp64 on the fp32 inputs, written out here beside the
    definition and not through it -> a list of dicts: behind / front (p_z), u<0, u>=W, v<0, v>=H (the first test that fails, in that
    order, among the points in front), then for the points inside the image nan / inf / nonpositive (the depth read), and for a valid
    depth cut (sdf < -trunc), clamped (sdf / trunc >= 1) and band."""
    lo, h = np.asarray(F32(LO)), np.asarray(F32(VOXEL))
    iz, iy, ix = np.meshgrid(*(np.arange(n) for n in SHAPE), indexing="ij")
    x = np.stack([lo[0] + ix * h[0], lo[1] + iy * h[1], lo[2] + iz * h[2]], -1).reshape(-1, 3)
    R, T, f, pp = (a.double().numpy() for a in (s.R, s.T, s.focal, s.pp))
    cen, depth, trunc = centres(s).double().numpy(), s.depth.numpy(), float(np.float32(TRUNC))
    out = []
    for b in range(B):
        p = x @ R[b] + T[b]
        front = p[:, 2] > 0
        c = {"behind": int((~front).sum()), "front": int(front.sum())}
        pz = np.where(front, p[:, 2], 1.0)
        u, v = pp[b, 0] - f[b, 0] * p[:, 0] / pz, pp[b, 1] - f[b, 1] * p[:, 1] / pz
        left = front
        for name, off in (("u<0", u < 0), ("u>=W", u >= IMAGE_W), ("v<0", v < 0), ("v>=H", v >= IMAGE_H)):
            c[name] = int((left & off).sum())
            left = left & ~off
        d = depth[b][np.where(left, np.floor(v), 0).astype(int), np.where(left, np.floor(u), 0).astype(int)].astype(np.float64)
        c["nan"], c["inf"] = int((left & np.isnan(d)).sum()), int((left & (d == np.inf)).sum())
        c["nonpositive"] = int((left & (d <= 0)).sum())
        valid = left & np.isfinite(d) & (d > 0)
        sdf = np.where(valid, d, 0.0) - np.linalg.norm(x - cen[b], axis=-1)
        c["cut"] = int((valid & (sdf < -trunc)).sum())
        c["clamped"] = int((valid & (sdf >= trunc)).sum())
        c["band"] = int((valid & (sdf >= -trunc) & (sdf < trunc)).sum())
        out.append(c)
    return out


# ---- single grid points, on any device ------------------------------------------------------------------------------------------

def axis_camera(depth, pp, focal=8.0, device="cpu"):
    """(depth [1,H,W] on the device, the camera R = I, T = (0, 0, 3) with the given principal point): the world point (0, 0, z) lies on
    the optical axis, p_x = p_y = 0, so u = pp_x and v = pp_y exactly, in every precision."""
    depth = torch.as_tensor(depth, dtype=torch.float32)
    depth = depth[None] if depth.dim() == 2 else depth
    return depth.to(device), mc.Cams(torch.eye(3, device=device)[None], torch.tensor([[0.0, 0.0, 3.0]], device=device),
                                     torch.tensor([[focal, focal]], device=device), torch.tensor([list(pp)], dtype=torch.float32, device=device))


def integrate_point(point, depth, cameras, trunc=0.5, device="cpu", image=None):
    """(tsdf, weight) of ONE grid point as two fp32 scalars on the host: a 2 x 2 x 2 volume of voxel 100 whose low corner is the point
    (tests/test_meshing_cpu.integrate_points, on any device).  On the host this is the definition in fp32.  With image [1,H,W,C] the
    volume has C channels and the point's attr [C] is appended."""
    from voge_amd.Meshing import TSDFVolume
    vol = TSDFVolume(point, voxel_size=100.0, resolution=2, device=device, channels=0 if image is None else image.shape[-1])
    vol.integrate(depth.to(device), cameras, trunc, attr=None if image is None else image.to(device))
    return (vol.tsdf[0, 0, 0].cpu(), vol.weight[0, 0, 0].cpu()) + (() if image is None else (vol.attr[0, 0, 0].cpu(),))
