"""Attribute images, attribute fields and derived bounds shared by tests/test_meshing_attr_cpu.py and tests/test_gpu_meshing_attr.py;
the grids, the views and the mesh checks are those of tests/meshing_cases.py.

Every bound here is derived from the arithmetic the kernels are documented to do (voge_amd/csrc/meshing.hip's header, step 6 of
Aggregation.tsdf_integrate and the attr rule of Aggregation.marching_tets), never fitted to what they return; eps = 2^-24 below.

fusion     fuse_bound = 3 B eps M, M = max |attr_image|, for a grid point that takes the definition's decisions in every view (the
           definition's own marks exclude the others) and therefore reads the same pixels and carries the same integer weights.  A
           pixel is an fp32 number, exact in fp32 and in fp64.  One step a' = (a w + p) / (w + 1) with |a|, |p| <= M (an average of
           numbers below M) and w an integer, exact: the incoming error is scaled by w / (w + 1) <= 1; the product a w rounds by
           eps M w, the sum by eps M (w + 1), and the division carries both over as eps M (w + (w + 1)) / (w + 1) <= 2 eps M; the
           quotient rounds by eps M.  3 eps M a step, and a step never amplifies what it receives: 3 B eps M after B views.  This is
           the running-average term of meshing_cases.TSDF_BOUND with M in the place of 1; the other terms of that bound belong to
           the distance and have no counterpart, because nothing is computed from a pixel before it is averaged.
vertices   vert_attr_bound = 6 * 2^-23 M = 12 eps M, M = max |attr|.  The kernel evaluates a_a + t (a_b - a_a) in fp32 with the t of
           the vertex: |dt| <= 3.01 eps (meshing_cases' header: three roundings, 0 <= t <= 1) acts on |a_b - a_a| <= 2 M: 6.02 eps M;
           the difference rounds by eps 2 M and the product, at most 2 M, by eps 2 M; the last sum, a number between a_a and a_b,
           by eps M.  Together 11.02 eps M < 12 eps M.
position   an attribute that IS the grid point's position ties the rows of vert_attr to the numbering of the vertices:
           |vert_attr - verts| <= vert_attr_bound(M) + meshing_cases.vert_bound.  The field is the fp64 position rounded to fp32 (eps M
           a point, an average of which stays below eps M); the fp64 definition's interpolation of it is the fp64 vertex up to that
           eps M; the kernel's vert_attr is within 11.02 eps M of the former, the kernel's vertex within eps (3 M + 5.01 D) of the
           latter (meshing_cases' header): 15.02 eps M + 5.01 eps D in all, below the sum of the two bounds used, 12 eps M and
           8 eps (M + D).
hit points  HIT_CAP = 1.0 h on the 24^3 grid of the end-to-end check.  The attribute image of a view is every pixel's own hit point,
           centre + depth * unit ray (zeros off the sphere), so a fused attribute is an average of points of the surface that the
           grid point's pixels look at, and a vertex's attribute should be the vertex: a transposed pixel index, another view or
           another centre moves it by several h.  Measured on the fp64 definition when the feature was specified: 0.66 h at the
           most and 0.20 h in the mean over 2 732 vertices, with a pixel footprint at the surface of (3 - 0.6) / 150 = 0.18 h; the
           cap is that maximum plus two footprints, because a grid point on a pixel boundary may take the neighbouring pixel,
           and it is the radial cap the geometry's own end-to-end test uses."""
import functools

import numpy as np
import torch

import meshing_cases as mc
from voge_amd import Aggregation

EPS = mc.EPS
HIT_CAP = 1.0      # in units of mc.GRID_H
MARK = (2.0 ** -10, 2.0 ** -18)      # the marks of test_integration_against_the_fp64_definition


def fuse_bound(B, M):
    return 3 * B * EPS * M


def vert_attr_bound(M):
    return 6 * 2.0 ** -23 * M


# ---- attribute images ----------------------------------------------------------------------------------------------------------

def noise_images(B, C, seed=0, H=mc.IMAGE, W=mc.IMAGE):
    """[B,H,W,C] fp32, uniform in [-1, 1], a different image per view"""
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (B, H, W, C)).astype(np.float32))


def same_in_every_channel(C, seed=0):
    """noise_images(3, 1, seed) repeated over C channels"""
    return noise_images(3, 1, seed).expand(3, mc.IMAGE, mc.IMAGE, C).contiguous()


@functools.lru_cache(maxsize=None)
def hit_point_images():
    """[14,96,96,3] fp32 beside mc.sphere_views(): every pixel's own hit point c + depth * unit ray, zeros off the sphere"""
    from oracle import camera_np
    depth, R, T, focal, pp = mc.sphere_views()
    rays, cen = camera_np.pixel_rays(R.numpy(), T.numpy(), focal.numpy(), pp.numpy(), (mc.IMAGE, mc.IMAGE))
    rays = rays.astype(np.float64)
    rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
    d = depth.numpy().astype(np.float64)
    on = np.isfinite(d)
    hit = cen.astype(np.float64)[:, None, None, :] + np.where(on, d, 0.0)[..., None] * rays
    return torch.from_numpy(np.where(on[..., None], hit, 0.0).astype(np.float32))


def definition_fp64(depth, R, T, focal, pp, trunc, attr_image, mark=None, max_weight=None, n=mc.GRID_N):
    """Aggregation.tsdf_integrate with an attribute in fp64 on the fp32 inputs (lo, h and trunc as the fp32 numbers the kernel gets)
    from an empty volume -> (tsdf, weight[, marked], attr)"""
    f32 = lambda x: float(np.float32(x))
    z = torch.zeros((n, n, n), dtype=torch.float64)
    centre = Aggregation.camera_centres(R.double(), T.double()).to(torch.float32)
    return Aggregation.tsdf_integrate(z, z.clone(), depth, R, T, focal, pp, [f32(mc.GRID_LO)] * 3, f32(mc.GRID_H), f32(trunc),
                                      max_weight=max_weight, centre=centre, mark=mark,
                                      attr=torch.zeros((n, n, n, attr_image.shape[-1]), dtype=torch.float64), attr_image=attr_image)


@functools.lru_cache(maxsize=None)
def three_view_reference(max_weight=None):
    """(attr_image [3,96,96,3], tsdf, weight, marked, attr) of mc.three_views() with trunc = 2 h and noise_images(3, 3): the fp64
    definition with its marks, computed once"""
    image = noise_images(3, 3)
    return (image,) + definition_fp64(*mc.three_views(), 2 * mc.GRID_H, image, mark=MARK, max_weight=max_weight)


def volume(device="cpu", channels=3):
    from voge_amd.Meshing import TSDFVolume
    return TSDFVolume([mc.GRID_LO] * 3, voxel_size=mc.GRID_H, resolution=mc.GRID_N, device=device, channels=channels)


def cams(R, T, focal, pp, device="cpu"):
    return mc.Cams(R.to(device), T.to(device), focal.to(device), pp.to(device))


# ---- attribute fields ----------------------------------------------------------------------------------------------------------

def noise_field(shape, C, seed=0):
    """[nz,ny,nx,C] fp32, standard normal"""
    return torch.from_numpy(np.random.default_rng(seed + 1000).standard_normal(tuple(shape) + (C,)).astype(np.float32))


def position_field(shape, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0)):
    """[nz,ny,nx,3] fp32: every grid point's own position lo + i h (from the fp32 lo and h, in fp64, rounded once)"""
    f32 = lambda xs: [float(np.float32(x)) for x in xs]
    lo, h = f32(lo), f32(h)
    x, y, z = mc.grid_xyz(shape)
    return torch.from_numpy(np.stack([lo[0] + x * h[0], lo[1] + y * h[1], lo[2] + z * h[2]], -1).astype(np.float32))


def extraction_cases():
    """[(label, values, weight, level, lo, h)]: the fields the extraction's own tests use"""
    unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    cases = [("random 7x8x9", mc.random_field(), None, 0.0) + unit,
             ("random 7x8x9, level 0.25, placed", mc.random_field(), None, 0.25, (-1.5, 0.25, 2.0), (0.5, 0.3, 0.125)),
             ("holes",) + mc.holes_field() + (0.0,) + unit,
             ("random 17x9x33", mc.random_field((33, 9, 17), 5), None, 0.0, (0.3, -2.0, 1.0), (0.1, 0.2, 0.3))]
    for corner in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
        values = torch.ones(2, 2, 2)
        values[corner] = -1.0
        cases.append((f"2x2x2, corner {corner}", values, None, 0.0) + unit)
    return cases


def edge_ends(verts, lo, h, tol=1e-9):
    """(ia, ib) [V,3] integer grid coordinates (x, y, z) of the two ends of the grid edge every vertex of a fp64 mesh lies on"""
    rel = (verts.double() - torch.tensor(lo, dtype=torch.float64)) / torch.tensor(h, dtype=torch.float64)
    ia = torch.floor(rel + tol).long()
    return ia, ia + ((rel - ia) > tol).long()
