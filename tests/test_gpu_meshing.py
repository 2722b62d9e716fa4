"""GPU tests of the mesh extraction kernels (voge_tsdf_integrate, voge_mtet_count / _scan / _emit; an extension, the reference and
the oracle have none) and of VoGE.Meshing on the device.

extraction   faces with torch.equal against the definition (Aggregation.marching_tets in fp64 on the host, from the same fp32
             values, level, lo and voxel size), vertices within meshing_cases.vert_bound -- 4 * 2^-23 (M + D), derived in that
             module's header from the three roundings of t and the roundings of the positions;
fusion       against the definition in fp64 on the grid points it does not mark itself (a pixel coordinate within 2^-10 of an
             integer, |sdf +- trunc| within 2^-18 of the distance): equal weights and tsdf within meshing_cases.tsdf_bound,
             derived there from the rounding of d - |x - c| over trunc and B running-average steps;
end to end   properties only (closed, chi = 2, radial error <= 1.0 h): a grid point at a pixel boundary may legitimately differ.
The grids are small on purpose."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import meshing_cases as mc
from util import log_line
from voge_amd import Aggregation, Losses, ops
from voge_amd.Meshing import TSDFVolume, extract_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = lambda xs: tuple(float(np.float32(x)) for x in xs)


def check_extraction(label, values, weight=None, level=0.0, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0)):
    lo, h = F32(lo), F32(h)
    ref_v, ref_f = Aggregation.marching_tets(values.double(), weight, level, lo, h)
    verts, faces = extract_mesh(values.to(DEV), None if weight is None else weight.to(DEV), level, lo, h)
    assert verts.is_cuda and verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert verts.shape == (len(ref_v), 3) and faces.shape == (len(ref_f), 3)
    assert torch.equal(faces.cpu(), ref_f.to(torch.int32))
    bound = mc.vert_bound(values.shape, lo, h)
    worst = float((verts.cpu().double() - ref_v).abs().max()) if len(ref_v) else 0.0
    log_line(f"[parity] marching_tets {label}: V {len(ref_v)}, F {len(ref_f)}, max |dv| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    return verts, faces


def bordered_noise(shape, seed):
    return mc.random_field(shape, seed)


def test_random_fields_meet_every_case():
    values = mc.random_field()
    check_extraction("random 7x8x9", values)
    check_extraction("random 7x8x9, level 0.25, placed", values, level=0.25, lo=(-1.5, 0.25, 2.0), h=(0.5, 0.3, 0.125))
    verts, faces = check_extraction("random 7x8x9, seed 1", mc.random_field(seed=1))
    mc.assert_closed(verts, faces)


@pytest.mark.parametrize("shape", [(9, 7, 5), (33, 9, 17)])      # nx x ny x nz = 5 x 7 x 9 and 17 x 9 x 33: no multiple of a block
def test_sizes_that_are_no_multiple_of_a_block(shape):
    n = shape[0] * shape[1] * shape[2]
    assert n % ops.MTET_BLOCK != 0
    verts, faces = check_extraction(f"random {shape[2]}x{shape[1]}x{shape[0]}", bordered_noise(shape, 5), lo=(0.3, -2.0, 1.0), h=(0.1, 0.2, 0.3))
    mc.assert_closed(verts, faces)


def test_analytic_fields_on_the_device():
    for name, field, chi in (("sphere", mc.sphere_field(), 2), ("torus", mc.torus_field(), 0), ("two spheres", mc.two_spheres_field(), 4)):
        verts, faces = check_extraction(name, field)
        mc.assert_closed(verts, faces, chi=chi)


def test_top_level_scan_runs_more_than_once():
    """65^3 = 274 625 grid points are 1073 scan blocks, more than the 1024 one round of the top level takes; a gyroid crosses every
    block, so vertex and face offsets on both sides of the round's boundary are used."""
    n = 65
    assert (n ** 3 + ops.MTET_BLOCK - 1) // ops.MTET_BLOCK > ops.MTET_TOP
    x, y, z = (a * (2 * np.pi / 13.7) for a in mc.grid_xyz((n, n, n)))
    g = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x) + 0.05
    values = torch.from_numpy(g.astype(np.float32))
    verts, faces, edge_mask, face_count = ops.marching_tets(values.to(DEV), None, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), return_tables=True)
    ref_v, ref_f = Aggregation.marching_tets(values.double())
    assert torch.equal(faces.cpu(), ref_f.to(torch.int32))
    worst = float((verts.cpu().double() - ref_v).abs().max())
    bound = mc.vert_bound(values.shape, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    log_line(f"[parity] marching_tets gyroid 65^3: V {len(ref_v)}, F {len(ref_f)}, max |dv| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    # blocks beyond the first round carry vertices and faces
    last = ops.MTET_TOP * ops.MTET_BLOCK
    assert int(edge_mask[last:].ne(0).sum()) > 0 and int(face_count[last:].sum()) > 0
    assert int(face_count.sum()) == len(ref_f) and int(face_count.max()) <= 12 and int(edge_mask.max()) < 128


def test_holes_empty_results_and_the_smallest_grid():
    values, weight = mc.holes_field()
    verts, faces = check_extraction("holes", values, weight)
    assert set(np.unique(mc.edge_stats(verts, faces)["counts"]).tolist()) == {1, 2}
    for fill in (-1.0, 1.0):
        verts, faces = extract_mesh(torch.full((5, 6, 7), fill, device=DEV))
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.is_cuda and faces.dtype == torch.int32
    verts, faces = extract_mesh(torch.full((5, 6, 7), -1.0, device=DEV), torch.zeros((5, 6, 7), device=DEV))      # nothing observed
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    for corner in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
        values = torch.ones(2, 2, 2)
        values[corner] = -1.0
        verts, faces = check_extraction(f"2x2x2, corner {corner}", values)
        assert faces.shape[0] >= 2
    with pytest.raises(ValueError):
        extract_mesh(torch.zeros((1, 4, 4), device=DEV))


# ---- fusion -------------------------------------------------------------------------------------------------------------------

def device_volume():
    return TSDFVolume([mc.GRID_LO] * 3, voxel_size=mc.GRID_H, resolution=mc.GRID_N, device=DEV)


def device_cams(R, T, focal, pp):
    return mc.Cams(R.to(DEV), T.to(DEV), focal.to(DEV), pp.to(DEV))


def test_integration_against_the_fp64_definition():
    depth, R, T, focal, pp = mc.three_views()
    B, trunc = 3, 2 * mc.GRID_H
    ref_t, ref_w, marked = mc.definition_fp64(depth, R, T, focal, pp, trunc, mark=(2.0 ** -10, 2.0 ** -18))
    share = float(marked.double().mean())
    assert share <= 0.02, share      # on the definition's own marks: expected 4 delta B = 1.2 % in generic position
    vol = device_volume().integrate(depth.to(DEV), device_cams(R, T, focal, pp), trunc)
    assert vol.tsdf.is_cuda and vol.tsdf.dtype == torch.float32 and vol.tsdf.shape == (mc.GRID_N,) * 3
    got_t, got_w = vol.tsdf.cpu().double(), vol.weight.cpu().double()
    keep = ~marked
    centre = Aggregation.camera_centres(R.double(), T.double())
    bound = mc.tsdf_bound(centre, float(np.float32(trunc)), B, float(depth[torch.isfinite(depth)].max()))
    worst = float((got_t - ref_t)[keep].abs().max())
    flips = int((got_w != ref_w)[marked].sum())
    log_line(f"[parity] tsdf_integrate 24^3 x 3 views: marked {share * 100:.2f} %, of them {flips} with another weight; "
             f"max |dtsdf| {worst:.3e}, bound {bound:.3e}; weights up to {int(ref_w.max())}")
    # the comparison is not empty: the views overlap, and they update more than 1000 grid points (the band of +-trunc around the
    # sphere alone holds 4 pi (r / h)^2 * 4 = 2390 of them, and three views from one octant see about half of the surface)
    assert int(ref_w.max()) == 3 and int((ref_w[keep] > 0).sum()) > 1000
    assert torch.equal(got_w[keep], ref_w[keep])
    assert worst <= bound
    # one call with three views is three calls with one view each, bit for bit
    three = device_volume()
    for b in range(B):
        three.integrate(depth[b:b + 1].to(DEV), device_cams(R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1]), trunc)
    assert torch.equal(three.tsdf, vol.tsdf) and torch.equal(three.weight, vol.weight)
    # max_weight caps the weight
    capped = device_volume().integrate(depth.to(DEV), device_cams(R, T, focal, pp), trunc, max_weight=2)
    assert torch.equal(capped.weight, vol.weight.clamp(max=2))
    # a mismatch of B with the cameras raises
    with pytest.raises(ValueError):
        device_volume().integrate(depth.to(DEV), device_cams(R[:2], T[:2], focal[:2], pp[:2]), trunc)


def test_end_to_end_on_the_device():
    depth, R, T, focal, pp = mc.sphere_views()
    vol = device_volume().integrate(depth.to(DEV), device_cams(R, T, focal, pp), 2 * mc.GRID_H)
    verts, faces = extract_mesh(vol)
    mc.assert_closed(verts, faces, chi=2)
    err = mc.radial_error(verts.cpu())
    log_line(f"[parity] meshing end to end: V {len(verts)}, F {len(faces)}, radial error {err / mc.GRID_H:.3f} h")
    assert err <= 1.0 * mc.GRID_H
    normal, centroid = mc.face_normals(verts, faces)
    assert ((normal * centroid).sum(-1) > 0).all()
    # the mesh side of the project takes it as it is
    topo = Losses.MeshTopology(faces, num_verts=len(verts), device=DEV)
    terms = Losses.mesh_regularisers(verts, topo)
    assert all(bool(torch.isfinite(t)) for t in terms) and float(terms[0]) > 0
    u = torch.from_numpy(np.random.default_rng(0).standard_normal((4000, 3)).astype(np.float32))
    sphere = (mc.SPHERE_R * u / u.norm(dim=-1, keepdim=True)).to(DEV)
    loss, _ = Losses.chamfer_distance(verts, sphere)
    assert bool(torch.isfinite(loss)) and 0 < float(loss) < mc.GRID_H ** 2
    points, _ = Losses.sample_points_from_meshes(verts, faces, return_normals=True, u=torch.rand((2000, 3), generator=torch.Generator().manual_seed(0)))
    assert float((points.norm(dim=-1) - mc.SPHERE_R).abs().max()) <= 1.0 * mc.GRID_H


def test_demo_path():
    """demo/ExtractMesh.py at 64^3 with 8 views of 64^2 depth from the renderer ends with a non-empty mesh."""
    spec = importlib.util.spec_from_file_location("extract_mesh_demo", os.path.join(ROOT, "demo", "ExtractMesh.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    verts, faces, report = demo.run(resolution=64, views=8, image=64, out=None)
    log_line(f"[parity] demo/ExtractMesh.py 64^3, 8 views of 64^2: {report}")
    assert len(verts) > 100 and len(faces) > 100 and torch.isfinite(verts).all()
    assert int(faces.max()) < len(verts) and int(faces.min()) >= 0
    assert float(verts.abs().max()) < 0.5      # inside the volume around the bunny
