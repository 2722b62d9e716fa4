"""CPU tests of the mesh extraction's definitions (Aggregation.marching_tets, Aggregation.tsdf_integrate), of VoGE.Meshing on
host tensors -- which takes the definitions -- and of the new entries' argument checks.  No GPU.

The meshes are checked by what a correct extraction must satisfy, not against stored results: every undirected edge in exactly
two faces, every directed edge met once by its opposite, the Euler characteristic of the surface, face normals along the field's
gradient (inside -> outside), every vertex used and on its grid edge.  meshing_cases has the fields and the checks."""
import itertools

import numpy as np
import pytest
import torch

import meshing_cases as mc
from voge_amd import Aggregation
from voge_amd.Meshing import TSDFVolume, extract_mesh

CENTRE = (5.3, 5.6, 5.45)


def test_module_is_aliased():
    import VoGE
    import VoGE.Meshing
    from voge_amd import Meshing
    assert VoGE.Meshing is Meshing and VoGE.Meshing.extract_mesh is extract_mesh


@pytest.mark.parametrize("name,field,chi,gradient", [
    ("sphere", mc.sphere_field, 2, mc.sphere_gradient(CENTRE)),
    ("torus", mc.torus_field, 0, mc.torus_gradient(CENTRE, 3.1)),
    ("two spheres", mc.two_spheres_field, 4, mc.two_spheres_gradient),
])
def test_analytic_fields(name, field, chi, gradient):
    verts, faces = extract_mesh(field())
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.shape[1] == 3 and faces.shape[1] == 3
    mc.assert_closed(verts, faces, chi=chi, all_used=True)
    normal, centroid = mc.face_normals(verts, faces)
    assert ((normal * gradient(centroid)).sum(-1) > 0).all()
    mc.assert_on_grid_edges(verts)
    if name == "sphere":
        assert (len(verts), len(faces)) == (776, 1548)
        assert float((verts.double() - torch.tensor(CENTRE, dtype=torch.float64)).norm(dim=-1).sub(3.7).abs().max()) < 0.1


def test_tables_are_positively_oriented_and_cover_the_cell():
    corners, count, tri = Aggregation._mtet_tables()
    vec = lambda c: np.array([(c >> k) & 1 for k in range(3)], float)
    assert len({tuple(sorted(c)) for c in corners}) == 6
    for c, perm in zip(corners, itertools.permutations(range(3))):
        assert c[0] == 0 and c[3] == 7 and {c[1], c[2]} == {1 << perm[0], (1 << perm[0]) | (1 << perm[1])}
        assert np.linalg.det(np.stack([vec(c[1]), vec(c[2]), vec(c[3])])) > 0
    assert count == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def test_random_field_is_closed_and_meets_every_case():
    values = mc.random_field()
    verts, faces = extract_mesh(values)
    mc.assert_closed(verts, faces, all_used=True)
    mc.assert_on_grid_edges(verts)
    # every non-trivial case of every tetrahedron occurs (6 x 14): what makes this field the kernels' parity case
    corners, _, _ = Aggregation._mtet_tables()
    ins = (values < 0).numpy()
    nz, ny, nx = ins.shape
    cell = lambda c: ins[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    for cs in corners:
        case = sum(cell(cs[j]).astype(int) << j for j in range(4))
        assert set(np.unique(case)) >= set(range(1, 15))


def test_level_and_placement():
    values = mc.sphere_field()
    lo, h = (-1.5, 0.25, 2.0), (0.5, 0.25, 0.125)
    v0, f0 = extract_mesh(values, level=0.25)
    v1, f1 = extract_mesh(values, level=0.25, lo=lo, voxel_size=h)
    assert torch.equal(f0, f1)
    assert torch.allclose(v1, v0 * torch.tensor(h) + torch.tensor(lo), atol=1e-5)
    mc.assert_closed(v1, f1, chi=2)
    mc.assert_on_grid_edges(v1, lo, h)
    assert float((v0.double() - torch.tensor(CENTRE, dtype=torch.float64)).norm(dim=-1).sub(3.95).abs().max()) < 0.1


def test_holes():
    values, weight = mc.holes_field()
    assert torch.isnan(values).any() and (weight == 0).any()
    verts, faces = extract_mesh(values, weight)
    stats = mc.edge_stats(verts, faces)
    assert set(np.unique(stats["counts"]).tolist()) == {1, 2}      # boundary edges exist, and nothing else
    assert stats["directed_once"]
    assert torch.isfinite(verts).all()
    # no face touches an unobserved corner: the corners of a vertex's grid edge are its coordinates rounded down and up
    obs = (torch.isfinite(values) & (weight > 0)).numpy()
    g = verts[faces.long().reshape(-1)].double().numpy()
    for corner in (np.floor(g + 1e-6), np.ceil(g - 1e-6)):
        c = corner.astype(int)
        assert obs[c[:, 2], c[:, 1], c[:, 0]].all()
    # the same field fully observed has more faces
    assert len(faces) < len(extract_mesh(mc.random_field())[1])


def test_degenerate_inputs():
    for fill in (-1.0, 1.0):      # all inside, all outside
        verts, faces = extract_mesh(torch.full((5, 6, 7), fill))
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.dtype == torch.float32 and faces.dtype == torch.int32
    # 2 x 2 x 2 with the origin inside: one vertex on each of its seven edges, one triangle in each of the six tetrahedra
    values = torch.ones(2, 2, 2)
    values[0, 0, 0] = -1.0
    verts, faces = extract_mesh(values)
    assert verts.shape == (7, 3) and faces.shape == (6, 3)
    assert torch.equal(verts, torch.tensor([[(d >> k) & 1 for k in range(3)] for d in range(1, 8)], dtype=torch.float32) * 0.5)
    normal, centroid = mc.face_normals(verts, faces)
    assert ((normal * centroid).sum(-1) > 0).all()
    # the far corner inside instead: its edges belong to the seven other points
    values = torch.ones(2, 2, 2)
    values[1, 1, 1] = -3.0
    verts, faces = extract_mesh(values)
    assert verts.shape == (7, 3) and faces.shape == (6, 3)
    normal, centroid = mc.face_normals(verts, faces)
    assert ((normal * (centroid - 1.0)).sum(-1) > 0).all()
    with pytest.raises(ValueError):
        extract_mesh(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError):
        extract_mesh(torch.zeros(4, 4))
    with pytest.raises(ValueError):
        extract_mesh(torch.zeros(2, 2, 2).expand(2, 2, 2), weight=torch.zeros(3, 2, 2))
    with pytest.raises(ValueError, match="32-bit"):
        extract_mesh(torch.zeros(1, 1, 1).expand(700, 700, 700))


def test_corners_exactly_at_the_level_follow_the_strict_rule():
    # value == level is OUTSIDE (inside <=> value < level): a field that only touches the level has no surface ...
    values = torch.ones(3, 3, 3)
    values[1, 1, 1] = 0.0
    verts, faces = extract_mesh(values)
    assert len(verts) == 0 and len(faces) == 0
    # ... and one that dips below it around a corner AT the level puts coincident vertices on that corner
    values[1, 1, 1] = -1.0
    values[1, 1, 2] = 0.0
    verts, faces = extract_mesh(values)
    mc.assert_closed(verts, faces, chi=2)
    at = (verts == torch.tensor([2.0, 1.0, 1.0])).all(-1)
    assert at.sum() >= 1 and torch.isfinite(verts).all()
    # the same decisions at another level
    verts2, faces2 = extract_mesh(values + 0.5, level=0.5)
    assert torch.equal(faces2, faces) and torch.allclose(verts2, verts)


# ---- fusion -------------------------------------------------------------------------------------------------------------------

def small_volume():
    return TSDFVolume([mc.GRID_LO] * 3, voxel_size=mc.GRID_H, resolution=mc.GRID_N)


def test_volume_constructor():
    a = TSDFVolume((-1, -1, -1), hi=(1, 1, 1), resolution=21)
    assert a.resolution == (21, 21, 21) and a.tsdf.shape == (21, 21, 21) and abs(a.voxel_size[0] - 0.1) < 1e-7
    b = TSDFVolume((-1, -1, -1), hi=(1, 2, 3), voxel_size=0.1)
    assert b.resolution == (21, 31, 41) and b.tsdf.shape == (41, 31, 21) and b.weight.shape == (41, 31, 21)
    c = TSDFVolume((0, 0, 0), voxel_size=(0.1, 0.2, 0.3), resolution=(4, 5, 6))
    assert c.tsdf.shape == (6, 5, 4) and c.tsdf.dtype == torch.float32 and float(c.tsdf.abs().max()) == 0 and float(c.weight.max()) == 0
    assert np.allclose(c.hi, (0.3, 0.8, 1.5))
    for kw in ({}, {"hi": (1, 1, 1)}, {"hi": (1, 1, 1), "voxel_size": 0.1, "resolution": 11}, {"voxel_size": 0.1, "resolution": 1},
               {"voxel_size": -0.1, "resolution": 4}, {"hi": (-2, 1, 1), "resolution": 4}, {"voxel_size": 1.0, "resolution": 700}):
        with pytest.raises(ValueError):
            TSDFVolume((-1, -1, -1), **kw)


def test_three_calls_equal_one_call_bit_for_bit():
    depth, R, T, focal, pp = mc.three_views()
    trunc = 2 * mc.GRID_H
    one = small_volume().integrate(depth[:3], mc.Cams(R[:3], T[:3], focal[:3], pp[:3]), trunc)
    three = small_volume()
    for b in range(3):
        three.integrate(depth[b:b + 1], mc.Cams(R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1]), trunc)
    assert torch.equal(one.tsdf, three.tsdf) and torch.equal(one.weight, three.weight)
    assert float(one.weight.max()) == 3 and float(one.tsdf.max()) == 1 and float(one.tsdf.min()) >= -1
    # the order of the views is part of the rule: the running average is not symmetric in fp32, but the weights are
    rev = small_volume().integrate(depth[:3].flip(0), mc.Cams(R[:3].flip(0), T[:3].flip(0), focal[:3], pp[:3]), trunc)
    assert torch.equal(rev.weight, one.weight) and torch.allclose(rev.tsdf, one.tsdf, atol=2e-6, rtol=0)
    # a mismatch of B raises
    with pytest.raises(ValueError):
        small_volume().integrate(depth[:3], mc.Cams(R[:2], T[:2], focal[:2], pp[:2]), trunc)
    with pytest.raises(ValueError):
        small_volume().integrate(depth[:3], mc.Cams(R[:3], T[:3], focal[:3], pp[:3]), 0.0)


def test_max_weight_caps_the_weight():
    depth, R, T, focal, pp = mc.sphere_views()
    cams = mc.Cams(R, T, focal, pp)
    free = small_volume().integrate(depth, cams, 2 * mc.GRID_H)
    capped = small_volume().integrate(depth, cams, 2 * mc.GRID_H, max_weight=2)
    assert float(free.weight.max()) > 2
    assert torch.equal(capped.weight, free.weight.clamp(max=2))
    assert not torch.equal(capped.tsdf, free.tsdf)      # a capped weight lets the later views count for more


def one_view(depth_value=3.0, size=8):
    """A camera at (0, 0, -3) that looks along +z with an 8 x 8 image of constant depth"""
    R = torch.eye(3)[None]
    T = torch.tensor([[0.0, 0.0, 3.0]])
    return torch.full((1, size, size), depth_value), mc.Cams(R, T, torch.tensor([[8.0, 8.0]]), torch.tensor([[size / 2, size / 2]]))


def integrate_points(points, depth, cams, trunc=0.5):
    """tsdf / weight of single grid points: a 2 x 2 x 2 volume whose low corner is the point (the other corners are far off)"""
    out = []
    for p in points:
        vol = TSDFVolume(p, voxel_size=100.0, resolution=2).integrate(depth, cams, trunc)
        out.append((float(vol.tsdf[0, 0, 0]), float(vol.weight[0, 0, 0])))
    return out


def test_a_view_is_skipped_where_the_rule_says():
    depth, cams = one_view()
    (t_in, w_in), (t_front, w_front) = integrate_points([(0.1, 0.1, 0.0), (0.1, 0.1, -1.0)], depth, cams)
    assert w_in == 1 and abs(t_in - (3.0 - np.linalg.norm([0.1, 0.1, 3.0])) / 0.5) < 1e-5      # updated: sdf / trunc
    assert w_front == 1 and t_front == 1.0                                                       # far in front: clamped to 1
    skipped = {"behind the camera": (0.1, 0.1, -4.0), "outside the image": (2.5, 0.1, 0.0), "sdf < -trunc": (0.1, 0.1, 0.6)}
    for name, p in skipped.items():
        (t, w), = integrate_points([p], depth, cams)
        assert (t, w) == (0.0, 0.0), name
    for bad in (float("inf"), float("nan"), 0.0, -1.0):      # an invalid depth
        (t, w), = integrate_points([(0.1, 0.1, 0.0)], *one_view(bad))
        assert (t, w) == (0.0, 0.0), bad
    # the pixel is the one the ray convention names: pixel (i, j) looks along ((px - j - 0.5) / fx, (py - i - 0.5) / fy, 1)
    depth, cams = one_view()
    depth[0, 1, 6] = float("nan")      # i = 1, j = 6: x_view / z = (4 - 6.5) / 8, y_view / z = (4 - 1.5) / 8
    (t, w), = integrate_points([(3.0 * (4 - 6.5) / 8, 3.0 * (4 - 1.5) / 8, 0.0)], depth, cams)
    assert (t, w) == (0.0, 0.0)
    (t, w), = integrate_points([(3.0 * (4 - 5.5) / 8, 3.0 * (4 - 1.5) / 8, 0.0)], depth, cams)
    assert w == 1


def test_depth_is_ray_distance_as_the_ray_kernel_defines_it():
    """The fused pixel and distance agree with oracle.camera_np.pixel_rays: a point at distance d along the ray of pixel (i, j)
    projects into that pixel and has sdf = depth - d."""
    from oracle import camera_np
    depth, R, T, focal, pp = mc.sphere_views()
    b, i, j, d = 9, 40, 57, 2.5
    rays, cen = camera_np.pixel_rays(R.numpy(), T.numpy(), focal.numpy(), pp.numpy(), (mc.IMAGE, mc.IMAGE))
    p = cen[b] + d * rays[b, i, j].astype(np.float64)
    dm = torch.full((1, mc.IMAGE, mc.IMAGE), float("nan"))
    dm[0, i, j] = 2.75
    vol = TSDFVolume(p.tolist(), voxel_size=100.0, resolution=2)
    vol.integrate(dm, mc.Cams(R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1]), 1.0)
    assert float(vol.weight[0, 0, 0]) == 1 and abs(float(vol.tsdf[0, 0, 0]) - 0.25) < 1e-5


def test_end_to_end_on_the_definition():
    depth, R, T, focal, pp = mc.sphere_views()
    assert depth.shape == (14, mc.IMAGE, mc.IMAGE)
    vol = small_volume().integrate(depth, mc.Cams(R, T, focal, pp), 2 * mc.GRID_H)
    verts, faces = extract_mesh(vol)
    mc.assert_closed(verts, faces, chi=2)
    err = mc.radial_error(verts)
    print(f"[meshing] end to end on the definition: V {len(verts)}, F {len(faces)}, radial error {err / mc.GRID_H:.3f} h")
    assert err <= 1.0 * mc.GRID_H
    normal, centroid = mc.face_normals(verts, faces)
    assert ((normal * centroid).sum(-1) > 0).all()


def test_definition_marks_the_close_calls():
    depth, R, T, focal, pp = mc.three_views()
    tsdf, weight, marked = mc.definition_fp64(depth, R, T, focal, pp, 2 * mc.GRID_H, mark=(2.0 ** -10, 2.0 ** -18))
    plain = mc.definition_fp64(depth, R, T, focal, pp, 2 * mc.GRID_H)
    assert torch.equal(plain[0], tsdf) and torch.equal(plain[1], weight)
    assert marked.dtype == torch.bool and 0 < float(marked.double().mean()) <= 0.02


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_new_entries_validate_before_any_hip_call():
    import os
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    P = 1234     # (a non-NULL pointer value: nothing is dereferenced before validation is through)
    grid = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    cams = (P, P, P, P, P)
    ok = (P, P, 8, 8, 8) + grid + (P, 1, 4, 4) + cams
    assert lib.voge_tsdf_integrate(None, P, 8, 8, 8, *grid, P, 1, 4, 4, *cams, 0.1, 0.0, None) == -1
    assert lib.voge_tsdf_integrate(P, P, 8, 1, 8, *grid, P, 1, 4, 4, *cams, 0.1, 0.0, None) == -1
    assert lib.voge_tsdf_integrate(*ok, 0.0, 0.0, None) == -1                  # trunc > 0
    assert lib.voge_tsdf_integrate(*ok, float("nan"), 0.0, None) == -1
    assert lib.voge_tsdf_integrate(P, P, 8, 8, 8, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, P, 1, 4, 4, *cams, 0.1, 0.0, None) == -1
    assert lib.voge_tsdf_integrate(P, P, 8, 8, 8, *grid, None, 1, 4, 4, *cams, 0.1, 0.0, None) == -1
    assert lib.voge_tsdf_integrate(P, P, 8, 8, 8, *grid, P, 1, 0, 4, *cams, 0.1, 0.0, None) == -1
    assert lib.voge_tsdf_integrate(P, P, 700, 700, 700, *grid, P, 1, 4, 4, *cams, 0.1, 0.0, None) == -3      # the 32-bit limit
    assert lib.voge_tsdf_integrate(P, P, 8, 8, 8, *grid, None, 0, 4, 4, None, None, None, None, None, 0.1, 0.0, None) == 0      # no view: nothing launched
    tabs = (P, P, P, P, P, P)
    assert lib.voge_mtet_count(None, None, 8, 8, 8, 0.0, *tabs, None) == -1
    assert lib.voge_mtet_count(P, None, 8, 8, 1, 0.0, *tabs, None) == -1
    assert lib.voge_mtet_count(P, None, 8, 8, 8, float("nan"), *tabs, None) == -1
    assert lib.voge_mtet_count(P, None, 8, 8, 8, 0.0, P, P, P, None, P, P, None) == -1
    assert lib.voge_mtet_count(P, None, 675, 675, 675, 0.0, *tabs, None) == -3      # 675^3 7 >= 2^31 > 674^3 7
    assert lib.voge_mtet_count(P, None, 65536, 65536, 2, 0.0, *tabs, None) == -3
    assert lib.voge_mtet_scan(P, P, 0, P, None) == -1
    assert lib.voge_mtet_scan(P, None, 4, P, None) == -1
    assert lib.voge_mtet_scan(P, P, 1 << 40, P, None) == -3
    assert lib.voge_mtet_emit(P, None, 8, 8, 8, 0.0, *grid, *tabs, 10, 10, None, P, None) == -1
    assert lib.voge_mtet_emit(P, None, 8, 8, 8, 0.0, *grid, *tabs, -1, 10, P, P, None) == -1
    assert lib.voge_mtet_emit(P, None, 8, 8, 8, 0.0, 0.0, 0.0, 0.0, 1.0, -1.0, 1.0, *tabs, 10, 10, P, P, None) == -1
    assert lib.voge_mtet_emit(P, None, 8, 8, 8, 0.0, *grid, *tabs, 1 << 31, 10, P, P, None) == -3
    assert lib.voge_mtet_emit(P, None, 700, 700, 700, 0.0, *grid, *tabs, 10, 10, P, P, None) == -3
    assert lib.voge_mtet_emit(P, None, 8, 8, 8, 0.0, *grid, *tabs, 0, 0, None, None, None) == 0      # an empty mesh: nothing launched


def test_device_routes_refuse_host_tensors():
    from voge_amd import _lib, ops
    with pytest.raises(_lib.VogeHipError):
        ops.marching_tets(torch.zeros(4, 4, 4), None, 0.0, (0, 0, 0), (1, 1, 1))
    z = torch.zeros(4, 4, 4)
    with pytest.raises(_lib.VogeHipError):
        ops.tsdf_integrate(z, z.clone(), torch.ones(1, 4, 4), torch.eye(3)[None], torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 2),
                           torch.ones(1, 2), (0, 0, 0), (1, 1, 1), 0.1)
