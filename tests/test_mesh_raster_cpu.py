"""CPU tests of mesh depth maps: Aggregation.mesh_rasterize, the definition, against an independent fp64 restatement, against
itself in fp32 off the marks of its step 7, and on the properties the rule promises (no crack in a closed mesh, culling, the closed
form of the gradient); Meshing.rasterize_mesh's argument checks and interpolate_vertex_attr; the workspace layout.  No GPU."""
import os

import numpy as np
import pytest
import torch

import mesh_raster_cases as rc
import meshing_cases as mc
import sample_meshes
from voge_amd import Aggregation
from voge_amd.Meshing import MeshFragments, TSDFVolume, extract_mesh, interpolate_vertex_attr, rasterize_mesh

CASES = rc.main_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def definitions():
    """name -> (fp64 outputs with marks, fp32 outputs with marks): computed once, shared, left unchanged"""
    out = {}
    for c in CASES:
        out[c.name] = (Aggregation.mesh_rasterize(c.verts.double(), c.faces, *c.args(torch.float64), mark=rc.MARK),
                       Aggregation.mesh_rasterize(c.verts, c.faces, *c.args(), mark=rc.MARK))
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_cases_cover_half_of_every_image(case, definitions):
    pix = definitions[case.name][0][0]
    assert pix.shape == (len(case.R), case.H, case.W) and (case.H % 16 or case.W % 16 or (case.H, case.W) == (40, 48))
    assert ((pix >= 0).float().mean(dim=(1, 2)) >= 0.5).all()
    assert bool((case.focal != case.focal.round()).all()) and bool((case.pp != case.pp.round()).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_definition_equals_the_numpy_restatement(case, definitions):
    pix, bary, depth, _ = definitions[case.name][0]
    pn, bn, dn = rc.rasterize_numpy(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W)
    assert (torch.from_numpy(pn) == pix).all()
    assert np.abs(dn - depth.numpy()).max() <= 1e-12 and np.abs(bn - bary.numpy()).max() <= 1e-11
    assert (depth[pix < 0] == 0).all() and (bary[pix < 0] == 0).all() and (depth[pix >= 0] > 0).all()
    assert ((bary[pix >= 0].sum(-1) - 1).abs() <= 1e-12).all() and (bary >= 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_equals_fp64_off_the_marks_and_the_marks_stay_under_their_cap(case, definitions):
    (p64, b64, d64, m64), (p32, b32, d32, m32) = definitions[case.name]
    for m in (m64, m32):
        share = float(m.float().mean())
        print(f"[mesh raster] {case.name}: {share * 100:.2f} % of the pixels marked")
        assert share <= rc.MARK_CAP
    clear = ~m64
    assert (p32[clear] == p64[clear]).all()
    e_b, e_d = rc.forward_bounds(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, p64)
    ok = clear & (p64 >= 0)
    assert ((d32.double() - d64).abs()[ok] <= e_d[ok]).all()
    assert ((b32.double() - b64).abs().max(-1).values[ok] <= e_b[ok]).all()


def test_a_closed_sphere_has_no_crack():
    """Every pixel whose ray meets the sphere inscribed in the level-2 icosphere is hit, in fp32 and in fp64"""
    case = CASES[1]
    v, f = case.verts.double(), case.faces
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.linalg.cross(b - a, c - a)
    r_in = float(((a * n).sum(-1) / n.norm(dim=-1)).min())
    assert 0.9 < r_in < 1.0
    R, T, focal, pp, H, W = case.args(torch.float64)
    cen = -torch.einsum("bk,bjk->bj", T, R)                                          # c = -T R^T (R orthonormal)
    d0 = (pp[:, 0:1] - (torch.arange(W).double() + 0.5)) / focal[:, 0:1]
    d1 = (pp[:, 1:2] - (torch.arange(H).double() + 0.5)) / focal[:, 1:2]
    d = torch.stack((d0[:, None, :].expand(-1, H, W), d1[:, :, None].expand(-1, H, W), torch.ones(len(R), H, W, dtype=torch.float64)), -1)
    ray = torch.einsum("bhwk,bjk->bhwj", d / d.norm(dim=-1, keepdim=True), R)
    bq = (ray * cen[:, None, None]).sum(-1)
    inside = bq * bq - ((cen * cen).sum(-1)[:, None, None] - r_in ** 2) > 0
    assert inside.float().mean() > 0.5
    for dt in (torch.float32, torch.float64):
        pix = Aggregation.mesh_rasterize(case.verts.to(dt), case.faces, *case.args(dt))[0]
        assert (pix[inside] >= 0).all()


def test_culling_keeps_an_outward_sphere_and_empties_a_reversed_sheet():
    case = CASES[0]
    plain = Aggregation.mesh_rasterize(case.verts, case.faces, *case.args())
    culled = Aggregation.mesh_rasterize(case.verts, case.faces, *case.args(), cull_backfaces=True)
    for x, y in zip(plain, culled):
        assert torch.equal(x, y)
    both = Aggregation.mesh_rasterize(case.verts, case.faces.flip(1), *case.args())
    assert torch.equal(both[0], plain[0]) and (both[2] - plain[2]).abs().max() <= 1e-5      # (another order of the same roundings)
    # reversed, every face the plain image shows is culled.  A CLOSED mesh does not go empty: a ray that leaves it meets the far
    # side, whose reversed faces now look at the camera -- what is left lies strictly behind what the plain image shows
    rev = Aggregation.mesh_rasterize(case.verts, case.faces.flip(1), *case.args(), cull_backfaces=True)
    for b in range(len(case.R)):
        seen = torch.zeros(len(case.faces), dtype=torch.bool)
        seen[plain[0][b][plain[0][b] >= 0]] = True
        assert (rev[0][b] >= 0).any() and not seen[rev[0][b][rev[0][b] >= 0]].any()
    assert ((rev[0] >= 0) <= (plain[0] >= 0)).all() and (rev[2] > plain[2])[rev[0] >= 0].all()
    # an OPEN sheet does go empty: the grid from its front (view 0) and from its back (view 1)
    sheet = CASES[2]
    assert sheet.T[0, 2] > 0 and float((sheet.R[0] @ torch.tensor([0.0, 0.0, 1.0]))[2]) < 0      # (view 0 looks down the sheet's normals)
    sv, sf = sample_meshes.grid_mesh(23, 13)      # (without the jitter, which tips a face at the border over)
    sv = sv - torch.tensor([0.5, 0.5, 0.0])
    plain = Aggregation.mesh_rasterize(sv, sf, *sheet.args())
    culled = Aggregation.mesh_rasterize(sv, sf, *sheet.args(), cull_backfaces=True)
    rev = Aggregation.mesh_rasterize(sv, sf.flip(1), *sheet.args(), cull_backfaces=True)
    assert ((plain[0] >= 0).float().mean(dim=(1, 2)) > 0.5).all()
    assert torch.equal(culled[0][0], plain[0][0]) and (culled[0][1] == -1).all() and (culled[2][1] == 0).all()
    assert (rev[0][0] == -1).all() and (rev[2][0] == 0).all() and torch.equal(rev[0][1], plain[0][1]) and (rev[2][1] - plain[2][1]).abs().max() <= 1e-5


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_autograd_of_the_definition_equals_the_closed_form(case):
    vd = case.verts.double().requires_grad_(True)
    pix, bary, depth = Aggregation.mesh_rasterize(vd, case.faces, *case.args(torch.float64))
    g = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(depth.shape)))
    got, = torch.autograd.grad((depth * g).sum(), vd)
    ref, _ = rc.closed_form_grad(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, pix, g)
    assert float(ref.abs().max()) > 1 and (got - ref).abs().max() <= 1e-10 * float(ref.abs().max())


def test_ties_keep_the_lower_index_and_a_nan_corner_hits_nothing():
    v = torch.tensor([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0], [float("nan"), 0.0, 1.0]])
    f = torch.tensor([[0, 1, 3], [0, 1, 2], [0, 1, 2], [1, 0, 2]])
    R, T = torch.eye(3)[None], torch.zeros(1, 3)
    focal, pp = torch.tensor([[8.0, 8.0]]), torch.tensor([[8.0, 8.0]])
    pix, bary, depth = Aggregation.mesh_rasterize(v, f, R, T, focal, pp, 16, 16)
    assert set(pix.unique().tolist()) == {-1, 1}
    assert (Aggregation.mesh_rasterize(v, f[[0, 3, 2, 1]], R, T, focal, pp, 16, 16)[0].unique() == torch.tensor([-1, 1])).all()


def test_rasterize_mesh_on_the_host_and_its_argument_errors():
    case = CASES[4]
    frags = rasterize_mesh(case.verts, case.faces, case.cameras(), (case.H, case.W))
    ref = Aggregation.mesh_rasterize(case.verts, case.faces, *case.args())
    assert isinstance(frags, MeshFragments) and frags.pix_to_face.dtype == torch.int32
    assert torch.equal(frags.pix_to_face.long(), ref[0]) and torch.equal(frags.bary, ref[1]) and torch.equal(frags.depth, ref[2])
    one = mc.Cams(case.R[:1], case.T, case.focal[0], case.pp[:1])      # one rotation, one focal length and one centre for all the views
    assert rasterize_mesh(case.verts, case.faces, one, (case.H, case.W)).depth.shape == (len(case.T), case.H, case.W)
    empty = rasterize_mesh(case.verts, case.faces[:0], case.cameras(), (5, 7))
    assert (empty.pix_to_face == -1).all() and empty.bary.shape == (len(case.R), 5, 7, 3) and (empty.depth == 0).all()
    none = rasterize_mesh(case.verts, case.faces, mc.Cams(case.R[:0], case.T[:0], case.focal[:0], case.pp[:0]), (5, 7))
    assert none.pix_to_face.shape == (0, 5, 7) and none.bary.shape == (0, 5, 7, 3) and none.depth.shape == (0, 5, 7)
    bad = [dict(verts=case.verts[:, :2]), dict(faces=case.faces.float()), dict(faces=case.faces[:, :2]), dict(image_size=(0, 5)),
           dict(image_size=7), dict(route="grid"), dict(cameras=mc.Cams(case.R, case.T[:1].expand(3, 3), case.focal, case.pp)),
           dict(cameras=mc.Cams(case.R, case.T, case.focal[:1].expand(3, 2), case.pp)), dict(faces=case.faces + 2)]
    for change in bad:
        kw = dict(verts=case.verts, faces=case.faces, cameras=case.cameras(), image_size=(case.H, case.W))
        kw.update(change)
        with pytest.raises(ValueError):
            rasterize_mesh(**kw)


def test_interpolate_vertex_attr():
    case = CASES[2]
    frags = rasterize_mesh(case.verts, case.faces, case.cameras(), (case.H, case.W))
    attr = torch.from_numpy(np.random.default_rng(2).standard_normal((len(case.verts), 4))).float().requires_grad_(True)
    bg = torch.tensor([0.5, -1.0, 2.0, 0.0])
    image = interpolate_vertex_attr(frags, case.faces, attr, background=bg)
    assert image.shape == (len(case.R), case.H, case.W, 4)
    covered = frags.pix_to_face >= 0
    assert (image[~covered] == bg).all()
    tri = case.faces[frags.pix_to_face.long().clamp(min=0)]
    ref = sum(attr.detach()[tri[..., i]] * frags.bary[..., i:i + 1] for i in range(3))
    assert (image.detach() - ref).abs()[covered].max() <= 4 * rc.U * float(attr.detach().abs().max())
    g, = torch.autograd.grad(image.sum(), attr)
    count = torch.zeros(len(case.verts)).index_add_(0, tri[covered].reshape(-1), frags.bary[covered].reshape(-1))
    assert (g - count[:, None]).abs().max() <= 1e-4 * float(count.max())
    assert (interpolate_vertex_attr(frags, case.faces, attr)[~covered] == 0).all()
    with pytest.raises(ValueError):
        interpolate_vertex_attr(frags, case.faces.float(), attr)
    with pytest.raises(ValueError):
        interpolate_vertex_attr(frags, case.faces, attr[:, 0])


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_workspace_bytes_equal_the_layout_restated(lib):
    BIG = 2 ** 28 - 1
    for n in (1, 255, 256, 257, 4095, 4096, 4097, BIG):
        for B, H, W in ((1, 29, 37), (3, 40, 48), (8, 512, 512)):
            for V, F in ((n, 4097), (4097, n), (n, n)):
                if B * max(V, F) > 2 ** 36:
                    continue
                assert lib.voge_mesh_raster_workspace_bytes(B, V, F, H, W) == rc.workspace_bytes(B, V, F, H, W), (B, V, F, H, W)
    assert lib.voge_mesh_raster_workspace_bytes(1, BIG, BIG, 16, 16) == rc.workspace_bytes(1, BIG, BIG, 16, 16) > 2 ** 34
    for bad in ((0, 10, 10, 16, 16), (1, BIG + 1, 10, 16, 16), (1, 10, BIG + 1, 16, 16), (1, 10, 10, 0, 16), (2, 10, 10, 2 ** 15, 2 ** 15),
                (-1, 10, 10, 16, 16), (1, -1, 10, 16, 16), (512, 10, BIG, 16, 16)):
        assert lib.voge_mesh_raster_workspace_bytes(*bad) == 0, bad


def test_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-null, aligned pointer value: nothing is dereferenced before validation is through)
    ok = (P, 10, P, 10, P, P, P, P, 1, 16, 16, 0)
    big = 1 << 30
    assert lib.voge_mesh_raster_fwd(*ok, 16, None, 0, P, P, P, None, P, big, None) == -1              # stages outside 1 .. 15
    assert lib.voge_mesh_raster_fwd(*ok, 9, None, 0, None, P, P, None, P, big, None) == -1            # the raster without an output
    assert lib.voge_mesh_raster_fwd(*ok, 3, None, 0, P, P, P, None, P, big, None) == -1               # the tables without a total
    assert lib.voge_mesh_raster_fwd(*ok, 12, None, 5, P, P, P, None, P, big, None) == -1              # a list of 5 entries at null
    assert lib.voge_mesh_raster_fwd(*ok, 9, None, 0, P, P, P, None, P + 4, big, None) == -1           # a misaligned workspace
    assert lib.voge_mesh_raster_fwd(*ok, 9, None, 0, P, P, P, None, P, 100, None) == -2               # a workspace too small
    assert lib.voge_mesh_raster_bwd(P, 10, P, 10, P, P, P, P, 1, 16, 16, P, P, None, P, big, None) == -1
    assert lib.voge_mesh_raster_bwd(P, 10, P, 10, P, P, P, P, 1, 16, 16, P, P, P, P, 100, None) == -2


def test_a_mesh_fused_from_its_own_depth_maps_is_closed():
    """The icosphere at r = 0.6 rasterised under the 14 sphere views of tests/meshing_cases.py (80 x 96 images), fused by integrate
    and extracted: a closed surface with chi = 2 -- rasterize_mesh's depth goes into integrate unchanged"""
    _, R, T, focal, pp = mc.sphere_views()
    v, f = sample_meshes.level2_sphere()
    frags = rasterize_mesh(v * mc.SPHERE_R, f, mc.Cams(R, T, focal, pp), (80, mc.IMAGE))
    assert ((frags.pix_to_face >= 0).float().mean(dim=(1, 2)) > 0.3).all()
    vol = TSDFVolume((mc.GRID_LO,) * 3, voxel_size=mc.GRID_H, resolution=mc.GRID_N).integrate(frags.depth, mc.Cams(R, T, focal, pp), 2 * mc.GRID_H)
    verts, faces = extract_mesh(vol)
    mc.assert_closed(verts, faces, chi=2)
    assert mc.radial_error(verts) <= 1.0 * mc.GRID_H
