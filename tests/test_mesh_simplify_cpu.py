"""Mesh simplification on the host: Aggregation.mesh_simplify, the definition, and Meshing.simplify_mesh against the independent
numpy restatement of tests/mesh_simplify_cases.py, and the properties the rule promises (closed meshes stay closed on the sphere
and the box, quadric placement keeps corners, duplicates and orientation, the index tables, the errors)."""
import numpy as np
import pytest
import torch

import mesh_simplify_cases as sc
import meshing_cases as mc
from voge_amd import Aggregation
from voge_amd.Meshing import simplify_mesh

PLACEMENTS = ("mean", "quadric")


def check_against_restatement(label, verts, faces, h, placement, attr=None):
    """Integers equal; positions and attributes within the bounds without the fixed-point quanta -> the definition's outputs"""
    ref = sc.restate(verts.numpy(), faces.numpy(), h, placement, None if attr is None else attr.numpy())
    got = Aggregation.mesh_simplify(verts, faces, h, placement, attr)
    v, f, a, vi, fi = got
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and vi.dtype == torch.int64 and fi.dtype == torch.int64
    assert np.array_equal(f.numpy(), ref["faces"]) and np.array_equal(vi.numpy(), ref["vert_index"]) and np.array_equal(fi.numpy(), ref["face_index"])
    assert v.shape == ref["verts"].shape
    bound = sc.position_bound(ref["verts"], ref["count"], ref["corners"], verts.numpy(), len(faces), h, placement, fixed_point=False)
    s, err = sc.share(v.numpy(), ref["verts"], bound)
    print(f"[parity] mesh_simplify definition, {label}, {placement}: V {len(verts)} -> {len(v)}, F {len(faces)} -> {len(f)}, "
          f"max error {err:.3e}, {s:.3f} of the bound")
    assert s <= 1.0
    if attr is not None:
        ab = sc.attr_bound(ref["attr"], ref["count"], attr.numpy(), len(verts), fixed_point=False)
        s, err = sc.share(a.numpy(), ref["attr"], ab)
        assert s <= 1.0, (s, err)
    return got


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_definition_matches_the_restatement(placement):
    for name, v, f, h in sc.extraction_cells() + [c for c in sc.other_cases() if len(c[1]) < 5000]:
        check_against_restatement(name, v, f, h, placement, sc.attr_of(v, 3))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_identity(placement):
    """A cell of 0.01 voxel returns the input bit for bit"""
    v, f, h = sc.sphere24()
    a = sc.attr_of(v, 3)
    v2, f2, a2, vi, fi = simplify_mesh(v, f.int(), 0.01 * h, placement, attr=a, return_index=True)
    assert torch.equal(v2, v) and torch.equal(f2, f.int()) and torch.equal(a2, a)
    assert torch.equal(vi, torch.arange(len(v), dtype=torch.int32)) and torch.equal(fi, torch.arange(len(f), dtype=torch.int32))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_empty(placement):
    """A cell larger than the mesh returns [0,3] tensors and [0,C]"""
    v, f, h = sc.sphere24()
    v2, f2, a2, vi, fi = simplify_mesh(v, f, 100.0, placement, attr=sc.attr_of(v, 5), return_index=True)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and a2.shape == (0, 5) and fi.shape == (0,)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and (vi == -1).all() and vi.shape == (len(v),)
    z = torch.zeros((0, 3))
    v2, f2 = simplify_mesh(z, z.long(), 1.0, placement)
    assert v2.shape == (0, 3) and f2.shape == (0, 3)
    v2, f2 = simplify_mesh(v, z.long(), 0.01, placement)      # no face names a vertex: no output vertices
    assert v2.shape == (0, 3) and f2.shape == (0, 3)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("cells,sizes", [(1, (755, 1506)), (2, (188, 372)), (3, (86, 168))])
def test_closed_sphere(cells, sizes, placement):
    v, f, h = sc.sphere24()
    assert (len(v), len(f)) == (2702, 5400)
    v2, f2 = simplify_mesh(v, f, cells * h, placement)
    assert (len(v2), len(f2)) == sizes
    mc.assert_closed(v2, f2, chi=2)
    err = mc.radial_error(v2) / h
    print(f"[mesh_simplify] sphere, {cells} voxels, {placement}: radial error {err:.3f} voxel")
    assert err <= 0.16


@pytest.mark.parametrize("cells", [2, 3, 4])
def test_box_corners(cells):
    v, f, h = sc.box33()
    worst = {}
    for placement in PLACEMENTS:
        v2, f2 = simplify_mesh(v, f, cells * h, placement)
        mc.assert_closed(v2, f2, chi=2)
        worst[placement] = sc.worst_corner_distance(v2) / h
    print(f"[mesh_simplify] box, {cells} voxels: worst corner distance {worst['quadric']:.2f} voxel (quadric) against {worst['mean']:.2f} (mean)")
    assert worst["quadric"] <= 0.5 * worst["mean"]


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_duplicates_and_orientation(placement):
    v, f = sc.small_soup()
    v2, f2, vi, fi = simplify_mesh(v, f, 1.0, placement, return_index=True)
    # 0 stays, its rotated repeat 1 goes; 2, the opposite orientation, stays; 3 names a vertex twice; 4 stays, its repeat 5 goes
    assert fi.tolist() == [0, 2, 4]
    assert f2.tolist() == [[0, 1, 2], [2, 1, 0], [3, 4, 5]]
    assert vi.tolist() == [0, 1, 2, -1, -1, 3, 4, 5]
    assert torch.equal(v2, v[[0, 1, 2, 5, 6, 7]])      # clusters of one vertex keep their bits
    # two vertices in one cell: the face between them and a third collapses
    v3 = torch.cat([v, v[:1] + 0.125])
    f3 = torch.cat([f, torch.tensor([[0, 8, 1]])])
    _, _, vi3, fi3 = simplify_mesh(v3, f3, 1.0, placement, return_index=True)
    assert fi3.tolist() == [0, 2, 4] and vi3[8] == vi3[0] == 0


def test_errors():
    v, f = sc.small_soup()
    bad = f.clone()
    bad[2, 1] = 8
    nan = v.clone()
    nan[3, 1] = float("nan")
    for fn in (simplify_mesh, Aggregation.mesh_simplify):
        with pytest.raises(ValueError):
            fn(v, bad, 1.0)
        with pytest.raises(ValueError):
            fn(v, -bad, 1.0)
        with pytest.raises(ValueError):
            fn(nan, f, 1.0)
        for h in (0.0, -1.0, float("inf"), float("nan"), (1.0, 0.0, 1.0)):
            with pytest.raises(ValueError):
                fn(v, f, h)
        with pytest.raises(ValueError):
            fn(v, f, 1.0, placement="median")
        with pytest.raises(ValueError):
            fn(v, f, 1.0, attr=torch.zeros(7, 3))
        with pytest.raises(ValueError):
            fn(v, f, 1e-7)      # more than 2^21 - 1 cells on an axis
    with pytest.raises(ValueError):
        simplify_mesh(v, f, 1.0, attr=torch.zeros(8))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_index_tables(placement):
    """vert_index and face_index reproduce the outputs; for "mean", verts' and attr' are the means grouped by vert_index"""
    v, f, h = sc.sphere24()
    a = sc.attr_of(v, 11)
    v2, f2, a2, vi, fi = simplify_mesh(v, f, 2 * h, placement, attr=a, return_index=True)
    vi, fi = vi.long(), fi.long()
    assert torch.equal(f2.long(), vi[f[fi]])
    assert sorted(set(vi[vi >= 0].tolist())) == list(range(len(v2)))
    on = vi >= 0
    n = torch.bincount(vi[on], minlength=len(v2)).double()[:, None]
    mean = lambda x: (torch.zeros((len(v2), x.shape[1]), dtype=torch.float64).index_add(0, vi[on], x.double()[on]) / n).float()
    assert torch.allclose(a2, mean(a), rtol=2e-7, atol=0)
    if placement == "mean":
        assert torch.allclose(v2, mean(v), rtol=2e-7, atol=0)
    # a dropped cluster: its vertices map to -1 and nothing else does
    dropped = ~on
    lab = torch.from_numpy(sc.restate(v.numpy(), f.numpy(), 2 * h)["label"])
    assert not set(lab[dropped].tolist()) & set(lab[on].tolist())


def test_exported():
    import VoGE.Meshing
    assert VoGE.Meshing.simplify_mesh is simplify_mesh and "simplify_mesh" in VoGE.Meshing.__all__
    from voge_amd import _lib
    for name in ("voge_mesh_simplify_scan", "voge_mesh_simplify_emit", "voge_mesh_simplify_attr", "voge_mesh_simplify_workspace_bytes"):
        assert name in _lib.SIGNATURES
