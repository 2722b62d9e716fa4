"""CPU tests of the point-to-mesh distance: the torch definitions (Aggregation.point_triangle_closest / point_mesh_term) against
literal values and the fp64 reference of tests/point_mesh_cases.py, the public functions of Losses on host tensors, and the
argument checks of the four C entries (the library loads without a GPU: anything that reached HIP would fail differently)."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import point_mesh_cases as cases
from voge_amd import Aggregation, Losses, ops
from voge_amd.Losses import MeshTopology

A, B, C = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
# point, region, d2, weights on (a, b, c) where they are unique and worth stating
TABLE = (((0.25, 0.25, 0.5), "interior", 0.25, (0.5, 0.25, 0.25)),
         ((0.2, 0.2, 0.0), "on the plane, inside", 0.0, None),
         ((-1.0, -1.0, 0.0), "vertex a", 2.0, None),
         ((2.0, -1.0, 0.0), "vertex b", 2.0, None),
         ((-1.0, 2.0, 0.0), "vertex c", 2.0, None),
         ((0.5, -1.0, 0.0), "edge ab", 1.0, (0.5, 0.5, 0.0)),
         ((1.0, 1.0, 0.0), "edge bc", 0.5, None),
         ((-1.0, 0.5, 0.0), "edge ca", 1.0, None))
REGION_POINT = {"vertex a": A, "vertex b": B, "vertex c": C, "edge ab": (0.5, 0.0, 0.0), "edge bc": (0.5, 0.5, 0.0),
                "edge ca": (0.0, 0.5, 0.0), "interior": (0.25, 0.25, 0.0), "on the plane, inside": (0.2, 0.2, 0.0)}


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _table(dtype=torch.float64):
    pts = torch.tensor([row[0] for row in TABLE], dtype=dtype)
    tri = torch.tensor([A, B, C], dtype=dtype)
    want = torch.tensor([row[2] for row in TABLE], dtype=torch.float64)
    q = torch.tensor([REGION_POINT[row[1]] for row in TABLE], dtype=torch.float64)
    return pts, tri, want, q


def _rigid():
    """a rotation (about (1, 2, 3) by 0.7 rad) and a shift, fp64"""
    k = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(0.7) * K + (1 - math.cos(0.7)) * (K @ K)
    return R, torch.tensor([0.3, -1.1, 2.5], dtype=torch.float64)


# ---- point_triangle_closest -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("moved", [False, True])
def test_region_table_for_every_order_of_the_corners(moved):
    pts, tri, want, q = _table()
    if moved:
        R, t = _rigid()
        pts, tri, q = pts @ R.T + t, tri @ R.T + t, q @ R.T + t
    tol = 1e-13
    for perm in itertools.permutations(range(3)):
        a, b, c = (tri[k] for k in perm)
        d2, bary = Aggregation.point_triangle_closest(pts, a, b, c)
        assert d2.shape == (len(TABLE),) and bary.shape == (len(TABLE), 3)
        assert (d2 - want).abs().max() <= tol, (perm, d2)
        assert (bary >= 0).all() and (bary.sum(-1) - 1).abs().max() <= tol
        got_q = bary[:, 0:1] * a + bary[:, 1:2] * b + bary[:, 2:3] * c
        assert (got_q - q).abs().max() <= 1e-12, perm
        for row, w in zip(TABLE, bary):
            if row[3] is not None:      # the stated weights, carried to this order of the corners
                assert (w - torch.tensor([row[3][k] for k in perm], dtype=torch.float64)).abs().max() <= tol, (perm, row[1])
        ref_d2, ref_q = cases.closest64(pts, a, b, c)
        assert (ref_d2 - want).abs().max() <= tol and (ref_q - q).abs().max() <= 1e-12      # the tests' own reference agrees


def test_degenerate_triangles_are_segments_and_points():
    g = torch.Generator().manual_seed(1)
    pts = torch.randn(200, 3, generator=g, dtype=torch.float64) * 1.5
    a, b = torch.tensor([0.5, -0.25, 0.125], dtype=torch.float64), torch.tensor([-0.75, 1.0, 0.5], dtype=torch.float64)
    mid, beyond = a + 0.25 * (b - a), a + 2.0 * (b - a)
    one = torch.zeros(1, 3, dtype=torch.float64)
    seg = lambda s, t: cases.segment_d2_64(pts, s[None], t[None])[:, 0]      # noqa: E731
    for label, tri, want in (("collinear, c between", (a, b, mid), seg(a, b)), ("collinear, c beyond", (a, b, beyond), seg(a, beyond)),
                             ("collinear, a between", (mid, a, b), seg(a, b)), ("a = b", (a, a, b), seg(a, b)),
                             ("b = c", (a, b, b), seg(a, b)), ("a = c", (a, b, a), seg(a, b)),
                             ("a = b = c", (a, a, a), ((pts - a) ** 2).sum(-1))):
        for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-5)):
            d2, bary = Aggregation.point_triangle_closest(pts.to(dtype), *(t.to(dtype) for t in tri))
            assert torch.isfinite(d2).all() and torch.isfinite(bary).all(), label
            assert (d2.double() - want).abs().max() <= tol * (1 + want.max()), (label, dtype)
            assert (bary >= 0).all() and (bary.double().sum(-1) - 1).abs().max() <= (1e-13 if dtype == torch.float64 else 2.0 ** -22), label
            q = sum(bary[:, k:k + 1].double() * tri[k] for k in range(3))
            assert (((pts - q) ** 2).sum(-1) - want).abs().max() <= 10 * tol * (1 + want.max()), label      # the weights name that point
    d2, bary = Aggregation.point_triangle_closest(one, a, a, a)
    assert torch.equal(bary, torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64))
    # zeros everywhere: nothing is NaN
    z = torch.zeros(3)
    d2, bary = Aggregation.point_triangle_closest(z, z, z, z)
    assert float(d2) == 0.0 and torch.equal(bary, torch.tensor([1.0, 0.0, 0.0]))
    # an edge so short that 1 / (e.e) overflows: treated as a point, still finite
    tiny = torch.tensor([1e-30, 0.0, 0.0])
    d2, bary = Aggregation.point_triangle_closest(torch.tensor([0.0, 1.0, 0.0]), z, tiny, tiny * 2)
    assert torch.isfinite(d2) and torch.isfinite(bary).all() and abs(float(d2) - 1.0) <= 1e-6


def test_a_translated_table_keeps_its_bounds_in_fp32():
    pts, tri, want, _ = _table(torch.float32)
    shift = torch.tensor([1000.0, 1000.0, 1000.0])
    pts, tri = pts + shift, tri + shift                      # rounded to fp32 here: the inputs of both evaluations
    edge = math.sqrt(2.0)
    for perm in itertools.permutations(range(3)):
        a, b, c = (tri[k] for k in perm)
        d2, bary = Aggregation.point_triangle_closest(pts, a, b, c)
        ref = cases.closest64(pts, a, b, c)[0]
        bound = 4 * 2.0 ** -23 * (ref.sqrt() + edge) ** 2
        assert ((d2.double() - ref).abs() <= bound).all(), (perm, (d2.double() - ref).abs() / bound)
        assert (ref - want).abs().max() <= 1e-3              # (the moved inputs are the table's within their own rounding)


def test_a_sliver_loses_nothing():
    """A triangle of height 1e-7 of its base: the interior weights are poor, the minimum over the four candidates is not."""
    a, b, c = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.3, 1e-7, 0.0])
    pts = cases.points_around(torch.stack((a, b, c)), torch.tensor([[0, 1, 2]]), 500, 2)
    d2, bary = Aggregation.point_triangle_closest(pts, a, b, c)
    ref = cases.closest64(pts, a, b, c)[0]
    assert ((d2.double() - ref).abs() <= cases.d2_bound(cases.VALUE_C, ref, torch.tensor(1.0, dtype=torch.float64))).all()
    assert (bary >= 0).all() and (bary.sum(-1) - 1).abs().max() <= 2.0 ** -22


# ---- point_mesh_term --------------------------------------------------------------------------------------------------------------

def _small(seed=0, V=12, F=17, P=23):
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(V, 3, generator=g, dtype=torch.float64)
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)])
    return verts, faces, torch.randn(P, 3, generator=g, dtype=torch.float64) * 1.2


@pytest.mark.parametrize("chunk_pairs", [1 << 20, 17 * 5, 1])
def test_term_is_the_matrix_minimum_in_both_directions(monkeypatch, chunk_pairs):
    monkeypatch.setattr(Aggregation, "POINT_MESH_CHUNK_PAIRS", chunk_pairs)      # the whole matrix, chunks of 5 points, of one
    verts, faces, points = _small()
    M = cases.d2_matrix64(points, verts, faces)
    dp, df = M.min(1).values, M.min(0).values
    for red, single, want in (("mean", False, dp.mean() + df.mean()), ("sum", False, dp.sum() + df.sum()), ("mean", True, dp.mean()),
                              ("sum", True, dp.sum())):
        loss, fi, pi = Aggregation.point_mesh_term(verts, faces, points, single, red, return_indices=True)
        assert abs(float(loss) - float(want)) <= 1e-12 * float(want), (red, single)
        # (faces share edges and corners: near ties are the rule, so the chosen pair is judged by its distance, not its index)
        assert (M[torch.arange(len(points)), fi] - dp).abs().max() <= 1e-12
        assert (pi is None) if single else (M[pi, torch.arange(len(faces))] - df).abs().max() <= 1e-12
        assert float(Losses.point_mesh_face_distance(verts, faces, points, single, red)) == float(loss)
    many = torch.cat([points] * 3)
    whole = Aggregation.point_mesh_term(verts, faces, many, return_indices=True)
    assert (whole[2] < len(points)).all()      # the copies tie exactly: the first one is kept
    lone = torch.tensor([[0, 1, 2], [3, 4, 5], [0, 1, 2]])
    assert (Aggregation.point_mesh_term(verts, lone, points, return_indices=True)[1] != 2).all()      # and the first of two equal faces


def test_definitions_autograd_is_the_closed_form():
    verts, faces, points = _small(3)
    for red, single in (("mean", False), ("sum", False), ("mean", True)):
        v, p = verts.clone().requires_grad_(True), points.clone().requires_grad_(True)
        loss, fi, pi = Aggregation.point_mesh_term(v, faces, p, single, red, return_indices=True)
        (loss * -1.75).backward()
        tri = faces[fi]
        bary_p = Aggregation.point_triangle_closest(points, verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]])[1]
        bary_f = None if single else Aggregation.point_triangle_closest(points[pi], verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]])[1]
        g_v, g_p, _, _ = cases.closed_form_grads(verts, faces, points, fi, bary_p, pi, bary_f, -1.75, red)
        assert (v.grad - g_v).abs().max() <= 1e-12 * g_v.abs().max() and (p.grad - g_p).abs().max() <= 1e-12 * g_p.abs().max()
        assert v.grad.abs().max() > 0 and p.grad.abs().max() > 0
    # and the closed form is the derivative: central differences of the fp64 reference's own loss
    v0, p0 = verts.clone(), points.clone()
    f = lambda vv, pp: float(cases.d2_matrix64(pp, vv, faces).min(1).values.mean() + cases.d2_matrix64(pp, vv, faces).min(0).values.mean())      # noqa: E731
    v, p = verts.clone().requires_grad_(True), points.clone().requires_grad_(True)
    Aggregation.point_mesh_term(v, faces, p).backward()
    h = 1e-6
    for t, grad, which in ((v0, v.grad, 0), (p0, p.grad, 1)):
        for (i, c) in ((0, 0), (3, 1), (7, 2)):
            up, dn = t.clone(), t.clone()
            up[i, c] += h
            dn[i, c] -= h
            fd = (f(up, p0) - f(dn, p0)) / (2 * h) if which == 0 else (f(v0, up) - f(v0, dn)) / (2 * h)
            assert abs(fd - float(grad[i, c])) <= 1e-6 * (1 + abs(fd)), (which, i, c, fd, float(grad[i, c]))


# ---- the public functions on host tensors ---------------------------------------------------------------------------------------

def test_closest_faces_on_host_tensors():
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 300, 4)
    d2, idx, bary = Losses.closest_faces(points, verts, faces.int())
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64 and bary.shape == (300, 3) and not d2.requires_grad
    cases.check_search("definition, level-2 sphere", points, verts, faces, idx, d2, bary)
    d2, idx, bary = Losses.closest_faces(points[:0], verts, faces)
    assert d2.shape == (0,) and idx.shape == (0,) and bary.shape == (0, 3)
    # fp64 inputs take the definition in fp64
    d64 = Losses.closest_faces(points.double(), verts.double(), faces)[0]
    assert d64.dtype == torch.float64 and (d64 - cases.d2_matrix64(points, verts, faces).min(1).values).abs().max() <= 1e-13


def test_batch_loop_and_edge_wrapper():
    verts, faces, points = _small(5)
    vb, pb = torch.stack((verts, verts * 1.1 + 0.05)), torch.stack((points, points - 0.2))
    lb = Losses.point_mesh_face_distance(vb, faces, pb)
    each = [Losses.point_mesh_face_distance(vb[k], faces, pb[k]) for k in range(2)]
    assert abs(float(lb) - 0.5 * float(each[0] + each[1])) <= 1e-14
    # edges: the direct segment formula
    topo = MeshTopology(faces=faces)
    edges = topo.edges.long()
    M = cases.segment_d2_64(points, verts[edges[:, 0]], verts[edges[:, 1]])
    for kw, want in ((dict(), M.min(1).values.mean() + M.min(0).values.mean()), (dict(point_reduction="sum"), M.min(1).values.sum() + M.min(0).values.sum()),
                     (dict(single_directional=True), M.min(1).values.mean())):
        for e in (topo, topo.edges, edges):
            got = Losses.point_mesh_edge_distance(verts, e, points, **kw)
            assert abs(float(got) - float(want)) <= 1e-12 * float(want), kw
    v = verts.clone().requires_grad_(True)
    Losses.point_mesh_edge_distance(v, topo, points).backward()
    assert torch.isfinite(v.grad).all() and v.grad.abs().max() > 0


def test_rejected_keywords_and_shapes():
    verts, faces, points = _small(6)
    for name in ("min_triangle_area", "meshes", "pcls", "weights", "norm"):
        for fn in (Losses.point_mesh_face_distance, Losses.point_mesh_edge_distance):
            with pytest.raises(ValueError, match=name):
                fn(verts, faces[:, :2] if fn is Losses.point_mesh_edge_distance else faces, points, **{name: 5e-3})
    with pytest.raises(TypeError, match="bogus"):
        Losses.point_mesh_face_distance(verts, faces, points, bogus=1)
    with pytest.raises(ValueError, match="point_reduction"):
        Losses.point_mesh_face_distance(verts, faces, points, point_reduction="max")
    bad = faces.clone()
    bad[3, 1] = len(verts)
    neg = faces.clone()
    neg[0, 0] = -1
    for v, f, p in ((verts, faces, points[:0]), (verts[:0], faces, points), (verts, faces[:0], points), (verts, bad, points), (verts, neg, points),
                    (verts, faces[:, :2], points), (verts, faces.double(), points), (verts[:, :2], faces, points), (verts, faces, points[:, :2]),
                    (verts[None], faces, points), (torch.stack((verts, verts)), faces, points[None]), (verts.numpy(), faces, points)):
        with pytest.raises(ValueError):
            Losses.point_mesh_face_distance(v, f, p)
    for f in (bad, neg, faces[:0], faces[:, :2]):
        with pytest.raises(ValueError):
            Losses.closest_faces(points, verts, f)
    with pytest.raises(ValueError):
        Losses.closest_faces(points, verts[:0], faces)
    with pytest.raises(ValueError):
        Losses.point_mesh_edge_distance(verts, faces, points)              # [F,3] is not an edge table
    # faces of any integer dtype, and as a numpy array
    want = float(Losses.point_mesh_face_distance(verts, faces, points))
    for f in (faces.int(), faces.short(), faces.numpy()):
        assert float(Losses.point_mesh_face_distance(verts, f, points)) == want
    # the VoGE package serves the same names
    import VoGE.Losses
    assert VoGE.Losses.point_mesh_face_distance is Losses.point_mesh_face_distance and VoGE.Losses.closest_faces is Losses.closest_faces


# ---- the C entries ----------------------------------------------------------------------------------------------------------------

def test_entries_validate_before_any_hip_call(lib):
    """No GPU in this container: anything that reached HIP would fail differently."""
    Q = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    BAD, WS, CAP = -1, -2, -3
    big = (1 << 28) - 1
    assert lib.voge_point_mesh_workspace_bytes(10, 20, 30) >= (10 + 30) * 24
    assert lib.voge_point_mesh_workspace_bytes(10, 20, 30) % 16 == 0
    for V, F, P in ((0, 20, 30), (10, 0, 30), (10, 20, 0), (big + 1, 20, 30), (10, big + 1, 30), (10, 20, big + 1)):
        assert lib.voge_point_mesh_workspace_bytes(V, F, P) == 0
    assert ops.POINT_MESH_MAX_PAIRS == 1 << 38
    side = 1 << 19      # 2^19 x 2^19 pairs: the cap itself passes the size checks, one more row does not
    # voge_closest_faces(points, P, verts, V, faces, F, face_idx, d2, bary, stream)
    assert lib.voge_closest_faces(Q, 0, Q, 10, Q, 20, Q, Q, Q, None) == 0      # P == 0: nothing is launched
    assert lib.voge_closest_faces(None, 0, None, 10, None, 20, None, None, None, None) == 0
    for args in ((Q, -1, Q, 10, Q, 20, Q, Q, Q), (Q, 30, Q, 0, Q, 20, Q, Q, Q), (Q, 30, Q, 10, Q, 0, Q, Q, Q), (Q, big + 1, Q, 10, Q, 20, Q, Q, Q),
                 (Q, 30, Q, big + 1, Q, 20, Q, Q, Q), (Q, 30, Q, 10, Q, big + 1, Q, Q, Q), (None, 30, Q, 10, Q, 20, Q, Q, Q),
                 (Q, 30, None, 10, Q, 20, Q, Q, Q), (Q, 30, Q, 10, None, 20, Q, Q, Q), (Q, 30, Q, 10, Q, 20, None, Q, Q),
                 (Q, 30, Q, 10, Q, 20, Q, None, Q), (Q, 30, Q, 10, Q, 20, Q, Q, None)):
        assert lib.voge_closest_faces(*args, None) == BAD, args
    assert lib.voge_closest_faces(Q, side + 1, Q, 10, Q, side, Q, Q, Q, None) == CAP
    assert lib.voge_closest_faces(Q, big, Q, 10, Q, big, Q, Q, Q, None) == CAP
    # voge_point_mesh_fwd(verts, V, faces, F, points, P, flags, loss, face_idx, bary_p, point_idx, bary_f, meta, ws, bytes, stream)
    need = lib.voge_point_mesh_workspace_bytes(10, 20, 30)
    ok = [Q, 10, Q, 20, Q, 30, 0, Q, Q, Q, Q, Q, Q, Q, need]

    def fwd(**change):
        a = list(ok)
        for k, val in change.items():
            a[int(k[1:])] = val
        return lib.voge_point_mesh_fwd(*a, None)
    for k in (0, 2, 4, 7, 8, 9, 10, 11, 12, 13):
        assert fwd(**{f"a{k}": None}) == BAD, k
    for k in (1, 3, 5):
        assert fwd(**{f"a{k}": 0}) == BAD and fwd(**{f"a{k}": big + 1}) == BAD, k
    assert fwd(a6=4) == BAD and fwd(a13=Q + 8) == BAD
    assert fwd(a14=need - 1) == WS
    assert fwd(a3=side, a5=side + 1, a14=1 << 40) == CAP
    assert fwd(a6=2, a10=None, a11=None, a14=need - 1) == WS      # single-directional: the two tables may be null (and the size is still checked)
    # voge_point_mesh_bwd(verts, V, faces, F, points, P, face_idx, bary_p, point_idx, bary_f, meta, g_loss, flags, g_verts, g_points, ws, bytes, stream)
    okb = [Q, 10, Q, 20, Q, 30, Q, Q, Q, Q, Q, Q, 0, Q, Q, Q, need]

    def bwd(**change):
        a = list(okb)
        for k, val in change.items():
            a[int(k[1:])] = val
        return lib.voge_point_mesh_bwd(*a, None)
    for k in (0, 2, 4, 6, 7, 8, 9, 10, 11, 13, 14, 15):
        assert bwd(**{f"a{k}": None}) == BAD, k
    for k in (1, 3, 5):
        assert bwd(**{f"a{k}": 0}) == BAD and bwd(**{f"a{k}": big + 1}) == BAD, k
    assert bwd(a12=8) == BAD and bwd(a15=Q + 4) == BAD
    assert bwd(a16=(10 + 30) * 24 - 1) == WS
    assert bwd(a3=side, a5=side + 1, a16=1 << 40) == CAP
    assert bwd(a12=2, a8=None, a9=None, a16=0) == WS

