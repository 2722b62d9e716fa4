"""Mesh regularisers without a GPU (voge_amd.Losses: MeshTopology, mesh_regularisers and the three PyTorch3D names; an extension,
the reference and the oracle have none): the topology tables against hand-written answers, the torch definitions
(Aggregation.mesh_edge_term / mesh_laplacian_term / mesh_normal_term) in fp64 against an independent numpy restatement written
with plain loops straight from the FACES (it shares nothing with the tables) and against central differences, the singular
rules, and the argument checks of the C ABI.  tests/test_gpu_mesh_reg.py reuses the hand cases below."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape_fitting_demo():
    spec = importlib.util.spec_from_file_location("shape_fitting_demo", os.path.join(ROOT, "demo", "ShapeFitting.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    return demo


# ---- the hand cases: small-integer coordinates, exact in fp32 and fp64 -------------------------------------------------------------
TETRA_V = [(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2)]
TETRA_F = [(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)]
# the hub of a centrally symmetric hexagon (an affine image of the regular one).  Antipodes carry CONSECUTIVE indices (1, 2),
# (3, 4), (5, 6), so a sum over the hub's neighbours in ascending order cancels pair by pair: exactly 0 in any precision.
HEX_V = [(0, 0, 0), (4, 0, 0), (-4, 0, 0), (2, 4, 0), (-2, -4, 0), (-2, 4, 0), (2, -4, 0)]
HEX_F = [(0, 1, 3), (0, 3, 5), (0, 5, 2), (0, 2, 4), (0, 4, 6), (0, 6, 1)]
FOLD_F = [(0, 1, 2), (1, 0, 3)]      # two faces on the edge (0, 1): v0 = 0, v1 = (2, 0, 0), a = (0, 2, 0), b varies


def fold(b):
    return [(0, 0, 0), (2, 0, 0), (0, 2, 0), b]


def hand_cases():
    """name -> (verts [V,3] float64 array, faces, num_verts, target_length)"""
    f8 = lambda v: np.asarray(v, np.float64)      # noqa: E731
    return {
        "tetrahedron": (f8(TETRA_V), TETRA_F, None, 0.25),
        "lone_triangle": (f8([(0, 0, 0), (2, 0, 0), (0, 2, 0)]), [(0, 1, 2)], None, 0.25),
        "fan_of_three": (f8([(0, 0, 0), (0, 0, 2), (2, 0, 0), (0, 2, 0), (-2, -1, 0)]), [(0, 1, 2), (0, 1, 3), (1, 0, 4)], None, 0.25),
        "unused_vertex": (f8(fold((0, -2, 1)) + [(7, 7, 7)]), FOLD_F, 5, 0.25),
        "coincident": (f8([(0, 0, 0), (0, 0, 0), (3, 4, 0), (0, 0, 2)]), [(0, 1, 2), (0, 2, 3)], None, 0.5),
        "hexagon_hub": (f8(HEX_V), HEX_F, None, 0.25),
        "zero_area": (f8(fold((0, -2, 0))[:2] + [(1, 0, 0), (0, -2, 0)]), FOLD_F, None, 0.25),
        "fold_flat": (f8(fold((0, -2, 0))), FOLD_F, None, 0.25),
        "fold_right_angle": (f8(fold((0, 0, 2))), FOLD_F, None, 0.25),
        "fold_back": (f8(fold((0, 1, 0))), FOLD_F, None, 0.25),
    }


# ---- an independent restatement: plain loops over the faces ---------------------------------------------------------------------
def restate(verts, faces, t):
    """(edge, laplacian, normal) of one mesh in fp64 with Python loops, from the faces alone."""
    v = np.asarray(verts, np.float64)
    V = v.shape[0]
    edge_faces = {}
    for f, (a, b, c) in enumerate(faces):
        for i, j, k in ((a, b, c), (b, c, a), (c, a, b)):
            edge_faces.setdefault((min(i, j), max(i, j)), []).append((f, k))
    edge = sum((np.linalg.norm(v[i] - v[j]) - t) ** 2 for i, j in edge_faces) / max(len(edge_faces), 1)
    nbrs = [set() for _ in range(V)]
    for i, j in edge_faces:
        nbrs[i].add(j)
        nbrs[j].add(i)
    lap = 0.0
    for i in range(V):
        if nbrs[i]:
            lap += np.linalg.norm(sum(v[j] - v[i] for j in sorted(nbrs[i])) / len(nbrs[i]))
    lap /= max(V, 1)
    total, count = 0.0, 0
    for (i, j), fs in sorted(edge_faces.items()):
        fs = sorted(fs)
        for x in range(len(fs)):
            for y in range(x + 1, len(fs)):
                n0 = np.cross(v[j] - v[i], v[fs[x][1]] - v[i])
                n1 = -np.cross(v[j] - v[i], v[fs[y][1]] - v[i])
                l0, l1 = np.linalg.norm(n0), np.linalg.norm(n1)
                total += 1.0 - (n0 @ n1) / (l0 * l1) if l0 > 0 and l1 > 0 else 1.0
                count += 1
    return edge, lap, total / max(count, 1)


def definition(verts, topo, t, terms=("edge", "laplacian", "normal")):
    """the torch definitions in fp64 on the host -> (values [3], gradient of each term alone [3][..,V,3])"""
    from voge_amd.Losses import mesh_regularisers
    vals, grads = [], []
    for k, name in enumerate(("edge", "laplacian", "normal")):
        v = torch.tensor(np.asarray(verts), dtype=torch.float64, requires_grad=True)
        out = mesh_regularisers(v, topo, t, terms)[k]
        if out.requires_grad:
            out.backward()
        vals.append(val(out))
        grads.append(np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy())
    return np.asarray(vals), grads


def val(x):
    return float(x.detach())


def tables(topo):
    return {n: getattr(topo, n).tolist() for n in ("edges", "nbr_off", "nbr", "pairs", "inc_off", "inc")}


# ---- 1. the topology ------------------------------------------------------------------------------------------------------------
def test_tetrahedron_tables():
    from voge_amd.Losses import MeshTopology
    topo = MeshTopology(faces=TETRA_F)
    assert (topo.num_verts, topo.num_edges, topo.num_pairs, topo.max_degree) == (4, 6, 6, 3)
    got = tables(topo)
    assert got["edges"] == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert got["nbr_off"] == [0, 3, 6, 9, 12]
    assert got["nbr"] == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    # edge (0,1): faces 0 (opposite 2) and 2 (opposite 3); (0,2): faces 0 (1), 1 (3); (0,3): 1 (2), 2 (1); (1,2): 0 (0), 3 (3); ...
    assert got["pairs"] == [[0, 1, 2, 3], [0, 2, 1, 3], [0, 3, 2, 1], [1, 2, 0, 3], [1, 3, 0, 2], [2, 3, 0, 1]]
    assert got["inc_off"] == [0, 6, 12, 18, 24]
    for vtx in range(4):      # every entry pair * 4 + role names the vertex, ascending
        ent = got["inc"][got["inc_off"][vtx]:got["inc_off"][vtx + 1]]
        assert ent == sorted(ent) and all(got["pairs"][e >> 2][e & 3] == vtx for e in ent)
    assert all(getattr(topo, n).dtype == torch.int32 for n in got)
    assert MeshTopology(faces=torch.tensor(TETRA_F)).pairs.tolist() == got["pairs"]


def test_one_two_and_three_triangles_on_an_edge():
    from voge_amd.Losses import MeshTopology
    one = MeshTopology(faces=[(0, 1, 2)])
    assert (one.num_verts, one.num_edges, one.num_pairs) == (3, 3, 0)
    assert tables(one)["pairs"] == [] and tables(one)["inc"] == [] and tables(one)["inc_off"] == [0, 0, 0, 0]
    two = MeshTopology(faces=[(2, 1, 0), (1, 2, 3)])
    assert tables(two)["pairs"] == [[1, 2, 0, 3]] and two.num_edges == 5
    assert tables(two)["inc_off"] == [0, 1, 2, 3, 4] and tables(two)["inc"] == [2, 0, 1, 3]
    three = MeshTopology(faces=[(0, 1, 2), (0, 1, 3), (1, 0, 4)])
    assert tables(three)["pairs"] == [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4]]      # (first face, second face): (0,1) (0,2) (1,2)
    assert tables(three)["inc"] == [0, 4, 8, 1, 5, 9, 2, 6, 3, 10, 7, 11] and three.max_degree == 4


def test_unused_vertex_and_edges_only():
    from voge_amd.Losses import MeshTopology
    topo = MeshTopology(faces=[(0, 1, 2)], num_verts=5)
    assert topo.num_verts == 5 and tables(topo)["nbr_off"] == [0, 2, 4, 6, 6, 6] and tables(topo)["inc_off"] == [0] * 6
    graph = MeshTopology(edges=[(1, 0), (0, 1), (2, 1), (3, 1)])      # direction and repeats do not matter
    assert tables(graph)["edges"] == [[0, 1], [1, 2], [1, 3]] and tables(graph)["nbr"] == [1, 0, 2, 3, 1, 1]
    assert (graph.num_verts, graph.num_pairs, graph.max_degree) == (4, 0, 3) and tables(graph)["inc_off"] == [0] * 5
    v = torch.tensor([(0, 0, 0), (1, 0, 0), (1, 2, 0), (1, 0, 2)], dtype=torch.float64, requires_grad=True)
    from voge_amd.Losses import mesh_regularisers
    e, lap, nrm = mesh_regularisers(v, graph, 1.0)
    assert val(e) == pytest.approx((0 + 1 + 1) / 3) and val(nrm) == 0.0 and not nrm.requires_grad
    # L = (1,0,0), (-1/3, 2/3, 2/3), (0,-2,0), (0,0,-2): norms 1, 1, 2, 2
    assert val(lap) == pytest.approx(6.0 / 4)
    empty = MeshTopology(edges=np.zeros((0, 2), np.int64), num_verts=3)
    assert [val(x) for x in mesh_regularisers(v[:3], empty)] == [0.0, 0.0, 0.0]
    assert MeshTopology(faces=np.zeros((0, 3), np.int64)).num_verts == 0
    assert topo.to("cpu") is topo


@pytest.mark.parametrize("kw", [
    dict(faces=[(0, 1, 3)], num_verts=3), dict(faces=[(0, 1, -1)]), dict(edges=[(0, 4)], num_verts=4), dict(edges=[(-1, 0)]),
    dict(faces=[(0, 1, 1)]), dict(faces=[(0, 1, 2), (2, 3, 2)]), dict(edges=[(1, 1)]),
    dict(faces=[(0, 1, 2)], edges=[(0, 1)]), dict(), dict(num_verts=3),
    dict(faces=[(0, 1)]), dict(faces=[(0.0, 1.0, 2.0)]), dict(edges=[(0, 1, 2)])])
def test_topology_refuses(kw):
    from voge_amd.Losses import MeshTopology
    with pytest.raises(ValueError):
        MeshTopology(**kw)


def test_regularisers_refuse_bad_arguments():
    from voge_amd.Losses import MeshTopology, mesh_regularisers
    topo = MeshTopology(faces=TETRA_F)
    with pytest.raises(ValueError):
        mesh_regularisers(torch.zeros(5, 3), topo)
    with pytest.raises(ValueError):
        mesh_regularisers(torch.zeros(4, 2), topo)
    with pytest.raises(ValueError):
        mesh_regularisers(torch.zeros(4, 3), topo, terms=("edge", "cot"))


# ---- 2. the definitions ---------------------------------------------------------------------------------------------------------
def noisy_sphere(level, noise, seed=3, shift=0.0):
    """demo/ShapeFitting.ico_sphere(level) scaled radially by 1 + noise * U(-1, 1) (one draw of shape (V, 1)), then translated;
    fp32."""
    v, f = shape_fitting_demo().ico_sphere(level)
    v = v.astype(np.float64) * (1.0 + noise * np.random.default_rng(seed).uniform(-1, 1, (v.shape[0], 1)))
    return (v + shift).astype(np.float32), f


@pytest.mark.parametrize("name", list(hand_cases()))
def test_definitions_match_the_restatement_on_hand_cases(name):
    from voge_amd.Losses import MeshTopology
    verts, faces, nv, t = hand_cases()[name]
    vals, grads = definition(verts, MeshTopology(faces=faces, num_verts=nv), t)
    np.testing.assert_allclose(vals, restate(verts, faces, t), rtol=0, atol=1e-14)
    assert all(np.isfinite(g).all() for g in grads)


def test_definitions_match_the_restatement_and_central_differences():
    from voge_amd.Losses import MeshTopology, mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency, mesh_regularisers
    v32, faces = noisy_sphere(1, 0.15)
    verts, t = v32.astype(np.float64), 0.25
    topo = MeshTopology(faces=faces)
    assert (topo.num_verts, topo.num_edges, topo.num_pairs) == (42, 120, 120)
    vals, grads = definition(verts, topo, t)
    np.testing.assert_allclose(vals, restate(verts, faces.tolist(), t), rtol=1e-13, atol=0)
    rng, h = np.random.default_rng(0), 1e-6
    for _ in range(12):      # central differences at a few coordinates
        i, c = int(rng.integers(42)), int(rng.integers(3))
        up, dn = verts.copy(), verts.copy()
        up[i, c] += h
        dn[i, c] -= h
        fd = (np.asarray(restate(up, faces.tolist(), t)) - np.asarray(restate(dn, faces.tolist(), t))) / (2 * h)
        np.testing.assert_allclose([g[i, c] for g in grads], fd, rtol=0, atol=2e-9)
    # the single-term names and `terms=` agree with the fused call; a term left out is an exact 0 without a gradient
    v = torch.tensor(verts, requires_grad=True)
    assert val(mesh_edge_loss(v, topo, t)) == vals[0] and val(mesh_laplacian_smoothing(v, topo)) == vals[1]
    assert val(mesh_normal_consistency(v, topo)) == vals[2]
    e, lap, nrm = mesh_regularisers(v, topo, t, terms=("edge", "normal"))
    assert val(lap) == 0.0 and not lap.requires_grad and val(e) == vals[0] and val(nrm) == vals[2]
    # a batch is the mean over its meshes
    batch = np.stack([verts, verts * 1.5, verts[::-1].copy()])
    bv, bg = definition(batch, topo, t)
    singles = [definition(x, topo, t) for x in batch]
    np.testing.assert_allclose(bv, np.mean([s[0] for s in singles], axis=0), rtol=1e-14)
    for k in range(3):
        np.testing.assert_allclose(bg[k], np.stack([s[1][k] for s in singles]) / 3, rtol=0, atol=1e-16)
    # fp32 host vertices take the definitions too
    assert mesh_regularisers(torch.tensor(v32), topo, t)[1].dtype == torch.float32


# ---- 3. the singular rules: finite values, exactly zero gradients, in fp32 and fp64 ------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_singular_rules(dtype):
    from voge_amd.Losses import MeshTopology, mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency
    cases = hand_cases()

    def run(fn, name, *args):
        verts, faces, nv, t = cases[name]
        v = torch.tensor(verts, dtype=dtype, requires_grad=True)
        out = fn(v, MeshTopology(faces=faces, num_verts=nv), *args)
        out.backward()
        assert torch.isfinite(v.grad).all()
        return val(out), v.grad.numpy()

    # coincident vertices 0 and 1, t = 0.5: the edge (0,1) counts t^2 and passes nothing; 0 and 1 then get the same gradient from
    # their edges to vertex 2 at distance 5, and vertex 0 one more from (0,3) at distance 2:  E = 5 edges
    got, g = run(mesh_edge_loss, "coincident", 0.5)
    assert got == pytest.approx((0.25 + 2 * 4.5 ** 2 + 1.5 ** 2 + (29 ** 0.5 - 0.5) ** 2) / 5)
    np.testing.assert_allclose(g[1], 2 * 4.5 * np.array([-0.6, -0.8, 0]) / 5, rtol=1e-6)
    np.testing.assert_allclose(g[0] - g[1], 2 * 1.5 * np.array([0, 0, -1.0]) / 5, rtol=0, atol=1e-6)
    got, g = run(mesh_edge_loss, "coincident", 0.0)      # t = 0: the term itself is 0 there
    assert np.isfinite(got)
    # the hub's L is exactly 0, and so is the gradient at the hub: nothing passes through |L_hub|, and the ring's u_j / d_j
    # cancel pair by pair
    got, g = run(mesh_laplacian_smoothing, "hexagon_hub")
    assert got > 0 and (g[0] == 0).all() and (g[1:] != 0).any()
    # a zero-area face: the pair counts 1 and passes no gradient at all
    got, g = run(mesh_normal_consistency, "zero_area")
    assert got == 1.0 and (g == 0).all()
    # folds: flat 0 with a zero gradient, a right angle 1, folded back 2
    got, g = run(mesh_normal_consistency, "fold_flat")
    assert got == 0.0 and (g == 0).all()
    assert run(mesh_normal_consistency, "fold_right_angle")[0] == 1.0
    assert run(mesh_normal_consistency, "fold_back")[0] == 2.0
    # an isolated vertex has L = 0 and gets nothing
    got, g = run(mesh_laplacian_smoothing, "unused_vertex")
    assert (g[4] == 0).all()


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entries_validate_before_any_hip_call(lib):
    Q = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)

    def fwd(B=2, V=10, E=20, P=20, terms=7, verts=Q, edges=Q, nbr_off=Q, nbr=Q, pairs=Q, lap_dir=Q, ws=Q, ws_bytes=1 << 20, out=Q):
        return lib.voge_mesh_reg_fwd(verts, edges, nbr_off, nbr, pairs, B, V, E, P, terms, 0.25, lap_dir, ws, ws_bytes, out, None)

    def bwd(B=2, V=10, E=20, P=20, terms=7, verts=Q, nbr_off=Q, nbr=Q, pairs=Q, inc_off=Q, inc=Q, lap_dir=Q, g=Q, out=Q):
        return lib.voge_mesh_reg_bwd(verts, nbr_off, nbr, pairs, inc_off, inc, lap_dir, g, g, g, B, V, E, P, terms, 0.25, out, None)
    for f in (fwd, bwd):
        assert f(V=0) == 0 and f(B=0) == 0 and f(B=0, V=0, verts=None, out=None) == 0      # nothing to do: nothing is launched
        assert f(V=-1) == -1 and f(B=-1) == -1 and f(E=-1) == -1 and f(P=-1) == -1 and f(B=-1, V=0) == -1
        assert f(terms=8) == -1 and f(terms=-1) == -1
        for name in ("verts", "nbr_off", "nbr", "pairs", "lap_dir", "out"):
            assert f(**{name: None}) == -1, name
        assert f(B=1 << 15, V=1 << 15) == -1                  # B * V * 3 does not fit an int
        assert f(E=1 << 30) == -1 and f(P=1 << 29) == -1      # 2 E and 4 P + 3 must
        assert f(pairs=Q + 8) == -1                           # a pair row is one 16-byte load
    assert fwd(edges=None) == -1 and fwd(edges=Q + 4) == -1 and bwd(inc=None) == -1 and bwd(inc_off=None) == -1
    assert fwd(ws=None) == -2 and fwd(ws_bytes=2 * 3 * 4 - 1) == -2      # one block a mesh: 2 * 3 floats
    # a pointer that belongs to a term that is off is not asked for
    assert fwd(B=0, terms=1, nbr=None) == 0 and fwd(terms=1, nbr=None, pairs=None, lap_dir=None, B=-1) == -1
    assert lib.voge_mesh_reg_workspace_bytes(2, 10, 20, 20) == 2 * 3 * 4
    assert lib.voge_mesh_reg_workspace_bytes(3, 642, 1920, 1920) == 3 * 18 * 3 * 4      # 4482 items: 18 blocks a mesh
    assert lib.voge_mesh_reg_workspace_bytes(0, 10, 20, 20) == 0 and lib.voge_mesh_reg_workspace_bytes(2, 10, -1, 0) == 0
    assert lib.voge_abi_version() == 7
