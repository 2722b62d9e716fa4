"""GPU tests of the grid route of the point-to-mesh kernels (voge_closest_faces_grid, voge_point_mesh_fwd_grid; an extension).

bits        route="grid" returns, element for element, the bits of route="brute": d2, face_idx and bary of closest_faces; the
            loss, every index and weight table and both gradients of the node -- on every case of tests/point_mesh_grid_cases.py
            and with the cell forced small, left alone and forced to one cell.  torch.equal on everything; a table that may hold
            a NaN (the case with a NaN vertex) is compared on its bit patterns.
bounds      the same searches against fp64 at the bounds tests/point_mesh_cases.py derives (check_search, both directions).
state       the same bits on two runs and from a workspace byte-filled 0x00 / 0x7F / 0xFF (tests/dirty.py); a graph captured on one
            cloud, replayed after the points and vertices changed in place, gives the bits of a fresh call.
above cap   a planar mesh of 525 312 triangles against 524 288 points, 2.8 10^11 pairs: the brute route and route=None refuse,
            the grid route returns, and every point's face is one an fp64 oracle over the 3 x 3 quads under it allows."""
import numpy as np
import pytest
import torch

import point_mesh_cases as cases
import point_mesh_grid_cases as gc
from dirty import dirty
from util import log_line
from voge_amd import Aggregation, Losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _dev(name):
    v, f, p = gc.case(name)
    return v.to(DEV), f.int().to(DEV), p.to(DEV)


def _node(v, f, p, route, cell_size=None, sum_reduction=False, single=False, upstream=-1.75):
    """(loss, face_idx, bary_p, point_idx, bary_f, g_verts, g_points) of one forward and backward"""
    vv, pp = v.detach().clone().requires_grad_(True), p.detach().clone().requires_grad_(True)
    out = ops.point_mesh(vv, f, pp, sum_reduction, single, route=route, cell_size=cell_size)
    (out[0] * upstream).backward()
    return tuple(out) + (vv.grad, pp.grad)


# ---- bits -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gc.NAMES)
def test_grid_route_returns_the_brute_routes_bits(hip_lib, name):
    v, f, p = _dev(name)
    want = ops.closest_faces(p, v, f, route="brute")
    nodes = {(s, single): _node(v, f, p, "brute", None, s, single) for s, single in ((False, False), (True, True))}
    for cell_size in gc.cell_sizes(name):
        got = ops.closest_faces(p, v, f, route="grid", cell_size=cell_size)
        for what, a, b in zip(("d2", "face_idx", "bary"), got, want):
            assert _same(a, b), (name, cell_size, what)
        for (s, single), ref in nodes.items():
            out = _node(v, f, p, "grid", cell_size, s, single)
            for what, a, b in zip(("loss", "face_idx", "bary_p", "point_idx", "bary_f", "g_verts", "g_points"), out, ref):
                assert _same(a, b), (name, cell_size, s, single, what)
    # the other two combinations of the reduction and the directions, on the default cell
    for s, single in ((True, False), (False, True)):
        assert all(_same(a, b) for a, b in zip(_node(v, f, p, "grid", None, s, single), _node(v, f, p, "brute", None, s, single))), (name, s, single)


def test_public_functions_take_the_route(hip_lib):
    v, f, p = _dev("soup, mixed sizes")
    assert all(_same(a, b) for a, b in zip(Losses.closest_faces(p, v, f, route="grid"), Losses.closest_faces(p, v, f, route="brute")))
    for kw in ({}, {"single_directional": True, "point_reduction": "sum"}):
        assert _same(Losses.point_mesh_face_distance(v, f, p, route="grid", **kw), Losses.point_mesh_face_distance(v, f, p, route="brute", **kw))
    v, f, p = gc.case("none large")
    topo = Losses.MeshTopology(faces=f).to(DEV)
    for kw in ({}, {"single_directional": True}):
        a = Losses.point_mesh_edge_distance(v.to(DEV), topo, p.to(DEV), route="grid", **kw)
        assert _same(a, Losses.point_mesh_edge_distance(v.to(DEV), topo, p.to(DEV), route="brute", **kw))
    with pytest.raises(ValueError, match="route"):
        Losses.closest_faces(p.to(DEV), v.to(DEV), f.to(DEV), route="bvh")
    with pytest.raises(ValueError, match="cell_size"):
        ops.closest_faces(p.to(DEV), v.to(DEV), f.int().to(DEV), route="grid", cell_size=-1.0)
    d2, idx, bary = Losses.closest_faces(p[:0].to(DEV), v.to(DEV), f.to(DEV), route="grid")
    assert d2.shape == (0,) and idx.shape == (0,) and bary.shape == (0, 3) and d2.is_cuda


# ---- bounds -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in gc.NAMES if n not in gc.NOT_FINITE])
def test_grid_route_against_fp64(hip_lib, name):
    """check_search's fp64 matrix holds every pair: a case of more than 2^20 pairs is checked on an evenly spaced subset of its
    queries, against ALL items (a query's search does not depend on the other queries)."""
    v, f, p = gc.case(name)
    vd, fd, pd = _dev(name)
    d2, idx, bary = ops.closest_faces(pd, vd, fd, route="grid")
    qp = torch.arange(0, len(p), max(1, len(p) * len(f) >> 20))
    cases.check_search(f"grid, {name}", p[qp], v, f, idx.cpu()[qp], d2.cpu()[qp], bary.cpu()[qp])
    _, face_idx, _, point_idx, bary_f = ops.point_mesh(vd, fd, pd, route="grid")
    assert torch.equal(face_idx, idx)
    # (the faces' d2 stay in the workspace: the definition's bits on the kernel's pairs, as tests/test_gpu_point_mesh.py takes them)
    qf = torch.arange(0, len(f), max(1, len(p) * len(f) >> 20))
    tri, pi = f[qf], point_idx.cpu()[qf]
    d2f = Aggregation.point_triangle_closest(p[pi.long()], v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]])[0]
    cases.check_search(f"grid, {name}", p, v, tri, pi, d2f, bary_f.cpu()[qf], by_face=True)


# ---- state ------------------------------------------------------------------------------------------------------------------------

def test_two_runs_and_a_dirty_workspace_give_the_same_bits(hip_lib):
    for name in ("300 large", "far points"):
        v, f, p = _dev(name)
        first = _node(v, f, p, "grid") + tuple(ops.closest_faces(p, v, f, route="grid"))
        again = _node(v, f, p, "grid") + tuple(ops.closest_faces(p, v, f, route="grid"))
        assert all(_same(a, b) for a, b in zip(first, again)), name
        need = hip_lib.voge_point_mesh_grid_workspace_bytes(len(v), len(f), len(p))
        for pattern in (0x00, 0x7F, 0xFF):
            with dirty(pattern, grow=max(need, 1 << 22)) as d:
                got = _node(v, f, p, "grid")
                d.refill()
                got = got + tuple(ops.closest_faces(p, v, f, route="grid"))
                assert d.taken and all(asked <= had for asked, had in d.taken)
            assert all(_same(a, b) for a, b in zip(got, first)), (name, hex(pattern))


def test_permuting_the_faces_permutes_the_indices(hip_lib):
    """Points inside the sphere: the nearest point of a convex mesh from inside is the foot on the nearest face's plane, interior
    to that face, so two faces tie only on a set of measure zero.  The few points that do tie exactly in fp32 are told by the brute
    route on the reversed order of the faces (a tie changes its answer) and left out."""
    v, f, _ = gc.case("icosphere")
    rng = np.random.default_rng(3)
    d = rng.normal(size=(3000, 3))
    p = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 0.9, (3000, 1))).astype(np.float32))
    perm = torch.from_numpy(rng.permutation(len(f)))
    rev = torch.arange(len(f) - 1, -1, -1)
    vd, pd = v.to(DEV), p.to(DEV)
    d2, idx, _ = ops.closest_faces(pd, vd, f.int().to(DEV), route="grid")
    d2q, idxq, _ = ops.closest_faces(pd, vd, f[perm].int().to(DEV), route="grid")
    assert torch.equal(d2q, d2)
    idx_rev = rev.to(DEV)[ops.closest_faces(pd, vd, f[rev].int().to(DEV), route="brute")[1].long()]
    unique = idx_rev == idx.long()
    assert float(unique.float().mean()) > 0.99
    assert torch.equal(perm.to(DEV)[idxq.long()][unique], idx.long()[unique])


def test_captured_grid_route_follows_the_data(hip_lib):
    """Nothing of the grid route depends on a value the host would read: a graph captured on one cloud gives, replayed after the
    points and the vertices changed in place -- another box, another cell, other large triangles --, the bits of a fresh call."""
    v0, f0, p0 = gc.case("soup, mixed sizes")
    v = v0.to(DEV).requires_grad_(True)
    f = f0.int().to(DEV)
    p = p0.to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            v.grad = p.grad = None
            Losses.point_mesh_face_distance(v, f, p, route="grid").backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    v.grad = p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = Losses.point_mesh_face_distance(v, f, p, route="grid")
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    first = _node(v, f, p, "grid", upstream=1.0)
    assert _same(loss, first[0]) and _same(v.grad, first[5]) and _same(p.grad, first[6])
    with torch.no_grad():
        p.mul_(torch.tensor([3.0, 0.5, 7.0], device=DEV)).add_(torch.tensor([-2.0, 4.0, 0.25], device=DEV))
        v.mul_(torch.tensor([0.25, 2.0, 1.0], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    second = _node(v, f, p, "grid", upstream=1.0)
    brute = _node(v, f, p, "brute", upstream=1.0)
    assert not _same(first[0], second[0])
    assert _same(loss, second[0]) and _same(v.grad, second[5]) and _same(p.grad, second[6])
    assert all(_same(a, b) for a, b in zip(second, brute))


def test_extract_mesh_demo_scores_its_mesh_with_the_grid_route(hip_lib):
    """demo/ExtractMesh.py ends with the exact score of its mesh against the scene's points, both roles, by the grid route; the
    brute route gives the same completeness to the bit."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("extract_mesh_demo_scored", os.path.join(root, "demo", "ExtractMesh.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    verts, faces, report = demo.run(resolution=64, views=8, image=64, out=None)
    log_line(f"[parity] demo/ExtractMesh.py 64^3, 8 views of 64^2, scored: {report}")
    assert "points -> mesh" in report and 0.0 <= demo.LAST["completeness"] < 0.05 and 0.0 <= demo.LAST["accuracy"] < 0.05
    pts = torch.from_numpy(np.load(os.path.join(root, "tests", "golden", "bunny_gaussians.npz"))["verts"]).float().to(DEV)
    brute = float(Losses.closest_faces(pts, verts, faces, route="brute")[0].sqrt().mean())
    assert brute == demo.LAST["completeness"]


# ---- routes by size ---------------------------------------------------------------------------------------------------------------

def _planar(nx, ny, P, seed):
    """A planar grid of 2 nx ny triangles (quads of side 1 / nx, vertices lifted by up to 0.1 quads) and P points over known quads
    at heights below 0.4 quads -> (verts, faces, points, row [P], col [P]); quad q = row * nx + col holds the faces 2 q and 2 q + 1"""
    xs, ys = torch.meshgrid(torch.arange(nx + 1, dtype=torch.float64) / nx, torch.arange(ny + 1, dtype=torch.float64) / nx, indexing="xy")
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(xs.shape, generator=g, dtype=torch.float64) - 0.5) * (0.2 / nx)
    verts = torch.stack((xs, ys, z), -1).reshape(-1, 3).float()
    i = (torch.arange(ny)[:, None] * (nx + 1) + torch.arange(nx)[None, :]).reshape(-1)
    faces = torch.stack((torch.stack((i, i + 1, i + nx + 2), 1), torch.stack((i, i + nx + 2, i + nx + 1), 1)), 1).reshape(-1, 3)
    col = torch.randint(0, nx, (P,), generator=g)
    row = torch.randint(0, ny, (P,), generator=g)
    u = torch.rand((P, 3), generator=g, dtype=torch.float64)
    points = torch.stack(((col + u[:, 0]) / nx, (row + u[:, 1]) / nx, (u[:, 2] - 0.5) * (0.8 / nx)), 1).float()
    return verts, faces, points, row, col


def test_auto_route_on_both_sides_of_the_crossover(hip_lib):
    """The measured crossover is the pair cap (ops.POINT_MESH_GRID_MIN_PAIRS = 2^38): 2^19 faces against 2^19 - 1 points are the
    brute force's under None, against 2^19 points the grid's.  Both sides give the bits of both explicit routes -- closest_faces
    here, where one brute-force search is 0.75 s; the node's loss and gradients under None at a small size."""
    assert ops.POINT_MESH_GRID_MIN_PAIRS == 1 << 38
    verts, faces, points, _, _ = _planar(512, 512, 1 << 19, seed=5)
    F = len(faces)
    assert F == 1 << 19
    vd, fd, pd = verts.to(DEV), faces.int().to(DEV), points.to(DEV)
    grid = ops.closest_faces(pd, vd, fd, route="grid")
    for P in ((1 << 19) - 1, 1 << 19):
        assert ops._point_mesh_route(None, F, P, "t") == ("grid" if P == 1 << 19 else "brute")
        auto = ops.closest_faces(pd[:P], vd, fd)
        assert all(_same(a, b[:P]) for a, b in zip(auto, grid)), P
    brute = ops.closest_faces(pd, vd, fd, route="brute")
    assert all(_same(a, b) for a, b in zip(brute, grid))
    v, f, p = _dev("soup, mixed sizes")
    auto = _node(v, f, p, None)
    for route in ("brute", "grid"):
        assert all(_same(a, b) for a, b in zip(_node(v, f, p, route), auto)), route


def test_above_the_pair_cap(hip_lib):
    """2 x 512 x 513 = 525 312 triangles of a planar grid and 2^19 points over known quads at heights below half a quad: 2.8 10^11
    pairs, above the cap.  The brute route and route=None refuse; the grid route returns, every point's face is among those an fp64
    oracle over the 3 x 3 quads under the point allows within check_search's selection bound, and d2 is within its value bound."""
    nx, ny, P = 512, 513, 1 << 19
    verts, faces, points, row, col = _planar(nx, ny, P, seed=7)
    F = len(faces)
    assert F == 2 * nx * ny and F > 1 << 19 and F * P > ops.POINT_MESH_MAX_PAIRS
    vd, fd, pd = verts.to(DEV), faces.int().to(DEV), points.to(DEV)
    for route in (None, "brute"):
        with pytest.raises(ValueError, match="chamfer_distance"):
            ops.closest_faces(pd, vd, fd, route=route)
        with pytest.raises(ValueError, match="chamfer_distance"):
            Losses.point_mesh_face_distance(vd, fd, pd, route=route)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.closest_faces(pd, vd, fd, route="grid")                       # (the first call allocates the workspace)
    start.record()
    d2, idx, bary = ops.closest_faces(pd, vd, fd, route="grid")
    stop.record()
    torch.cuda.synchronize()
    log_line(f"[parity] point-mesh grid above the cap: {P} points x {F} faces in {start.elapsed_time(stop):.2f} ms")
    assert ((idx >= 0) & (idx < F)).all()
    # the fp64 oracle on the device: the 18 faces of the 3 x 3 quads around the point's quad.  A face outside them is farther than
    # one quad (1 / nx) from the point in the plane, the point's own quad nearer than 0.4 + 0.1 quads in height: the true minimum
    # is among the 18
    dq = torch.tensor([-1, 0, 1])
    rr = (row[:, None, None] + dq[None, :, None]).clamp(0, ny - 1)
    cc = (col[:, None, None] + dq[None, None, :]).clamp(0, nx - 1)
    quad = (rr * nx + cc).reshape(P, 9)
    cand = torch.stack((2 * quad, 2 * quad + 1), -1).reshape(P, 18).to(DEV)
    v64 = vd.double()
    tri = fd.long()[cand]                                             # [P,18,3]
    m = cases.closest64(pd.double()[:, None], v64[tri[..., 0]], v64[tri[..., 1]], v64[tri[..., 2]])[0]
    least = m.min(1).values
    chosen_tri = fd.long()[idx.long()]
    chosen, _ = cases.closest64(pd.double(), v64[chosen_tri[:, 0]], v64[chosen_tri[:, 1]], v64[chosen_tri[:, 2]])
    edge = float(cases.longest_edge(verts, faces[:4096]).max()) * 1.5      # (every face's edges are below 1.5 x a quad's diagonal)
    assert edge >= 2.0 ** 0.5 / nx
    select = float(((chosen - least) / cases.d2_bound(cases.SELECT_C, least, edge)).max())
    value = float(((d2.double() - chosen).abs() / cases.d2_bound(cases.VALUE_C, chosen, edge)).max())
    log_line(f"[parity] point-mesh grid above the cap: measured / bound selection {select:.3f}, value {value:.3f}")
    assert select <= 1.0 and value <= 1.0
    among = (cand == idx.long()[:, None]).any(1)
    assert among.all(), int((~among).sum())
    assert (bary >= 0).all() and float((bary.sum(-1) - 1).abs().max()) <= 2.0 ** -22
