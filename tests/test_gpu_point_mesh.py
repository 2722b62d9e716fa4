"""GPU tests of the point-to-mesh kernels (voge_closest_faces, voge_point_mesh_fwd / _bwd; an extension, the reference and the
oracle have none), of Losses.closest_faces / point_mesh_face_distance / point_mesh_edge_distance on the device and of
demo/FitMeshToScan.py.

selection   the fp64 distance to the element the kernel chose is at most the fp64 minimum plus SELECT_C 2^-23 (d + L)^2, for
            every point and every face; face indices are never compared with the definition's (a second face inside the bound
            is almost always the neighbour across a shared edge, with the same closest point).
values      d2 and the closest point a + (w1 e0 + w2 e1) against the fp64 closest point of the kernel's own pair, at the bounds
            tests/point_mesh_cases.py derives; weights >= 0 that sum to 1 within 2^-22.
bits        the kernel's d2 and weights on its own pairs are the bits of Aggregation.point_triangle_closest in fp32 on the host
            -- the pair function is the definition operation by operation; this is also how the faces' d2, which stay in the
            workspace, are known to the loss test.
loss        the fp64 reduction of the kernel's own d2, rounded once.
gradients   the closed form in fp64 on the kernel's own pairs and weights, element by element, no exclusions.
The shapes are the smallest that cross the kernels' boundaries: tiles of 256 triangles and 1024 points, 64 queries a workgroup."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import point_mesh_cases as cases
from util import log_line
from voge_amd import Aggregation, Losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FT, PT = ops.POINT_MESH_FACE_TILE, ops.POINT_MESH_POINT_TILE


def _definition_on_pairs(points, verts, faces, pi, fi):
    tri = faces.long()[fi.long()]
    return Aggregation.point_triangle_closest(points[pi.long()], verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]])


def check_both_directions(label, verts, faces, points):
    """closest_faces and the node's forward on one mesh and one cloud: every promise of the module's docstring.  Returns
    (the node's outputs, d2 of the points, d2 of the faces)."""
    vd, fd, pd = verts.to(DEV), faces.to(DEV), points.to(DEV)
    d2, idx, bary = Losses.closest_faces(pd, vd, fd)
    assert d2.is_cuda and d2.dtype == torch.float32 and idx.dtype == torch.int32 and bary.shape == (len(points), 3)
    P, F = len(points), len(faces)
    ref_d2, ref_bary = _definition_on_pairs(points, verts, faces, torch.arange(P), idx.cpu())
    assert torch.equal(d2.cpu(), ref_d2) and torch.equal(bary.cpu(), ref_bary), label      # the definition's bits on the kernel's pairs
    cases.check_search(label, points, verts, faces, idx, d2, bary)
    loss, face_idx, bary_p, point_idx, bary_f = ops.point_mesh(vd, fd.int(), pd)
    assert torch.equal(face_idx, idx) and torch.equal(bary_p, bary), label                  # one search, two entries
    d2f, ref_bary = _definition_on_pairs(points, verts, faces, point_idx.cpu(), torch.arange(F))
    assert torch.equal(bary_f.cpu(), ref_bary), label
    cases.check_search(label, points, verts, faces, point_idx, d2f, bary_f, by_face=True)
    return (loss, face_idx, bary_p, point_idx, bary_f), d2.cpu(), d2f


# ---- the searches ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, FT - 1, FT, FT + 1, 2 * FT + 3])
def test_face_tile_boundaries(hip_lib, F):
    verts, faces = cases.soup(F)
    for P in (1, 63, 64, 65, 257):
        check_both_directions(f"soup F={F}", verts, faces, cases.points_around(verts, faces, P, seed=F + P))


@pytest.mark.parametrize("P", [PT - 1, PT, PT + 1, 2 * PT + 3])
def test_point_tile_boundaries(hip_lib, P):
    for F in (1, 63, 64, 65, 257):
        verts, faces = cases.soup(F)
        check_both_directions(f"soup P={P}", verts, faces, cases.points_around(verts, faces, P, seed=F + P))


@pytest.mark.parametrize("name", sorted(cases.all_test_meshes()))
def test_every_test_mesh(hip_lib, name):
    verts, faces = cases.all_test_meshes()[name]
    check_both_directions(name, verts, faces, cases.points_around(verts, faces, 300, seed=len(name)))


def test_exact_ties_keep_the_lower_index(hip_lib):
    verts, faces = cases.level2_sphere()
    twice = torch.cat((faces, faces))                                   # every face twice: the first copy must win
    points = cases.points_around(verts, faces, 500, seed=9)
    _, idx, _ = Losses.closest_faces(points.to(DEV), verts.to(DEV), twice.to(DEV))
    assert (idx < len(faces)).all()
    both = torch.cat((points, points))                                  # every point twice
    out = ops.point_mesh(verts.to(DEV), faces.int().to(DEV), both.to(DEV))
    assert (out[3] < len(points)).all()


def test_edge_shapes_and_refusals(hip_lib):
    verts, faces = cases.level2_sphere()
    vd, fd = verts.to(DEV), faces.to(DEV)
    points = cases.points_around(verts, faces, 700, seed=3).to(DEV)
    d2, idx, bary = Losses.closest_faces(points[:0], vd, fd)
    assert d2.shape == (0,) and idx.shape == (0,) and bary.shape == (0, 3) and d2.is_cuda
    want = Losses.closest_faces(points, vd, fd)
    wide = torch.zeros(700, 6, device=DEV)
    wide[:, 1:4] = points
    strided = wide[:, 1:4]                                              # a strided view, faces of another integer dtype
    assert not strided.is_contiguous()
    got = Losses.closest_faces(strided, vd, fd.short())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="chamfer_distance"):           # the pair cap, before any launch: 2^19 x (2^19 + 1) pairs
        big_f = torch.zeros((1 << 19) + 1, 3, dtype=torch.int32, device=DEV)
        ops.closest_faces(torch.zeros(1 << 19, 3, device=DEV), vd, big_f)
    with pytest.raises(ValueError):
        Losses.point_mesh_face_distance(vd, fd.clone().index_fill_(0, torch.tensor([5], device=DEV), len(verts)), points)
    # the kernels themselves never follow a face that names a vertex out of range: it never wins, nothing else moves
    bad = fd.int().clone()
    bad[7, 2] = len(verts) + 100
    loss, face_idx, _, point_idx, _ = ops.point_mesh(vd, bad, points)
    assert (face_idx != 7).all() and (point_idx >= 0).all()


# ---- loss -----------------------------------------------------------------------------------------------------------------------

def test_loss_is_the_fp64_reduction_of_the_kernels_d2(hip_lib):
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 2500, seed=1)           # three partial sums of points, one of faces
    _, dp, df = check_both_directions("level-2 sphere, loss", verts, faces, points)
    dp, df = dp.double(), df.double()
    vd, fd, pd = verts.to(DEV), faces.to(DEV), points.to(DEV)
    for label, kw, want in (("mean", {}, dp.mean() + df.mean()), ("sum", {"point_reduction": "sum"}, dp.sum() + df.sum()),
                            ("single", {"single_directional": True}, dp.mean()),
                            ("single sum", {"single_directional": True, "point_reduction": "sum"}, dp.sum())):
        loss = Losses.point_mesh_face_distance(vd, fd, pd, **kw)
        assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0
        want = float(want)
        bound = 2.0 ** -24 * abs(want) + 1e-12
        err = abs(float(loss.double().cpu()) - want)
        log_line(f"[parity] point-mesh loss {label}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (label, err, bound)
    lb = Losses.point_mesh_face_distance(torch.stack((vd, vd * 1.1)), fd, torch.stack((pd, pd - 0.05)))
    each = Losses.point_mesh_face_distance(vd, fd, pd) + Losses.point_mesh_face_distance(vd * 1.1, fd, pd - 0.05)
    assert abs(float(lb) - 0.5 * float(each)) <= 1e-6 * float(lb)


def test_edge_wrapper_is_the_segment_distance(hip_lib):
    verts, faces = cases.level2_sphere()
    topo = Losses.MeshTopology(faces=faces)
    edges = topo.edges.long()
    points = cases.points_around(verts, faces, 400, seed=2)
    M = cases.segment_d2_64(points, verts[edges[:, 0]], verts[edges[:, 1]])
    L = float((verts[edges[:, 0]] - verts[edges[:, 1]]).double().norm(dim=-1).max())
    dp, de = M.min(1).values, M.min(0).values
    for kw, want, slack in (({}, dp.mean() + de.mean(), cases.d2_bound(cases.SELECT_C, dp, L).mean() + cases.d2_bound(cases.SELECT_C, de, L).mean()),
                            ({"single_directional": True, "point_reduction": "sum"}, dp.sum(), cases.d2_bound(cases.SELECT_C, dp, L).sum())):
        for e in (topo.to(DEV), topo.edges.to(DEV)):
            got = Losses.point_mesh_edge_distance(verts.to(DEV), e, points.to(DEV), **kw)
            err, bound = abs(float(got) - float(want)), float(slack) + 2.0 ** -23 * float(want)
            log_line(f"[parity] point-mesh edge wrapper {sorted(kw)}: error {err:.3e}, bound {bound:.3e}")
            assert err <= bound


# ---- gradients ------------------------------------------------------------------------------------------------------------------

def check_grads(label, verts, faces, points, upstream=-1.75, **kw):
    vd, pd = verts.to(DEV).requires_grad_(True), points.to(DEV).requires_grad_(True)
    single, red = kw.get("single_directional", False), kw.get("point_reduction", "mean")
    loss, face_idx, bary_p, point_idx, bary_f = ops.point_mesh(vd, faces.int().to(DEV), pd, red == "sum", single)
    (loss * upstream).backward()
    ref_v, ref_p, bound_v, bound_p = cases.closed_form_grads(verts, faces, points, face_idx, bary_p, point_idx, bary_f, upstream, red)
    worst = 0.0
    for name, got, ref, bound in (("g_verts", vd.grad, ref_v, bound_v), ("g_points", pd.grad, ref_p, bound_p)):
        assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all(), (label, name)
        err = (got.double().cpu() - ref).abs()
        ratio = float((err / bound).max())
        log_line(f"[parity] point-mesh {label} {name}: max error {float(err.max()):.3e} of {float(ref.abs().max()):.3e}, measured / bound {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 1.0, (label, worst)
    return vd.grad, pd.grad, face_idx, point_idx


def test_gradients_on_the_sphere(hip_lib):
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 700, seed=4)             # inside and outside
    gv, gp, _, _ = check_grads("sphere", verts, faces, points)
    assert gv.abs().max() > 0 and gp.abs().max() > 0
    check_grads("sphere sum", verts, faces, points, point_reduction="sum")
    gv, gp, _, point_idx = check_grads("sphere single", verts, faces, points, single_directional=True)
    assert point_idx is None


def test_gradients_when_every_item_picks_one_element(hip_lib):
    """One triangle and 5 000 points: every point scatters to the one face; 300 faces and one point: every face to the point."""
    verts, faces = cases.sample_meshes.ONE_FACE
    points = cases.points_around(verts, faces, 5000, seed=5)
    _, _, face_idx, _ = check_grads("one face, 5000 points", verts, faces, points)
    assert (face_idx == 0).all()
    verts, faces = cases.soup(300)
    _, _, _, point_idx = check_grads("300 faces, one point", verts, faces, torch.tensor([[0.4, 0.6, 0.3]]))
    assert (point_idx == 0).all()


def test_gradients_far_from_the_origin_and_on_faces_without_area(hip_lib):
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 700, seed=6)
    shift = torch.tensor([1000.0, 1000.0, 1000.0])
    # (the moved inputs are rounded to fp32 -- another problem, whose faces may pick other points: it is judged on its own pairs)
    check_grads("sphere at 1000", verts + shift, faces, points + shift)
    verts, faces = cases.all_test_meshes()["zero-area 4 x 4"]
    gv, gp, _, _ = check_grads("zero-area 4 x 4", verts, faces, cases.points_around(verts, faces, 300, seed=7))
    assert torch.isfinite(gv).all() and torch.isfinite(gp).all()
    verts, faces = cases.all_test_meshes()["zero-area grid"]
    check_grads("zero-area grid", verts, faces, cases.points_around(verts, faces, 300, seed=8))


# ---- reproducibility, capture ---------------------------------------------------------------------------------------------------

def _loss_and_grads(verts, faces, points):
    v, p = verts.detach().clone().requires_grad_(True), points.detach().clone().requires_grad_(True)
    loss = Losses.point_mesh_face_distance(v, faces, p)
    loss.backward()
    return loss.detach().clone(), v.grad.clone(), p.grad.clone()


def test_two_calls_give_the_same_bits(hip_lib):
    verts, faces = cases.level2_sphere()
    rng = np.random.default_rng(5)
    points = torch.from_numpy((rng.random((30000, 3), dtype=np.float32) ** 2).astype(np.float32)).to(DEV)      # crowded towards a corner: long lists
    a, b = _loss_and_grads(verts.to(DEV), faces.int().to(DEV), points), _loss_and_grads(verts.to(DEV), faces.int().to(DEV), points)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[1]).all() and a[1].abs().max() > 0 and a[2].abs().max() > 0


def test_the_split_over_the_waves_changes_no_bit(hip_lib):
    """The product splits every tile over the 16 or 4 waves of a workgroup, by the number of queries; the A/B build
    (libvoge_hip_ab.so, a test artefact) can force either, or one wave a workgroup over whole tiles.  The winner is a property of the
    candidate set: the same bits, forward and backward."""
    import ctypes
    from voge_amd import _lib
    verts, faces = cases.soup(2 * FT + 3)
    v, f = verts.to(DEV), faces.int().to(DEV)
    p = cases.points_around(verts, faces, 2 * PT + 3, seed=12).to(DEV)
    product = _loss_and_grads(v, f, p) + tuple(ops.point_mesh(v, f, p)[1:])
    with _lib.using(_lib.AB_LIB_PATH) as ab:
        ab.voge_debug_point_mesh_waves.restype, ab.voge_debug_point_mesh_waves.argtypes = ctypes.c_int, [ctypes.c_int]
        assert ab.voge_debug_point_mesh_waves(3) == -1
        try:
            for waves in (1, 4, 16, 0):
                assert ab.voge_debug_point_mesh_waves(waves) == 0
                got = _loss_and_grads(v, f, p) + tuple(ops.point_mesh(v, f, p)[1:])
                assert all(torch.equal(a, b) for a, b in zip(got, product)), waves
        finally:
            ab.voge_debug_point_mesh_waves(0)


def test_captured_iteration_follows_the_data(hip_lib):
    """No host value leaks into the launch chain: a graph captured on one cloud gives, replayed after the points changed in place
    (other pairs, another scale of the backward), the bits of an eager call on the new points."""
    verts, faces = cases.level2_sphere()
    v = verts.to(DEV).requires_grad_(True)
    f = faces.int().to(DEV)
    p = cases.points_around(verts, faces, 1500, seed=11).to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            v.grad = p.grad = None
            Losses.point_mesh_face_distance(v, f, p).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    v.grad = p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = Losses.point_mesh_face_distance(v, f, p)
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    first = _loss_and_grads(v, f, p)
    assert torch.equal(loss, first[0]) and torch.equal(v.grad, first[1]) and torch.equal(p.grad, first[2])
    with torch.no_grad():
        p.mul_(torch.tensor([3.0, 0.5, 7.0], device=DEV)).add_(torch.tensor([-2.0, 4.0, 0.25], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    second = _loss_and_grads(v, f, p)
    assert not torch.equal(first[0], second[0])
    assert torch.equal(loss, second[0]) and torch.equal(v.grad, second[1]) and torch.equal(p.grad, second[2])


# ---- loops ----------------------------------------------------------------------------------------------------------------------

ADAM_MARGIN = 3.7e-7      # twice the 1.84e-7 measured on the first run (the loop gives the same bits on every run)


def test_adam_on_the_point_mesh_term_alone(hip_lib):
    """60 Adam steps (lr 0.01) of the level-2 sphere towards 1 000 of the bunny's points, once with the kernels and once with the
    fp64 definition on the host, from the same start.  The device's final loss is within ADAM_MARGIN, relative, of the host's."""
    verts, faces = cases.level2_sphere()
    target = cases.bunny_points(1000)
    final = {}
    for name, dev, dtype in (("kernels", DEV, torch.float32), ("definition", "cpu", torch.float64)):
        x = (verts * 0.6).to(device=dev, dtype=dtype).clone().requires_grad_(True)
        f, y = faces.to(dev), target.to(device=dev, dtype=dtype)
        opt = torch.optim.Adam([x], lr=0.01)
        first = float(Losses.point_mesh_face_distance(x, f, y).detach())
        for _ in range(60):
            opt.zero_grad()
            Losses.point_mesh_face_distance(x, f, y).backward()
            opt.step()
        final[name] = (float(Losses.point_mesh_face_distance(x, f, y).detach()), first)
    rel = abs(final["kernels"][0] - final["definition"][0]) / final["definition"][0]
    log_line(f"[parity] point-mesh Adam loop: final loss {final['kernels'][0]:.6e} (kernels), {final['definition'][0]:.6e} (fp64 definition), "
             f"relative difference {rel:.3e}; initial {final['definition'][1]:.6e}")
    assert final["definition"][0] < 0.5 * final["definition"][1]
    assert rel <= ADAM_MARGIN, rel


def test_fit_mesh_to_scan_demo(hip_lib):
    spec = importlib.util.spec_from_file_location("demo_FitMeshToScan", os.path.join(ROOT, "demo", "FitMeshToScan.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    for graph in (True, False):
        h = demo.fit(iters=40, level=2, points=1500, lr=1e-2, graph=graph, quiet=True)
        log_line(f"[parity] FitMeshToScan 40 iterations ({'graph' if graph else 'eager'}): mean distance to the mesh {h['before'][0]:.5f} -> {h['after'][0]:.5f}")
        assert np.isfinite(h["final_verts"]).all() and h["after"][0] < h["before"][0]
