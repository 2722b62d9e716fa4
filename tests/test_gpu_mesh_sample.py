"""GPU tests of the mesh sampling kernels (voge_mesh_sample_fwd / _bwd; an extension, the reference and the oracle have none), of
Losses.sample_points_from_meshes on the device and of the demo's sampled chamfer term.

faces      against the definition (Aggregation.mesh_surface_points on the host from the same fp32 inputs) by the two rules of
           sample_meshes.check_face_choice; the first test shows that the areas both choose by are the same bits.
values     points, bary and normals against the fp64 evaluation at the faces the device returned, at the bounds
           sample_meshes derives from the op sequence.
gradients  against fp64 autograd of the definition at the device's faces, element by element (sample_meshes.fp64_sample_grads).
The meshes are small on purpose."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from sample_meshes import (ONE_FACE, check_face_choice, check_outputs, face_cdf, fp64_sample_grads, grid_mesh, random_u, skewed_mesh,
                           tetrahedron, zero_area_grid)
from util import log_line
from voge_amd import Aggregation, Losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = ops.MESH_SAMPLE_BLOCK


def device_sample(verts, faces, u, normals=True, areas=False):
    sampler = Losses.SurfaceSampler(faces, num_verts=len(verts), device=DEV)
    out = ops.mesh_sample(verts.to(DEV), sampler, u.to(DEV), normals, areas)
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.int32 and out[2].shape == (len(u),)
    return tuple(None if t is None else t.cpu() for t in out)


def check_forward(label, verts, faces, u, cap=0.01):
    p, n, idx, bary = device_sample(verts, faces, u)
    second = check_face_choice(verts, faces, u, idx)
    worst = check_outputs(verts, faces, torch.where(torch.isnan(u), torch.zeros_like(u), u).clamp(0, 1 - 2.0 ** -24), idx, p, bary, n)
    log_line(f"[parity] mesh_sample {label}: {second} of {len(u)} samples by the boundary rule; measured / bound "
             + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if cap is not None:
        assert second <= cap * len(u), second
    p2, n2, idx2, bary2 = device_sample(verts, faces, u, normals=False)
    assert n2 is None and torch.equal(p2, p) and torch.equal(idx2, idx) and torch.equal(bary2, bary)
    return p, n, idx, bary


def check_grads(label, verts, faces, u, with_normals=True, seed=0):
    """Gradients of a random linear functional of points (and normals) against fp64 autograd at the device's faces."""
    g = torch.Generator().manual_seed(seed)
    cp = torch.randn(len(u), 3, generator=g)
    cn = torch.randn(len(u), 3, generator=g) if with_normals else None
    sampler = Losses.SurfaceSampler(faces, num_verts=len(verts), device=DEV)
    vd = verts.to(DEV).requires_grad_(True)
    p, n, idx, _ = ops.mesh_sample(vd, sampler, u.to(DEV), with_normals)
    loss = (p * cp.to(DEV)).sum()
    if with_normals:
        loss = loss + (n * cn.to(DEV)).sum()
    loss.backward()
    ref, bound = fp64_sample_grads(verts, faces, u, idx.cpu(), cp, cn)
    got = vd.grad.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    log_line(f"[parity] mesh_sample gradients {label}: max error {float(err.max()):.3e}, measured / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    return got


# ---- 1: the areas, one face -----------------------------------------------------------------------------------------------------

def test_areas_are_the_definitions_bits(hip_lib):
    for verts, faces in (tetrahedron(), grid_mesh(23, 13, jitter=0.3), skewed_mesh(), tetrahedron(1e-2, 1000.0)):
        out = device_sample(verts, faces, random_u(16, 1), areas=True)
        assert torch.equal(out[4], Aggregation.mesh_face_areas2(verts, faces))


def test_one_face(hip_lib):
    verts, faces = ONE_FACE
    u = random_u(4096, 2)
    p, n, idx, bary = check_forward("one face", verts, faces, u, cap=0.0)
    assert (idx == 0).all() and (bary >= 0).all() and ((bary.double().sum(-1) - 1).abs() <= 2 * 2.0 ** -23).all()
    check_grads("one face (4096 samples on three vertices)", verts, faces, u)
    check_grads("one face, points only", verts, faces, u, with_normals=False)


# ---- 2, 8: the tetrahedron ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_normals", [False, True])
def test_tetrahedron(hip_lib, with_normals):
    verts, faces = tetrahedron()
    verts = verts + torch.tensor([[0.05, -0.02, 0.0], [0.0, 0.03, 0.01], [-0.04, 0.0, 0.02], [0.01, 0.01, -0.03]])
    u = random_u(8192, 3)
    _, _, idx, _ = check_forward("tetrahedron", verts, faces, u)
    assert set(idx.tolist()) == {0, 1, 2, 3}
    check_grads(f"tetrahedron, normals {with_normals}", verts, faces, u, with_normals)


def test_far_from_the_origin(hip_lib):
    verts, faces = tetrahedron(1e-2, 1000.0)
    u = random_u(2048, 4)
    check_forward("tetrahedron of edge 1e-2 at 1000", verts, faces, u)
    check_grads("tetrahedron of edge 1e-2 at 1000", verts, faces, u)


# ---- 3: several scan blocks -----------------------------------------------------------------------------------------------------

def block_u(verts, faces):
    """u0 that lands in the first and the last face of every scan block and just either side of every block boundary"""
    _, cdf = face_cdf(verts, faces)
    total, F = float(cdf[-1]), len(cdf)
    t = []
    for b in range(0, F, BLOCK):
        first, last = b, min(b + BLOCK, F) - 1
        lo = float(cdf[first - 1]) if first else 0.0
        t += [0.5 * (lo + float(cdf[first])), 0.5 * (float(cdf[last - 1]) + float(cdf[last]))]      # inside the first / last face
        t += [lo * (1 - 1e-6), lo * (1 + 1e-6) + 1e-9 * total]                                      # either side of the boundary
    u = random_u(len(t), 5)
    u[:, 0] = torch.tensor(t, dtype=torch.float64).div(total).clamp(0, 1 - 2.0 ** -24).float()
    return u


def test_several_scan_blocks(hip_lib):
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    F = len(faces)
    assert F > 2 * BLOCK + 37
    u = random_u(8192, 6)
    _, _, idx, _ = check_forward("grid of 598 faces", verts, faces, u)
    assert set((idx // BLOCK).tolist()) == set(range((F + BLOCK - 1) // BLOCK))
    ub = block_u(verts, faces)
    _, _, idx, _ = check_forward("grid of 598 faces, hand-built u", verts, faces, ub, cap=None)
    got = set(idx.tolist())
    for b in range(0, F, BLOCK):
        assert b in got and min(b + BLOCK, F) - 1 in got, b
    check_grads("grid of 598 faces", verts, faces, u)


# ---- 4, 5: degenerate faces -----------------------------------------------------------------------------------------------------

def test_zero_area_faces(hip_lib):
    verts, faces, run = zero_area_grid(BLOCK)                                  # the run straddles the first block boundary
    F = len(faces)
    A2, _ = face_cdf(verts, faces)
    assert run[0] < BLOCK <= run[-1] and (A2[[0, F - 1] + run] == 0).all() and (A2 > 0).sum() == F - 2 - len(run)
    u = random_u(8192, 7)
    _, _, idx, _ = check_forward("zero-area faces", verts, faces, u)                # (asserts that none was chosen; the 1 % cap)
    assert BLOCK - 4 in idx.tolist() and BLOCK + 4 in idx.tolist()
    check_forward("zero-area faces, hand-built u", verts, faces, block_u(verts, faces), cap=None)
    edge = torch.tensor([[0.0, 0.3, 0.3], [1 - 2.0 ** -24, 0.3, 0.3], [-2.0, 0.3, 0.3], [5.0, 0.3, 0.3], [float("nan"), 0.3, 0.3],
                         [1.0, 0.3, 0.3], [0.5, float("nan"), 7.0]])
    p, n, idx, bary = device_sample(verts, faces, edge)
    assert idx[:6].tolist() == [1, F - 2, 1, F - 2, 1, F - 2]
    check_face_choice(verts, faces, edge, idx)
    assert bary[6].tolist() == [1.0, 0.0, 0.0] and torch.equal(p[6], verts[faces[idx[6].long(), 0]])
    check_grads("zero-area faces", verts, faces, u[:4096])


def test_table_in_memory_and_long_block_scan(hip_lib):
    """More scan blocks than the sampler stages in LDS (the block table is searched in memory) and more than the 1024 threads of
    the block scan (a thread scans several entries): the smallest grid past both."""
    verts, faces = grid_mesh(512, 513, jitter=0.3)
    nb = (len(faces) + BLOCK - 1) // BLOCK
    assert nb > ops.MESH_SAMPLE_LDS_BLOCKS and nb > 1024 and len(faces) == 525312
    u = random_u(20000, 12)
    _, _, idx, _ = check_forward("grid of 525312 faces", verts, faces, u)
    assert len(set((idx // BLOCK).tolist())) > 2000 and int(idx.max()) // BLOCK > 2040 and int(idx.min()) // BLOCK < 10
    check_grads("grid of 525312 faces", verts, faces, u)


def test_all_degenerate_and_nan_meshes_return(hip_lib):
    """Every loop of the kernels is bounded by a table size (32 and 9 trips of the searches, the corner walk by 3 F), so a mesh
    without area and a NaN vertex are ordinary returns: face -1, zero outputs, zero gradients."""
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    flat = verts * torch.tensor([1.0, 0.0, 0.0])
    nanv = verts.clone()
    nanv[300, 1] = float("nan")
    u = random_u(1000, 8)
    sampler = Losses.SurfaceSampler(faces, device=DEV)
    for v in (flat, nanv):
        vd = v.to(DEV).requires_grad_(True)
        p, n, idx, bary = ops.mesh_sample(vd, sampler, u.to(DEV), True)
        assert (idx == -1).all() and not p.any() and not n.any() and not bary.any()
        (p.sum() + n.sum()).backward()
        torch.cuda.synchronize()
        assert vd.grad.shape == v.shape and not vd.grad.any()


# ---- 6, 7: ties, skewed areas ---------------------------------------------------------------------------------------------------

def test_exact_ties(hip_lib):
    verts, faces = grid_mesh(16, 16, lift=False)
    F = len(faces)
    A2, cdf = face_cdf(verts, faces)
    assert F == 512 and (A2 == A2[0]).all() and float(cdf[-1]) == F * float(A2[0])      # equal areas, exact sums
    u = random_u(F, 9)
    u[:, 0] = torch.arange(F) / F                                                        # t is exactly the boundary k A2
    a = device_sample(verts, faces, u)
    check_face_choice(verts, faces, u, a[2])
    k = torch.arange(F)
    assert ((a[2] == k) | (a[2] == (k - 1).clamp(min=0))).all()
    b = device_sample(verts, faces, u)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_skewed_areas(hip_lib):
    """2000 tiny faces (1e-6 of the area together) in front of one large face: a u0 for the middle of each reaches exactly it.
    Behind the large face an fp32 cumulative sum would not even see them; the fp32 u0 there are the few 1 - k 2^-24."""
    verts, faces = skewed_mesh(2000)
    A2, cdf = face_cdf(verts, faces)
    assert float(A2[-1] / cdf[-1]) > 1 - 2e-6 and len(faces) == 2001
    lo = torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-2]])
    u0 = (0.5 * (lo + cdf[:-1]) / cdf[-1]).float()
    t = u0.double() * cdf[-1]
    assert ((t > lo) & (t < cdf[:-1])).all()                                             # each fp32 u0 is inside its face
    u = random_u(2000, 10)
    u[:, 0] = u0
    _, _, idx, _ = check_forward("skewed areas", verts, faces, u, cap=0.0)
    assert torch.equal(idx.long(), torch.arange(2000))
    verts, faces = skewed_mesh(2000, big_first=True)
    A2, cdf = face_cdf(verts, faces)
    assert float(np.cumsum(A2.numpy())[-1]) == float(A2[0])                              # what a sequential fp32 table would hold
    u = random_u(17, 11)
    u[:, 0] = 1 - torch.arange(1, 18) * 2.0 ** -24
    _, _, idx, _ = check_forward("skewed areas, the large face first", verts, faces, u, cap=None)
    assert (idx[:10] > 0).all() and len(set(idx[:10].tolist())) == 10                    # 6e-8 apart: some hundred faces each


# ---- 9: reproducibility, capture ------------------------------------------------------------------------------------------------

def _step(verts, sampler, u=None, generator=None, S=4096):
    verts.grad = None
    p, n, idx, bary = Losses.sample_points_from_meshes(verts, sampler, S, True, generator, u, True)
    ((p * p).sum() + (n[:, 0] * p[:, 1]).sum()).backward()
    # detached: an output that keeps its grad_fn keeps the vertices' AccumulateGrad node -- and the stream it was made on -- alive
    # into the next step, and a captured step whose two backward edges meet in that node would pull that stream into the capture
    return p.detach(), n.detach(), idx, bary, verts.grad


def test_two_runs_give_the_same_bits_and_capture(hip_lib):
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    sampler = Losses.SurfaceSampler(faces, device=DEV)
    vd = verts.to(DEV).requires_grad_(True)
    u = random_u(4096, 20).to(DEV)
    a = [t.clone() for t in _step(vd, sampler, u)]
    b = [t.clone() for t in _step(vd, sampler, u)]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[4].abs().max() > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(vd, sampler, u)
            _step(vd, sampler, None, None)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    vd.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(vd, sampler, u)
    for seed in (21, 22):
        u.copy_(random_u(4096, seed))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        eager = _step(vd.detach().clone().requires_grad_(True), sampler, u)
        for x, y in zip(got, eager):
            assert torch.equal(x, y)
    # u=None: the draw is part of the graph, every replay draws anew
    vd.grad = None
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        out2 = _step(vd, sampler, None, None)
    graph2.replay()
    torch.cuda.synchronize()
    first = out2[0].clone()
    graph2.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first, out2[0]) and torch.isfinite(out2[4]).all()


def test_captured_draw_with_a_registered_generator(hip_lib):
    """u=None with the CALLER'S generator under capture: registered with the graph before the capture, every replay draws anew
    from it, and after the same seed the first replay draws what an eager call draws."""
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    sampler = Losses.SurfaceSampler(faces, device=DEV)
    vd = verts.to(DEV).requires_grad_(True)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(123)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(vd, sampler, None, gen)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    vd.grad = None
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(gen)
    with torch.cuda.graph(graph):
        out = _step(vd, sampler, None, gen)
    gen.manual_seed(77)
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in out]
    graph.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in out]
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[2], second[2])
    for o in (first, second):
        assert torch.isfinite(o[4]).all() and o[4].abs().max() > 0 and (o[2] >= 0).all()
    gen.manual_seed(77)
    eager = _step(vd.detach().clone().requires_grad_(True), sampler, None, gen)
    for x, y in zip(first, eager):
        assert torch.equal(x, y)


# ---- 10: routing ----------------------------------------------------------------------------------------------------------------

def test_routing(hip_lib):
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    u = random_u(2000, 30)
    node = Losses.sample_points_from_meshes(verts.to(DEV), Losses.SurfaceSampler(faces, device=DEV), u=u.to(DEV), return_normals=True,
                                            return_faces=True)
    assert node[2].dtype == torch.int32
    routes = {"host tensors": (verts, Losses.SurfaceSampler(faces), u),
              "fp64 vertices": (verts.double().to(DEV), Losses.SurfaceSampler(faces, device=DEV), u.to(DEV)),
              "a sampler on another device": (verts.to(DEV), Losses.SurfaceSampler(faces), u.to(DEV)),
              "a faces tensor": (verts.to(DEV), faces.to(DEV), u.to(DEV))}
    for name, (v, s, uu) in routes.items():
        p, n, idx, bary = Losses.sample_points_from_meshes(v, s, u=uu, return_normals=True, return_faces=True)
        assert p.device == v.device and p.dtype == v.dtype, name
        assert (idx.dtype == torch.int32) == (name == "a faces tensor"), name      # (the node's index type: which route ran)
        if name != "fp64 vertices":      # (their areas are fp64: other boundaries, by 2^-24 of a face)
            check_face_choice(verts, faces, u, idx.cpu())
        same = idx.cpu().long() == node[2].cpu().long()
        assert same.float().mean() >= 0.99
        # both are within the bounds of the fp64 evaluation at their own faces
        check_outputs(verts, faces, u, idx.cpu(), p.cpu().float(), bary.cpu().float(), n.cpu().float())
    vb = torch.stack((verts, verts * 1.5 + 0.25)).to(DEV)
    ub = torch.stack((u, random_u(2000, 31))).to(DEV)
    sampler = Losses.SurfaceSampler(faces, device=DEV)
    pb, nb, fb, bb = Losses.sample_points_from_meshes(vb, sampler, u=ub, return_normals=True, return_faces=True)
    for b in range(2):
        one = Losses.sample_points_from_meshes(vb[b], sampler, u=ub[b], return_normals=True, return_faces=True)
        for x, y in zip((pb[b], nb[b], fb[b], bb[b]), one):
            assert torch.equal(x, y)
    p = Losses.sample_points_from_meshes(vb[0], sampler, 1234)
    assert p.shape == (1234, 3) and p.is_cuda
    p, f, b = Losses.sample_points_from_meshes(vb[0], sampler, 0, return_faces=True)
    assert p.shape == b.shape == (0, 3) and f.shape == (0,) and p.is_cuda
    with pytest.raises(ValueError):
        Losses.sample_points_from_meshes(vb[0], torch.zeros((0, 3), dtype=torch.long), 10)
    with pytest.raises(ValueError):
        Losses.sample_points_from_meshes(vb[0, :50], sampler, 10)
    with pytest.raises(ValueError):
        Losses.SurfaceSampler([[0, 1, 1]])


# ---- 11, 12: with chamfer, the demo ---------------------------------------------------------------------------------------------

def _demo():
    spec = importlib.util.spec_from_file_location("demo_ShapeFitting_sampled", os.path.join(ROOT, "demo", "ShapeFitting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_chamfer_of_two_sampled_surfaces(hip_lib):
    """d chamfer(sample(src), sample(tgt)) / d src vertices: the composition of the two fp64 references.  The chamfer node's
    gradient g_x is checked in tests/test_gpu_chamfer.py at its own bound; here it is the upstream of the sampler's backward,
    which must hold fp64_sample_grads' bound for THAT upstream."""
    demo = _demo()
    sv, sf = demo.ico_sphere(2)
    src, faces = torch.from_numpy(sv), torch.from_numpy(sf)
    tgt = src * torch.tensor([0.8, 0.9, 0.7])
    S = 3000
    ux, uy = random_u(S, 40), random_u(S, 41)
    sampler = Losses.SurfaceSampler(faces, device=DEV)
    vd = src.to(DEV).requires_grad_(True)
    x, fx, _ = Losses.sample_points_from_meshes(vd, sampler, u=ux.to(DEV), return_faces=True)
    x.retain_grad()
    with torch.no_grad():
        y = Losses.sample_points_from_meshes(tgt.to(DEV), sampler, u=uy.to(DEV))
    loss = Losses.chamfer_distance(x, y, point_reduction="sum")[0]
    loss.backward()
    g_x = x.grad.cpu()
    # the chamfer gradient against its own fp64 reference at the device's samples
    xr = x.detach().cpu().double().requires_grad_(True)
    Aggregation.chamfer_term(xr, y.cpu().double(), point_reduction="sum").backward()
    # (a sanity check that the upstream is the chamfer gradient, no bound of this file: tests/test_gpu_chamfer.py holds g_x to its
    # derived bound.  2^-16 of the largest entry: far above fp32 rounding, far below a wrong neighbour)
    assert (g_x.double() - xr.grad).abs().max() <= 2.0 ** -16 * xr.grad.abs().max()
    ref, bound = fp64_sample_grads(src, faces, ux, fx.cpu(), g_x)
    err = (vd.grad.cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    log_line(f"[parity] mesh_sample under chamfer: max error {float(err.max()):.3e}, measured / bound {ratio:.3f}")
    assert ratio <= 1.0
    # and the whole composition in fp64 from the vertices, at the device's faces and neighbours
    vr = src.double().requires_grad_(True)
    xp = Aggregation.mesh_surface_points(vr, faces, ux.double(), face_idx=fx.cpu())[0]
    Aggregation.chamfer_term(xp, y.cpu().double(), point_reduction="sum").backward()
    # (again a sanity check of the pairing only -- the fp64 points differ from the device's fp32 ones by their rounding, which the
    # chamfer gradient 2 (x - y) passes on --; the assertion that carries a derived bound is the one above)
    assert (vd.grad.cpu().double() - vr.grad).abs().max() <= 2.0 ** -13 * vr.grad.abs().max()


def test_shape_fitting_demo_with_the_sampled_chamfer_term(hip_lib):
    import inspect
    demo = _demo()
    assert inspect.signature(demo.fit).parameters["chamfer_samples"].default == 0      # off unless asked for
    kw = dict(iters=30, level=2, size=64, quiet=True, rgb_on=10, w_chamfer=1.0, chamfer_samples=2000)
    eager, graph = demo.fit(**kw), demo.fit(graph=True, **kw)
    sv, sf = demo.ico_sphere(2)
    gv, gf, _ = demo.ground_truth_shape(2)
    ue, ug = random_u(4000, 50).double(), random_u(4000, 51).double()
    y = Aggregation.mesh_surface_points(torch.from_numpy(gv).double(), torch.from_numpy(gf), ug)[0]

    def score(v):
        return float(Aggregation.chamfer_term(Aggregation.mesh_surface_points(torch.from_numpy(v).double(), torch.from_numpy(sf), ue)[0], y))

    start = score(sv)
    for name, h in (("eager", eager), ("graph", graph)):
        assert len(h["silhouette"]) == 30 and np.isfinite(h["silhouette"]).all() and np.isfinite(h["final_verts"]).all()
        end = score(h["final_verts"])
        log_line(f"[parity] ShapeFitting 30 iterations, sampled chamfer ({name}): surface chamfer {start:.5f} -> {end:.5f}")
        assert end < start
    # the first iteration's losses are taken before any step
    assert np.isclose(eager["silhouette"][0], graph["silhouette"][0], rtol=1e-6) and np.isclose(eager["rgb"][0], graph["rgb"][0], rtol=1e-6)


def test_sample_mesh_surface_demo(hip_lib):
    spec = importlib.util.spec_from_file_location("demo_SampleMeshSurface", os.path.join(ROOT, "demo", "SampleMeshSurface.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, "demo"))
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "demo"))
    lines = []
    r = mod.run(samples=4000, level=2, size=64, device=DEV, log=lines.append)
    assert r["points"].shape == r["normals"].shape == (4000, 3) and r["image"].shape == (64, 64, 3)
    assert torch.isfinite(r["image"]).all() and r["covered"] > 0.05
    assert ((r["normals"].norm(dim=-1) - 1).abs() <= 1e-5).all() and (r["face_idx"] >= 0).all()
    log_line("[parity] SampleMeshSurface: " + lines[0])
    assert r["agree"] > 0.8      # PCA normals of 16 neighbours on a smooth surface: loose, a sanity check of the pairing
