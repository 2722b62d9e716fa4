"""GPU tests of the chamfer kernels (voge_nearest_points, voge_chamfer_fwd / _bwd; an extension, the reference and the oracle have
none), of Losses.chamfer_distance on the device and of the demo's chamfer term.

nearest_points: the reference is the DEFINITION (the torch form of Converters.nearest_points) computed on the host; indices and
               distances must be the same bits (torch.equal) on both routes and under every grid.
loss:          within 2^-24 relative + 1e-12 of the fp64 reduction of the definition's fp32 d2 (the kernel sums in fp64 and rounds
               once).
gradients:     against fp64 autograd of Aggregation.chamfer_term on the same fp32 inputs, element by element, at the bound
               grad_bound() derives from the kernel's arithmetic.  No element is left out.
The clouds are small; the 20 000 x 15 000 case spends its time in the host's definition."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from chamfer_clouds import fp64_chamfer_grads, surface_pair
from knn_clouds import lattice
from util import log_line
from voge_amd import Aggregation, Losses, ops
from voge_amd.Converter import Converters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"default": None, "one_cell": 1.0, "fine": 2 / 1024, "faces": 8 / 1024}


def same_as_definition(q, p, routes=("brute", "grid")):
    """Device result == host definition, bit for bit, on every route asked for (and on the default one)."""
    ref_idx, ref_d2 = Converters.nearest_points(q.cpu(), p.cpu())
    for route in tuple(routes) + (None,):
        idx, d2 = Converters.nearest_points(q.to(DEV), p.to(DEV), route=route)
        assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(q),)
        assert torch.equal(idx.cpu(), ref_idx), route
        assert torch.equal(d2.cpu(), ref_d2), route
    return ref_idx, ref_d2


# ---- bits -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True])
def test_lattice_both_routes_and_every_grid_give_the_definitions_bits(hip_lib, swap):
    q, p = lattice()[:1400], lattice()[1400:]
    if swap:
        q, p = p, q
    ref_idx, ref_d2 = Converters.nearest_points(q, p)
    qd, pd = q.to(DEV), p.to(DEV)
    idx, d2 = Converters.nearest_points(qd, pd, route="brute")
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(d2.cpu(), ref_d2)
    grids = {}
    for name, cell_size in GRIDS.items():
        idx, d2, grid = ops.nearest_points(qd, pd, cell_size=cell_size, route="grid", return_grid=True)
        assert torch.equal(idx.cpu(), ref_idx), name
        assert torch.equal(d2.cpu(), ref_d2), name
        grids[name] = tuple(grid[5:8].tolist())
        assert grid[3:4].view(torch.float32).item() > 0
    assert grids["one_cell"] == (1, 1, 1) and grids["fine"] == (32, 32, 32) and grids["faces"] == (8, 8, 8)
    assert len(set(grids.values())) == 4      # they really differed


def test_uniform_clouds_default_route(hip_lib):
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.random((20000, 3), dtype=np.float32))
    p = torch.from_numpy(rng.random((15000, 3), dtype=np.float32))
    ref_idx, ref_d2 = Converters.nearest_points(q, p)
    idx, d2, grid = ops.nearest_points(q.to(DEV), p.to(DEV), return_grid=True)
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(d2.cpu(), ref_d2)
    gx, gy, gz = grid[5:8].tolist()
    assert 20000 <= gx * gy * gz <= 8 * 20000      # the default route of 3e8 pairs is the grid, of about 2 n cells


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------

def test_edge_shapes(hip_lib):
    rng = np.random.default_rng(2)

    def rand(n, scale=1.0, shift=0.0):
        return torch.from_numpy((rng.random((n, 3), dtype=np.float32) * scale + shift).astype(np.float32))

    same_as_definition(torch.tensor([[0.25, -1.0, 3.0]]), torch.tensor([[0.5, 0.5, 0.5]]))                  # 1 x 1
    same_as_definition(rand(5), rand(3000))
    same_as_definition(rand(3000), rand(5))
    idx, _ = same_as_definition(torch.full((500, 3), 0.375), rand(700))                                     # coincident queries
    assert len(set(idx.tolist())) == 1
    idx, _ = same_as_definition(rand(700), torch.full((500, 3), 0.375))                                     # coincident points
    assert (idx == 0).all()
    idx, _ = same_as_definition(torch.full((500, 3), 0.375), torch.full((500, 3), -0.125))                  # both
    assert (idx == 0).all()
    same_as_definition(rand(2000), rand(1500, shift=100.0))        # disjoint boxes: empty rings to the end of the grid
    plane = rand(3000)
    plane[:, 2] = 0
    same_as_definition(rand(1000, shift=0.25), plane)              # a planar database, queries off the plane
    same_as_definition(plane, rand(1000))
    outside = rand(1000)
    outside[:, 0] += 1.5                                           # queries outside the database's box on one side only
    same_as_definition(outside, rand(2000))
    big_q, big_p = rand(1501).to(DEV), rand(2001).to(DEV)
    off_q, off_p = big_q[1:], big_p[1:]                            # rows off the 16-byte boundary
    assert off_q.data_ptr() % 16 != 0 and off_p.data_ptr() % 16 != 0
    same_as_definition(off_q, off_p)
    wide = rand(1200 * 2).reshape(1200, 6).to(DEV)
    strided = wide[:, 1:4]                                         # a strided view
    assert not strided.is_contiguous()
    same_as_definition(strided, big_p[::2])
    for route in (None, "brute", "grid"):
        idx, d2 = Converters.nearest_points(big_q[:0], big_p, route=route)
        assert idx.shape == d2.shape == (0,) and idx.is_cuda
    with pytest.raises(ValueError):
        Converters.nearest_points(big_q, big_p[:0])


# ---- value ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["brute", "grid"])
def test_loss_is_the_fp64_reduction_of_the_definitions_d2(hip_lib, route):
    x, y = surface_pair()
    dx, dy = Converters.nearest_points(x, y)[1].double(), Converters.nearest_points(y, x)[1].double()
    xd, yd = x.to(DEV), y.to(DEV)
    for label, sum_red, single, want in (("mean", False, False, dx.mean() + dy.mean()), ("sum", True, False, dx.sum() + dy.sum()),
                                         ("single", False, True, dx.mean()), ("single sum", True, True, dx.sum())):
        loss, nn_x, nn_y = ops.chamfer(xd, yd, sum_red, single, route)
        want = float(want)
        bound = 2.0 ** -24 * abs(want) + 1e-12
        err = abs(float(loss.double().cpu()) - want)
        log_line(f"[parity] chamfer loss {route} {label}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (label, err, bound)
        assert torch.equal(nn_x.cpu(), Converters.nearest_points(x, y)[0])
        assert (nn_y is None) if single else torch.equal(nn_y.cpu(), Converters.nearest_points(y, x)[0])
    # the public function on the device: the same node on the route the shapes choose
    loss, normals = Losses.chamfer_distance(xd, yd)
    assert normals is None and abs(float(loss.double().cpu()) - float(dx.mean() + dy.mean())) <= 2.0 ** -24 * float(dx.mean() + dy.mean()) + 1e-12
    assert abs(float(Losses.chamfer_distance(xd, yd, point_reduction="sum")[0]) - float(dx.sum() + dy.sum())) <= 2.0 ** -24 * float(dx.sum() + dy.sum()) + 1e-12


def test_loss_normals_and_batch_on_the_device(hip_lib):
    x, y = surface_pair()
    g = torch.Generator().manual_seed(3)
    nx, ny = torch.randn(1600, 3, generator=g), torch.randn(576, 3, generator=g)
    want = Losses.chamfer_distance(x.double(), y.double(), nx.double(), ny.double())
    got = Losses.chamfer_distance(x.to(DEV), y.to(DEV), nx.to(DEV), ny.to(DEV))
    assert abs(float(got[0]) - float(want[0])) <= 1e-6 * float(want[0]) and abs(float(got[1]) - float(want[1])) <= 1e-5
    xb, yb = torch.stack((x, x * 1.1)).to(DEV), torch.stack((y, y - 0.05)).to(DEV)
    lb = Losses.chamfer_distance(xb, yb)[0]
    assert abs(float(lb) - 0.5 * float(Losses.chamfer_distance(xb[0], yb[0])[0] + Losses.chamfer_distance(xb[1], yb[1])[0])) <= 1e-7 * float(lb)


# ---- gradients ------------------------------------------------------------------------------------------------------------------

def grad_bound(upstream, mag, length, w_scatter, d2max, n):
    """Per element of a gradient: what the kernel's arithmetic may differ from the exact value of the same formula by.
    Every term of an element is w * (a - b) with a, b fp32: the kernel rounds the difference to fp32 (2^-24 relative of the term),
    the scattered ones further to a multiple of the quantum q = 2^-s (q / 2 absolute each, `length` of them, weighted w_scatter);
    the sums are fp64 (2^-50 of sum |terms| covers them with room) and the result is rounded to fp32 once (2^-24 of |result| <=
    sum |terms|).  s = 62 - L - e with 2^L >= n = max(Nx, Ny) and D = sqrt(d2max (1 + 2^-20) + 2^-148) < 2^e, the rule of
    chamfer.hip's header; `mag` is sum |terms| of the element with the weights in."""
    L = max(n - 1, 0).bit_length()
    e = math.frexp(math.sqrt(d2max * (1 + 2.0 ** -20) + 2.0 ** -148))[1]
    q = 2.0 ** -(62 - L - e)
    return abs(upstream) * ((2.0 ** -23 + 2.0 ** -50) * mag + w_scatter * length[:, None].double() * q / 2) + 1e-45


def check_grads(label, x, y, route, upstream=-1.75, **kw):
    loss_ref, gx_ref, gy_ref, mag_x, mag_y, len_x, len_y = fp64_chamfer_grads(x, y, upstream, **kw)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    single, sum_red = kw.get("single_directional", False), kw.get("point_reduction", "mean") == "sum"
    loss, nn_x, nn_y = ops.chamfer(xd, yd, sum_red, single, route)
    (loss * upstream).backward()
    d2max = float(Converters.nearest_points(x, y)[1].max())
    if not single:
        d2max = max(d2max, float(Converters.nearest_points(y, x)[1].max()))
    n = max(len(x), len(y))
    wx, wy = (2.0 if sum_red else 2.0 / len(x)), (0.0 if single else (2.0 if sum_red else 2.0 / len(y)))
    worst = 0.0
    for name, got, ref, mag, length, w in (("g_x", xd.grad, gx_ref, mag_x, len_x, wy), ("g_y", yd.grad, gy_ref, mag_y, len_y, wx)):
        assert got.shape == ref.shape and got.dtype == torch.float32
        err = (got.double().cpu() - ref).abs()
        bound = grad_bound(upstream, mag, length, w, d2max, n)
        ratio = float((err / bound).max())
        log_line(f"[parity] chamfer {label} {route} {name}: max error {float(err.max()):.3e}, measured / bound {ratio:.3f} "
                 f"(longest list {int(length.max())})")
        worst = max(worst, ratio)
    assert worst <= 1.0, worst
    return xd.grad, yd.grad


@pytest.mark.parametrize("route", ["brute", "grid"])
def test_gradients_on_the_surfaces(hip_lib, route):
    x, y = surface_pair()
    check_grads("surfaces", x, y, route)
    check_grads("surfaces sum", x, y, route, point_reduction="sum")
    check_grads("surfaces single", x, y, route, single_directional=True)


@pytest.mark.parametrize("route", ["brute", "grid"])
def test_gradients_with_all_points_coincident(hip_lib, route):
    """Every x picks y_0 and every y picks x_0: the two scatter lists are as long as the other cloud."""
    x = torch.tensor([[0.3, -0.7, 1.1]]).repeat(500, 1)
    y = torch.tensor([[0.25, 0.1, 0.9]]).repeat(400, 1)
    gx, gy = check_grads("coincident", x, y, route)
    assert (gx[1:] == gx[1]).all() and (gy[1:] == gy[1]).all() and not torch.equal(gx[0], gx[1]) and not torch.equal(gy[0], gy[1])
    check_grads("coincident, the same point", x, x[:300].clone(), route)


# ---- reproducibility, capture ---------------------------------------------------------------------------------------------------

def _loss_and_grads(x, y):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    loss = Losses.chamfer_distance(xd, yd)[0]
    loss.backward()
    return loss.detach().clone(), xd.grad.clone(), yd.grad.clone()


def test_two_calls_give_the_same_bits(hip_lib):
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((30000, 3), dtype=np.float32)).to(DEV)
    y = torch.from_numpy((rng.random((30000, 3), dtype=np.float32) ** 2).astype(np.float32)).to(DEV)      # (crowded towards a corner: long lists)
    a, b = _loss_and_grads(x, y), _loss_and_grads(x, y)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[1]).all() and a[1].abs().max() > 0 and a[2].abs().max() > 0


@pytest.mark.parametrize("shape", ["grid", "brute"])
def test_captured_iteration_follows_the_data(hip_lib, shape):
    """No host value leaks into the launch chain: a graph captured on one x gives, replayed after x changed in place (another box,
    another grid, another scale of the backward), the bits of an eager call on the new x."""
    rng = np.random.default_rng(6)
    nx, ny = (9000, 7000) if shape == "grid" else (1600, 576)      # (6.3e7 pairs: the grid route; 9.2e5: the brute one)
    x = torch.from_numpy(rng.random((nx, 3), dtype=np.float32)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(rng.random((ny, 3), dtype=np.float32)).to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            x.grad = y.grad = None
            Losses.chamfer_distance(x, y)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    x.grad = y.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = Losses.chamfer_distance(x, y)[0]
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    first = _loss_and_grads(x, y)
    assert torch.equal(loss, first[0]) and torch.equal(x.grad, first[1]) and torch.equal(y.grad, first[2])
    with torch.no_grad():
        x.mul_(torch.tensor([3.0, 0.5, 7.0], device=DEV)).add_(torch.tensor([-2.0, 4.0, 0.25], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    second = _loss_and_grads(x, y)
    assert not torch.equal(first[0], second[0])
    assert torch.equal(loss, second[0]) and torch.equal(x.grad, second[1]) and torch.equal(y.grad, second[2])


# ---- loops ----------------------------------------------------------------------------------------------------------------------

def _demo():
    spec = importlib.util.spec_from_file_location("demo_ShapeFitting_chamfer", os.path.join(ROOT, "demo", "ShapeFitting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_adam_on_the_chamfer_term_alone(hip_lib):
    """20 Adam steps (lr 0.02) of a level-2 icosphere towards the points of ground_truth_shape(3): the torch definition ends at
    0.053 of its initial loss on the host (below the 0.25 the step count was chosen for); the kernels must end below 0.5."""
    demo = _demo()
    sv, gv = demo.ico_sphere(2)[0], demo.ground_truth_shape(3)[0]
    final = {}
    for name, dev, fn in (("kernels", DEV, lambda a, b: Losses.chamfer_distance(a, b)[0]), ("definition", "cpu", Aggregation.chamfer_term)):
        x = torch.from_numpy(sv).to(dev).clone().requires_grad_(True)
        y = torch.from_numpy(gv).to(dev)
        opt = torch.optim.Adam([x], lr=0.02)
        first = float(fn(x, y).detach())
        for _ in range(20):
            opt.zero_grad()
            fn(x, y).backward()
            opt.step()
        final[name] = float(fn(x, y).detach()) / first
    log_line(f"[parity] chamfer Adam loop: final / initial loss {final['kernels']:.4f} (kernels), {final['definition']:.4f} (definition)")
    assert final["definition"] < 0.25
    assert final["kernels"] < 0.5


def test_shape_fitting_demo_with_the_chamfer_term(hip_lib):
    import inspect
    demo = _demo()
    assert inspect.signature(demo.fit).parameters["w_chamfer"].default == 0.0      # off unless asked for
    kw = dict(iters=20, level=2, size=64, graph=True, quiet=True, rgb_on=10)
    on, off = demo.fit(w_chamfer=1.0, **kw), demo.fit(**kw)
    for h in (on, off):
        assert len(h["silhouette"]) == 20 and np.isfinite(h["silhouette"]).all() and np.isfinite(h["rgb"]).all()
        assert np.isfinite(h["final_verts"]).all()
    # the losses of the first iteration are taken before any step: the term changes nothing there, and moves the fit afterwards
    assert np.isclose(on["silhouette"][0], off["silhouette"][0], rtol=1e-6) and on["silhouette"][1:] != off["silhouette"][1:]
    gt = torch.from_numpy(demo.ground_truth_shape(2)[0])
    c_on = float(Aggregation.chamfer_term(torch.from_numpy(on["final_verts"]), gt))
    c_off = float(Aggregation.chamfer_term(torch.from_numpy(off["final_verts"]), gt))
    log_line(f"[parity] ShapeFitting 20 iterations: chamfer to the ground truth {c_on:.5f} with the term, {c_off:.5f} without")
