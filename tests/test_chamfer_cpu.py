"""CPU tests of the chamfer distance: the torch definitions (Converters.nearest_points, Aggregation.chamfer_term,
Losses.chamfer_distance) against fp64 references written out here, and the argument checks of the four C entries (the library
loads without a GPU: anything that reached HIP would fail differently)."""
import os

import numpy as np
import pytest
import torch

from chamfer_clouds import brute_force_nearest
from knn_clouds import lattice
from voge_amd import Aggregation, Losses
from voge_amd.Converter import Converters


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _clouds(nx=7, ny=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(nx, 3, generator=g, dtype=torch.float64), torch.randn(ny, 3, generator=g, dtype=torch.float64) * 0.8 + 0.1


def _cdist_min(x, y):
    """(min_j |x_i - y_j|^2 [Nx], min_i |y_j - x_i|^2 [Ny]) by the cdist-min formula"""
    d = torch.cdist(x, y) ** 2
    return d.min(1).values, d.min(0).values


# ---- nearest_points -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True])
def test_definition_equals_fp64_brute_force_on_the_lattice(swap):
    q, p = lattice()[:1400], lattice()[1400:]
    if swap:
        q, p = p, q
    idx, d2 = Converters.nearest_points(q, p)
    ref_idx, ref_d2 = brute_force_nearest(q, p)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(q),)
    assert np.array_equal(idx.numpy(), ref_idx)
    assert np.array_equal(d2.numpy().astype(np.float64), ref_d2)      # (every lattice d2 is exact in fp32)
    # the lattice has exact ties (about 7 % of the rows): the lower index must have won them
    d = ((q.double()[:, None, :] - p.double()[None, :, :]) ** 2).sum(-1)
    assert ((d == d.min(1, keepdim=True).values).sum(1) > 1).float().mean() > 0.05


def test_nearest_points_edges_and_bad_arguments():
    q, p = lattice()[:10], lattice()[10:30]
    idx, d2 = Converters.nearest_points(q[:0], p)
    assert idx.shape == d2.shape == (0,) and idx.dtype == torch.int32
    a = Converters.nearest_points(q, p)
    b = Converters.nearest_points(q.double(), p.double(), cell_size=0.5, route="grid")      # other dtypes: the fp32 definition
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[1].dtype == torch.float32
    same = torch.full((5, 3), 0.25)
    assert Converters.nearest_points(same, same)[0].tolist() == [0] * 5
    assert not Converters.nearest_points(q.clone().requires_grad_(True), p)[1].requires_grad
    with pytest.raises(ValueError):
        Converters.nearest_points(q, p[:0])
    for bad in (q[:, :2], q.reshape(-1), q[None]):
        with pytest.raises(ValueError):
            Converters.nearest_points(bad, p)
        with pytest.raises(ValueError):
            Converters.nearest_points(q, bad)
    with pytest.raises(ValueError):
        Converters.nearest_points(q, p, route="tree")
    for cs in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            Converters.nearest_points(q, p, cell_size=cs)


# ---- chamfer_term / chamfer_distance --------------------------------------------------------------------------------------------

def test_chamfer_term_is_the_cdist_min_formula():
    x, y = _clouds()
    mx, my = _cdist_min(x, y)
    assert abs(float(Aggregation.chamfer_term(x, y)) - float(mx.mean() + my.mean())) < 1e-13
    assert abs(float(Aggregation.chamfer_term(x, y, point_reduction="sum")) - float(mx.sum() + my.sum())) < 1e-12
    assert abs(float(Aggregation.chamfer_term(x, y, single_directional=True)) - float(mx.mean())) < 1e-13
    assert abs(float(Aggregation.chamfer_term(x, y, True, "sum")) - float(mx.sum())) < 1e-12
    loss, nn_x, nn_y = Aggregation.chamfer_term(x, y, return_indices=True)
    d = torch.cdist(x, y)
    assert torch.equal(nn_x, d.argmin(1)) and torch.equal(nn_y, d.argmin(0))      # (no ties in these clouds)
    assert Aggregation.chamfer_term(x, y, True, return_indices=True)[2] is None


def test_chamfer_term_gradcheck():
    x, y = _clouds()
    x.requires_grad_(True)
    y.requires_grad_(True)
    for single in (False, True):
        for red in ("mean", "sum"):
            assert torch.autograd.gradcheck(lambda a, b: Aggregation.chamfer_term(a, b, single, red), (x, y), eps=1e-6, atol=1e-7)
    # the gradient is the written-out one: 2 / Nx (x_i - y_nn(i)) + 2 / Ny sum_{j: nn(j) = i} (x_i - y_j)
    loss, nn_x, nn_y = Aggregation.chamfer_term(x, y, return_indices=True)
    gx, = torch.autograd.grad(loss * 3.0, x)
    want = 2 / 7 * (x - y[nn_x]).detach()
    for j in range(9):
        want[nn_y[j]] += 2 / 9 * (x[nn_y[j]] - y[j]).detach()
    assert (gx - 3.0 * want).abs().max() < 1e-13


def test_chamfer_distance_host_route_and_reductions():
    x, y = _clouds(11, 6, seed=3)
    mx, my = _cdist_min(x, y)
    loss, normals = Losses.chamfer_distance(x, y)
    assert normals is None and abs(float(loss) - float(mx.mean() + my.mean())) < 1e-13
    assert abs(float(Losses.chamfer_distance(x, y, point_reduction="sum")[0]) - float(mx.sum() + my.sum())) < 1e-12
    assert abs(float(Losses.chamfer_distance(x, y, single_directional=True)[0]) - float(mx.mean())) < 1e-13
    assert abs(float(Losses.chamfer_distance(x, y, norm=2, batch_reduction="mean")[0]) - float(loss)) == 0
    # fp32 host tensors take the definition too
    l32 = Losses.chamfer_distance(x.float(), y.float())[0]
    assert l32.dtype == torch.float32 and abs(float(l32) - float(loss)) < 1e-5
    # a batch is the mean over its pairs
    x2, y2 = _clouds(11, 6, seed=4)
    lb, _ = Losses.chamfer_distance(torch.stack((x, x2)), torch.stack((y, y2)))
    assert abs(float(lb) - 0.5 * float(loss + Losses.chamfer_distance(x2, y2)[0])) < 1e-13
    import VoGE.Losses
    assert VoGE.Losses.chamfer_distance is Losses.chamfer_distance


def test_loss_normals_is_the_written_out_formula():
    x, y = _clouds(11, 6, seed=5)
    g = torch.Generator().manual_seed(6)
    nx, ny = torch.randn(11, 3, generator=g, dtype=torch.float64), torch.randn(6, 3, generator=g, dtype=torch.float64)
    d = torch.cdist(x, y)
    ix, iy = d.argmin(1), d.argmin(0)

    def term(a, b):
        cos = (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))
        return 1 - cos.abs()

    tx, ty = term(nx, ny[ix]), term(ny, nx[iy])
    assert abs(float(Losses.chamfer_distance(x, y, nx, ny)[1]) - float(tx.mean() + ty.mean())) < 1e-12
    assert abs(float(Losses.chamfer_distance(x, y, nx, ny, point_reduction="sum")[1]) - float(tx.sum() + ty.sum())) < 1e-12
    assert abs(float(Losses.chamfer_distance(x, y, nx, ny, single_directional=True)[1]) - float(tx.mean())) < 1e-12
    nx.requires_grad_(True)
    Losses.chamfer_distance(x, y, nx, ny)[1].backward()
    assert torch.isfinite(nx.grad).all() and nx.grad.abs().max() > 0


def test_chamfer_bad_arguments_raise():
    x, y = _clouds()
    for bad in (x[:, :2], x.reshape(-1), x[None]):
        with pytest.raises(ValueError):
            Losses.chamfer_distance(bad, y)
        with pytest.raises(ValueError):
            Losses.chamfer_distance(x, bad)
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x, y[:0])
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x[:0], y)
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x, y, point_reduction="max")
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x, y, point_reduction=None)
    with pytest.raises(ValueError, match="norm"):
        Losses.chamfer_distance(x, y, norm=1)
    with pytest.raises(ValueError, match="x_lengths"):
        Losses.chamfer_distance(x, y, x_lengths=torch.tensor([7]))
    with pytest.raises(ValueError, match="weights"):
        Losses.chamfer_distance(x, y, weights=torch.ones(1))
    with pytest.raises(ValueError, match="batch_reduction"):
        Losses.chamfer_distance(x, y, batch_reduction="sum")
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x, y, x_normals=x)
    with pytest.raises(ValueError):
        Losses.chamfer_distance(x, y, x_normals=x[:3], y_normals=y)
    with pytest.raises(ValueError):
        Aggregation.chamfer_term(x, y, point_reduction="max")
    with pytest.raises(ValueError):
        Aggregation.chamfer_term(x, y[:0])


# ---- the C entries --------------------------------------------------------------------------------------------------------------

def test_chamfer_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    big = 1 << 40
    assert lib.voge_abi_version() == 7
    need = lib.voge_chamfer_workspace_bytes(100, 300)
    # both clouds' cell-ordered copies and cell ids, two count and two start arrays for the cap of 2^15 cells, the backward's accumulators
    assert need >= 400 * 20 + 4 * 32768 * 4 and need >= 400 * 24 and need % 16 == 0
    assert lib.voge_chamfer_workspace_bytes(1 << 20, 1 << 20) > lib.voge_chamfer_workspace_bytes(1 << 19, 1 << 20) > need
    for nx, ny in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 28, 5), (5, 1 << 28)):
        assert lib.voge_chamfer_workspace_bytes(nx, ny) == 0

    def nearest(q=P, Nq=100, p=P, Np=300, route=0, cell=0.0, idx=P, d2=P, ws=P, nbytes=big):
        return lib.voge_nearest_points(q, Nq, p, Np, route, cell, idx, d2, ws, nbytes, None)

    assert nearest(Nq=-1) == -1 and nearest(Np=0) == -1 and nearest(Np=-3) == -1 and nearest(Nq=1 << 28) == -1 and nearest(Np=1 << 28) == -1
    assert nearest(route=3) == -1 and nearest(route=-1) == -1
    for cell in (-1.0, float("nan"), float("inf")):
        assert nearest(cell=cell) == -1
    assert nearest(q=None) == -1 and nearest(p=None) == -1 and nearest(idx=None) == -1 and nearest(d2=None) == -1
    assert nearest(ws=None) == -1 and nearest(ws=P + 4) == -1      # scratch off the 16-byte boundary
    assert nearest(nbytes=need - 1) == -2 and nearest(nbytes=0) == -2
    assert nearest(route=1, nbytes=need - 1) == -2
    assert nearest(Nq=0, q=None, idx=None, d2=None, ws=None, nbytes=0) == 0      # no query: a success without a launch
    assert nearest(Nq=0, Np=0) == -1

    def fwd(x=P, Nx=100, y=P, Ny=300, route=0, flags=0, loss=P, nn_x=P, nn_y=P, meta=P, ws=P, nbytes=big):
        return lib.voge_chamfer_fwd(x, Nx, y, Ny, route, flags, loss, nn_x, nn_y, meta, ws, nbytes, None)

    assert fwd(Nx=0) == -1 and fwd(Ny=0) == -1 and fwd(Nx=-1) == -1 and fwd(Ny=1 << 28) == -1
    assert fwd(route=3) == -1 and fwd(flags=4) == -1 and fwd(flags=-1) == -1
    assert fwd(x=None) == -1 and fwd(y=None) == -1 and fwd(loss=None) == -1 and fwd(nn_x=None) == -1 and fwd(meta=None) == -1
    assert fwd(nn_y=None) == -1 and fwd(nn_y=None, flags=2, nbytes=16) == -2      # (single-directional: nn_y may be null)
    assert fwd(ws=None) == -1 and fwd(ws=P + 8) == -1
    assert fwd(nbytes=need - 1) == -2 and fwd(route=1, nbytes=need - 1) == -2 and fwd(route=2, nbytes=16) == -2

    def bwd(x=P, Nx=100, y=P, Ny=300, nn_x=P, nn_y=P, meta=P, g=P, flags=0, g_x=P, g_y=P, ws=P, nbytes=big):
        return lib.voge_chamfer_bwd(x, Nx, y, Ny, nn_x, nn_y, meta, g, flags, g_x, g_y, ws, nbytes, None)

    assert bwd(Nx=0) == -1 and bwd(Ny=-2) == -1 and bwd(Nx=1 << 28) == -1 and bwd(flags=8) == -1
    for name in ("x", "y", "nn_x", "nn_y", "meta", "g", "g_x", "g_y", "ws"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(nn_y=None, flags=2, nbytes=16) == -2
    assert bwd(ws=P + 4) == -1
    assert bwd(nbytes=400 * 24 - 1) == -2
