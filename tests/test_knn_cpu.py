"""CPU tests of the point-cloud primitives: the torch definitions of Converters.knn_points / point_cloud_frames /
point_cloud_converter against fp64 references made here, and the argument checks of the three C entries (the library loads
without a GPU: anything that reached HIP would fail differently)."""
import math
import os

import numpy as np
import pytest
import torch

from knn_clouds import brute_force_knn, eigh_frames, isigma_reference, lattice, surface, surface_normals
from voge_amd import Aggregation
from voge_amd.Converter import Converters


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- knn_points ---------------------------------------------------------------------------------------------------------------

def test_lattice_has_ties_and_duplicates():
    """The tie-break cloud is what the tests below take it for."""
    idx, d2 = brute_force_knn(lattice(), 8, False)
    assert (d2[:, 1:] == d2[:, :-1]).any(1).mean() > 0.7
    assert len(np.unique(lattice().numpy(), axis=0)) < 3000


@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_definition_equals_fp64_brute_force_on_the_lattice(k, include_self):
    idx, d2 = Converters.knn_points(lattice(), k, include_self=include_self)
    ref_idx, ref_d2 = brute_force_knn(lattice(), k, include_self)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (3000, k)
    assert np.array_equal(idx.numpy(), ref_idx)
    assert np.array_equal(d2.numpy().astype(np.float64), ref_d2)      # (every lattice d2 is exact in fp32)
    if include_self:
        assert (d2[:, 0] == 0).all()


def test_padding_of_short_rows():
    pts = lattice()[:5]
    idx, d2 = Converters.knn_points(pts, 8)
    ref_idx, ref_d2 = brute_force_knn(pts, 8, False)
    assert np.array_equal(idx.numpy(), ref_idx) and np.array_equal(d2.numpy().astype(np.float64), ref_d2)
    assert (idx[:, 4:] == -1).all() and torch.isinf(d2[:, 4:]).all() and (idx[:, :4] >= 0).all()
    idx, d2 = Converters.knn_points(pts, 8, include_self=True)
    assert (idx[:, 0] == torch.arange(5)).all() and (idx[:, 5:] == -1).all() and (idx[:, :5] >= 0).all()
    idx, d2 = Converters.knn_points(pts[:1], 3)
    assert idx.tolist() == [[-1, -1, -1]] and torch.isinf(d2).all()
    idx, d2 = Converters.knn_points(pts[:1], 3, include_self=True)
    assert idx.tolist() == [[0, -1, -1]] and d2[0, 0] == 0 and torch.isinf(d2[0, 1:]).all()
    idx, d2 = Converters.knn_points(pts[:0], 3)
    assert idx.shape == d2.shape == (0, 3)


def test_other_dtypes_take_the_fp32_definition():
    a = Converters.knn_points(lattice()[:200], 4)
    b = Converters.knn_points(lattice()[:200].double(), 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[1].dtype == torch.float32


def test_bad_arguments_raise():
    pts = lattice()[:10].clone()
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            Converters.knn_points(pts, k)
    for bad in (pts[:, :2], pts.reshape(-1), pts[None]):
        with pytest.raises(ValueError):
            Converters.knn_points(bad, 2)
    for v in (float("nan"), float("inf")):
        q = pts.clone()
        q[3, 1] = v
        with pytest.raises(ValueError):
            Converters.knn_points(q, 2)


def test_grid_choice_respects_the_caps():
    from voge_amd import ops
    # default: about 2 N cells; a request goes through the same enlargement
    cell, gx, gy, gz = ops.knn_grid([0, 0, 0], [1, 1, 1], 4000)
    assert 4000 <= gx * gy * gz <= 16000 and gx == gy == gz
    assert ops.knn_grid([0, 0, 0], [63 / 1024] * 3, 3000, 2 / 1024)[1:] == (32, 32, 32)
    assert ops.knn_grid([0, 0, 0], [63 / 1024] * 3, 3000, 8 / 1024)[1:] == (8, 8, 8)
    assert ops.knn_grid([0, 0, 0], [63 / 1024] * 3, 3000, 1.0)[1:] == (1, 1, 1)
    for lo, hi, n, cs in (([0, 0, 0], [1, 1, 1], 10, 1e-6), ([0, 0, 0], [1e3, 1e-3, 0], 500, None), ([5, 5, 5], [5, 5, 5], 100, None),
                          ([0, 0, 0], [1, 1, 0], 2000, None), ([-1e30] * 3, [1e30] * 3, 7, 1e-30)):
        cell, gx, gy, gz = ops.knn_grid(lo, hi, n, cs)
        assert cell > 0 and math.isfinite(cell) and np.float32(cell) == cell
        assert 1 <= min(gx, gy, gz) and max(gx, gy, gz) <= 1024 and gx * gy * gz <= max(8 * n, 1 << 15)
        for g, l, h in zip((gx, gy, gz), lo, hi):
            assert g > (h - l) / cell - 1e-9 * g      # the grid covers the box
    assert ops.knn_grid([0, 0, 0], [1, 1, 0], 2000)[3] == 1
    with pytest.raises(ValueError):
        ops.knn_grid([0, 0, 0], [1, 1, 1], 10, 0.0)
    idx, d2, grid = Converters.knn_points(lattice()[:50], 2, cell_size=8 / 1024, return_grid=True)
    assert len(grid) == 4 and grid[0] == 8 / 1024


# ---- point_cloud_frames -------------------------------------------------------------------------------------------------------

def _normals_of(quats):
    return Aggregation.quaternion_to_matrix(quats)[:, :, 2]


def test_frames_definition_on_the_surface():
    pts = surface(40)
    idx, _ = Converters.knn_points(pts, 16, include_self=True)
    p64 = pts.double()
    quats, eig = Converters.point_cloud_frames(p64, idx)
    assert quats.dtype == torch.float64 and quats.shape == (1600, 4) and eig.shape == (1600, 3)
    R = Aggregation.quaternion_to_matrix(quats)
    eye = torch.eye(3, dtype=torch.float64)
    assert (R.transpose(1, 2) @ R - eye).abs().max() < 1e-12 and (torch.linalg.det(R) - 1).abs().max() < 1e-12
    assert (quats.norm(dim=1) - 1).abs().max() < 1e-12 and (quats[:, 0] >= 0).all()
    assert (eig[:, 0] <= eig[:, 1]).all() and (eig[:, 1] <= eig[:, 2]).all()
    n = R[:, :, 2].numpy()
    cos = np.abs((n * surface_normals(pts)).sum(1)).clip(0, 1)
    angle = np.degrees(np.arccos(cos))
    print(f"angle to the analytic normal: max {angle.max():.3f} deg, median {np.median(angle):.3f} deg")
    assert angle.max() <= 6.5
    # the frame is that of the fp64 eigenvectors of the same rows
    lam, nrm, tan = eigh_frames(pts, idx)
    assert np.abs(eig.numpy() - lam).max() < 1e-15
    assert np.abs(np.abs((n * nrm).sum(1)) - 1).max() < 1e-12 and np.abs(np.abs((R[:, :, 0].numpy() * tan).sum(1)) - 1).max() < 1e-12
    # default sign: the component of largest magnitude is positive
    big = np.take_along_axis(n, np.abs(n).argmax(1)[:, None], 1)
    assert (big > 0).all()
    # toward, [3] and [N,3]
    sensor = torch.tensor([0.3, -0.2, 5.0], dtype=torch.float64)
    for toward in (sensor, -sensor, sensor[None].expand(1600, 3).contiguous(),
                   torch.where((torch.arange(1600) % 2 == 0)[:, None], sensor, -sensor)):
        q2, e2 = Converters.point_cloud_frames(p64, idx, toward)
        n2 = _normals_of(q2)
        assert ((n2 * (toward - p64)).sum(1) >= 0).all()
        assert ((n2 * torch.from_numpy(n)).sum(1).abs() > 1 - 1e-12).all() and torch.equal(e2, eig)
        R2 = Aggregation.quaternion_to_matrix(q2)
        assert (torch.linalg.det(R2) - 1).abs().max() < 1e-12
    # fp32 points give fp32 frames of the same definition
    q32, e32 = Converters.point_cloud_frames(pts, idx)
    assert q32.dtype == torch.float32 and (q32.double() - quats).abs().max() < 1e-6


def test_frames_degenerate_rows_get_the_identity():
    identity = torch.tensor([1.0, 0.0, 0.0, 0.0])
    line = torch.tensor([[i / 1024, 3 * i / 1024, 0.25 - 2 * i / 1024] for i in range(12)], dtype=torch.float32)      # collinear lattice points
    idx = torch.arange(12, dtype=torch.int32)[None].expand(12, 12).contiguous()
    quats, eig = Converters.point_cloud_frames(line, idx)
    assert torch.equal(quats, identity.expand(12, 4)) and (eig[:, 2] > 0).all() and (eig[:, 1] <= 1e-6 * eig[:, 2]).all()
    pts = surface(24)
    idx, _ = Converters.knn_points(pts, 8, include_self=True)
    idx = idx.clone()
    idx[0, 2:] = -1           # two valid entries
    idx[1, :] = -1            # none
    idx[2, 1:] = 576          # one valid entry; the others point past the end
    idx[3, 4:] = -7           # four valid entries: a frame
    quats, eig = Converters.point_cloud_frames(pts, idx)
    assert torch.equal(quats[:3], identity.expand(3, 4)) and not torch.equal(quats[3], identity)
    assert torch.isfinite(eig).all() and torch.isfinite(quats).all()
    full, _ = Converters.point_cloud_frames(pts, Converters.knn_points(pts, 8, include_self=True)[0])
    assert torch.equal(quats[4:], full[4:])


# ---- point_cloud_converter ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_nearest, percentage, thr_max", [(4, 0.5, 2), (7, 0.75, 1.2)])
def test_converter_isigma_is_the_reference_formula(n_nearest, percentage, thr_max):
    for pts in (surface(40), lattice()):
        verts, isigma, none = Converters.point_cloud_converter(pts, percentage=percentage, n_nearest=n_nearest, thr_max=thr_max)
        assert none is None and verts is pts and isigma.shape == (len(pts),) and isigma.dtype == torch.float32
        idx, _ = Converters.knn_points(pts, n_nearest, include_self=True)
        ref = isigma_reference(pts, idx, percentage, thr_max)
        rel = np.abs(isigma.numpy().astype(np.float64) - ref) / ref
        bound = (4 * n_nearest + 32) * 2.0 ** -24
        print(f"isigma: max relative error {rel.max():.3e}, bound {bound:.3e}")
        assert rel.max() <= bound


def test_converter_numpy_in_numpy_out():
    v, s, r = Converters.point_cloud_converter(surface(24).numpy())
    assert isinstance(v, np.ndarray) and isinstance(s, np.ndarray) and r is None
    assert np.array_equal(s, Converters.point_cloud_converter(surface(24))[1].numpy())


def test_converter_oriented_output():
    pts = surface(40)
    flatten = 4.0
    toward = torch.tensor([0.0, 0.0, 5.0])
    verts, scales, quats = Converters.point_cloud_converter(pts, oriented=True, n_frame=16, flatten=flatten, toward=toward)
    isigma = Converters.point_cloud_converter(pts)[1]
    assert scales.shape == (1600, 3) and quats.shape == (1600, 4) and scales.dtype == quats.dtype == torch.float32
    assert torch.equal(scales[:, 0], isigma) and torch.equal(scales[:, 1], isigma) and torch.equal(scales[:, 2], isigma * flatten)
    idx, _ = Converters.knn_points(pts, 16, include_self=True)
    nrm = torch.from_numpy(eigh_frames(pts, idx)[1])
    want = isigma.double()[:, None, None] * (torch.eye(3, dtype=torch.float64) + (flatten - 1) * nrm[:, :, None] * nrm[:, None, :])
    S = Aggregation.oriented_sigma(scales, quats).double()
    rel = ((S - want).abs().amax((1, 2)) / (isigma.double() * flatten)).max()
    print(f"oriented S: max relative error {rel:.3e}")
    assert rel <= 1e-5
    cam = torch.tensor([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]])
    gn = Aggregation.gaussian_normals(scales, quats, verts, cam).reshape(2, 1600, 3).double()
    assert ((gn * nrm[None]).sum(-1).abs() >= 1 - 1e-5).all()
    assert (gn[0, :, 2] > 0).all() and (gn[1, :, 2] < 0).all()      # camera-facing
    assert ((Aggregation.quaternion_to_matrix(quats)[:, :, 2] * (toward - pts)).sum(1) > 0).all()
    # a collinear cloud: isotropic scales with the identity
    line = torch.tensor([[i / 1024, 3 * i / 1024, 0.25 - 2 * i / 1024] for i in range(40)], dtype=torch.float32)
    v, s, q = Converters.point_cloud_converter(line, oriented=True, n_frame=8)
    assert (q == torch.tensor([1.0, 0, 0, 0])).all() and torch.equal(s[:, 0], s[:, 2]) and torch.equal(s[:, 1], s[:, 2])


# ---- the C entries --------------------------------------------------------------------------------------------------------------

def test_knn_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    big = 1 << 30

    def points(N=100, k=4, cell=0.1, g=(8, 8, 8), ws=big, lo=(0.0, 0.0, 0.0)):
        return lib.voge_knn_points(P, N, k, 0, *lo, cell, *g, P, P, P, ws, None)

    assert lib.voge_abi_version() == 7
    assert points(k=0) == -1 and points(k=-3) == -1 and points(k=33) == -3
    assert points(N=-1) == -1
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert points(cell=cell) == -1
    assert points(lo=(float("nan"), 0.0, 0.0)) == -1
    for g in ((1025, 1, 1), (1, 1, 1025), (0, 8, 8), (8, -1, 8), (64, 64, 64)):      # over an axis' cap, empty, over max(8 N, 2^15)
        assert points(g=g) == -1
        assert lib.voge_knn_workspace_bytes(100, *g) == 0
    need = lib.voge_knn_workspace_bytes(100, 8, 8, 8)
    assert need >= 100 * 16 + 100 * 4 + 2 * 512 * 4
    assert points(ws=need - 1) == -2 and points(ws=16) == -2
    assert lib.voge_knn_points(None, 100, 4, 0, 0.0, 0.0, 0.0, 0.1, 8, 8, 8, P, P, P, big, None) == -1
    assert lib.voge_knn_points(P, 100, 4, 0, 0.0, 0.0, 0.0, 0.1, 8, 8, 8, P, P, P + 4, big, None) == -1      # scratch off the 16-byte boundary
    assert lib.voge_knn_workspace_bytes(-1, 8, 8, 8) == 0
    assert lib.voge_knn_workspace_bytes(1 << 20, 128, 128, 128) > lib.voge_knn_workspace_bytes(1 << 20, 64, 64, 64) > 0
    # an empty cloud is a success without a launch
    assert lib.voge_knn_points(None, 0, 4, 0, 0.0, 0.0, 0.0, 0.1, 1, 1, 1, None, None, None, 0, None) == 0

    def frames(N=100, k=8, pts=P, idx=P, q=P, e=P):
        return lib.voge_knn_frames(pts, idx, N, k, None, 0, q, e, None)

    assert frames(k=0) == -1 and frames(k=33) == -3 and frames(N=-1) == -1
    assert frames(pts=None) == -1 and frames(idx=None) == -1 and frames(q=None) == -1 and frames(e=None) == -1
    assert frames(N=0, pts=None, idx=None, q=None, e=None) == 0
