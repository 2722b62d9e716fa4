"""GPU tests of the point-cloud kernels (voge_knn_points, voge_knn_frames; an extension, the reference and the oracle have
none) and of Converters.point_cloud_converter on the device.

knn_points: the reference is the DEFINITION (the torch form of Converters.knn_points) computed on the host, once per case;
           indices and distances must be the same bits (torch.equal), under every grid.
frames:    the reference is an fp64 eigh on the same rows (knn_clouds.eigh_frames).  Angle between the normals <= 2^-16 /
           gap_rel_i radians per point (Davis-Kahan, sin theta <= 2 |dC| / gap, the fp32 covariance and the 24 Jacobi rotations
           budgeted at <= 128 roundings of <= 2^-24 tr C each); eig / tr within 2^-16.  No point is left out of any comparison.
converter: device against host: the same indices, isigma to (4 n_nearest + 32) 2^-24 relative (each side is that close to the
           fp64 formula at most; the sides share everything but the square root, the sums and the division), S to 1e-5.
The 20 000-point case spends most of its time in the host's definition (20 000 rows of 20 000 sorted columns)."""
import functools

import numpy as np
import pytest
import torch

from knn_clouds import eigh_frames, lattice, surface
from util import log_line
from voge_amd import Aggregation
from voge_amd.Converter import Converters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = {"default": None, "one_cell": 1.0, "fine": 2 / 1024, "faces": 8 / 1024}


@functools.lru_cache(maxsize=None)
def lattice_definition(k, include_self):
    return Converters.knn_points(lattice(), k, include_self=include_self)


def same_as_definition(pts, k, include_self=False, cell_size=None):
    """Device result == host definition, bit for bit -> the grid that ran."""
    ref_idx, ref_d2 = Converters.knn_points(pts.cpu(), k, include_self=include_self)
    idx, d2, grid = Converters.knn_points(pts.to(DEV), k, include_self=include_self, cell_size=cell_size, return_grid=True)
    assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(d2.cpu(), ref_d2)
    return grid


@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("k", [1, 4, 8, 32])
def test_lattice_every_grid_gives_the_definitions_bits(hip_lib, k, include_self):
    ref_idx, ref_d2 = lattice_definition(k, include_self)
    pts = lattice().to(DEV)
    grids = {}
    for name, cell_size in GRIDS.items():
        idx, d2, grids[name] = Converters.knn_points(pts, k, include_self=include_self, cell_size=cell_size, return_grid=True)
        assert torch.equal(idx.cpu(), ref_idx), name
        assert torch.equal(d2.cpu(), ref_d2), name
    assert grids["one_cell"][1:] == (1, 1, 1) and grids["fine"][1:] == (32, 32, 32) and grids["faces"] == (8 / 1024, 8, 8, 8)
    assert len({g[1:] for g in grids.values()}) == 4      # they really differed


def test_uniform_cloud(hip_lib):
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.random((20000, 3), dtype=np.float32))
    grid = same_as_definition(pts, 16)
    assert 20000 <= grid[1] * grid[2] * grid[3] <= 8 * 20000


def test_edge_cases(hip_lib):
    rng = np.random.default_rng(2)
    one = torch.tensor([[0.25, -1.0, 3.0]])
    assert same_as_definition(one, 3)[1:] == (1, 1, 1)
    same_as_definition(one, 3, include_self=True)
    five = torch.from_numpy(rng.random((5, 3), dtype=np.float32))
    same_as_definition(five, 8)
    same_as_definition(five, 8, include_self=True)
    same = torch.full((100, 3), 0.375)
    assert same_as_definition(same, 4)[1:] == (1, 1, 1)      # zero-extent box
    crowd = torch.from_numpy(np.concatenate((rng.random((2000, 3), dtype=np.float32) * 1e-3, [[100.0, 100.0, 100.0]])).astype(np.float32))
    grid = same_as_definition(crowd, 8)      # one crowded cell, and an outlier that walks empty rings to the end of the grid
    assert min(grid[1:]) > 4
    plane = torch.from_numpy(rng.random((3000, 3), dtype=np.float32))
    plane[:, 2] = 0
    assert same_as_definition(plane, 8)[3] == 1
    big = torch.from_numpy(rng.random((1501, 3), dtype=np.float32)).to(DEV)
    off = big[1:]      # rows off the 16-byte boundary
    assert off.data_ptr() % 16 != 0
    same_as_definition(off, 8)
    wide = torch.from_numpy(rng.random((1500, 6), dtype=np.float32)).to(DEV)
    view = wide[:, 1:4]      # a strided view
    assert not view.is_contiguous()
    same_as_definition(view, 8)
    same_as_definition(wide[::2, :3], 8)
    with pytest.raises(ValueError):
        bad = big.clone()
        bad[7, 0] = float("nan")
        Converters.knn_points(bad, 4)
    idx, d2 = Converters.knn_points(big[:0], 4)
    assert idx.shape == d2.shape == (0, 4) and idx.is_cuda


def test_two_calls_return_identical_bits(hip_lib):
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(rng.random((30000, 3), dtype=np.float32)).to(DEV)
    a = Converters.knn_points(pts, 16, include_self=True)
    b = Converters.knn_points(pts, 16, include_self=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[0][:, 0] == torch.arange(30000, device=DEV)).all() and (a[1][:, 1:] >= a[1][:, :-1]).all()


def _axis2(quats):
    return Aggregation.quaternion_to_matrix(quats.double().cpu())[:, :, 2].numpy()


@pytest.mark.parametrize("n, k", [(40, 16), (24, 8)])
def test_frames_against_fp64_eigh(hip_lib, n, k):
    pts = surface(n)
    N = len(pts)
    idx, _ = Converters.knn_points(pts, k, include_self=True)
    lam, nrm, _ = eigh_frames(pts, idx)
    tr = lam.sum(1)
    gap = (lam[:, 1] - lam[:, 0]) / tr
    assert gap.min() >= (0.157 if n == 40 else 0.0926)      # (what the bound below divides by: every point has a clear normal)
    dpts, didx = pts.to(DEV), idx.to(DEV)
    quats, eig = Converters.point_cloud_frames(dpts, didx)
    assert quats.is_cuda and quats.dtype == eig.dtype == torch.float32 and quats.shape == (N, 4) and eig.shape == (N, 3)
    got = _axis2(quats)
    angle = np.arcsin(np.linalg.norm(np.cross(got, nrm), axis=1).clip(0, 1))
    ratio = (angle * gap / 2.0 ** -16).max()
    eig_err = (np.abs(eig.double().cpu().numpy() - lam) / tr[:, None]).max()
    log_line(f"[knn] frames {n}^2 k={k}: normal angle / (2^-16 / gap) max {ratio:.4f} (angle max {angle.max():.3e} rad), "
             f"eig / tr error max {eig_err / 2.0 ** -16:.4f} x 2^-16")
    assert (angle <= 2.0 ** -16 / gap).all()
    assert eig_err <= 2.0 ** -16
    q = quats.double().cpu()
    assert (q.norm(dim=1) - 1).abs().max() <= 1e-6 and (q[:, 0] >= 0).all()
    # the default sign, where the two largest |components| of the fp64 normal differ by more than 1e-3
    a = np.sort(np.abs(nrm), axis=1)
    clear = a[:, 2] - a[:, 1] > 1e-3
    assert clear.sum() > N // 2
    big = np.take_along_axis(got, np.abs(nrm).argmax(1)[:, None], 1)[:, 0]
    assert (big[clear] > 0).all()
    # toward: [3] and [N,3]; the sensor is far off every tangent plane
    sensor = torch.tensor([0.3, -0.2, 5.0])
    per_point = torch.where((torch.arange(N) % 2 == 0)[:, None], sensor, -sensor).contiguous()
    for toward in (sensor, -sensor, per_point):
        q2, e2 = Converters.point_cloud_frames(dpts, didx, toward.to(DEV))
        n2 = _axis2(q2)
        assert ((n2 * (toward.double().numpy() - pts.double().numpy())).sum(1) > 0).all()
        assert (np.abs((n2 * got).sum(1)) > 1 - 1e-6).all() and torch.equal(e2, eig)
    # the frame is a rotation whose first axis is the eigenvector of the largest eigenvalue
    R = Aggregation.quaternion_to_matrix(quats.double().cpu())
    tan = eigh_frames(pts, idx)[2]
    gap2 = (lam[:, 2] - lam[:, 1]) / tr
    t_angle = np.arcsin(np.linalg.norm(np.cross(R[:, :, 0].numpy(), tan), axis=1).clip(0, 1))
    ok = gap2 > 1e-3
    assert (t_angle[ok] <= 2.0 ** -16 / gap2[ok] + 2.0 ** -16 / gap[ok]).all()


def test_frames_degenerate_and_foreign_indices(hip_lib):
    identity = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV)
    line = torch.tensor([[i / 1024, 3 * i / 1024, 0.25 - 2 * i / 1024] for i in range(12)], dtype=torch.float32, device=DEV)
    idx = torch.arange(12, dtype=torch.int32, device=DEV)[None].expand(12, 12).contiguous()
    quats, eig = Converters.point_cloud_frames(line, idx)
    assert torch.equal(quats, identity.expand(12, 4)) and (eig[:, 2] > 0).all()
    pts = surface(24)
    full_idx, _ = Converters.knn_points(pts, 8, include_self=True)
    idx = full_idx.clone()
    idx[0, 2:] = -1                        # two valid entries
    idx[1, :] = -1                         # none
    idx[2, 1:] = 576                       # one valid entry; the others point just past the end
    idx[3, 4:] = -7                        # four valid entries: a frame
    idx[4, 5:] = 2 ** 31 - 1               # far past the end
    idx[5, 6:] = -2 ** 31
    quats, eig = Converters.point_cloud_frames(pts.to(DEV), idx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(quats[:3], identity.expand(3, 4)) and torch.isfinite(quats).all() and torch.isfinite(eig).all()
    full, full_eig = Converters.point_cloud_frames(pts.to(DEV), full_idx.to(DEV))
    assert torch.equal(quats[6:], full[6:]) and torch.equal(eig[6:], full_eig[6:])
    # the skipped entries are ignored: rows 3 .. 5 are the frames of the rows cut to their valid entries, bit for bit
    for row, keep in ((3, 4), (4, 5), (5, 6)):
        cut_q, cut_e = Converters.point_cloud_frames(pts.to(DEV), full_idx[:, :keep].contiguous().to(DEV))
        assert torch.equal(quats[row], cut_q[row]) and torch.equal(eig[row], cut_e[row])
        assert not torch.equal(quats[row], identity)


def test_converter_on_the_device_equals_the_host(hip_lib):
    pts = surface(40)
    n_nearest, flatten = 4, 4.0
    toward = torch.tensor([0.0, 0.0, 5.0])
    hv, hs, hq = Converters.point_cloud_converter(pts, n_nearest=n_nearest, oriented=True, flatten=flatten, toward=toward)
    dv, ds, dq = Converters.point_cloud_converter(pts.to(DEV), n_nearest=n_nearest, oriented=True, flatten=flatten, toward=toward.to(DEV))
    assert dv.is_cuda and ds.is_cuda and dq.is_cuda and ds.dtype == dq.dtype == torch.float32
    for k in (n_nearest, 16):
        assert torch.equal(Converters.knn_points(pts.to(DEV), k, include_self=True)[0].cpu(), Converters.knn_points(pts, k, include_self=True)[0])
    h_iso = Converters.point_cloud_converter(pts, n_nearest=n_nearest)[1]
    d_iso = Converters.point_cloud_converter(pts.to(DEV), n_nearest=n_nearest)[1]
    rel = ((d_iso.cpu().double() - h_iso.double()).abs() / h_iso.double()).max()
    log_line(f"[knn] converter isigma device vs host: max relative difference {rel:.3e}")
    assert rel <= (4 * n_nearest + 32) * 2.0 ** -24
    assert torch.equal(ds[:, 0], d_iso) and torch.equal(ds[:, 2], d_iso * flatten)
    S_h = Aggregation.oriented_sigma(hs, hq).double()
    S_d = Aggregation.oriented_sigma(ds, dq).double().cpu()
    s_rel = ((S_d - S_h).abs().amax((1, 2)) / (h_iso.double() * flatten)).max()
    log_line(f"[knn] converter oriented S device vs host: max relative difference {s_rel:.3e}")
    assert s_rel <= 1e-5

    # the output renders, and its Gaussians' own normals are the camera-facing third axes
    from voge_amd.Meshes import OrientedGaussianMeshes
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, gaussian_normals, to_white_background
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    cams = PerspectiveCameras(focal_length=80.0, principal_point=((32.0, 32.0),), image_size=((64, 64),), device=DEV)
    R, T = look_at_view_transform(3.0, 20.0, 30.0, device=DEV)
    cams.R, cams.T = R, T
    renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(64, 64), max_assign=16, max_point_per_bin=-1)).to(DEV)
    gm = OrientedGaussianMeshes(dv, ds, dq).to(DEV)
    with torch.no_grad():
        frag = renderer(gm, R=R, T=T)
        colors = torch.rand((len(pts), 3), device=DEV)
        img = to_white_background(frag, colors)
        centres = cams.get_camera_center()
        table = gaussian_normals(ds, dq, dv, centres)
    assert img.shape[-3:] == (64, 64, 3) and torch.isfinite(img).all() and bool((frag.valid_num > 0).any())
    axis = Aggregation.quaternion_to_matrix(dq)[:, :, 2]
    facing = torch.where(((axis * (dv - centres[0])).sum(-1) > 0)[:, None], -axis, axis)
    assert table.shape == (len(pts), 3) and (table - facing).abs().max() <= 1e-5
