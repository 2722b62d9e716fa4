"""Mesh / point-cloud -> isotropic Gaussian converters (VoGE/Converter/Converters.py:10-139).

The isotropic rule everywhere: a vertex whose neighbours are at mean distance l gets
sigma = l^2 / (2 ln(1/percentage)) + 1e-10 and the renderer's input is 1/sigma."""
import numpy as np
import torch

from ..Meshes import GaussianMeshes


def get_vert_edge_length(verts, faces, default_l=1e-3):
    """Mean distance from every vertex to the distinct vertices it shares a face with
    (Converters.py:10-32); vertices in no face get default_l."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces)[:, :3].astype(np.int64)
    pairs = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [0, 2]]], axis=0)
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    d = np.linalg.norm(verts[pairs[:, 0]] - verts[pairs[:, 1]], axis=1)
    total = np.zeros(len(verts))
    deg = np.zeros(len(verts))
    for col in (0, 1):
        np.add.at(total, pairs[:, col], d)
        np.add.at(deg, pairs[:, col], 1)
    out = np.full(len(verts), float(default_l))
    touched = np.zeros(len(verts), bool)
    touched[faces.ravel()] = True
    has = deg > 0
    out[has] = total[has] / deg[has]
    out[touched & ~has] = np.nan   # degenerate face (all three indices equal): 0/0 in the reference too
    return out


def _iso_from_length(length, percentage):
    return 1.0 / (length ** 2 / (2 * np.log(1 / percentage)) + 1e-10)


def naive_vertices_converter(vertices, faces, percentage=0.5, max_sig_rate=-1):
    """One isotropic Gaussian per mesh vertex (Converters.py:74-95) -> (verts, isigma, None)."""
    is_torch = torch.is_tensor(vertices)
    if is_torch:
        vertices, faces = vertices.numpy(), faces.numpy()
    default_l = 10 * np.sum((vertices.max(axis=0) - vertices.min(axis=0)) ** 2) ** 0.5 / vertices.shape[0]
    isigma = _iso_from_length(get_vert_edge_length(vertices, faces, default_l), percentage)
    if max_sig_rate > 0:
        isigma = np.minimum(isigma, np.mean(isigma) * max_sig_rate)
    if is_torch:
        return torch.from_numpy(vertices).type(torch.float32), torch.from_numpy(isigma).type(torch.float32), None
    return vertices, isigma, None


def matrix_to_quaternion(rot):
    """[n,3,3] rotation matrices -> [n,4] unit quaternions (w, x, y, z), numpy fp64: the eigenvector of the largest eigenvalue of
    the symmetric 4x4 matrix K(R) (Bar-Itzhack), with w >= 0.  For a proper rotation Aggregation.quaternion_to_matrix gives the
    matrix back; an improper or non-orthogonal matrix gets the nearest rotation's quaternion."""
    m = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    k = np.empty((m.shape[0], 4, 4))
    k[:, 0, 0] = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    k[:, 0, 1] = k[:, 1, 0] = m[:, 2, 1] - m[:, 1, 2]
    k[:, 0, 2] = k[:, 2, 0] = m[:, 0, 2] - m[:, 2, 0]
    k[:, 0, 3] = k[:, 3, 0] = m[:, 1, 0] - m[:, 0, 1]
    k[:, 1, 1] = m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2]
    k[:, 1, 2] = k[:, 2, 1] = m[:, 0, 1] + m[:, 1, 0]
    k[:, 1, 3] = k[:, 3, 1] = m[:, 0, 2] + m[:, 2, 0]
    k[:, 2, 2] = m[:, 1, 1] - m[:, 0, 0] - m[:, 2, 2]
    k[:, 2, 3] = k[:, 3, 2] = m[:, 1, 2] + m[:, 2, 1]
    k[:, 3, 3] = m[:, 2, 2] - m[:, 0, 0] - m[:, 1, 1]
    q = np.linalg.eigh(k / 3.0)[1][:, :, -1]
    return q * np.where(q[:, :1] < 0, -1.0, 1.0)


def normal_mesh_converter(vertices, faces, normals, percentage=0.5, shape_ratio=0.5, max_sig_rate=-1, auto_fix=True, oriented=False):
    """One Gaussian per mesh vertex, flattened along the vertex normal (Converters.py:35-71): in the frame whose third
    axis is the normal, Sigma^-1 = s * diag(1, 1, shape_ratio) with s the isotropic scale of naive_vertices_converter;
    the frame is look_at_rotation(-normal) (third column = normal; PyTorch3D's convention, cameras.look_at_rotation
    here).  Returns (verts, isigma [n,3,3], None); oriented=True: (verts, scales [n,3], quats [n,4]) -- the same frame and the
    same (s, s, shape_ratio * s) without multiplying them out (Meshes.OrientedGaussianMeshes; Aggregation.oriented_sigma gives
    isigma back), degenerate frames becoming (s, s, s) with the identity under auto_fix."""
    from ..cameras import look_at_rotation
    if oriented and max_sig_rate > 0:
        raise ValueError("max_sig_rate clamps the matrix elementwise, which has no oriented form: use oriented=False")
    is_torch = torch.is_tensor(vertices)
    if is_torch:
        vertices, faces = vertices.numpy(), faces.numpy()
    else:
        normals = torch.from_numpy(np.asarray(normals))
    default_l = 10 * np.sum((vertices.max(axis=0) - vertices.min(axis=0)) ** 2) ** 0.5 / vertices.shape[0]
    base = _iso_from_length(get_vert_edge_length(vertices, faces, default_l), percentage)
    n2 = (normals ** 2).sum(-1)
    assert torch.max(n2) < 1.1 and torch.min(n2) > 0.9
    shape = np.array([[1, 0, 0], [0, 1, 0], [0, 0, shape_ratio]])[None] * base.reshape(-1, 1, 1)
    rot = look_at_rotation(-normals.type(torch.float32)).numpy()
    if oriented:
        scales = base.reshape(-1, 1) * np.array([[1.0, 1.0, shape_ratio]])
        quats = matrix_to_quaternion(rot)
        # (look_at_rotation's frames are right-handed rotations, or all zeros when the normal is parallel to its up axis)
        flat = np.linalg.det(rot) < 0.5
        if auto_fix:
            scales[flat] = base[flat].reshape(-1, 1)
            quats[flat] = np.array([1.0, 0.0, 0.0, 0.0])
        if is_torch:
            return (torch.from_numpy(vertices).type(torch.float32), torch.from_numpy(scales).type(torch.float32),
                    torch.from_numpy(quats).type(torch.float32))
        return vertices, scales, quats
    isigma = rot @ shape @ rot.transpose(0, 2, 1)
    if auto_fix:
        flat = np.linalg.det(isigma) == 0
        isigma[flat] = np.eye(3)[None] * base[flat].reshape(-1, 1, 1)
    if max_sig_rate > 0:
        isigma = np.minimum(isigma, np.mean(isigma) * max_sig_rate)
    if is_torch:
        return torch.from_numpy(vertices).type(torch.float32), torch.from_numpy(isigma).type(torch.float32), None
    return vertices, isigma, None


def fixed_pointcloud_converter(points, radius, percentage=0.5):
    """Isotropic Gaussians of a given radius per point (Converters.py:125-139)."""
    to_np = not torch.is_tensor(points)
    if to_np:
        points = torch.from_numpy(np.asarray(points))
        if not isinstance(radius, float):
            radius = torch.from_numpy(np.asarray(radius))
    isigma = torch.ones(points.shape[0]) / ((radius ** 2) / (2 * np.log(1 / percentage)) + 1e-10)
    return (points.numpy(), isigma.numpy(), None) if to_np else (points, isigma, None)


def naive_point_cloud_converter(points, percentage=0.5, n_nearest=4, thr_max=2, chunk=4096):
    """Isotropic Gaussians from the mean distance to the n nearest neighbours, each neighbour
    distance capped at thr_max x their mean (Converters.py:98-122; note the 4 ln(1/p) divisor)."""
    to_np = not torch.is_tensor(points)
    pts = torch.as_tensor(points).type(torch.float32)
    out = []
    with torch.no_grad():
        for s in range(0, pts.shape[0], chunk):
            dist = torch.cdist(pts[s:s + chunk], pts)
            top = torch.topk(dist, k=n_nearest, dim=1, largest=False)[0]
            length = torch.min(top, top.mean(dim=1, keepdim=True) * thr_max).mean(dim=1)
            out.append(length ** 2 / (4 * np.log(1 / percentage)))
    isigma = 1 / (torch.cat(out) + 1e-8)
    return (pts.numpy(), isigma.numpy(), None) if to_np else (pts, isigma, None)


KNN_MAX_K = 32


def _on_hip(t):
    return t.is_cuda and t.dtype == torch.float32


def knn_points(points, k, include_self=False, cell_size=None, return_grid=False):
    """Exact k nearest neighbours of every point among the points of its own cloud -> (idx [N,k] int32, d2 [N,k] fp32); an
    extension (the reference searches only inside naive_point_cloud_converter, Converters.py:98-122, over all N^2 pairs).

    d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j, dy, dz, every operation a single fp32 operation.  Row i holds the k
    lexicographically smallest (d2, j) over all j, ascending, without j = i unless include_self: an exact tie keeps the lower
    index, a duplicate of point i at another index is a neighbour at distance 0.  A row with fewer than k candidates is padded
    with idx -1 and d2 +inf.  1 <= k <= 32; non-finite coordinates raise ValueError; coordinates whose d2 overflows fp32 are out
    of contract.

    This torch form (rows of the N x N matrix in chunks, +inf on the diagonal when the point itself is left out, a stable sort)
    is the definition, and what host tensors and other dtypes (cast to fp32) get.  fp32 points on a HIP device go to the grid
    search of ops.knn_points, which returns the same bits whatever grid it uses; cell_size asks it for a cell edge of that size
    instead of the default (about 2 N cells over the bounding box), and return_grid=True appends the grid (cell, gx, gy, gz)
    that ran, or would run, to the result."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("knn_points: points must be a [N,3] tensor")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_points: k must be in 1 .. {KNN_MAX_K}, got {k}")
    from .. import ops
    if _on_hip(points):
        idx, d2, grid = ops.knn_points(points, k, include_self, cell_size)
        return (idx, d2, grid) if return_grid else (idx, d2)
    pts = points.detach().to(torch.float32)
    N = pts.shape[0]
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("knn_points: points hold non-finite coordinates")
    idx = torch.full((N, k), -1, dtype=torch.int32, device=pts.device)
    d2 = torch.full((N, k), float("inf"), dtype=torch.float32, device=pts.device)
    have = min(k, N if include_self else N - 1)
    if have > 0:
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        chunk = max(1, (1 << 24) // N)
        for s in range(0, N, chunk):
            e = min(s + chunk, N)
            dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
            d = (dx * dx + dy * dy) + dz * dz
            if not include_self:
                d[torch.arange(e - s), torch.arange(s, e)] = float("inf")
            val, order = torch.sort(d, dim=1, stable=True)
            d2[s:e, :have] = val[:, :have]
            idx[s:e, :have] = order[:, :have].to(torch.int32)
    if return_grid:
        grid = (1.0, 1, 1, 1)
        if N > 0:
            grid = ops.knn_grid(pts.amin(0).tolist(), pts.amax(0).tolist(), N, cell_size)
        return idx, d2, grid
    return idx, d2


def nearest_points(queries, points, cell_size=None, route=None):
    """The nearest point of `points` [Np,3] for every row of `queries` [Nq,3] -> (idx [Nq] int32, d2 [Nq] fp32); an extension
    (knn_points searches inside one cloud; this is the search between two that the chamfer distance needs).

    d2 = (dx*dx + dy*dy) + dz*dz, every operation a single fp32 operation -- knn_points' convention --, and a query gets the
    lexicographically smallest (d2, index) over the points: an exact tie keeps the lower index.  Nq == 0 gives empty outputs,
    Np == 0 raises ValueError.  Not differentiable.

    The torch form (Aggregation.nearest_rows on the fp32 values: rows of the Nq x Np matrix in chunks) is the definition, and what
    host tensors and other dtypes (cast to fp32) get.  fp32 tensors on a HIP device go to the kernels of ops.nearest_points, which
    return the same bits: route "brute" (all pairs, the points tiled through LDS), "grid" (a uniform grid over both clouds, chosen
    on the device: no host synchronisation, capturable) or None (chosen by Nq Np); cell_size asks the grid for a cell of that
    edge.  Both arguments are ignored by the definition, which validates them all the same."""
    if not torch.is_tensor(queries) or not torch.is_tensor(points) or queries.dim() != 2 or points.dim() != 2 \
            or queries.shape[1] != 3 or points.shape[1] != 3:
        raise ValueError("nearest_points: queries [Nq,3] and points [Np,3] tensors expected")
    if points.shape[0] == 0:
        raise ValueError("nearest_points: points is empty")
    from .. import Aggregation, ops
    if route not in ops.CHAMFER_ROUTES:
        raise ValueError(f"nearest_points: route must be None, 'brute' or 'grid', got {route!r}")
    if cell_size is not None and not (0.0 < float(cell_size) < 3.0e38):
        raise ValueError(f"nearest_points: cell_size must be a positive finite fp32 number, got {cell_size}")
    if _on_hip(queries) and _on_hip(points) and queries.device == points.device:
        return ops.nearest_points(queries.detach(), points.detach(), cell_size, route)
    idx, d2 = Aggregation.nearest_rows(queries.detach().to(torch.float32), points.detach().to(torch.float32).to(queries.device))
    return idx.to(torch.int32), d2


def _rotation_to_quaternion(R):
    """[n,3,3] rotations -> [n,4] unit quaternions (w, x, y, z) with w >= 0, in R's dtype (the branch on the largest of the
    trace and the diagonal entries, so that no branch divides by a small number)."""
    m = [[R[:, i, j] for j in range(3)] for i in range(3)]
    tr = m[0][0] + m[1][1] + m[2][2]
    one = torch.ones_like(tr)
    s0 = 2 * torch.sqrt(torch.clamp(tr + 1, min=1e-30))
    s1 = 2 * torch.sqrt(torch.clamp(one + m[0][0] - m[1][1] - m[2][2], min=1e-30))
    s2 = 2 * torch.sqrt(torch.clamp(one + m[1][1] - m[0][0] - m[2][2], min=1e-30))
    s3 = 2 * torch.sqrt(torch.clamp(one + m[2][2] - m[0][0] - m[1][1], min=1e-30))
    q0 = torch.stack((0.25 * s0, (m[2][1] - m[1][2]) / s0, (m[0][2] - m[2][0]) / s0, (m[1][0] - m[0][1]) / s0), -1)
    q1 = torch.stack(((m[2][1] - m[1][2]) / s1, 0.25 * s1, (m[0][1] + m[1][0]) / s1, (m[0][2] + m[2][0]) / s1), -1)
    q2 = torch.stack(((m[0][2] - m[2][0]) / s2, (m[0][1] + m[1][0]) / s2, 0.25 * s2, (m[1][2] + m[2][1]) / s2), -1)
    q3 = torch.stack(((m[1][0] - m[0][1]) / s3, (m[0][2] + m[2][0]) / s3, (m[1][2] + m[2][1]) / s3, 0.25 * s3), -1)
    b0 = (tr > 0)[:, None]
    b1 = ((m[0][0] > m[1][1]) & (m[0][0] > m[2][2]))[:, None]
    b2 = (m[1][1] > m[2][2])[:, None]
    q = torch.where(b0, q0, torch.where(b1, q1, torch.where(b2, q2, q3)))
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[:, :1] < 0, -q, q)


FRAME_DEGENERATE = 64.0 * 2.0 ** -24      # eig1 <= this x eig2: an fp32 covariance of <= 32 terms cannot tell eig1 from zero


def point_cloud_frames(points, idx, toward=None):
    """Local PCA frames of a point cloud -> (quats [N,4] (w, x, y, z), unit, w >= 0; eig [N,3], ascending); an extension.

    Row i uses the valid entries of idx[i] (0 <= idx < N; make the rows with knn_points(..., include_self=True)): their mean m,
    C = sum (p - m)(p - m)^T / n in two passes, eigenvalues eig0 <= eig1 <= eig2, n = the eigenvector of eig0, t1 = that of eig2,
    t2 = n x t1, R = [t1 t2 n] (columns), a right-handed rotation whose third axis is the surface normal.  n's sign: with
    toward ([3] or [N,3], a sensor position) n . (toward - p_i) >= 0; otherwise n's component of largest magnitude is positive
    (the lowest index on a tie).  A row with n < 3, or with eig1 <= 64 * 2^-24 * eig2 (the neighbours lie on a line), is
    degenerate and gets the identity quaternion; eig is reported all the same.

    This torch form works in fp64 (torch.linalg.eigh) and returns points' dtype: it is the definition, and what host tensors
    and other dtypes get.  fp32 points on a HIP device go to the kernel (ops.knn_frames: fp32, a fixed number of Jacobi sweeps)."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("point_cloud_frames: points must be a [N,3] tensor")
    N = points.shape[0]
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[0] != N:
        raise ValueError("point_cloud_frames: idx must be a [N,k] tensor")
    if toward is not None:
        toward = torch.as_tensor(toward, device=points.device)
        if tuple(toward.shape) not in ((3,), (N, 3)):
            raise ValueError("point_cloud_frames: toward must be [3] or [N,3]")
    if _on_hip(points) and 1 <= idx.shape[1] <= KNN_MAX_K:
        from .. import ops
        return ops.knn_frames(points, idx.to(points.device), None if toward is None else toward.to(torch.float32))
    out_dtype = points.dtype if points.dtype in (torch.float32, torch.float64) else torch.float32
    p = points.detach().to(torch.float64)
    idx = idx.to(points.device).long()
    valid = (idx >= 0) & (idx < N)
    nb = p[torch.where(valid, idx, torch.zeros_like(idx))]                      # [N,k,3]
    w = valid.to(torch.float64)[..., None]
    n = valid.sum(1)
    nn = n.clamp(min=1).to(torch.float64)[:, None]
    mean = (nb * w).sum(1) / nn
    diff = (nb - mean[:, None, :]) * w
    C = diff.transpose(1, 2) @ diff / nn[..., None]
    lam, vec = torch.linalg.eigh(C)
    normal, t1 = vec[:, :, 0], vec[:, :, 2]
    if toward is not None:
        flip = (normal * (toward.to(torch.float64) - p)).sum(-1) < 0
    else:
        a = normal.abs()
        best = normal[:, 0]
        take1 = a[:, 1] > a[:, 0]
        best = torch.where(take1, normal[:, 1], best)
        best = torch.where(a[:, 2] > torch.where(take1, a[:, 1], a[:, 0]), normal[:, 2], best)
        flip = best < 0
    normal = torch.where(flip[:, None], -normal, normal)
    t2 = torch.cross(normal, t1, dim=-1)
    quats = _rotation_to_quaternion(torch.stack((t1, t2, normal), dim=-1))
    degenerate = (n < 3) | (lam[:, 1] <= FRAME_DEGENERATE * lam[:, 2]) | ~torch.isfinite(quats).all(-1)
    identity = torch.zeros_like(quats)
    identity[:, 0] = 1
    quats = torch.where(degenerate[:, None], identity, quats)
    return quats.to(out_dtype), lam.to(out_dtype)


def point_cloud_converter(points, percentage=0.5, n_nearest=4, thr_max=2, oriented=False, n_frame=16, flatten=4.0, toward=None):
    """Gaussians from a raw point cloud by exact neighbour search; an extension on the formula of the reference's
    naive_point_cloud_converter (Converters.py:98-122), which stays as it is.

    Isotropic: (verts, isigma [N], None).  d = sqrt(d2) of knn_points(points, n_nearest, include_self=True) -- the reference's
    topk keeps the zero self-distance too --, L = mean(min(d, mean(d) * thr_max)) over the row's valid entries and
    isigma = 1 / (L^2 / (4 ln(1 / percentage)) + 1e-8).

    oriented=True: (verts, scales [N,3], quats [N,4]) for OrientedGaussianMeshes.  quats are point_cloud_frames' over the
    n_frame nearest (the point included; toward orients the normals), scales = isigma * (1, 1, flatten): the third axis of R(q)
    is the PCA normal, flatten > 1 times thinner in the inverse_sigma=False sense, so Aggregation.gaussian_normals picks exactly
    that axis.  A degenerate frame gets (isigma, isigma, isigma) with the identity, as normal_mesh_converter's auto_fix does.

    Tensors in, tensors out, on the device of `points` (a HIP device takes the kernels); a numpy cloud gives numpy back."""
    to_np = not torch.is_tensor(points)
    pts = torch.as_tensor(points)
    if pts.dtype != torch.float32:
        pts = pts.to(torch.float32)
    N = pts.shape[0]
    with torch.no_grad():
        idx, d2 = knn_points(pts, n_nearest, include_self=True)
        valid = idx >= 0
        cnt = valid.sum(1).clamp(min=1).to(torch.float32)
        d = torch.where(valid, torch.sqrt(d2), torch.zeros_like(d2))
        mean = d.sum(1) / cnt
        capped = torch.where(valid, torch.min(d, (mean * thr_max)[:, None]), torch.zeros_like(d))
        length = capped.sum(1) / cnt
        isigma = 1 / (length ** 2 / (4 * np.log(1 / percentage)) + 1e-8)
        if not oriented:
            return (pts.numpy(), isigma.numpy(), None) if to_np else (pts, isigma, None)
        fidx, _ = knn_points(pts, n_frame, include_self=True)
        quats, eig = point_cloud_frames(pts, fidx, toward)
        degenerate = (((fidx >= 0) & (fidx < N)).sum(1) < 3) | (eig[:, 1] <= FRAME_DEGENERATE * eig[:, 2])
        axes = torch.tensor([1.0, 1.0, float(flatten)], dtype=torch.float32, device=pts.device)
        scales = isigma[:, None] * torch.where(degenerate[:, None], torch.ones_like(axes), axes)
    return (pts.numpy(), scales.numpy(), quats.numpy()) if to_np else (pts, scales, quats)


def to_gaussian_meshes(converter, **kwargs):
    """converter(verts, faces, **kwargs) -> GaussianMeshes factory taking (verts, faces) tensors; the
    PyTorch3D-free counterpart of pytorch3d2gaussian (Converters.py:176-194)."""
    def wrapper(verts, faces=None, device="cpu", **mesh_kwargs):
        args = (verts.cpu(), faces.cpu()) if faces is not None else (verts.cpu(),)
        v, s, r = converter(*args, **kwargs)
        return GaussianMeshes(v.type(torch.float32), s.type(torch.float32), None if r is None else r.type(torch.float32),
                              **mesh_kwargs).to(device)
    return wrapper
