"""Seeded point clouds shared by tests/test_knn_cpu.py and tests/test_gpu_knn.py, and the fp64 references of both."""
import functools

import numpy as np
import torch


@functools.lru_cache(maxsize=None)
def lattice():
    """3000 points on a 64^3 lattice of pitch 2^-10: every difference and every d2 is exact in fp32, 75 % of the rows hold an
    exact distance tie among their 8 nearest, 17 points are duplicated -- the tie-break cloud."""
    rng = np.random.default_rng(0)
    return torch.from_numpy((rng.integers(0, 64, (3000, 3)) / 1024).astype(np.float32))


@functools.lru_cache(maxsize=None)
def surface(n):
    """A jittered n x n lattice on z = 0.15 sin 3x cos 4y over [-1, 1]^2, rows permuted, fp32."""
    rng = np.random.default_rng(0)
    g = (np.arange(n) + 0.5) / n * 2 - 1
    x, y = np.meshgrid(g, g, indexing="ij")
    x = x + rng.uniform(-0.3, 0.3, x.shape) * 2 / n
    y = y + rng.uniform(-0.3, 0.3, y.shape) * 2 / n
    z = 0.15 * np.sin(3 * x) * np.cos(4 * y)
    pts = np.stack((x.ravel(), y.ravel(), z.ravel()), 1)
    return torch.from_numpy(pts[rng.permutation(len(pts))].astype(np.float32))


def surface_normals(points):
    """Unit normals of z = 0.15 sin 3x cos 4y at the points' (x, y), fp64, z component positive."""
    p = points.double().numpy()
    fx = 0.45 * np.cos(3 * p[:, 0]) * np.cos(4 * p[:, 1])
    fy = -0.6 * np.sin(3 * p[:, 0]) * np.sin(4 * p[:, 1])
    n = np.stack((-fx, -fy, np.ones_like(fx)), 1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def brute_force_knn(points, k, include_self):
    """fp64 brute force with a stable argsort -> (idx [N,k] int32, d2 [N,k] fp64), padded with (-1, inf)."""
    p = points.double().numpy()
    N = len(p)
    diff = p[:, None, :] - p[None, :, :]
    d = (diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2
    if not include_self:
        np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind="stable")
    val = np.take_along_axis(d, order, 1)
    idx = np.full((N, k), -1, np.int32)
    d2 = np.full((N, k), np.inf)
    have = min(k, N if include_self else N - 1)
    idx[:, :have] = order[:, :have]
    d2[:, :have] = val[:, :have]
    return idx, d2


def eigh_frames(points, idx):
    """fp64 eigh on the rows of idx (every entry valid) -> (eig [N,3] ascending, normals [N,3] unsigned, tangents of eig2)."""
    p = points.double().numpy()
    nb = p[idx.cpu().numpy().astype(np.int64)]
    d = nb - nb.mean(1, keepdims=True)
    C = np.einsum("nki,nkj->nij", d, d) / nb.shape[1]
    lam, vec = np.linalg.eigh(C)
    return lam, vec[:, :, 0], vec[:, :, 2]


def isigma_reference(points, idx, percentage, thr_max):
    """The reference's formula (Converters.py:98-122) in fp64 on the neighbours idx lists (the self entry included)."""
    p = points.double().numpy()
    i = idx.cpu().numpy().astype(np.int64)
    d = np.linalg.norm(p[i] - p[:, None, :], axis=-1)
    length = np.minimum(d, d.mean(1, keepdims=True) * thr_max).mean(1)
    return 1.0 / (length ** 2 / (4 * np.log(1 / percentage)) + 1e-8)
