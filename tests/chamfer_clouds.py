"""References and clouds shared by tests/test_chamfer_cpu.py and tests/test_gpu_chamfer.py."""
import functools

import numpy as np
import torch

from knn_clouds import surface


def brute_force_nearest(queries, points):
    """fp64 brute force with a stable argmin -> (idx [Nq] int32, d2 [Nq] fp64): the lowest index among the exact minima."""
    q, p = queries.double().numpy(), points.double().numpy()
    diff = q[:, None, :] - p[None, :, :]
    d = (diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2
    idx = np.argsort(d, axis=1, kind="stable")[:, 0]
    return idx.astype(np.int32), d[np.arange(len(q)), idx]


@functools.lru_cache(maxsize=None)
def surface_pair():
    """surface(40) and a shifted, jittered surface(24): 1600 x 576 points, no ties."""
    rng = np.random.default_rng(7)
    y = surface(24).numpy() + np.float32([0.03, -0.02, 0.05]) + rng.normal(0, 0.01, (576, 3)).astype(np.float32)
    return surface(40), torch.from_numpy(y.astype(np.float32))


def fp64_chamfer_grads(x, y, upstream, **kw):
    """(loss, g_x, g_y, sum of |terms| per element of g_x, of g_y, list lengths into x, into y) of Aggregation.chamfer_term by fp64
    autograd on the fp32 inputs, with the upstream gradient `upstream`; the |terms| sums are those of the written-out gradient
    (the weights included, the upstream gradient not)."""
    from voge_amd import Aggregation
    a, b = x.double().requires_grad_(True), y.double().requires_grad_(True)
    loss, nn_x, nn_y = Aggregation.chamfer_term(a, b, return_indices=True, **kw)
    g_x, g_y = torch.autograd.grad(loss * upstream, (a, b))
    mean = kw.get("point_reduction", "mean") == "mean"
    wx, wy = (2.0 / len(x) if mean else 2.0), (2.0 / len(y) if mean else 2.0)
    ad, bd = a.detach(), b.detach()
    mag_x, mag_y = wx * (ad - bd[nn_x]).abs(), torch.zeros_like(bd)
    mag_y.index_add_(0, nn_x, wx * (bd[nn_x] - ad).abs())
    len_y = torch.bincount(nn_x, minlength=len(y))
    len_x = torch.zeros(len(x), dtype=torch.long)
    if nn_y is not None:
        mag_y = mag_y + wy * (bd - ad[nn_y]).abs()
        mag_x = mag_x.index_add(0, nn_y, wy * (ad[nn_y] - bd).abs())
        len_x = torch.bincount(nn_y, minlength=len(x))
    return loss.detach(), g_x, g_y, mag_x, mag_y, len_x, len_y
