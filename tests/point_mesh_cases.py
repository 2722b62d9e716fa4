"""References, bounds and meshes shared by tests/test_point_mesh_cpu.py and tests/test_gpu_point_mesh.py.

The fp64 reference here is written on its own (divisions, no reciprocal, torch.linalg.cross) and returns the closest POINT, which
is unique on every triangle -- a triangle is convex --, where the weights are not on a degenerate one.

Every bound is derived from the arithmetic of Aggregation.point_triangle_closest / voge_amd/csrc/point_mesh.hip, never fitted
to what the code returns.  u = 2^-24, d = the distance of the pair, L = the triangle's longest edge, so |p - a| <= d + L:

d2, values   a residual component is v - (w1 e0 + w2 e1) or (v - e0) - t (e1 - e0) of rounded differences: at most
             u (3 d + 7 L) <= 7 u (d + L) in norm; d2 = (rx rx + ry ry) + rz rz adds 3 u d2 and takes 2 d |delta r|:
             17 u (d + L)^2 with exact weights.  The weights: a segment's t is off by a few u |v| / |e| and costs |e|^2 dt^2, second
             order.  The interior weights are off by dw ~ 8 u (d + L) / h, h the triangle's least height; a closest point that
             lies inside is then either kept, displaced by at most dw L, or lost to an edge at most h away -- the four candidates'
             minimum is above the truth by at most min((dw L)^2, h^2) <= dw L h = 8 u (d + L) L.  Together 25 u (d + L)^2; VALUE_C =
             32 (in units of 2^-23) is 64 u and leaves the estimate of dw a factor of four.
selection    the kernel keeps the smallest fp32 d2: chosen_true <= chosen_fp32 + B <= best_fp32 + B <= best_true + 2 B, B taken
             with the mesh's longest edge as it covers both triangles: SELECT_C = 2 VALUE_C = 64.
closest      for q the closest point of a convex set to p and any point y of the set, |p - y|^2 >= |p - q|^2 + |y - q|^2.  The
point        kernel's q' = a + (w1 e0 + w2 e1) is a point of the triangle up to 4 u L, and |p - q'|^2 is within the value bound
             of the true minimum and of the kernel's d2: |q' - q| <= sqrt(2 B) + 4 u (d + L).
gradients    compared with the closed form in fp64 on the kernel's own pairs AND weights (the closest point has its own
             check), r = (p - a) - (w1 e0 + w2 e1): the kernel's fp32 residual is within 8 u (|v_c| + |e0_c| + |e1_c|) per
             component (the count above, component-wise, with the rounding of 1 - t), a term fl(w r) adds u |w r|, a scattered
             term is rounded to a multiple of q = 2^-s (q / 2 each); the sums are fp64 (2^-50 of sum |terms| covers them) and the
             result is rounded once.  s = 62 - ceil(log2(P + F)) - e with D = sqrt(max d2 (1 + 2^-20) + 2^-148) < 2^e; e is
             recomputed here from the fp64 residuals, and q is taken twice as large in case the kernel's fp32 maximum sits in
             the next binade."""
import functools
import math
import os

import numpy as np
import torch

import sample_meshes

VALUE_C = 32.0
SELECT_C = 64.0
U = 2.0 ** -24


def _seg_point(p, s, e):
    ee = (e * e).sum(-1)
    pos = ee > 0
    t = torch.where(pos, ((p - s) * e).sum(-1) / torch.where(pos, ee, torch.ones_like(ee)), torch.zeros_like(ee)).clamp(0, 1)
    return s + t[..., None] * e


def closest64(p, a, b, c):
    """fp64 (d2 [...], q [..., 3]): the closest point of the triangle (a, b, c) to p, all broadcast"""
    p, a, b, c = torch.broadcast_tensors(p.double(), a.double(), b.double(), c.double())
    e0, e1, v = b - a, c - a, p - a
    n = torch.linalg.cross(e0, e1)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nns = torch.where(ok, nn, torch.ones_like(nn))
    w2 = (torch.linalg.cross(e0, v) * n).sum(-1) / nns
    w1 = (torch.linalg.cross(v, e1) * n).sum(-1) / nns
    inside = ok & (w1 >= 0) & (w2 >= 0) & (1 - w1 - w2 >= 0)
    qs = torch.stack((a + w1[..., None] * e0 + w2[..., None] * e1, _seg_point(p, a, e0), _seg_point(p, b, c - b), _seg_point(p, c, a - c)))
    d = ((p[None] - qs) ** 2).sum(-1)
    d[0] = torch.where(inside, d[0], torch.full_like(d[0], float("inf")))
    best = d.argmin(0)
    return d.gather(0, best[None])[0], qs.gather(0, best[None, ..., None].expand((1,) + qs.shape[1:]))[0]


def d2_matrix64(points, verts, faces):
    """fp64 [P,F]: the squared distance of every point to every face"""
    v, f = verts.double(), faces.long()
    return closest64(points.double()[:, None], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])[0]


def longest_edge(verts, faces):
    """fp64 [F]"""
    v, f = verts.double(), faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return torch.stack(((b - a).norm(dim=-1), (c - b).norm(dim=-1), (a - c).norm(dim=-1))).max(0).values


def d2_bound(c, d2, edge):
    """c 2^-23 (distance + longest edge)^2"""
    return c * 2.0 ** -23 * (d2.clamp(min=0).sqrt() + edge) ** 2 + 1e-300


def point_bound(d2, edge):
    return (2 * d2_bound(VALUE_C, d2, edge)).sqrt() + 4 * U * (d2.clamp(min=0).sqrt() + edge)


def check_search(label, points, verts, faces, idx, d2, bary, by_face=False):
    """Everything the module's docstring promises of one direction of the search, for every query, no exclusions.
    by_face=False: idx [P] faces chosen by the points; True: idx [F] points chosen by the faces.  Returns the largest
    measured / bound ratios {selection, value, point, sum}."""
    from util import log_line
    F, P = faces.shape[0], points.shape[0]
    idx = idx.long().cpu()
    d2, bary = d2.double().cpu(), bary.double().cpu()
    assert ((idx >= 0) & (idx < (P if by_face else F))).all(), label
    M = d2_matrix64(points, verts, faces)                       # [P,F]
    edges = longest_edge(verts, faces)
    v, f = verts.double(), faces.long()
    if by_face:
        chosen, least = M[idx, torch.arange(F)], M.min(0).values
        pf, ff, edge = points.double()[idx], f, edges
    else:
        chosen, least = M[torch.arange(P), idx], M.min(1).values
        pf, ff, edge = points.double(), f[idx], edges[idx]
    a, b, c = v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]]
    worst = {"selection": float(((chosen - least) / d2_bound(SELECT_C, least, edges.max())).max())}
    ref_d2, ref_q = closest64(pf, a, b, c)
    worst["value"] = float(((d2 - ref_d2).abs() / d2_bound(VALUE_C, ref_d2, edge)).max())
    q = a + (bary[:, 1:2] * (b - a) + bary[:, 2:3] * (c - a))
    worst["point"] = float(((q - ref_q).norm(dim=-1) / point_bound(ref_d2, edge)).max())
    assert (bary >= 0).all() and torch.isfinite(bary).all(), label
    worst["sum"] = float((bary.sum(-1) - 1).abs().max() / 2.0 ** -22)
    log_line(f"[parity] point-mesh {label} ({'faces -> points' if by_face else 'points -> faces'}, {P} x {F}): measured / bound "
             + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    for k, r in worst.items():
        assert r <= 1.0, (label, k, r)
    return worst


def closed_form_grads(verts, faces, points, face_idx, bary_p, point_idx, bary_f, upstream=1.0, point_reduction="mean"):
    """fp64 (g_verts [V,3], g_points [P,3], bound_verts, bound_points): the gradients of upstream * loss by the closed form of
    point_mesh.hip's header on the GIVEN pairs and weights (point_idx None: single_directional), and the bound of the module's
    docstring per element."""
    v, p, f = verts.double().cpu(), points.double().cpu(), faces.long().cpu()
    V, P, F = v.shape[0], p.shape[0], f.shape[0]
    g_v, g_p = torch.zeros(V, 3, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64)
    mag_v, mag_p = torch.zeros_like(g_v), torch.zeros_like(g_p)        # sum |terms|
    rnd_v, rnd_p = torch.zeros_like(g_v), torch.zeros_like(g_p)        # the fp32 roundings of the terms
    cnt_v, cnt_p = torch.zeros(V, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    dmax = 0.0
    items = [(torch.arange(P), face_idx.long().cpu(), bary_p.double().cpu(), 1.0 if point_reduction == "sum" else 1.0 / P, True)]
    if point_idx is not None:
        items.append((point_idx.long().cpu(), torch.arange(F), bary_f.double().cpu(), 1.0 if point_reduction == "sum" else 1.0 / F, False))
    for pi, fi, w, u, gather in items:
        tri = f[fi]
        a = v[tri[:, 0]]
        e0, e1, vv = v[tri[:, 1]] - a, v[tri[:, 2]] - a, p[pi] - a
        r = vv - (w[:, 1:2] * e0 + w[:, 2:3] * e1)
        dr = 8 * U * (vv.abs() + e0.abs() + e1.abs())
        dmax = max(dmax, float((r * r).sum(-1).max()))
        g_p.index_add_(0, pi, 2 * u * r)
        mag_p.index_add_(0, pi, 2 * u * r.abs())
        rnd_p.index_add_(0, pi, 2 * u * dr)
        if not gather:
            cnt_p.index_add_(0, pi, torch.ones(len(pi), dtype=torch.float64))
        for k in range(3):
            wk = w[:, k:k + 1]
            g_v.index_add_(0, tri[:, k], -2 * u * wk * r)
            mag_v.index_add_(0, tri[:, k], 2 * u * wk * r.abs())
            rnd_v.index_add_(0, tri[:, k], 2 * u * wk * (dr + U * r.abs()))
            cnt_v.index_add_(0, tri[:, k], (wk[:, 0] != 0).double())
    L = (P + F - 1).bit_length()      # the forward takes ceil(log2(P + F)) in both forms
    e = math.frexp(math.sqrt(dmax * (1 + 2.0 ** -20) + 2.0 ** -148))[1]
    q = 2 * 2.0 ** -(62 - L - e)
    g = abs(upstream)
    bound_v = g * (rnd_v + cnt_v[:, None] * q / 2 + (U + 2.0 ** -50) * mag_v) + 1e-45
    bound_p = g * (rnd_p + cnt_p[:, None] * q / 2 + (U + 2.0 ** -50) * mag_p) + 1e-45
    return upstream * g_v, upstream * g_p, bound_v, bound_p


# ---- meshes and clouds ----------------------------------------------------------------------------------------------------------

def points_around(verts, faces, n, seed):
    """n fp32 points for a mesh: uniform in its bounding box enlarged by half its extent (inside and outside), with every
    eighth point ON the mesh -- a vertex, or the midpoint of a face's first edge, so exact zeros and ties are among them"""
    rng = np.random.default_rng(seed)
    v = verts.double().numpy()
    lo, hi = v.min(0), v.max(0)
    ext = max(float((hi - lo).max()), 1e-6)
    pts = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * (hi - lo + ext)
    f = faces.long().numpy()
    for k in range(0, n, 8):
        tri = f[rng.integers(len(f))]
        pts[k] = v[tri[0]] if (k // 8) % 2 else (v[tri[0]] + v[tri[1]]) / 2
    return torch.from_numpy(pts.astype(np.float32))


def soup(F):
    """The first F faces of a jittered 16 x 17 height field (544 faces): a mesh of exactly F faces"""
    verts, faces = sample_meshes.grid_mesh(16, 17, jitter=0.3, seed=5)
    return verts, faces[:F].contiguous()


all_test_meshes = sample_meshes.all_test_meshes
level2_sphere = functools.lru_cache(maxsize=None)(sample_meshes.level2_sphere)


def bunny_points(n, seed=0):
    """n of the bunny's Gaussian centres (tests/golden/bunny_gaussians.npz), scaled into the unit sphere's neighbourhood"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny_gaussians.npz"))
    v = g["verts"].astype(np.float64)
    v = (v - v.mean(0)) / np.abs(v - v.mean(0)).max()
    pick = np.random.default_rng(seed).choice(len(v), n, replace=False)
    return torch.from_numpy(v[pick].astype(np.float32))


def segment_d2_64(points, s, t):
    """fp64 [P,E]: the squared distance of every point to every segment (s_e, t_e), by the direct formula"""
    p, s, t = points.double()[:, None], s.double()[None], t.double()[None]
    return ((p - _seg_point(p, s, t - s)) ** 2).sum(-1)
