"""Meshes, references and derived bounds shared by tests/test_mesh_sample_cpu.py and tests/test_gpu_mesh_sample.py.

Every bound here is derived from the arithmetic the kernels are documented to do (voge_amd/csrc/mesh_sample.hip's header and
Aggregation.mesh_surface_points), never fitted to what they return:

face choice   the device's cumulative sums and the definition's are two summation orders of the same F non-negative fp64 terms,
              each within (F - 1) 2^-53 total of the exact sum; with the one rounding of t a sample may sit on the other side of a
              boundary B only if |t - B| <= tau = 2 F 2^-52 total.
points        e1, e2, r, 1 - u2, w1, w2, w1 e1, w2 e2, their sum and a + (..): at most 7 roundings on any path to a component, each
              2^-24 relative of a partial result bounded by |a_c| + |e1_c| + |e2_c| (|w| <= 1); 8 with the second-order terms.
bary          r, 1 - u2 and the product: 3 roundings of values <= 1.
normals       n = cr / A2.  A component of cr is (p q) - (r s) of rounded differences: 4 roundings of M_c = |p q| + |r s|; A2 takes
              |delta cr| and 3 more roundings, the division one: delta n_c <= 2^-24 (4 M_c / A2 + |n_c| (4 |M| / A2 + 4)).  Nothing
              in it is relative to the position of the mesh, only to its edges.
gradients     a vertex sums w_r g over the samples on its faces: the fp32 weights of bary carry 3 roundings each (4 covers
              1 - w1 - w2), every scattered term is rounded to a multiple of q = 2^-s (q / 2 each), and -- with normals -- a corner
              adds e_opp x (P G_f / A2) where G_f, a sum of m_f scattered terms, is off by m_f q / 2 per component, P a projection:
              |e_opp| sqrt(3) m_f (q / 2) / A2.  The sums are fp64 (2^-45 of sum |terms| covers them with room); one rounding to fp32.
              s = 62 - L - e with 2^L >= S and 2^e > D = max |g|."""
import functools
import math

import numpy as np
import torch

from voge_amd import Aggregation


def tetrahedron(edge=1.0, offset=0.0):
    """A regular tetrahedron of the given edge around `offset` -> (verts [4,3] fp32, faces [4,3] int64, outward)."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (edge / (2 * math.sqrt(2))) + offset
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)


def grid_mesh(nx, ny, jitter=0.0, seed=0, lift=True):
    """A height field over [0,1]^2 of nx x ny cells, two triangles a cell -> (verts [(nx+1)(ny+1),3] fp32, faces [2 nx ny,3]).
    jitter = 0 and lift=False: nx, ny powers of two give faces of exactly equal area."""
    xs, ys = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="xy")
    z = 0.2 * np.sin(3 * xs) * np.cos(2 * ys) if lift else np.zeros_like(xs)
    v = np.stack([xs, ys, z], -1).reshape(-1, 3)
    if jitter:
        v = v + np.random.default_rng(seed).uniform(-jitter, jitter, v.shape) * [1 / nx, 1 / ny, 0.05]
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)], 1).reshape(-1, 3)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int64))


def with_zero_area_faces(verts, faces, positions):
    """The mesh with a face of three distinct collinear vertices (area exactly 0) inserted so that it sits at every index of
    `positions` (ascending, indices of the RESULT) -> (verts, faces)."""
    V = verts.shape[0]
    verts = torch.cat([verts, torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])])
    zero = torch.tensor([V, V + 1, V + 2])
    out, src = [], list(faces)
    positions = set(int(p) for p in positions)
    n = len(src) + len(positions)
    for k in range(n):
        out.append(zero if k in positions else src.pop(0))
    return verts, torch.stack(out)


def skewed_mesh(n_tiny=2000, big_first=False):
    """n_tiny tiny faces, together about 1e-6 of the area, in front of ONE large face (big_first: behind it) -> (verts, faces).
    In front they sit where an fp32 u0 is fine enough to address each of them; behind the large face an fp32 u0 (spacing 2^-24
    below 1) reaches only a few, and an fp32 cumulative sum would not see them at all."""
    big = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)                      # A2 = 1
    side = math.sqrt(1e-6 / n_tiny)                                                      # each tiny face: A2 = 1e-6 / n_tiny
    k = np.arange(n_tiny)
    base = np.stack([2.0 + 3 * side * (k % 50), 3 * side * (k // 50), np.zeros(n_tiny)], 1)
    tiny = np.stack([base, base + [side, 0, 0], base + [0, side, 0]], 1).reshape(-1, 3)
    v = np.concatenate([big, tiny] if big_first else [tiny, big])
    f = np.arange(3 + 3 * n_tiny).reshape(-1, 3)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int64))


@functools.lru_cache(maxsize=None)
def unequal_mesh():
    """A jittered 6 x 5 grid: 60 faces of visibly different areas."""
    return grid_mesh(6, 5, jitter=0.35, seed=3)


ONE_FACE = (torch.tensor([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.1, 0.5]]), torch.tensor([[0, 1, 2]]))


def level2_sphere():
    """demo/ShapeFitting.ico_sphere(2): (verts [162,3] fp32, faces [320,3])"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("shape_fitting_demo_meshes", os.path.join(root, "demo", "ShapeFitting.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    v, f = demo.ico_sphere(2)
    return torch.from_numpy(v), torch.from_numpy(f)


def zero_area_grid(block):
    """The 23 x 13 grid with zero-area faces at index 0, at index F - 1 and as a run of 7 that straddles the first block boundary
    -> (verts, faces, the run's indices)"""
    verts, faces = grid_mesh(23, 13, jitter=0.3)
    run = list(range(block - 3, block + 4))
    F = len(faces) + 2 + len(run)
    return with_zero_area_faces(verts, faces, [0] + run + [F - 1]) + (run,)


def all_test_meshes():
    """name -> (verts, faces) of every mesh tests/test_mesh_sample_cpu.py and tests/test_gpu_mesh_sample.py sample (the 525 312-face
    grid of the large-table test excepted: its F^2 reversed sums are not a CPU test's work)"""
    from voge_amd import ops
    return {"one face": ONE_FACE, "tetrahedron": tetrahedron(), "tetrahedron at 1000": tetrahedron(1e-2, 1000.0),
            "grid 23 x 13": grid_mesh(23, 13, jitter=0.3), "zero-area grid": zero_area_grid(ops.MESH_SAMPLE_BLOCK)[:2],
            "zero-area 4 x 4": with_zero_area_faces(*grid_mesh(4, 4), [0, 7, 8, 9, 36]), "equal areas": grid_mesh(16, 16, lift=False),
            "skewed": skewed_mesh(), "skewed, large face first": skewed_mesh(2000, True), "unequal": unequal_mesh(),
            "level-2 sphere": level2_sphere()}


def random_u(S, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((S, 3), dtype=np.float32))


def clamp_u(u):
    return torch.where(torch.isnan(u), torch.zeros_like(u), u).clamp(0.0, 1.0 - 2.0 ** -24)


def face_cdf(verts, faces):
    """(A2 fp32 [F], cdf fp64 [F]) of the definition"""
    A2 = Aggregation.mesh_face_areas2(verts, faces)
    return A2, torch.cumsum(A2.double(), 0)


def check_face_choice(verts, faces, u, got, cdf=None):
    """Asserts the face rule for every sample and returns the number that passed by the second rule (the boundary rule).
    got: the indices under test [S]; cdf: another cumulative sum to take t's faces from (default: the definition's)."""
    A2, ref_cdf = face_cdf(verts, faces)
    F, total = len(A2), ref_cdf[-1]
    t = clamp_u(u)[:, 0].double() * total
    ref = torch.searchsorted(ref_cdf, t, right=True).clamp(max=F - 1)
    got = got.long()
    assert ((got >= 0) & (got < F)).all(), "a face index out of range"
    assert (A2[got] > 0).all(), "a zero-area face was chosen"
    differ = got != ref
    lo, hi = torch.minimum(got, ref)[differ], torch.maximum(got, ref)[differ]
    B = ref_cdf[lo]
    tau = 2 * F * 2.0 ** -52 * float(total)
    between_empty = ref_cdf[hi - 1] == B                       # only zero-area faces between the two
    near = (t[differ] - B).abs() <= tau
    assert (between_empty & near).all(), (int(differ.sum()), int((~between_empty).sum()), int((~near).sum()))
    return int(differ.sum())


def check_outputs(verts, faces, u, got_idx, points, bary, normals=None):
    """points / bary / normals of the device against the fp64 evaluation at the faces the device returned; returns the worst
    measured / bound ratio of each."""
    vd, ud = verts.double(), u.double()
    ref_p, ref_n, _, ref_b = Aggregation.mesh_surface_points(vd, faces, ud, True, face_idx=got_idx)
    tri = faces.long()[got_idx.long()]
    a = vd[tri[:, 0]]
    e1, e2 = vd[tri[:, 1]] - a, vd[tri[:, 2]] - a
    worst = {}
    bound = 8 * 2.0 ** -24 * (a.abs() + e1.abs() + e2.abs()) + 1e-45
    worst["points"] = float(((points.double() - ref_p).abs() / bound).max())
    worst["bary"] = float(((bary.double() - ref_b).abs() / (3 * 2.0 ** -24)).max())
    if normals is not None:
        M = torch.stack((e1[:, 1].abs() * e2[:, 2].abs() + e1[:, 2].abs() * e2[:, 1].abs(),
                         e1[:, 2].abs() * e2[:, 0].abs() + e1[:, 0].abs() * e2[:, 2].abs(),
                         e1[:, 0].abs() * e2[:, 1].abs() + e1[:, 1].abs() * e2[:, 0].abs()), -1)
        A2 = torch.linalg.cross(e1, e2).norm(dim=-1, keepdim=True)
        nb = 2.0 ** -24 * (4 * M / A2 + ref_n.abs() * (4 * M.norm(dim=-1, keepdim=True) / A2 + 4)) + 1e-45
        worst["normals"] = float(((normals.double() - ref_n).abs() / nb).max())
    for name, ratio in worst.items():
        assert ratio <= 1.0, (name, ratio)
    return worst


def fp64_sample_grads(verts, faces, u, face_idx, g_points, g_normals=None):
    """(g_verts fp64 [V,3], bound [V,3]) of the functional sum(g_points * points) + sum(g_normals * normals) by fp64 autograd of
    the definition on the fp32 inputs at the given faces, and the bound of the module's docstring per element."""
    vd = verts.double().requires_grad_(True)
    p, n, _, bary = Aggregation.mesh_surface_points(vd, faces, u.double(), g_normals is not None, face_idx=face_idx)
    loss = (p * g_points.double()).sum()
    if g_normals is not None:
        loss = loss + (n * g_normals.double()).sum()
    ref, = torch.autograd.grad(loss, vd)
    V, F, S = verts.shape[0], faces.shape[0], u.shape[0]
    idx = face_idx.long()
    tri = faces.long()[idx]                                                            # [S,3]
    D = float(g_points.abs().max()) if g_normals is None else max(float(g_points.abs().max()), float(g_normals.abs().max()))
    L = max(S - 1, 0).bit_length()
    q = 2.0 ** -(62 - L - math.frexp(D)[1])
    count = torch.bincount(tri.reshape(-1), minlength=V).double()
    mag = torch.zeros(V, 3, dtype=torch.float64)
    for r in range(3):
        mag.index_add_(0, tri[:, r], bary[:, r:r + 1].detach().abs() * g_points.double().abs())
    sumabs = torch.zeros(V, 3, dtype=torch.float64)
    for r in range(3):
        sumabs.index_add_(0, tri[:, r], g_points.double().abs())
    bound = 4 * 2.0 ** -24 * sumabs + count[:, None] * q / 2
    if g_normals is not None:
        m_f = torch.bincount(idx, minlength=F).double()
        f = faces.long()
        v0 = verts.double()
        a, b, c = v0[f[:, 0]], v0[f[:, 1]], v0[f[:, 2]]
        A2 = torch.linalg.cross(b - a, c - a).norm(dim=-1)
        Gabs = torch.zeros(F, 3, dtype=torch.float64).index_add_(0, idx, g_normals.double().abs()).norm(dim=-1)
        for r, opp in enumerate((c - b, a - c, b - a)):
            per = opp.norm(dim=-1) / A2
            corner = torch.where(m_f > 0, per * math.sqrt(3) * m_f * q / 2, torch.zeros_like(per))
            bound.index_add_(0, f[:, r], corner[:, None].expand(-1, 3))
            mag.index_add_(0, f[:, r], torch.where(m_f > 0, per * Gabs, torch.zeros_like(per))[:, None].expand(-1, 3))
    bound = bound + 2.0 ** -45 * mag
    bound = bound + 2.0 ** -24 * (ref.abs() + bound) + 1e-45
    return ref, bound
