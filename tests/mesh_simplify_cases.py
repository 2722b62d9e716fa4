"""Meshes, an independent restatement of the rule and the derived bounds shared by tests/test_mesh_simplify_cpu.py and
tests/test_gpu_mesh_simplify.py.

restatement  restate() is numpy with dictionaries and loops (a lexsort for the labels, np.linalg.solve for the quadric system),
             written from the five steps of the issue, not from Aggregation.mesh_simplify's tensor code.  Labels, faces and index
             tables are integers: every comparison with them is array_equal.

bounds       POSITION_BOUND and ATTR_BOUND, derived from the arithmetic voge_amd/csrc/mesh_simplify.hip's header documents, never
             fitted to what the kernels return; eps = 2^-24, u = 2^-53, M = max |coordinate|, h the cell, a cluster of n vertices
             that m corners of faces name, 2^Lv >= V, 2^Lf >= 3 F, qp = 2^(Lv - 60), qq = 2^(Lf - 60).
             mean     kernel and definition round c + h mean(x) resp. mean(p) once to fp32, equal in exact arithmetic.  The kernel's
                      fixed-point mean is off by qp / 2 cells, the fp64 steps on either side by (n + 8) u (M + h):
                          B_mean = 2 eps |def| + h qp / 2 + (n + 8) u (M + h)                      per axis.
             quadric  (A + lambda m I) x = -b + lambda m mu is SPD with eigenvalues in [lambda m, (1 + lambda) m].  The kernel's
                      matrix is off by E, |E_ij| <= m Q / 2 with Q = qq + 2 m u (fixed point; fp64 sums in another order), so
                      |E|_2 <= 3 m Q / 2; the right side by e, |e| <= sqrt(3) m (Q + lambda P) / 2 with P = qp + 2 n u; before the clamp
                      |x| <= X = 2 (1 + lambda) / lambda (|b| <= 2 m, |mu| <= 2).  |dx| <= (|e| + |E|_2 X) / (lambda m); the clamp does
                      not increase it; 2^-28 cells cover Cramer's rule against any other fp64 solve at a condition of 10^3:
                          B_quadric = B_mean + h ((sqrt(3) (Q + lambda P) + 3 Q X) / (2 lambda) + 2^-28)  per axis.
             attr     D = the largest finite |value| of the eight-channel slice, 2^e > D, qa = 2^(Lv + e - 62):
                          B_attr = 2 eps |def| + qa / 2 + (n + 8) u D.
             A cluster of one vertex keeps its bits: bound 0.  The CPU tests compare two fp64 computations and use the same
             formulas without the fixed-point quanta (fixed_point=False)."""
import functools
import math

import numpy as np
import torch

import mesh_clean_cases as mcc
import meshing_cases as mc

EPS = 2.0 ** -24
U = 2.0 ** -53
LAMBDA = 1e-3
MAX_CELLS = 2 ** 21 - 1


# ---- the independent restatement ----------------------------------------------------------------------------------------------

def _cell_size(h):
    h = np.asarray(h, np.float32).reshape(-1)
    return np.repeat(h, 3) if h.size == 1 else h


def restate(verts, faces, cell_size, placement="mean", attr=None):
    """dict(verts [V',3] fp64 before the rounding, exact [V'] bool (a cluster of one vertex), faces [F',3], attr [V',C] fp64 or None,
    vert_index [V], face_index [F'], label [V], count [V'], corners [V'])"""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    h32 = _cell_size(cell_size)
    V, F = len(v32), len(f)
    if not np.isfinite(v32).all():
        raise ValueError("a vertex is not finite")
    if F and (V == 0 or f.min() < 0 or f.max() >= V):
        raise ValueError("index outside [0, V)")
    lo32 = v32.min(0) if V else np.zeros(3, np.float32)
    cell = np.floor((v32 - lo32) / h32)      # three fp32 operations
    if V and cell.max() > MAX_CELLS - 1:
        raise ValueError("too many cells")
    cell = cell.astype(np.int64)
    # step 2: a lexsort by (cell, index); the first of every run is the label
    label = np.empty(V, np.int64)
    order = np.lexsort((np.arange(V), cell[:, 0], cell[:, 1], cell[:, 2]))
    start = None
    for k, i in enumerate(order.tolist()):
        if k == 0 or (cell[i] != cell[order[k - 1]]).any():
            start = i
        label[i] = start
    # step 3
    seen = {}
    face_index = []
    for i, (a, b, c) in enumerate(label[f].tolist() if F else []):
        if a == b or b == c or c == a:
            continue
        key = min((a, b, c), (b, c, a), (c, a, b))
        if key not in seen:
            seen[key] = i
            face_index.append(i)
    face_index = np.asarray(face_index, np.int64)
    # step 4
    out_label = sorted(set(label[f[face_index]].reshape(-1).tolist())) if len(face_index) else []
    row_of = {l: r for r, l in enumerate(out_label)}
    vert_index = np.asarray([row_of.get(l, -1) for l in label.tolist()], np.int64)
    new_faces = np.asarray([[row_of[l] for l in tri] for tri in label[f[face_index]].tolist()], np.int64).reshape(-1, 3)
    # step 5
    Vk = len(out_label)
    members = [[] for _ in range(Vk)]
    for i, r in enumerate(vert_index.tolist()):
        if r >= 0:
            members[r].append(i)
    p = v32.astype(np.float64)
    h, lo = h32.astype(np.float64), lo32.astype(np.float64)
    pos = np.zeros((Vk, 3))
    count = np.asarray([len(m) for m in members], np.int64)
    for r, m in enumerate(members):
        pos[r] = p[m].sum(0) / len(m)
    corners = np.zeros(Vk, np.int64)
    for r in vert_index[f.reshape(-1)].tolist() if F else []:
        if r >= 0:
            corners[r] += 1
    if placement == "quadric":
        A = np.zeros((Vk, 3, 3))
        b = np.zeros((Vk, 3))
        m = np.zeros(Vk)
        centre = np.asarray([lo + (cell[l] + 0.5) * h for l in out_label]).reshape(-1, 3)
        for i0, i1, i2 in f.tolist():
            cr = np.cross((p[i1] - p[i0]) / h, (p[i2] - p[i0]) / h)
            norm = math.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
            if not (norm > 0 and math.isfinite(norm)):
                continue
            n = cr / norm
            for i in (i0, i1, i2):
                r = vert_index[i]
                if r < 0:
                    continue
                x = (p[i] - centre[r]) / h
                d = -float(n @ x)
                A[r] += np.outer(n, n)
                b[r] += n * d
                m[r] += 1
        for r in range(Vk):
            if m[r] > 0 and count[r] > 1:
                mu = ((p[members[r]] - centre[r]) / h).sum(0) / count[r]
                x = np.linalg.solve(A[r] + LAMBDA * m[r] * np.eye(3), -b[r] + LAMBDA * m[r] * mu)
                pos[r] = centre[r] + np.clip(x, -0.5, 0.5) * h
    exact = count == 1
    for r in np.nonzero(exact)[0].tolist():
        pos[r] = p[members[r][0]]
    new_attr = None
    if attr is not None:
        a = np.asarray(attr, np.float32).astype(np.float64)
        new_attr = np.asarray([a[m].sum(0) / len(m) for m in members]).reshape(Vk, a.shape[1])
    return {"verts": pos, "exact": exact, "faces": new_faces, "attr": new_attr, "vert_index": vert_index, "face_index": face_index,
            "label": label, "count": count, "corners": corners}


# ---- the bounds ---------------------------------------------------------------------------------------------------------------

def _bits(n):
    return max(int(n) - 1, 0).bit_length()      # n <= 2^bits


def position_bound(ref_verts, count, corners, verts, F, cell_size, placement, fixed_point=True):
    """POSITION_BOUND [V',3] of the header, from the definition's positions, the clusters' sizes and the input"""
    ref = np.abs(np.asarray(ref_verts, np.float64))
    n = np.asarray(count, np.float64)[:, None]
    m = np.asarray(corners, np.float64)[:, None]
    h = _cell_size(cell_size).astype(np.float64)[None]
    V = len(verts)
    M = float(np.abs(np.asarray(verts, np.float64)).max()) if V else 0.0
    qp = 2.0 ** (_bits(V) - 60) if fixed_point else 0.0
    qq = 2.0 ** (_bits(3 * F) - 60) if fixed_point else 0.0
    bound = 2 * EPS * ref + h * qp / 2 + (n + 8) * U * (M + h)
    if placement == "quadric":
        Q, P, X = qq + 2 * m * U, qp + 2 * n * U, 2 * (1 + LAMBDA) / LAMBDA
        bound = bound + h * ((math.sqrt(3) * (Q + LAMBDA * P) + 3 * Q * X) / (2 * LAMBDA) + 2.0 ** -28)
    return np.where(n == 1, 0.0, bound)


def attr_bound(ref_attr, count, attr, V, fixed_point=True, channels=8):
    """ATTR_BOUND [V',C] of the header; D and qa per slice of `channels` channels"""
    ref = np.abs(np.asarray(ref_attr, np.float64))
    a = np.abs(np.asarray(attr, np.float64))
    n = np.asarray(count, np.float64)[:, None]
    bound = np.zeros_like(ref)
    for c0 in range(0, ref.shape[1], channels):
        sl = a[:, c0:c0 + channels]
        D = float(sl[np.isfinite(sl)].max()) if np.isfinite(sl).any() else 0.0
        e = math.frexp(D)[1]
        qa = 2.0 ** (_bits(V) + e - 62) if fixed_point else 0.0
        bound[:, c0:c0 + channels] = 2 * EPS * ref[:, c0:c0 + channels] + qa / 2 + (n + 8) * U * D
    return np.where(n == 1, 0.0, bound)


def share(got, ref, bound):
    """The largest |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf) -> (share, largest error)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    if err.size == 0:
        return 0.0, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / bound)
    return float(s.max()), float(err.max())


# ---- the cases ----------------------------------------------------------------------------------------------------------------

_mesh = mcc._mesh


@functools.lru_cache(maxsize=None)
def sphere24():
    """The analytic sphere r = 0.6 on meshing_cases' 24^3 grid: 2 702 vertices, 5 400 faces -> (verts, faces, voxel)"""
    lo, h = np.float32(mc.GRID_LO), np.float32(mc.GRID_H)
    x, y, z = (lo.astype(np.float64) + c * float(h) for c in mc.grid_xyz((mc.GRID_N,) * 3))
    field = torch.from_numpy((np.sqrt(x * x + y * y + z * z) - mc.SPHERE_R).astype(np.float32))
    from voge_amd.Meshing import extract_mesh
    v, f = extract_mesh(field, lo=[float(lo)] * 3, voxel_size=float(h))
    return v, f.long(), float(h)


BOX_HALF = 0.613
BOX_N = 33


@functools.lru_cache(maxsize=None)
def box33():
    """The box |x|, |y|, |z| <= 0.613 (the field max(|x|, |y|, |z|) - 0.613) on a 33^3 grid over [-1, 1]^3 -> (verts, faces, voxel)"""
    g = np.linspace(-1.0, 1.0, BOX_N)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    field = torch.from_numpy((np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z)) - BOX_HALF).astype(np.float32))
    from voge_amd.Meshing import extract_mesh
    h = 2.0 / (BOX_N - 1)
    v, f = extract_mesh(field, lo=[-1.0] * 3, voxel_size=h)
    return v, f.long(), h


def worst_corner_distance(verts):
    """The largest distance from a corner of the box to its nearest vertex"""
    c = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float64) * BOX_HALF
    return float((verts.double()[None] - c[:, None]).norm(dim=-1).min(1).values.max())


def small_soup():
    """Eight vertices, one per unit cell at cell size 1, and six faces: 1 repeats 0 rotated, 2 is 0 reversed, 3 names a vertex twice,
    4 is its own triple, 5 repeats 4"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float64) + 0.25
    f = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [3, 3, 4], [5, 6, 7], [5, 6, 7]])
    return _mesh(v, f)


def attr_of(verts, C, seed=5):
    """[V,C] fp32: smooth in the position plus noise, channels of very different size"""
    rng = np.random.default_rng(seed + C)
    v = verts.double().numpy()
    a = np.concatenate([v, np.sin(3 * v), 1e3 * v, 1e-3 * rng.standard_normal((len(v), 3))], -1)[:, :C]
    return torch.from_numpy((a + 0.01 * rng.standard_normal(a.shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def one_cell(n=20000, seed=6):
    """n vertices inside one cell (cell size 1) and two vertices in cells of their own, a few faces between them: ONE slot of the
    table is lowered n times"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(0.0, 0.999, (n, 3)), [[2.5, 0.5, 0.5], [0.5, 2.5, 0.5]]])
    v[0] = 0.0      # (lo: the cell grid starts here)
    i = rng.integers(0, n, 64)
    f = np.stack([i, np.full(64, n), np.full(64, n + 1)], -1)
    return _mesh(v, f)


@functools.lru_cache(maxsize=None)
def one_triple(F=20000, seed=7):
    """Three clusters of seven vertices and F faces between them, every one the same triple (in the three rotations): ONE slot of the
    face table is lowered F times; face 0 stays"""
    rng = np.random.default_rng(seed)
    base = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    v = (base[:, None] + rng.uniform(0.0, 0.9, (3, 7, 3))).reshape(-1, 3)
    v[0] = 0.0
    f = np.stack([rng.integers(0, 7, F), 7 + rng.integers(0, 7, F), 14 + rng.integers(0, 7, F)], -1)
    turn = rng.integers(0, 3, F)
    f = np.stack([f[np.arange(F), (turn + k) % 3] for k in range(3)], -1)
    return _mesh(v, f)


@functools.lru_cache(maxsize=None)
def lattice(n=16, seed=8):
    """n^3 = 4096 vertices, one per cell at cell size 1 (V a power of two: the table exactly half full of distinct keys), faces
    between lattice neighbours"""
    rng = np.random.default_rng(seed)
    k = np.arange(n ** 3)
    v = np.stack([k % n, (k // n) % n, k // (n * n)], -1) + rng.uniform(0.1, 0.9, (n ** 3, 3))
    v[0] = 0.0
    i = rng.integers(0, n ** 3 - n * n - n - 1, 6000)
    f = np.stack([i, i + 1, i + n], -1)
    return _mesh(v, f)


@functools.lru_cache(maxsize=None)
def stepped(V, F=700, seed=9):
    """V random vertices and F local faces: V at 2^k - 1, 2^k, 2^k + 1 steps the table's capacity"""
    return mcc.sized(V, F, seed)


def extraction_cells():
    """(name, verts, faces, cell_size) of the four extractions of mesh_clean_cases (voxel 1) at 0.5, 1, 2 and 3.7 voxels and an
    anisotropic cell"""
    out = []
    for name in mcc.EXTRACTION_COMPONENTS:
        v, f = mcc.extraction(name)
        out += [(f"{name}, cell {h}", v, f, h) for h in (0.5, 1.0, 2.0, 3.7, (1.5, 2.0, 0.7))]
    return out


def other_cases():
    """(name, verts, faces, cell_size) of everything but the extractions"""
    sv, sf = mcc.extraction("sphere")
    out = [("soup", *mcc.soup(), 0.5), ("translated sphere", sv + 1000.0, sf, 2.0), ("small soup", *small_soup(), 1.0)]
    out += [(f"sized V {V} F {F}", *mcc.sized(V, F), 0.3 if V < 1000 else 0.04) for V, F in mcc.SIZES]
    out += [(f"stepped V {V}", *stepped(V), 0.25) for V in (1023, 1024, 1025)]
    out += [("one cell", *one_cell(), 1.0), ("one triple", *one_triple(), 1.0), ("lattice", *lattice(), 1.0)]
    return out


def all_cases():
    return extraction_cells() + other_cases()


CASE_NAMES = [c[0] for c in extraction_cells()] + ["soup", "translated sphere", "small soup"] + [f"sized V {V} F {F}" for V, F in mcc.SIZES] + \
    [f"stepped V {V}" for V in (1023, 1024, 1025)] + ["one cell", "one triple", "lattice"]


@functools.lru_cache(maxsize=None)
def case(name):
    for c in all_cases():
        if c[0] == name:
            return c[1:]
    raise KeyError(name)
