"""Meshes, an independent reference and the derived bound shared by tests/test_mesh_clean_cpu.py and tests/test_gpu_mesh_clean.py.

reference   components() is a plain union-find over Python lists (path halving, the smaller root wins), written without a look at
            Aggregation.mesh_components' label propagation; clean() and brute_force_keep() rank and filter with numpy.  Labels, counts
            and index tables are integers: every comparison with them is torch.equal / array_equal.

normals     NORMAL_BOUND, derived from the arithmetic voge_amd/csrc/mesh_clean.hip's header documents, never fitted to what the
            kernels return; eps = 2^-24.  Kernel, fp32 definition and the fp64 reference start from the same fp32 positions.
            A component of cr_f = (b - a) x (c - a) is (p q) - (r s) of ROUNDED differences: p, q, r, s carry one rounding each, the
            products one, the difference one -- four roundings on any path to the component, each eps relative of a partial result
            bounded by M_c = |p q| + |r s| (4.01 covers the second-order terms), as in sample_meshes.py:
                |delta cr_fc| <= 4.01 eps M_fc.
            The vertex sum is fp64 in the definition (2^-53 relative of sum |terms|: covered by the 0.01 above) and fixed point in
            the kernel: every one of the m corners that name the vertex adds round(cr 2^s), off by at most q / 2 with q = 2^-s,
            s = 62 - L - e, 2^L >= 3 F, 2^e > D >= 2^(e - 1), D the largest |cr| component: q <= 2^(L - 61) D.  So per component
                E_vc <= sum over the corners of 4.01 eps M_fc + m q / 2.
            A unit vector moves by at most 2 |delta| / |n| when n moves by delta (|n + delta| >= |n| - |delta| twice), a component by
            no more than the vector; norm and quotient are fp64 and the one rounding to fp32 is at most eps of a component <= 1:
                |delta normal_vc| <= 2 |E_v| / |n_v| + eps + 2^-40.
            The bound says nothing where the sum cancels: a vertex with |n_v| / sum |cr_f| < 1 / 32 is left out, and the tests assert
            that at most 1 % of a case's used vertices are."""
import functools
import math

import numpy as np
import torch

import meshing_cases as mc
from voge_amd import Aggregation

EPS = 2.0 ** -24
SCAN_BLOCK = 256            # ops.MESH_CLEAN_BLOCK, asserted by the GPU tests
SCAN_TOP = 1024             # ops.MESH_CLEAN_TOP
RATIO_FLOOR = 1.0 / 32
LEFT_OUT_CAP = 0.01


# ---- the independent reference ------------------------------------------------------------------------------------------------

def components(faces, V):
    """(vert_label [V], face_label [F], num_components) int64 numpy: a component's label is its smallest vertex index"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= V):
        raise ValueError("index outside [0, V)")
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i0, i1, i2 in f.tolist():
        for other in (i1, i2):
            ra, rb = find(i0), find(other)
            if ra != rb:
                if ra < rb:
                    parent[rb] = ra
                else:
                    parent[ra] = rb
    vert_label = np.array([find(x) for x in range(V)], np.int64).reshape(V)
    face_label = vert_label[f[:, 0]] if len(f) else np.zeros((0,), np.int64)
    return vert_label, face_label, len(set(face_label.tolist()))


def brute_force_keep(face_label, V, keep_largest=None, min_faces=1):
    """The set of labels that stay: components sorted by (-faces, label), the first keep_largest of those with >= min_faces faces"""
    labels, counts = np.unique(face_label, return_counts=True)
    ranked = sorted(zip((-counts).tolist(), labels.tolist()))
    ranked = [(c, l) for c, l in ranked if -c >= min_faces]
    if keep_largest is not None:
        ranked = ranked[:keep_largest]
    return set(l for _, l in ranked)


def clean(verts, faces, keep_largest=None, min_faces=1):
    """(verts', faces', vert_index, face_index) as numpy, from components() and brute_force_keep()"""
    v, f = np.asarray(verts), np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    _, face_label, _ = components(f, V)
    keep = brute_force_keep(face_label, V, keep_largest, min_faces)
    face_index = np.array([i for i, l in enumerate(face_label.tolist()) if l in keep], np.int64)
    kept = f[face_index]
    vert_index = np.unique(kept.reshape(-1)) if len(kept) else np.zeros((0,), np.int64)
    new_id = np.full(V, -1, np.int64)
    new_id[vert_index] = np.arange(len(vert_index))
    return v[vert_index], new_id[kept].reshape(-1, 3), vert_index, face_index


# ---- the normal bound ---------------------------------------------------------------------------------------------------------

def normal_bound(verts, faces, fixed_point=True):
    """(reference normals [V,3] fp64, bound [V] on every component, compared [V] bool, used [V] bool) from fp32 verts and integer
    faces: NORMAL_BOUND of the header.  fixed_point=False leaves out the kernel's m q / 2."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    a = v[f[:, 0]]
    e1, e2 = v[f[:, 1]] - a, v[f[:, 2]] - a
    cr = np.cross(e1, e2)
    M = np.stack([np.abs(e1[:, 1] * e2[:, 2]) + np.abs(e1[:, 2] * e2[:, 1]), np.abs(e1[:, 2] * e2[:, 0]) + np.abs(e1[:, 0] * e2[:, 2]),
                  np.abs(e1[:, 0] * e2[:, 1]) + np.abs(e1[:, 1] * e2[:, 0])], -1)
    corners = f.reshape(-1)
    n = np.zeros((V, 3))
    E = np.zeros((V, 3))
    mass = np.zeros(V)
    np.add.at(n, corners, np.repeat(cr, 3, 0))
    np.add.at(E, corners, np.repeat(4.01 * EPS * M, 3, 0))
    np.add.at(mass, corners, np.repeat(np.linalg.norm(cr, axis=-1), 3))
    m = np.bincount(corners, minlength=V).astype(np.float64)
    if fixed_point and F:
        L = max(0, math.ceil(math.log2(3 * F)))
        D = float(np.abs(cr).max()) * (1 + 2.0 ** -20)      # (the kernel's D is the fp32 one: within 4.01 eps of this)
        E = E + (m * 2.0 ** (L - 61) * D / 2)[:, None]
    norm = np.linalg.norm(n, axis=-1)
    used = m > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(mass > 0, norm / mass, 0.0)
        ref = np.where((norm > 0)[:, None], n / norm[:, None], 0.0)
        bound = 2 * np.linalg.norm(E, axis=-1) / norm + EPS + 2.0 ** -40
    compared = used & (ratio >= RATIO_FLOOR)
    return ref, bound, compared, used


def check_normals(label, got, verts, faces, fixed_point=True, log=None):
    """Assert got [V,3] against the fp64 reference at NORMAL_BOUND and the cap on the vertices left out -> the share of the bound used"""
    ref, bound, compared, used = normal_bound(verts, faces, fixed_point)
    got = np.asarray(got, np.float64)
    n_used = int(used.sum())
    left_out = int((used & ~compared).sum())
    err = np.abs(got - ref).max(-1) if len(got) else np.zeros(0)
    share = float((err[compared] / bound[compared]).max()) if compared.any() else 0.0
    line = (f"[parity] vertex_normals {label}: V {len(got)}, F {len(np.asarray(faces))}, {left_out} of {n_used} used vertices left out, "
            f"max error {float(err[compared].max()) if compared.any() else 0.0:.3e}, {share:.3f} of the bound")
    (log or print)(line)
    assert left_out <= LEFT_OUT_CAP * max(n_used, 1), line
    assert share <= 1.0, line
    assert (got[~used] == 0).all()
    return share


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _mesh(verts, faces):
    return torch.from_numpy(np.ascontiguousarray(verts, np.float32)), torch.from_numpy(np.ascontiguousarray(faces, np.int64).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def extraction(name):
    field = {"sphere": mc.sphere_field, "torus": mc.torus_field, "two spheres": mc.two_spheres_field, "random field": mc.random_field}[name]()
    v, f = Aggregation.marching_tets(field.double())
    return v.to(torch.float32), f


EXTRACTION_COMPONENTS = {"sphere": 1, "torus": 1, "two spheres": 2, "random field": 2}


@functools.lru_cache(maxsize=None)
def soup(V=1000, F=300, seed=0):
    """Random faces over V vertices: unused vertices, a duplicate face, a face that names a vertex twice and one that names it thrice"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V, (F, 3))
    f[10] = f[3]
    f[20, 1] = f[20, 0]
    f[21] = f[21, 0]
    f[22] = f[5][[1, 2, 0]]
    return _mesh(rng.standard_normal((V, 3)), f)


@functools.lru_cache(maxsize=None)
def strip(order, F=100000, seed=1):
    """A triangle strip of F faces, its vertex indices 'ascending' along the strip, 'descending' or 'permuted' at random"""
    V = F + 2
    k = np.arange(V)
    rng = np.random.default_rng(seed)
    v = np.stack([0.01 * k, (k % 2) * 0.013, 0.002 * rng.standard_normal(V)], -1)
    i = np.arange(F)
    f = np.stack([i, i + 1 + (i % 2), i + 2 - (i % 2)], -1)      # consistent winding
    p = {"ascending": k, "descending": k[::-1].copy(), "permuted": rng.permutation(V)}[order]
    out = np.empty_like(v)
    out[p] = v
    return _mesh(out, p[f])


@functools.lru_cache(maxsize=None)
def fan(hub_last, F=20000):
    """F faces around one hub vertex (index 0, or the last index): every link contends for one address"""
    V = F + 2
    t = np.arange(F + 1) * (1.9 * np.pi / F)
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * np.sin(7 * t)], -1)
    hub = np.array([[0.0, 0.0, 0.3]])
    i = np.arange(F)
    if hub_last:
        return _mesh(np.concatenate([rim, hub]), np.stack([np.full(F, V - 1), i, i + 1], -1))
    return _mesh(np.concatenate([hub, rim]), np.stack([np.zeros(F, np.int64), i + 1, i + 2], -1))


@functools.lru_cache(maxsize=None)
def crumbs(n=20000, seed=2):
    """n disjoint triangles (equal face counts: the tie rule), pairs of them joined into two-face blobs, then the sphere"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4, 4, (n, 1, 3))
    tv = (centre + 0.05 * rng.standard_normal((n, 3, 3))).reshape(-1, 3)
    tf = np.arange(3 * n).reshape(n, 3)
    tf[1:400:2, 0] = tf[0:399:2, 1]      # 200 blobs of two faces sharing a vertex (one vertex of each pair becomes unused)
    sv, sf = extraction("sphere")
    return _mesh(np.concatenate([tv, sv.numpy()]), np.concatenate([tf, sf.numpy() + 3 * n]))


SIZES = tuple((V, F) for base in (SCAN_BLOCK, SCAN_BLOCK * SCAN_TOP) for V, F in ((base - 1, base + 1), (base, base), (base + 1, base - 1)))


@functools.lru_cache(maxsize=None)
def sized(V, F, seed=3):
    """Exactly V vertices and F faces of local random triangles: many components of different sizes, some vertices unused"""
    rng = np.random.default_rng(seed + V + F)
    i0 = rng.integers(0, V, F)
    f = np.stack([i0, (i0 + rng.integers(1, 3, F)) % V, (i0 + rng.integers(3, 5, F)) % V], -1)
    drop = rng.random(F) < 0.5      # half of the faces sit on a coarse lattice of vertices: gaps between the components
    f[drop] = (f[drop] // 8) * 8 + np.array([0, 1, 2])
    f = np.minimum(f, V - 1)
    return _mesh(rng.standard_normal((V, 3)), f)


def degenerate():
    z3 = np.zeros((0, 3))
    return [("no faces", *_mesh(np.random.default_rng(4).standard_normal((5, 3)), z3)), ("no vertices", *_mesh(z3, z3)),
            ("one face", *_mesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]]), np.array([[2, 0, 1]])))]


def small_cases():
    """(name, verts, faces) of every case but the sized ones"""
    out = [(name, *extraction(name)) for name in EXTRACTION_COMPONENTS]
    out.append(("soup", *soup()))
    out += [(f"strip {o}", *strip(o)) for o in ("ascending", "descending", "permuted")]
    out += [("fan, hub first", *fan(False)), ("fan, hub last", *fan(True)), ("crumbs", *crumbs())]
    return out + degenerate()


def sized_cases():
    return [(f"sized V {V} F {F}", *sized(V, F)) for V, F in SIZES]


def all_cases():
    return small_cases() + sized_cases()


CASE_NAMES = [c[0] for c in small_cases()] + [f"sized V {V} F {F}" for V, F in SIZES]


@functools.lru_cache(maxsize=None)
def case(name):
    for c in all_cases():
        if c[0] == name:
            return c[1], c[2]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference_components(name):
    verts, faces = case(name)
    return components(faces.numpy(), len(verts))
