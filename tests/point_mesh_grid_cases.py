"""Cases and a numpy restatement of the grid route of the point-to-mesh searches (voge_amd/csrc/point_mesh_grid.h), shared by
tests/test_point_mesh_grid_cpu.py and tests/test_gpu_point_mesh_grid.py.

The cases are a few thousand items at most and cover what the grid route adds to the brute force: the large list (empty, one
entry, more than one LDS tile, everything), degenerate faces, a coordinate offset, long walks, a flat grid, exact ties, ragged
sizes and forced cells.  `model` restates the cell arithmetic in fp32 -- the half-extents, the classification, the cells -- with
the constants ops mirrors as POINT_MESH_GRID_*; `walk` restates the ring walk and its stopping rule on a matrix of keys.  The grid
itself is chosen by `choose_grid`, the rule of the device's kernel in Python floats: the proof the tests make holds on any grid,
so nothing depends on the device choosing the same cell to the last bit."""
import functools
import importlib.util
import math
import os

import numpy as np
import torch

import point_mesh_cases as cases
import sample_meshes
from voge_amd import Aggregation, ops

F32 = np.float32
MAX_KEY = np.int64(2 ** 63 - 1)


def _ico(level):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("shape_fitting_demo_meshes", os.path.join(root, "demo", "ShapeFitting.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    v, f = demo.ico_sphere(level)
    return torch.from_numpy(v).float(), torch.from_numpy(f).long()


def _random_triangles(n, size, seed, centre=0.5):
    """n triangles of about `size` across, anywhere in the unit cube around `centre` -> (verts [3n,3], faces [n,3])"""
    rng = np.random.default_rng(seed)
    c = centre + (rng.random((n, 1, 3)) - 0.5)
    v = (c + (rng.random((n, 3, 3)) - 0.5) * size).reshape(-1, 3)
    return torch.from_numpy(v.astype(np.float32)), torch.arange(3 * n).reshape(n, 3)


def _join(*meshes):
    verts, faces, at = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(f.long() + at)
        at += len(v)
    return torch.cat(verts), torch.cat(faces)


def _case_icosphere():
    v, f = _ico(4)                                                    # the cfg5 icosphere: 5 120 faces
    return v, f, cases.points_around(v, f, 5000, seed=1)


def _case_soup_mixed():
    v, f = _join(cases.soup(544), _random_triangles(40, 0.9, 2))     # small triangles in cells, 40 large ones in the list
    return v, f, cases.points_around(v, f, 1500, seed=2)


def _case_one_spanning():
    v, f = sample_meshes.grid_mesh(32, 32, jitter=0.3, seed=3)
    span = torch.tensor([[-0.2, -0.2, -0.3], [1.3, -0.1, 0.4], [0.4, 1.3, 0.2]])
    v, f = _join((v, f[:2000]), (span, torch.tensor([[0, 1, 2]])))
    return v, f, cases.points_around(v, f, 1000, seed=3)


def _case_300_large():
    # 3 200 small faces keep the mean extent, and so the cell, small: the 300 are more than one LDS tile of the large list
    v, f = _join(sample_meshes.grid_mesh(40, 40, jitter=0.3, seed=4), _random_triangles(300, 1.2, 4))
    return v, f, cases.points_around(v, f, 700, seed=4)


def _case_all_large():
    """400 triangles about as large as the box.  The default cell's floor follows them (they are small then); the forced small
    cell of cell_sizes() leaves every one of them large and the cell table empty."""
    v, f = _random_triangles(400, 1.0, 5)
    return v, f, cases.points_around(v, f, 500, seed=5)


def _case_none_large():
    v, f = cases.level2_sphere()
    return v.float(), f, cases.points_around(v, f, 700, seed=6)


def _case_degenerate():
    v, f = cases.all_test_meshes()["zero-area grid"]
    pts = torch.tensor([[0, 0, 0], [5, 5, 5], [17, 17, 17]])         # three faces that are points
    f = torch.cat((f, pts))
    return v, f, cases.points_around(v, f, 500, seed=7)


def _case_edges():
    from voge_amd.Losses import MeshTopology
    v, f = cases.level2_sphere()
    e = MeshTopology(faces=f).edges.long()
    return v.float(), e[:, [0, 1, 1]].contiguous(), cases.points_around(v, f, 400, seed=8)


def _case_offset():
    v, f = cases.level2_sphere()
    shift = torch.tensor([1000.0, 1000.0, 1000.0])
    return v.float() + shift, f, cases.points_around(v, f, 700, seed=9) + shift


def _case_far_points():
    v, f = cases.level2_sphere()
    rng = np.random.default_rng(10)
    d = rng.normal(size=(300, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(8.0, 40.0, (300, 1))
    return v.float(), f, torch.cat((torch.from_numpy(far.astype(np.float32)), cases.points_around(v, f, 100, seed=10)))


def _case_points_in_one_cell():
    v, f = cases.level2_sphere()
    rng = np.random.default_rng(11)
    p = np.array([0.55, 0.6, 0.62]) + rng.uniform(-1e-3, 1e-3, (400, 3))
    return v.float(), f, torch.from_numpy(p.astype(np.float32))


def _case_flat():
    v, f = sample_meshes.grid_mesh(20, 20, jitter=0.3, seed=12, lift=False)
    v = v.clone()
    v[:, 2] = 0.0
    rng = np.random.default_rng(12)
    p = np.concatenate((rng.uniform(-0.5, 1.5, (600, 2)), np.zeros((600, 1))), 1)      # coplanar with the mesh: G_z = 1
    p[::8] = v[rng.integers(len(v), size=len(p[::8]))].numpy()
    return v, f, torch.from_numpy(p.astype(np.float32))


def _case_duplicated_faces():
    v, f = cases.level2_sphere()
    return v.float(), torch.cat((f, f)), cases.points_around(v, f, 500, seed=13)


def _case_points_on_vertices():
    v, f = cases.level2_sphere()
    return v.float(), f, v.float().clone()                            # d2 = 0 on five or six faces each: the lowest index wins


def _case_one_point():
    v, f = cases.soup(131)
    return v, f, torch.tensor([[0.4, 0.6, 0.3]])


def _case_one_face():
    v, f = sample_meshes.ONE_FACE
    return v, f, cases.points_around(v, f, 67, seed=15)


def _case_ragged():
    v, f = cases.soup(131)
    return v, f, cases.points_around(v, f, 67, seed=16)


def _case_rod():
    """800 faces along x, 100 long and 0.2 wide: a small forced cell drives G_x to the axis limit (cell = extent / 1023)"""
    v, f = sample_meshes.grid_mesh(200, 2, jitter=0.2, seed=17)
    v = v * torch.tensor([100.0, 0.2, 0.2])
    rng = np.random.default_rng(17)
    p = rng.uniform([0.0, -0.05, -0.05], [100.0, 0.25, 0.1], (300, 3))      # along the rod: the box stays thin
    p[::8] = v[rng.integers(len(v), size=len(p[::8]))].numpy()
    return v, f, torch.from_numpy(p.astype(np.float32))


def _case_nan_vertex():
    v, f = cases.level2_sphere()
    v = v.float().clone()
    v[7, 1] = float("nan")                                            # its faces' records are not finite: the large list, never a winner
    p = cases.points_around(torch.nan_to_num(v), f, 300, seed=18)
    return v, f, p


_BUILDERS = {"icosphere": _case_icosphere, "soup, mixed sizes": _case_soup_mixed, "one spanning triangle": _case_one_spanning,
             "300 large": _case_300_large, "all large": _case_all_large, "none large": _case_none_large, "degenerate faces": _case_degenerate,
             "edge mesh": _case_edges, "offset 1000": _case_offset, "far points": _case_far_points,
             "points in one cell": _case_points_in_one_cell, "flat": _case_flat, "duplicated faces": _case_duplicated_faces,
             "points on vertices": _case_points_on_vertices, "one point": _case_one_point, "one face": _case_one_face,
             "ragged": _case_ragged, "rod": _case_rod, "nan vertex": _case_nan_vertex}
NAMES = tuple(_BUILDERS)
NOT_FINITE = ("nan vertex",)           # compared with the brute route bit for bit, never with fp64
HAS_TIES = ("duplicated faces", "points on vertices", "degenerate faces", "edge mesh", "nan vertex")


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts [V,3] fp32, faces [F,3] int64, points [P,3] fp32) on the host, built once"""
    v, f, p = _BUILDERS[name]()
    return v.float().contiguous(), f.long().contiguous(), p.float().contiguous()


def cell_sizes(name):
    """The three cells a case is searched with: the default, one so small that the rule's enlargement decides (on the rod: G_x at the
    axis limit), one so large that the grid is one cell"""
    v, _, p = case(name)
    both = torch.nan_to_num(torch.cat((v, p)))
    ext = max(float((both.max(0).values - both.min(0).values).max()), 1e-3)
    return (None, ext / 4000.0, ext * 4.0)


# ---- the grid route restated ----------------------------------------------------------------------------------------------------

def tri_boxes(verts, faces):
    """fp32 (centre [F,3], h [F], finite [F]) of pm_grid_tribox"""
    with np.errstate(invalid="ignore", over="ignore"):
        tri = verts.numpy()[faces.numpy()]
        lo, hi = tri.min(1), tri.max(1)
        mid = np.minimum(np.maximum(F32(0.5) * lo + F32(0.5) * hi, lo), hi)
        h = np.maximum(hi - mid, mid - lo).max(1) * F32(ops.POINT_MESH_GRID_HALF_UP)
        fin = np.isfinite(tri).all((1, 2)) & np.isfinite(h)
    mid = np.where(fin[:, None], mid, F32(0.0)).astype(F32)
    return mid, np.where(fin, h, F32(np.inf)).astype(F32), fin


def choose_grid(lo, hi, F, P, mean_extent, cell_size=None):
    """(cell fp32, gx, gy, gz) by pm_grid_choose_kernel's rule: ops.knn_grid with n = max(F, P) and the floor on the default cell"""
    n = max(F, P)
    if cell_size is None:
        ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
        pos = [e for e in ext if e > 0.0]
        cell = 1.0
        if pos:
            cell = (math.prod(pos) / (2.0 * max(n, 1))) ** (1.0 / len(pos))
        if mean_extent > 0.0 and math.isfinite(mean_extent):
            cell = max(cell, ops.POINT_MESH_GRID_FLOOR * mean_extent)
        cell_size = cell
    return ops.knn_grid(lo, hi, n, cell_size)


def axis_cells(x, lo, inv, g):
    with np.errstate(invalid="ignore"):
        u = np.floor((x.astype(F32) - F32(lo)) * F32(inv))
    return np.minimum(np.maximum(np.nan_to_num(u, nan=0.0), 0), g - 1).astype(np.int32)


def model(name, cell_size=None):
    """The grid and the binning of a case: dict(cell, g, H, pcell [P,3], fcell [F,3], h [F], small [F])"""
    v, f, p = case(name)
    both = torch.cat((v, p)).numpy()
    lo, hi = np.nanmin(both, 0), np.nanmax(both, 0)
    mid, h, fin = tri_boxes(v, f)
    mean_extent = float((2.0 * h[fin].astype(np.float64)).sum() / len(f))
    cell, gx, gy, gz = choose_grid(lo, hi, len(f), len(p), mean_extent, cell_size)
    cell = F32(cell)
    inv = F32(1.0) / cell
    g = (gx, gy, gz)
    H = F32(ops.POINT_MESH_GRID_BIG) * cell
    pcell = np.stack([axis_cells(p.numpy()[:, a], lo[a], inv, g[a]) for a in range(3)], 1)
    fcell = np.stack([axis_cells(mid[:, a], lo[a], inv, g[a]) for a in range(3)], 1)
    return dict(cell=cell, g=g, H=H, pcell=pcell, fcell=fcell, h=h, small=fin & (h <= H))


def d2_matrix32(name):
    """fp32 [P,F]: the definition's d2 of every pair, on the host (the bits the kernels' pm_pair returns)"""
    return _d2_matrix32(name)


@functools.lru_cache(maxsize=4)
def _d2_matrix32(name):
    v, f, p = case(name)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    chunk = max(1, (1 << 21) // len(f))
    return torch.cat([Aggregation.point_triangle_closest(p[s:s + chunk, None], a, b, c)[0] for s in range(0, len(p), chunk)])


def keys_of(d2, by_face=False):
    """int64 [Q,N] keys (d2 bits << 32 | index) of a [P,F] matrix of fp32 d2 >= 0 (or NaN), queries along the rows"""
    m = d2.t().contiguous() if by_face else d2
    bits = m.numpy().view(np.int32).astype(np.int64)
    return (bits << 32) | np.arange(m.shape[1], dtype=np.int64)[None, :]


def walk(keys, ring, rmax, cell, hq, has_rings=True):
    """The ring walk and its stopping rule.  keys [Q,N] int64; ring [Q,N]: the ring at which a query meets an item, -1 for an
    item it met before the walk (the large list); rmax [Q]: the ring at which a query's cube covers the grid; hq [Q] fp32: H or
    the query's own h_f.  -> (kept key [Q], the ring after which each query stopped [Q]; -1: no walk)."""
    Q = keys.shape[0]
    pre = ring < 0
    kept = np.where(pre, keys, MAX_KEY).min(1) if pre.any() else np.full(Q, MAX_KEY)
    stop = np.full(Q, -1, np.int64)
    if not has_rings:
        return kept, stop
    active = np.arange(Q)
    one, slack = F32(1.0), F32(ops.POINT_MESH_GRID_RING_SLACK)
    m, m_h, b_min = F32(ops.POINT_MESH_GRID_M), F32(ops.POINT_MESH_GRID_M_H), F32(ops.POINT_MESH_GRID_B_MIN)
    r = 0
    while len(active):
        met = ring[active] == r
        kept[active] = np.minimum(kept[active], np.where(met, keys[active], MAX_KEY).min(1))
        with np.errstate(invalid="ignore", over="ignore"):
            X = cell * (F32(r) - slack) - hq[active]
            b = X * (one - m) - m_h * hq[active]
            kept_d2 = (kept[active] >> 32).astype(np.int32).view(F32)
            fire = (kept[active] != MAX_KEY) & (b > b_min) & (kept_d2 <= b * b)
        done = fire | (rmax[active] <= r)
        stop[active[done]] = r
        active = active[~done]
        r += 1
    return kept, stop


def search_model(name, cell_size=None, by_face=False):
    """One direction of a case by the restated grid route -> dict(kept [Q] keys, stop [Q] rings, keys [Q,N], ring [Q,N], model)"""
    mdl = model(name, cell_size)
    keys = keys_of(d2_matrix32(name), by_face)
    g = np.array(mdl["g"])
    qc, ic = (mdl["fcell"], mdl["pcell"]) if by_face else (mdl["pcell"], mdl["fcell"])
    ring = np.abs(qc[:, None, :].astype(np.int16) - ic[None, :, :].astype(np.int16)).max(2)
    rmax = np.maximum(qc, g[None, :] - 1 - qc).max(1)
    if by_face:
        kept, stop = walk(keys, ring, rmax, mdl["cell"], mdl["h"])
    else:
        ring = np.where(mdl["small"][None, :], ring, np.int16(-1))
        hq = np.full(len(qc), mdl["H"], F32)
        kept, stop = walk(keys, ring, rmax, mdl["cell"], hq, has_rings=bool(mdl["small"].any()))
    return dict(kept=kept, stop=stop, keys=keys, ring=ring, model=mdl)
