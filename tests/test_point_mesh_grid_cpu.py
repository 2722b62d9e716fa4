"""CPU tests of the grid route of the point-to-mesh distance: the `route` keyword on host tensors, the size checks of the two
routes, the stopping rules of voge_amd/csrc/point_mesh_grid.h proven on every case of tests/point_mesh_grid_cases.py by a numpy
restatement of the cell arithmetic, and the argument checks of the new C entries (the library loads without a GPU: anything that
reached HIP would fail differently)."""
import os

import numpy as np
import pytest
import torch

import point_mesh_grid_cases as gc
from voge_amd import Losses, ops


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the keyword ------------------------------------------------------------------------------------------------------------------

def test_route_keyword_on_host_tensors():
    """Host tensors take the definition, which has no routes: every route returns what None returns, a bad one is refused."""
    v, f, p = gc.case("ragged")
    want = Losses.closest_faces(p, v, f)
    for route in ("grid", "brute", None):
        got = Losses.closest_faces(p, v, f, route=route)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), route
    e = f[:, :2].contiguous()
    for kw in ({}, {"single_directional": True, "point_reduction": "sum"}):
        want = Losses.point_mesh_face_distance(v, f, p, **kw)
        want_e = Losses.point_mesh_edge_distance(v, e, p, **kw)
        for route in ("grid", "brute"):
            assert torch.equal(Losses.point_mesh_face_distance(v, f, p, route=route, **kw), want)
            assert torch.equal(Losses.point_mesh_edge_distance(v, e, p, route=route, **kw), want_e)
    vb, pb = torch.stack((v, v * 1.1)), torch.stack((p, p - 0.1))
    assert torch.equal(Losses.point_mesh_face_distance(vb, f, pb, route="grid"), Losses.point_mesh_face_distance(vb, f, pb))
    for bad in ("Grid", "bvh", 2, ""):
        with pytest.raises(ValueError, match="route"):
            Losses.closest_faces(p, v, f, route=bad)
        with pytest.raises(ValueError, match="route"):
            Losses.point_mesh_face_distance(v, f, p, route=bad)
        with pytest.raises(ValueError, match="route"):
            Losses.point_mesh_edge_distance(v, e, p, route=bad)
    import VoGE.Losses
    assert VoGE.Losses.closest_faces is Losses.closest_faces


def test_the_pair_cap_binds_the_brute_route_and_none():
    side = 1 << 19
    assert ops.POINT_MESH_MAX_PAIRS == side * side
    for route in (None, "brute"):
        assert ops._point_mesh_route(route, side, side, "t") == ("grid" if route is None else "brute")      # the cap itself passes
        with pytest.raises(ValueError, match="chamfer_distance"):
            ops._point_mesh_route(route, side + 1, side, "t")
        with pytest.raises(ValueError, match='route="grid"'):
            ops._point_mesh_route(route, side, side + 1, "t")
    assert ops._point_mesh_route("grid", side + 1, side, "t") == "grid"
    assert ops._point_mesh_route("grid", ops.POINT_MESH_MAX_N, ops.POINT_MESH_MAX_N, "t") == "grid"
    with pytest.raises(ValueError):
        ops._point_mesh_route("grid", ops.POINT_MESH_MAX_N + 1, 10, "t")
    with pytest.raises(ValueError, match="route"):
        ops._point_mesh_route("fast", 10, 10, "t")
    # None: the brute force below the measured crossover, the grid from there on
    n = ops.POINT_MESH_GRID_MIN_PAIRS
    assert n & (n - 1) == 0 and n <= ops.POINT_MESH_MAX_PAIRS
    k = n.bit_length() - 1
    lo, hi = 1 << (k // 2), 1 << (k - k // 2)
    assert ops._point_mesh_route(None, lo, hi - 1, "t") == "brute" and ops._point_mesh_route(None, lo, hi, "t") == "grid"
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size"):
            ops._point_mesh_cell(bad, "t")
    assert ops._point_mesh_cell(None, "t") == 0.0 and ops._point_mesh_cell(0.25, "t") == 0.25


# ---- the stopping rules -----------------------------------------------------------------------------------------------------------

def _combos():
    out = []
    for name in gc.NAMES:
        for k, tag in enumerate(("default", "small", "huge")):
            if name == "icosphere" and tag != "default":
                continue      # (25.6 million pairs a matrix: the forced cells are proven on the smaller cases)
            out.append(pytest.param(name, k, id=f"{name}-{tag}"))
    return out


@pytest.mark.parametrize("name,which", _combos())
def test_stopping_rules_never_skip_the_winner(name, which):
    """For every query of the case, in both directions: the key the restated walk keeps is the brute-force minimum, and every item
    outside the cube it visited has an fp32 d2 (the definition's, on the host) STRICTLY above the kept one -- no tie is missed."""
    cell_size = gc.cell_sizes(name)[which]
    for by_face in (False, True):
        s = gc.search_model(name, cell_size, by_face)
        keys, ring, kept, stop = s["keys"], s["ring"], s["kept"], s["stop"]
        assert (kept == keys.min(1)).all(), (name, by_face, int((kept != keys.min(1)).sum()))
        unvisited = ring > stop[:, None]
        assert ((keys >> 32) > (kept >> 32)[:, None])[unvisited].all(), (name, by_face)
        mdl = s["model"]
        if by_face:
            continue
        small, g = mdl["small"], mdl["g"]
        if which == 2:
            assert g == (1, 1, 1)
        if name == "rod" and which == 1:
            assert g[0] >= 1023 and not small.any()      # cell = extent / 1023, the axis limit (1023 or 1024 by its rounding)
        if name == "all large" and which == 1:
            assert not small.any()                                   # the cell table is empty
        if which == 0:
            if name == "one spanning triangle":
                assert int((~small).sum()) == 1 and not small[-1]
            if name == "300 large":
                assert int((~small).sum()) > ops.POINT_MESH_GRID_LARGE_TILE and small.sum() > 1000
            if name == "soup, mixed sizes":
                assert 0 < int((~small).sum()) <= 40 and small.sum() >= 500
            if name in ("none large", "icosphere"):
                assert small.all()
            if name == "flat":
                assert g[2] == 1 and min(g[:2]) > 4
            if name == "points in one cell":
                assert (mdl["pcell"] == mdl["pcell"][0]).all() and max(g) > 4
            if name == "far points":
                assert int(stop.max()) >= 3                          # a far point walks until its cube reaches the mesh
            if name == "nan vertex":
                assert 0 < int((~small).sum()) <= 6


def test_the_rule_cannot_fire_before_the_bound_is_positive():
    """b of the header: negative at r <= kPmGridBig (nothing is proven yet), 0.987 cell at r = 2 with H = cell, and below the
    distance every unvisited triangle is proven to keep: cell (r - 2^-11) - H."""
    cell = np.float32(0.37)
    H = np.float32(ops.POINT_MESH_GRID_BIG) * cell
    for r in range(0, 1024):
        X = cell * (np.float32(r) - np.float32(ops.POINT_MESH_GRID_RING_SLACK)) - H
        b = X * (np.float32(1) - np.float32(ops.POINT_MESH_GRID_M)) - np.float32(ops.POINT_MESH_GRID_M_H) * H
        proven = float(cell) * (r - 2.0 ** -11) - float(H)
        if r <= 1:
            assert b < 0
        else:
            # the derivation's inequality: sqrt(fp32 d2) >= d (1 - 2^-9) - 3.47 2^-9 H > b (1 + 2^-23) for every d > proven
            assert float(b) * (1 + 2.0 ** -23) < proven * (1 - 2.0 ** -9) - 3.47 * 2.0 ** -9 * float(H)
    assert abs(float(cell * (np.float32(2) - np.float32(2.0 ** -10)) - H) / float(cell) - 1.0) < 2.0 ** -9


# ---- the C entries ----------------------------------------------------------------------------------------------------------------

def test_grid_entries_validate_before_any_hip_call(lib):
    """No GPU in this container: anything that reached HIP would fail differently."""
    Q = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    BAD, WS = -1, -2
    big = (1 << 28) - 1
    side = 1 << 19
    need = lib.voge_point_mesh_grid_workspace_bytes(10, 20, 30)
    assert need % 16 == 0 and need >= 64 + 20 * 64 + 30 * 16 + 4 * 32768 * 4
    assert need >= lib.voge_point_mesh_workspace_bytes(10, 20, 30)                    # it serves the backward too
    for V, F, P in ((0, 20, 30), (10, 0, 30), (10, 20, 0), (big + 1, 20, 30), (10, big + 1, 30), (10, 20, big + 1)):
        assert lib.voge_point_mesh_grid_workspace_bytes(V, F, P) == 0
    assert lib.voge_point_mesh_grid_workspace_bytes(side, side + 1, side) > 0        # above the pair cap: a size like any other
    huge = lib.voge_point_mesh_grid_workspace_bytes(big, big, big)
    assert 0 < huge < 1 << 40
    # voge_closest_faces_grid(points, P, verts, V, faces, F, cell_size, face_idx, d2, bary, ws, ws_bytes, stream)
    ok = [Q, 30, Q, 10, Q, 20, 0.0, Q, Q, Q, Q, need]

    def cf(**change):
        a = list(ok)
        for k, val in change.items():
            a[int(k[1:])] = val
        return lib.voge_closest_faces_grid(*a, None)
    assert cf(a1=0) == 0 and lib.voge_closest_faces_grid(None, 0, None, 10, None, 20, 0.0, None, None, None, None, 0, None) == 0
    for k in (0, 2, 4, 7, 8, 9, 10):
        assert cf(**{f"a{k}": None}) == BAD, k
    assert cf(a1=-1) == BAD and cf(a1=big + 1) == BAD
    for k in (3, 5):
        assert cf(**{f"a{k}": 0}) == BAD and cf(**{f"a{k}": big + 1}) == BAD, k
    for cell in (-1.0, float("inf"), float("nan")):
        assert cf(a6=cell) == BAD, cell
    assert cf(a10=Q + 8) == BAD and cf(a11=need - 1) == WS
    assert cf(a1=side + 1, a5=side, a11=16) == WS                                     # above the pair cap: only the workspace is short
    assert lib.voge_closest_faces(Q, side + 1, Q, 10, Q, side, Q, Q, Q, None) == -3   # where the brute entry still refuses
    # voge_point_mesh_fwd_grid(verts, V, faces, F, points, P, flags, cell_size, loss, face_idx, bary_p, point_idx, bary_f, meta, ws, bytes, stream)
    okf = [Q, 10, Q, 20, Q, 30, 0, 0.0, Q, Q, Q, Q, Q, Q, Q, need]

    def fwd(**change):
        a = list(okf)
        for k, val in change.items():
            a[int(k[1:])] = val
        return lib.voge_point_mesh_fwd_grid(*a, None)
    for k in (0, 2, 4, 8, 9, 10, 11, 12, 13, 14):
        assert fwd(**{f"a{k}": None}) == BAD, k
    for k in (1, 3, 5):
        assert fwd(**{f"a{k}": 0}) == BAD and fwd(**{f"a{k}": big + 1}) == BAD, k
    assert fwd(a6=4) == BAD and fwd(a7=-0.5) == BAD and fwd(a7=float("nan")) == BAD and fwd(a14=Q + 8) == BAD
    assert fwd(a15=need - 1) == WS
    assert fwd(a3=side, a5=side + 1, a15=16) == WS
    assert fwd(a6=2, a11=None, a12=None, a15=need - 1) == WS      # single-directional: the two tables may be null
    # the backward's flag bit 2 lifts its pair cap and nothing else
    okb = [Q, 10, Q, side, Q, side + 1, Q, Q, Q, Q, Q, Q, 0, Q, Q, Q, 16]
    assert lib.voge_point_mesh_bwd(*okb, None) == -3
    okb[12] = 4
    assert lib.voge_point_mesh_bwd(*okb, None) == WS
    okb[12] = 8
    assert lib.voge_point_mesh_bwd(*okb, None) == BAD
