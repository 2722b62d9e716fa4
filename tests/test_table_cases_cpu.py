"""CPU proof of what tests/test_gpu_accumulation_tables.py relies on: every case of tests/table_cases.py sends the keys it claims
down the straight-to-memory path of its kernel's accumulation table -- under BOTH extreme orders of the lanes inside a look-up --,
the fp32 evaluation of the reference alone stays within TOL / 4 of scale, and a lost memory-path term would be seen: every such
slot's own contribution to the per-Gaussian output is at least 10 TOL of the scale util.grad_close divides by (the fused backward's
slots carry the composite's gradients, which decay along a list: there a number of such slots is asserted instead of all).
Nothing in this file measures a kernel."""
import numpy as np
import pytest
import torch

import oracle
import table_cases as T
import test_attr_routes_cpu as A
from util import TOL, log_line

ORDERS = ("asc", "desc")
POOL_SLOTS = set(range(120, 128)) | set(range(0, 8))


def _scaled(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(1.0, float(np.abs(b).max()))


def _log_tiles(label, order, tiles):
    rows = ", ".join(f"({t['x0']},{t['y0']}) {len(t['tabled'])}/{len(t['memory'])}"
                     + (f" free {min(t['memory'].values())}" if t["memory"] else "") for t in tiles)
    log_line(f"[table cases] {label} {order}: tabled/memory keys per tile (free slots at the first run-out): {rows}")


def test_sizes_in_the_sources_are_the_ones_the_cases_were_built_for():
    assert T.source_sizes() == T.BUILT_FOR
    assert (T.NE, T.PROBE, T.TH, T.GW, T.GH, T.NEV, T.ND) == (128, 16, 2, 4, 3, 96, 256)
    ids = np.arange(T.P_ALL)
    per_home = np.bincount(T.home(ids, 7).astype(int), minlength=128)
    assert per_home.min() >= 62 and per_home.max() <= 66 and len(T.pool()) == 65
    assert T.FRAME[1] % 8 == 3 and T.FRAME[0] % T.TH == 1      # a partial tile on each edge


def check_tile_claims(label, kind, live_keys, nrows, W, K, planted=(), n_full=0):
    """The claims of a kind on an 8 x 2 kernel's lists, under both orders -> mem [slots] bool (either order)."""
    either = None
    for order in ORDERS:
        tiles, mem = T.run_tiles(live_keys, nrows, W, K, order)
        _log_tiles(label, order, tiles)
        either = mem if either is None else either | mem
        keys2 = np.asarray(live_keys).reshape(nrows, W, K)
        full = [t for t in tiles if t["tw"] == 8 and t["th"] == 2]
        assert len(full) >= 4
        for t in tiles:
            seen = keys2[t["y0"]:t["y0"] + t["th"], t["x0"]:t["x0"] + t["tw"]]
            distinct = len(np.unique(seen[seen >= 0]))
            assert len(t["tabled"]) + len(t["memory"]) == distinct and not (t["tabled"] & set(t["memory"]))
            if kind.startswith("capacity"):
                assert len(t["memory"]) >= distinct - T.NE
                if t in full:
                    assert distinct > T.NE + 20, (distinct, label)
            if kind in ("probe_runout", "hot") and t in full:
                assert t["slots"] == POOL_SLOTS and t["wrapped"]      # exactly 16 tabled, through the & (NE - 1) wrap
                assert len(t["memory"]) >= (8 if kind == "probe_runout" else 1) and set(t["memory"].values()) == {T.NE - 16}
        if kind.startswith("capacity"):      # keys refused by a FULL table (one with a few slots left that no late key's probes reach does not count)
            assert sum(f == 0 for t in tiles for f in t["memory"].values()) >= n_full, label
        if kind in ("probe_runout", "hot"):
            assert sum(len(t["memory"]) for t in tiles) >= 40
        by_origin = {(t["y0"], t["x0"]): t for t in tiles}
        for origin, t_id, m_id in planted:
            t = by_origin[origin]
            assert t_id in t["tabled"] and m_id in t["memory"] and t["memory"][m_id] == T.NE - 16
            assert (keys2[origin[0], origin[1]:origin[1] + 8] == t_id).sum() == 8 and (keys2[origin[0] + 1, origin[1]:origin[1] + 8] == m_id).sum() == 8
            assert (keys2[origin[0]:origin[0] + 2, origin[1]:origin[1] + 8] == m_id).sum() == 8      # (row 1 alone names it)
        if kind == "hot":
            assert len(planted) >= 4
        if kind == "mixed":      # one Gaussian tabled in one tile and on the memory path in another: both meet in one accumulator row
            both = set().union(*[t["tabled"] for t in tiles]) & set().union(*[set(t["memory"]) for t in tiles])
            assert len(both) >= 8
            assert any(t["memory"] and min(t["memory"].values()) > 0 for t in tiles)
    return either


# ---- trace backward -----------------------------------------------------------------------------------------------------------------------
TRACE_CASES = [(k, s, 1) for s in (False, True) for k in T.TILE_KINDS] + [("capacity40", True, 2)]


def trace_id(c):
    return f"{c[0]}-{'scalar' if c[1] else '3x3'}-B{c[2]}"


def trace_planted(case):
    """planted ids with their tile's origin in the flat [B * H] rows the kernel sees (B = 1: the frame's own rows)"""
    return [((b * case["H"] + y0, x0), t_id, m_id) for b, (y0, x0), t_id, m_id in case["planted"]]


@pytest.mark.parametrize("c", TRACE_CASES, ids=trace_id)
def test_trace_case(c):
    case = T.trace_case(*c)
    K, B, H, W = case["K"], case["B"], case["H"], case["W"]
    label = f"trace {trace_id(c)}"
    idx = case["idx"]
    assert idx.min() >= 0 and idx.max() < B * case["N"]
    srt = np.sort(idx, -1)
    assert (srt[..., 1:] != srt[..., :-1]).all()      # a list names a Gaussian once
    for b in range(B):
        assert idx[b].min() >= b * case["N"] and idx[b].max() < (b + 1) * case["N"]
    if case["cnt"] is not None:
        assert (case["cnt"] == 0).any() and (case["cnt"] == K).any() and ((case["cnt"] > 0) & (case["cnt"] < K)).any()
    for g in ("g_len", "g_act"):
        assert np.abs(case[g]).min() >= 0.5 and np.abs(case[g]).max() <= 1.5
    live_keys = np.where(case["live"], idx, -1)
    mem = check_tile_claims(label, c[0], live_keys, B * H, W, K, trace_planted(case), n_full=1000 if K == 40 else 50).reshape(idx.shape)
    # the reference alone
    mus, isg, idx_ref = T.trace_reference_inputs(case)
    rays = case["rays"]
    r64 = oracle.trace_bwd(mus, isg, rays, idx_ref, case["g_len"], case["g_act"], case["g_dsd"])
    r32 = oracle.trace_bwd(mus, isg, rays, idx_ref, case["g_len"], case["g_act"], case["g_dsd"], precision="f32")
    errs = [_scaled(a, b) for a, b in zip(r32, r64)]
    log_line(f"[table cases] {label}: fp32 reference g_rays {errs[0]:.2e}, g_mus {errs[1]:.2e}, g_isigmas {errs[2]:.2e} of scale")
    assert max(errs) <= TOL / 4, errs
    # a lost memory-path term is visible
    terms = T.trace_mu_terms(case)
    scale = max(1.0, float(np.abs(r64[1]).max()))
    assert mem.any() and not (mem & ~case["live"]).any()
    ratio = float(terms[mem].min()) / (TOL * scale)
    log_line(f"[table cases] {label}: {int(mem.sum())} memory-path slots, smallest g_mu term {ratio:.1f} x TOL x scale (scale {scale:.2f})")
    assert ratio >= 10
    unread = np.setdiff1d(np.arange(mus.shape[0]), idx[case["live"]])
    assert unread.size > 0 and (r64[1][unread] == 0).all()


# ---- shade / merge backward -----------------------------------------------------------------------------------------------------------------
SHADE_CASES = [(k, C, False) for k in T.SHADE_KINDS for C in (1, 3, 4)] + [(k, C, True) for k in T.SHADE_KINDS for C in (3, 4)]


def shade_id(c):
    return f"{c[0]}-C{c[1]}" + ("-blend" if c[2] else "")


@pytest.mark.parametrize("c", SHADE_CASES, ids=shade_id)
def test_shade_case(c):
    kind, C, blend = c
    case = T.shade_case(*c)
    K = case["K"]
    label = f"shade {shade_id(c)}"
    idx, vn, w = A._check_fragments(case)
    assert np.abs(case["g"]).min() >= 0.5 and case["Nattr"] == T.P_ALL
    P = w.shape[0]
    passes, gch = None, np.abs(case["g"].reshape(P, C).astype(np.float64))
    if blend:
        img64, rgb64, ga64, gw64 = A.blend_reference(case, -1.0)
        s = w.astype(np.float64).sum(-1)
        x = rgb64.reshape(P, C) + (1 - np.minimum(s, 1.0))[:, None] * case["bg"][None].astype(np.float64)
        assert np.abs(x - 1).min() >= A.MARGIN and (x > 1).any() and (x < 1).any()      # every pixel and channel: nothing is left out later
        gch = gch * (x < 1)
        passes = (x < 1).any(-1)
        img32, _, ga32, gw32 = A.blend_reference(case, -1.0, torch.float32)
        errs = (A._rel(img32, img64), _scaled(ga32, ga64), A._rel(gw32, gw64))
    else:
        out64, ga64, gw64 = A.merge_reference(case)
        out32, ga32, gw32 = A.merge_reference(case, torch.float32)
        errs = (A._rel(out32, out64), _scaled(ga32, ga64), A._rel(gw32, gw64))
    log_line(f"[table cases] {label}: fp32 reference out {errs[0]:.2e}, g_attr {errs[1]:.2e} of scale, g_weight {errs[2]:.2e}")
    assert max(errs) <= TOL / 4, errs
    live_keys = T.shade_live_keys(case, passes)
    mem = check_tile_claims(label, kind, live_keys, T.FRAME[0], T.FRAME[1], K, case["planted"], n_full=300 if K == 40 else 20).reshape(P, K)
    assert mem.any()
    term = w.astype(np.float64) * gch.max(-1)[:, None]
    scale = max(1.0, float(np.abs(ga64).max()))
    ratio = float(term[mem].min()) / (TOL * scale)
    log_line(f"[table cases] {label}: {int(mem.sum())} memory-path slots, smallest w g term {ratio:.1f} x TOL x scale (scale {scale:.2f})")
    assert ratio >= 10
    unread = np.setdiff1d(np.arange(case["Nattr"]), live_keys[live_keys >= 0])
    assert unread.size > 0 and (ga64[np.setdiff1d(unread, np.maximum(idx, 0)[np.arange(K)[None] < vn[:, None]])] == 0).all()


# ---- fused backward -------------------------------------------------------------------------------------------------------------------------
FUSED_MIN_VISIBLE = 16      # memory-path slots whose own g_mu term is at least 10 TOL of scale


@pytest.mark.parametrize("kind", list(T.FUSED_KINDS))
def test_fused_case(kind):
    case = T.fused_case(kind)
    K, P, H, W, nv, idx = case["K"], case["P"], case["H"], case["W"], case["nv"], case["idx"]
    label = f"fused {kind} K={K}"
    for p in range(H * W):
        assert (np.diff(case["ln"][p, :nv[p]]) >= 0).all() and (idx[p, nv[p]:] == -1).all() and len(set(idx[p, :nv[p]].tolist())) == nv[p]
        assert idx[p, :nv[p]].min(initial=0) >= 0 and idx[p, :nv[p]].max(initial=0) < P
    assert np.abs(case["gw"]).min() >= 0.5
    slot64, gm64, gs64 = T.fused_reference(case)
    _, gm32, gs32 = T.fused_reference(case, "f32")
    errs = (_scaled(gm32, gm64), _scaled(gs32, gs64))
    log_line(f"[table cases] {label}: fp32 reference g_mus {errs[0]:.2e}, g_isigmas {errs[1]:.2e} of scale")
    assert max(errs) <= TOL / 4, errs
    # the slots that reach the table: inside the count, and with a gradient fp32 cannot round to nothing
    strong = (idx >= 0) & (np.abs(np.stack(slot64)).max(0) > 1e-20)
    live_keys = np.where(strong, idx, -1)
    either = np.zeros(idx.size, bool)
    for order in ORDERS:
        groups, mem = T.run_groups(live_keys, nv, H, W, K, order)
        either |= mem
        rows = ", ".join(f"({g['x0']},{g['y0']}) {len(g['tabled'])}/{len(g['memory'])}" for g in groups)
        log_line(f"[table cases] {label} {order}: tabled/memory keys per group: {rows}")
        k3 = live_keys.reshape(H, W, K)
        distinct = np.array([len(np.unique(k3[g["y0"]:g["y0"] + T.GH, g["x0"]:g["x0"] + T.GW][k3[g["y0"]:g["y0"] + T.GH, g["x0"]:g["x0"] + T.GW] >= 0]))
                             for g in groups])
        causes = [c for g in groups for c in g["memory"].values()]
        if kind == "entries":
            assert distinct.max() <= T.ND and (distinct > T.NEV).sum() >= 8
            assert sum(c[0] == "entries" for c in causes) >= 200 and all(len(g["tabled"]) <= T.NEV for g in groups)
        if kind == "directory":
            assert distinct[0] > T.ND + 100
            first = list(groups[0]["memory"].values())
            assert sum(c[0] == "probes" for c in first) >= 20      # wd_find2's "probes ran out" result
            assert sum(c == ("probes", 0) for c in first) >= 1     # ... and with the directory itself full
            assert sum(c[0] == "entries" for c in first) >= 100
        if kind == "capacity":
            assert (distinct > T.NE).sum() >= 8 and sum(c == 0 for c in causes) >= 200
        if kind == "probe_runout":
            assert all(len(g["tabled"]) <= 16 for g in groups) and sum(c == T.NE - 16 for c in causes) >= 200
    either = either.reshape(idx.shape)
    terms = T.trace_mu_terms(T.fused_as_trace_case(case, slot64)).reshape(idx.shape)
    scale = max(1.0, float(np.abs(gm64).max()))
    visible = int((terms[either] >= 10 * TOL * scale).sum())
    log_line(f"[table cases] {label}: {int(either.sum())} memory-path slots, {visible} of them with a g_mu term of at least 10 x TOL x scale "
             f"(scale {scale:.2f}); the largest {float(terms[either].max()) / (TOL * scale):.0f} x TOL x scale")
    assert visible >= FUSED_MIN_VISIBLE
