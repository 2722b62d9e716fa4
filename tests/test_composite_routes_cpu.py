"""The composite's route choice restated (composite.hip: launch_composite, composite_shade_fwd_impl), the lists the GPU tests of
tests/test_gpu_composite_routes.py run on, and the weight bound they hold the kernels to -- everything about those tests that
needs no GPU: the K lists reach every route and its extremes, the lists are conditioned, the pixel counts hold an empty and a
partial workgroup and an unsorted pixel beside a sorted one on every route, and the bound is not already spent on input rounding.

The bound.  S_m = sum_j E_j Phi_mj, w_m = exp(-occ S_m) E_m e^(1/2), so |dw| <= w occ |dS| + (the exp2 and the products).
The kernel forms S_m of a sorted pixel as  prefix_m - sum_front E_j h_mj + sum_back E_j h_mj  with h = erfc / 2 <= 1 / 2:
  * the evaluator and the window: test_gpu_erfc_walks.py's EPS = 7.5e-7 + 3.7e-7 charges a column the evaluator's error AND the
    window's drop.  A column is either evaluated (fit 6.0e-7 + two ulp of exp2: 7.5e-7) or lies outside its window and is dropped
    (erfc(3.5) / 2 = 3.7e-7), never both: |dh| <= EPS_COL = max of the two = 7.5e-7 per column;
  * the additions: a term t that passes through n fp32 additions picks up at most n 2^-24 |t| (first order).  A column in front of
    the row brings E_j through the prefix's chain (n_pre additions) and E_j h <= E_j / 2 through the walk's chain (n_h additions),
    a column behind only the latter: at most (n_pre + n_h / 2) 2^-24 sum_j E_j =: gamma_K sum_j E_j.
  n_pre and n_h by route, read off the code (`chains`):
    one-wave forward (compn_fwd_rows): the lane's NS slots (NS - 1), the shuffle scan over the pixel's LP lanes (ceil(log2 LP)),
      the lane's own inclusive prefix (NS), then - front, + back, + the row's cell (3);  h terms: every OTHER lane adds its NS
      columns into the row's cell one after the other ((LP - 1) NS) and the cell is added once (1) -- or the diagonal block's
      NS - 1 and three merges, whichever is longer;
    workgroup forward (NS = 2): the same prefix through the LDS scan with two merges behind it;  h terms: the row's two packed
      accumulators take a column PAIR per trip (ceil(K / 2) per component), the diagonal block (1), x + y (1), two merges (2);
    unsorted pixel (any route): one sequential fma chain over the K columns of E_j Phi_mj <= E_j, 1 - h rounded once more: K + 1.
  Both sums run over the columns that can contribute to row m, not over the whole list (`weight_bound`): the EPS term and the h
  chain over the columns within |x_mj| < 5 (further off, erfc / 2 and the polynomial are both below 1e-12: nothing is evaluated
  wrongly and nothing is dropped at a cost), the prefix chain over the columns in front of the row.
  Six pixels (SHELL) carry a column 3.02 .. 3.3 windows behind a row that has weight (`_shell`): the product's window of 3.5
  evaluates it, a window cut at 3.0 drops up to erfc(3.02) / 2 = 9.8e-6 there.  A library built with kSat = 3.0 fails
  test_weights_within_the_derived_bound at 12 of the 24 K, in both count modes (measured once on MI355X: max |dw| / bound 2.4, 2.7,
  2.1 at K = 5, 6, 8; 1.02 - 1.37 at K = 63 .. 66, 129 .. 131, 170, 254; 0.65 - 0.96 at the other K >= 126, where the chain of
  column adds is longest; product: at most 0.29), and the gradients at TOL at 13 K; test_composite_random_vs_oracle's 1e-4 accepts it.
  gamma_256 = 8.5e-6 (one wave, four slots: 16 + 253 / 2 additions), gamma_255 = 4.6e-6 (workgroup: 12 + 132 / 2); the sequential
  worst case K 2^-24 would be 1.5e-5.  The second term of the bound, 1e-6 max w, is for the few ulp of exp2 and the products."""
import math
import os

import numpy as np
import pytest

import oracle
from test_gpu_erfc_walks import _conditioned, _pixel, EPS, OCC

K_LIST = (1, 2, 3, 4, 5, 6, 8, 63, 64, 65, 66, 126, 127, 128, 129, 130, 131, 132, 170, 171, 253, 254, 255, 256)      # stand-alone entries
K_ONEPASS = (1, 2, 3, 5, 6, 7, 125, 126, 127, 128)                                                                    # one-pass entries
PASSES = ("fwd", "bwd_given", "bwd_recomputed")
NPIX = 193
EMPTY = range(64, 128)
UNSORTED = (130, 191)
COPIES = {151: 2, 152: 3, 148: 5, 146: 7, 153: 8, 155: 130}      # pixel -> the pixel it repeats, at another place in its wave / workgroup
C_PROD = 1e-6
EPS_EVAL, EPS_DROP = 7.5e-7, 3.7e-7      # test_gpu_erfc_walks.py's two parts of EPS
EPS_COL = max(EPS_EVAL, EPS_DROP)
SHELL = {7: 3.02, 14: 3.03, 21: 3.05, 28: 3.1, 35: 3.2, 42: 3.3}      # pixel (a full list) -> where its shell column sits, in windows
NO_EMPTY_WG = {("bwd_recomputed", 1), ("bwd_recomputed", 2), ("bwd_recomputed", 3), ("bwd_recomputed", 5)}      # 256, 128, 85, 51 pixels a workgroup: none inside 64 .. 127


def route(K, which):
    """What launch_composite picks from K alone.  which: fwd | bwd_given | bwd_recomputed | fwd_iso (voge_composite_fwd_iso: the forward's
    choice, from the records) | onepass (composite_shade_fwd_impl, voge_frame_depth_fwd_iso: four slots whatever K is)."""
    if which == "bwd_recomputed":      # composite_recompute_bwd_kernel: one slot per lane, 256 threads
        return dict(NS=1, wide=False, wave=False, lanes=K, ppw=256 // K, idle=256 - (256 // K) * K)
    NS = 4 if which == "onepass" or (which in ("fwd", "fwd_iso") and K % 4 == 0) else 2
    lanes = -(-K // NS)
    wave = lanes <= 64
    assert wave or which != "onepass"
    T = 64 if wave else 256
    ppw = T // lanes
    return dict(NS=NS, wide=K % NS == 0, wave=wave, lanes=lanes, ppw=ppw, idle=T - ppw * lanes)


def chains(K, unsorted=False):
    """(n_pre, n_h) of the forward's row sums: the additions a prefix term / an E h term passes through (module docstring)."""
    if unsorted:
        return K + 1, 0
    r = route(K, "fwd")
    NS, LP = r["NS"], r["lanes"]
    scan = math.ceil(math.log2(LP)) if LP > 1 else 0
    if r["wave"]:
        return (NS - 1) + scan + NS + 3, max((LP - 1) * NS + 1, (NS - 1) + 3)
    return (NS - 1) + scan + NS + 2, -(-K // 2) + 1 + 1 + 2


def gamma(K, unsorted=False):
    n_pre, n_h = chains(K, unsorted)
    return (n_pre + 0.5 * n_h) * 2.0 ** -24


X_FAR = 5.0      # beyond it erfc / 2 <= 7.7e-13 and the walks' polynomial <= 3.6e-13 (composite_core.h): no error to speak of
E_FAR = 1e-12


def weight_bound(K, idx, act, ln, dsd, wr, unsorted_rows=()):
    """Per slot m: |dw| <= w occ [EPS_COL sum_near E_j + 2^-24 (n_pre sum_front E_j + n_h / 2 sum_near E_j)] + 1e-6 max w, the module
    docstring's bound with the sums taken over the columns that can contribute: near = |x_mj| < X_FAR (a column further off is
    neither evaluated with an error nor dropped at a cost: 1e-12 each), front = len_j <= len_m (the prefix's terms; the row's own
    E among them).  An unsorted pixel: one chain of K + 1 over the columns that are in front or near, each counted once.
    wr: the fp64 weights."""
    out = np.empty(wr.shape)
    for p in range(len(idx)):
        live = idx[p] >= 0
        E = np.where(live, np.exp(-act[p].astype(np.float64)), 0.0)
        l, sj = ln[p].astype(np.float64), np.sqrt(dsd[p].astype(np.float64) + 1e-10)
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.abs(l[:, None] - l[None, :]) * sj[None, :]
        near = (x < X_FAR) & live[None, :]
        front = (l[None, :] <= l[:, None]) & live[None, :]
        e_near, e_front = (near * E[None, :]).sum(1), (front * E[None, :]).sum(1)
        n_pre, n_h = chains(K, unsorted=p in unsorted_rows)
        if p in unsorted_rows:
            add = n_pre * ((near | front) * E[None, :]).sum(1)
        else:
            add = n_pre * e_front + 0.5 * n_h * e_near
        out[p] = wr[p] * OCC * (EPS_COL * e_near + E_FAR * E.sum() + 2.0 ** -24 * add)
    return out + C_PROD * wr.max()


def _shell(px, nv, X):
    """Put column 4 of a list X windows (of its own) behind row 3, in another lane's group than the row (slots 2, 3 | 4 ..), and give
    the row weight: E_3 = E_4 = e^-0.05, the rows in front E = e^-3.  Slots 3 .. 7 take the list's smallest dsd, so neither a
    neighbour's wider window (the column walks go as far as the lane's widest column) nor the pixel-wide radius of the workgroup
    form reaches across the gap on column 4's behalf."""
    idx, act, ln, dsd = (a.copy() for a in px)
    d = dsd[:nv].min()
    dsd[3:min(8, nv)] = d
    act[:3], act[3:5] = 3.0, 0.05
    sd = np.sqrt(np.float64(d) + 1e-10)
    l4 = np.float32(np.float64(ln[3]) + X / sd)
    while (np.float64(l4) - np.float64(ln[3])) * sd < X:      # (fp32 depths: the first one at or beyond X)
        l4 = np.nextafter(l4, np.float32(np.inf))
    ln[4:nv] += l4 - ln[4]
    ln[4] = l4
    if (np.float64(l4) - np.float64(ln[3])) * sd > X + 0.01 or (np.diff(ln[:nv]) < 0).any():
        return None      # (depths too coarse for this window: another draw)
    return idx, act, ln, dsd


def counts_of(K):
    c = [[K, K - 1, max(K - 3, 1), K // 2 + 1, 3, 2, 1][p % 7] for p in range(NPIX)]
    c[0], c[1] = 0, K
    for p in EMPTY:
        c[p] = 0
    c = np.minimum(np.array(c), K)
    if K >= 2:
        c[list(UNSORTED)] = K
    for dst, src in COPIES.items():
        c[dst] = c[src]
    return c


def build_lists(K):
    """-> idx [NPIX, K] int32, act, ln, dsd fp32, nv [NPIX], tries (the most draws a pixel took until _conditioned held)."""
    rng = np.random.default_rng(1700 + K)
    nv = counts_of(K)
    out = [np.empty((NPIX, K), t) for t in (np.int32, np.float32, np.float32, np.float32)]
    tries = 0
    for p in range(NPIX):
        s_pix = float(np.exp(rng.uniform(np.log(0.3), np.log(1e3)))) if p % 3 else float(rng.uniform(1.5, 40.0))
        for n_try in range(1, 201):
            px = _pixel(rng, K, nv[p], s_pix, p)
            if p in SHELL and nv[p] >= 5:
                px = _shell(px, nv[p], SHELL[p])
                if px is None:
                    continue
            if _conditioned(px[2], px[3], nv[p]):
                break
        else:
            raise AssertionError("no conditioned list found")
        tries = max(tries, n_try)
        for o, v in zip(out, px):
            o[p] = v
    idx, act, ln, dsd = out
    if K >= 2:
        a, b = (1, K - 2) if K >= 4 else (0, K - 1)
        for p in UNSORTED:      # two live depths swapped (test_gpu_erfc_walks.build_lists)
            ln[p, [a, b]] = ln[p, [b, a]]
            if ln[p, a] == ln[p, b]:
                ln[p, a] += 1.0
    for dst, src in COPIES.items():
        for o in out:
            o[dst] = o[src]
    return idx, act, ln, dsd, nv, tries


@pytest.fixture(scope="module", params=K_LIST)
def lists(request):
    return (request.param,) + build_lists(request.param)


def test_route_table():
    """The table of DESIGN.md, row by row, and the extremes the K lists were chosen for."""
    got = {}
    for which in PASSES:
        for K in K_LIST:
            r = route(K, which)
            got.setdefault((which, r["NS"], r["wave"], r["wide"]), []).append(K)
    assert got[("fwd", 4, True, True)] == [4, 8, 64, 128, 132, 256]
    assert got[("fwd", 2, True, True)] == [2, 6, 66, 126]
    assert got[("fwd", 2, True, False)] == [1, 3, 5, 63, 65, 127]
    assert got[("fwd", 2, False, True)] == [130, 170, 254]
    assert got[("fwd", 2, False, False)] == [129, 131, 171, 253, 255]
    assert sorted(k for k in got if k[0] == "fwd") == sorted([("fwd", 4, True, True), ("fwd", 2, True, True), ("fwd", 2, True, False),
                                                             ("fwd", 2, False, True), ("fwd", 2, False, False)])
    for wave, wide in ((True, True), (True, False), (False, True), (False, False)):      # the backward: two slots always
        ks = got[("bwd_given", 2, wave, wide)]
        assert ks and all((K <= 128) == wave and (K % 2 == 0) == wide for K in ks)
    assert all(k[1] == 2 for k in got if k[0] == "bwd_given")
    assert got[("bwd_recomputed", 1, False, False)] == list(K_LIST)
    f = {K: route(K, "fwd") for K in K_LIST}
    assert (f[4]["lanes"], f[256]["lanes"], f[256]["idle"]) == (1, 64, 0) and f[2]["ppw"] == f[4]["ppw"] == 64 and f[3]["ppw"] == 32
    assert (f[130]["lanes"], f[130]["ppw"], f[130]["idle"]) == (65, 3, 61) and (f[170]["lanes"], f[170]["ppw"], f[170]["idle"]) == (85, 3, 1)
    assert (f[171]["lanes"], f[171]["ppw"]) == (86, 2) and (f[255]["lanes"], f[255]["ppw"], f[255]["idle"]) == (128, 2, 0)
    assert f[127]["wave"] and f[128]["wave"] and not f[129]["wave"] and f[127]["lanes"] == 64 and f[127]["idle"] == 0
    b = {K: route(K, "bwd_given") for K in K_LIST}
    assert b[128]["wave"] and b[128]["lanes"] == 64 and not b[129]["wave"] and b[129]["lanes"] == 65
    iso = {K: route(K, "fwd_iso") for K in K_ONEPASS}      # voge_composite_fwd_iso: the forward's own choice -- two slots unless K % 4 == 0
    assert all(iso[K] == route(K, "fwd") for K in K_ONEPASS) and {K for K, r in iso.items() if r["wide"]} == {2, 6, 126, 128}
    one = {K: route(K, "onepass") for K in K_ONEPASS}      # four slots always: every residue, small and at the limit
    assert {K % 4 for K in K_ONEPASS if K < 8} == {1, 2, 3} and {K % 4 for K in K_ONEPASS if K > 100} == {0, 1, 2, 3}
    assert all(r["NS"] == 4 and r["wave"] for r in one.values()) and one[128]["lanes"] == 32 and one[1]["ppw"] == 64
    assert {K for K, r in one.items() if not r["wide"]} == set(K_ONEPASS) - {128}


def test_bound_is_derived_not_fitted():
    """gamma_K against the sequential worst case K 2^-24 and the 1e-4 it replaces."""
    for K in K_LIST:
        n_pre, n_h = chains(K)
        assert gamma(K) <= (K + 16) * 2.0 ** -24 and n_pre <= 17 and n_h <= K + 4, (K, n_pre, n_h)
    assert chains(256) == (3 + 6 + 4 + 3, 63 * 4 + 1) and chains(255) == (1 + 7 + 2 + 2, 128 + 4) and chains(5) == (1 + 2 + 2 + 3, 2 * 2 + 1)
    assert EPS + gamma(256) < 1e-4 / 6 and gamma(255, unsorted=True) == 256 * 2.0 ** -24


def test_counts_reach_every_workgroup_case():
    for K in K_LIST:
        nv = counts_of(K)
        assert nv[0] == 0 and nv[1] == K and (nv[list(EMPTY)] == 0).all() and nv.max() <= K and len(nv) == NPIX
        if K >= 4:
            assert ((nv % 2 == 1) & (nv > 0) & (nv < K)).any() or K % 2 == 0      # dead slots inside a lane's group
            assert ((nv > 0) & (nv < K)).sum() >= 20
        for which in PASSES:
            ppw = route(K, which)["ppw"]
            wg = np.arange(NPIX) // ppw
            live = np.bincount(wg, weights=(nv > 0))
            fits = any(g * ppw >= EMPTY[0] and (g + 1) * ppw <= EMPTY[-1] + 1 for g in range(NPIX))
            assert fits == ((which, K) not in NO_EMPTY_WG), (K, which)
            if fits:      # a wholly empty workgroup between live ones: the early-out with cnt
                e = [g for g in np.nonzero(live == 0)[0] if g * ppw >= EMPTY[0]]
                assert len(e) and live[:e[0]].any() and live[e[-1] + 1:].any(), (K, which)
            if ppw >= 2:
                assert NPIX % ppw != 0, (K, which)      # the last workgroup is partial
                if K >= 2:      # an unsorted pixel beside a sorted, live one
                    for p in UNSORTED:
                        mates = [m for m in range(NPIX) if wg[m] == wg[p] and m not in UNSORTED]
                        assert any(nv[m] > 0 for m in mates), (K, which, p)
                # a repeated pixel sits at another place of its workgroup than its original
                assert sum(dst % ppw != src % ppw for dst, src in COPIES.items()) >= 3, (K, which)


def test_lists_are_conditioned(lists):
    K, idx, act, ln, dsd, nv, tries = lists
    assert tries <= 5, tries
    for p in range(NPIX):
        if p in UNSORTED and K >= 2:
            assert not (np.diff(ln[p]) >= 0).all()
            continue
        src = COPIES.get(p, p)
        assert _conditioned(ln[p], dsd[p], nv[p]) or src in UNSORTED, p
        assert (idx[p, :nv[p]] >= 0).all() and (idx[p, nv[p]:] == -1).all() and (act[p, nv[p]:] == np.float32(1e10)).all()
    for dst, src in COPIES.items():
        for a in (idx, act, ln, dsd):
            assert np.array_equal(a[dst], a[src])
    for p, X in SHELL.items():      # the shell column: between a 3.0 and a 3.5 window of row 3, which carries weight
        if K >= 5:
            assert nv[p] == K
            x = (np.float64(ln[p, 4]) - np.float64(ln[p, 3])) * np.sqrt(np.float64(dsd[p, 4]) + 1e-10)
            assert 3.01 < X <= x <= X + 0.01 and dsd[p, 4] == dsd[p, :K].min(), (p, x)
            wr, _ = oracle.composite_fwd(idx[[p]], act[[p]], ln[[p]], dsd[[p]], OCC)
            assert wr[0, 3] > 0.5, (p, wr[0, 3])


def test_bound_is_not_spent_on_input_rounding(lists):
    """The kernel keeps E = exp(-act) and s = sqrt(dsd + 1e-10) as fp32.  The fp64 oracle on inputs that reproduce exactly those
    fp32 values moves the weights by less than the bound's second term alone."""
    K, idx, act, ln, dsd, nv, _ = lists
    wr, vr = oracle.composite_fwd(idx, act, ln, dsd, OCC)
    assert (vr == nv).all()
    a64, d64 = act.astype(np.float64), dsd.astype(np.float64)
    E32 = np.exp(-a64).astype(np.float32).astype(np.float64)
    s32 = np.sqrt(d64 + 1e-10).astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        a_r = np.where(E32 > 0, -np.log(np.where(E32 > 0, E32, 1.0)), a64)
    w2, _ = oracle.composite_fwd(idx, a_r, ln.astype(np.float64), s32 * s32 - 1e-10, OCC)
    assert np.abs(w2 - wr).max() <= C_PROD * wr.max(), (K, np.abs(w2 - wr).max(), wr.max())
    live = wr[idx >= 0]
    assert np.isfinite(wr).all() and (wr[idx < 0] == 0).all() and live.size and live.max() > 1e-3
    bound = weight_bound(K, idx, act, ln, dsd, wr, UNSORTED if K >= 2 else ())
    E = np.where(idx >= 0, np.exp(-act.astype(np.float64)), 0.0).sum(-1, keepdims=True)
    g = np.full((NPIX, 1), gamma(K))
    if K >= 2:
        g[list(UNSORTED)] = gamma(K, unsorted=True)
    loose = wr * OCC * (EPS + g) * E + C_PROD * wr.max()      # the issue's form: EPS and every sum over all the columns
    assert EPS == EPS_EVAL + EPS_DROP and EPS_COL < EPS
    assert (bound > 0).all() and (bound <= loose * (1 + 1e-5)).all() and bound.max() < 1e-4 / 2 and np.median(bound) < 1e-4 / 50, bound.max()
    if K >= 5:      # what a window cut at 3.0 drops at the shell rows: beyond the bound wherever the chains are short
        for p, X in SHELL.items():
            drop = wr[p, 3] * OCC * np.exp(-np.float64(act[p, 4])) * 0.5 * math.erfc(X)
            assert drop > 8e-7 and (drop > 1.25 * bound[p, 3] or X > 3.1 or K > 8), (K, p, drop, bound[p, 3])


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_wide_routes_refuse_pointers_off_their_boundary(lib):
    """voge_composite_fwd / _bwd look at the pointers before anything is launched: with K % NS == 0 one array 4 bytes -- or, four
    slots, 8 or 12 bytes -- off the boundary is VOGE_ERR_BAD_ARG.  The addresses are invented, so this runs only where no HIP
    device is visible: there nothing can be launched whatever the guard does.  With a device, tests/test_gpu_composite_routes.py
    makes the same calls on real buffers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: the refusals are tested on real buffers by test_gpu_composite_routes.py")
    base = 1 << 20
    for K in (2, 4, 6, 8, 128, 130, 254, 256):
        offs = (4, 8, 12) if route(K, "fwd")["NS"] == 4 else (4,)
        for off in offs:
            for bad in range(4):      # act, len, dsd, weight
                a = [base + (off if i == bad else 0) for i in range(4)]
                assert lib.voge_composite_fwd(base, None, a[0], a[1], a[2], 1.0, NPIX, K, a[3], base, None) == -1, (K, off, bad)
        for bad in range(8):      # act, len, dsd, weight, g_weight, g_act, g_len, g_dsd: two slots, 8 bytes
            a = [base + (4 if i == bad else 0) for i in range(8)]
            assert lib.voge_composite_bwd(a[0], a[1], a[2], a[3], None, a[4], 1.0, NPIX, K, a[5], a[6], a[7], None) == -1, (K, bad)
