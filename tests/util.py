"""Shared helpers for the parity tests (scene builders + comparison metrics)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fp32 tolerance from BASELINE.json's north_star ("within 1e-4 fp32"), applied relative to
# max(1, |reference|) so depths of ~6 and activations of ~20 are judged at the same ulp scale.
TOL = 1e-4


def close(a, b, tol=TOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


def max_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


FLIP_LOG = []   # (label, flipped pixels, pixels) of every compare_trace call of the session


def _report_flips(label, n_flip, n_pix):
    """Every trace comparison states how many pixels' index lists actually differed ("print it and
    assert a ceiling per config"); the lines also go to gpurun_out/parity_flips.txt when that directory exists."""
    FLIP_LOG.append((label, int(n_flip), int(n_pix)))
    line = f"[parity] {label}: {int(n_flip)} of {int(n_pix)} pixels have a different index list"
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        try:
            with open(os.path.join(out, "parity_flips.txt"), "a") as f:
                f.write(line + "\n")
        except OSError:
            pass


def log_line(line):
    """Print a measured quantity and keep it in gpurun_out/parity_flips.txt (when that directory exists)."""
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        try:
            with open(os.path.join(out, "parity_flips.txt"), "a") as f:
                f.write(line + "\n")
        except OSError:
            pass


def grad_close(label, got, want, tol):
    """|got - want| <= tol * max(1, |want|_max); the measured ratio goes to the same log as the flip counts, so the
    tolerances in the tests can be seen against what the kernels actually deliver."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    line = f"[parity] {label}: max gradient error {err / scale:.2e} of scale (tolerance {tol:.1e})"
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        try:
            with open(os.path.join(out, "parity_flips.txt"), "a") as f:
                f.write(line + "\n")
        except OSError:
            pass
    assert err <= tol * scale, f"{label}: {err:.3e} vs scale {scale:.3e} (tolerance {tol:.1e})"


def compare_trace(got, ref, thr_act, min_match=0.999, max_flips=None, label=None):
    """got / ref = (idx, len, act, dsd).  Top-K membership and the act < thr test are
    discontinuous, so a 1-ulp difference may flip a member at isolated pixels (SURVEY.md §7
    "selection discontinuities").  Require: the index lists agree exactly on >= min_match of the
    pixels; on those pixels every value agrees within TOL; on the others the disagreement must be
    explainable by a candidate within TOL of a decision boundary (threshold or K-th depth)."""
    if label is None:
        import inspect
        label = inspect.stack()[1].function
    gi, gl, ga, gd = (np.asarray(x) for x in got)
    ri, rl, ra, rd = (np.asarray(x) for x in ref)
    K = gi.shape[-1]
    gi2, ri2 = gi.reshape(-1, K), ri.reshape(-1, K)
    same = (gi2 == ri2).all(axis=1)
    frac = same.mean() if same.size else 1.0
    _report_flips(label, (~same).sum(), same.size)
    assert frac >= min_match, f"index lists agree on only {frac:.5f} of pixels"
    if max_flips is not None:
        assert (~same).sum() <= max_flips, f"{label}: {(~same).sum()} pixels flipped, ceiling {max_flips}"
    m = same.reshape(gi.shape[:-1])
    valid = (ri >= 0) & m[..., None]
    for name, g, r in (("len", gl, rl), ("act", ga, ra), ("dsd", gd, rd)):
        bad = ~close(g[valid], r[valid])
        assert not bad.any(), f"{name}: max rel err {max_rel(g[valid], r[valid]):.3e} on matched pixels"
    # sentinels on matched pixels
    sent = (ri < 0) & m[..., None]
    assert (gi[sent] == -1).all() and (gl[sent] == np.float32(1e10)).all()
    assert (ga[sent] == np.float32(1e10)).all() and (gd[sent] == 0).all()
    # mismatching pixels: symmetric difference must sit on a decision boundary
    for p in np.nonzero(~same)[0]:
        gs, rs = set(gi2[p][gi2[p] >= 0].tolist()), set(ri2[p][ri2[p] >= 0].tolist())
        ra_p, rl_p = ra.reshape(-1, K)[p], rl.reshape(-1, K)[p]
        ga_p, gl_p = ga.reshape(-1, K)[p], gl.reshape(-1, K)[p]
        for q in gs ^ rs:
            if q in rs:
                a_q, l_q = ra_p[ri2[p] == q][0], rl_p[ri2[p] == q][0]
            else:
                a_q, l_q = ga_p[gi2[p] == q][0], gl_p[gi2[p] == q][0]
            near_thr = abs(a_q - thr_act) <= 10 * TOL * max(1.0, abs(thr_act))
            kth = max(rl_p[ri2[p] >= 0].max(initial=-1e30), gl_p[gi2[p] >= 0].max(initial=-1e30))
            near_k = abs(l_q - kth) <= 10 * TOL * max(1.0, abs(kth))
            assert near_thr or near_k, f"pixel {p}: candidate {q} differs away from any boundary"
        if gs == rs:  # same members, different order: depths must be (near-)tied
            assert np.abs(np.sort(gl_p[gi2[p] >= 0]) - np.sort(rl_p[ri2[p] >= 0])).max() <= 10 * TOL * 10
    return frac


def _runs(ln, live, delta):
    """Per row: a label per slot such that neighbouring live slots whose lens are closer than delta * max(1, |len|) share it."""
    a, b = ln[:, :-1], ln[:, 1:]
    with np.errstate(invalid="ignore"):
        brk = ~((b - a) <= delta * np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))) | ~live[:, 1:]
    return np.concatenate([np.zeros((ln.shape[0], 1), np.int64), np.cumsum(brk, axis=1)], axis=1)


def compare_trace_strict(got, oracle_fn, K, thr_act, delta, cap, label, bounds=None, n_per_batch=None, also=None):
    """The trace's result against the fp64 oracle where the oracle DECIDES it, with nothing forgiven there.

    got = (idx, len, act | None, dsd | None[, cnt]) of [B,H,W,K] ([B,H,W]); oracle_fn(K', thr') -> the oracle's (idx, len, act, dsd)
    at K' slots.  It is called at K + 1 slots with thr_act (1 - delta) and thr_act (1 + delta) (and at K + 4 with the latter when a
    pixel is undecided).  A pixel's membership is decided when the two lists are identical and the (K+1)-th len exceeds the K-th by
    more than delta * max(1, |len|) (or there is no (K+1)-th hit).  Decided pixels: the kernel's SET of indices equals the oracle's,
    cnt equals the number of hits, sentinels are bit-exact, len / act / dsd lie within `bounds(pixel numbers, indices)` of the fp64
    values, and a member's position differs from the oracle's only inside a run of oracle lens closer than delta * max(1, |len|).
    Every pixel, from the kernel's own outputs: lens non-decreasing over the live slots, bit-equal lens in ascending index order, live
    slots a prefix, no index twice, every index inside the pixel's batch element (n_per_batch Gaussians each).  Undecided pixels: every
    member is in the (1 + delta) list at K + 4 slots, and every (1 - delta) member more than delta in front of the kernel's K-th len is
    present.  The share of undecided pixels must be <= cap.
    also: {name: (idx, len, act, dsd)} further results that are only MEASURED against the bounds (on decided pixels where their
    set is the oracle's).  -> dict(undecided=share, use={"kernel": (len, act, dsd shares of the bound), name: ...})."""
    gi = np.asarray(got[0]).reshape(-1, K).astype(np.int64)
    P = gi.shape[0]
    gl = np.asarray(got[1]).reshape(P, K)
    ga = None if got[2] is None else np.asarray(got[2]).reshape(P, K)
    gd = None if got[3] is None else np.asarray(got[3]).reshape(P, K)
    gc = None if len(got) < 5 or got[4] is None else np.asarray(got[4]).reshape(P).astype(np.int64)
    B = np.asarray(got[0]).shape[0]
    lo = [np.asarray(x).reshape(P, K + 1) for x in oracle_fn(K + 1, thr_act * (1.0 - delta))]
    hi = [np.asarray(x).reshape(P, K + 1) for x in oracle_fn(K + 1, thr_act * (1.0 + delta))]
    oi, ol = lo[0].astype(np.int64), lo[1].astype(np.float64)
    o_live = oi >= 0
    nh = o_live.sum(1)
    same = (lo[0] == hi[0]).all(1)
    kth, nxt = ol[:, K - 1], ol[:, K]
    gap_ok = (nh <= K) | ((nxt - kth) > delta * np.maximum(1.0, np.maximum(np.abs(kth), np.abs(nxt))))
    decided = same & gap_ok
    und = float((~decided).mean()) if P else 0.0

    # ---- every pixel, from the kernel's own outputs
    live = gi >= 0
    n_live = live.sum(1)
    assert (live == (np.arange(K)[None, :] < n_live[:, None])).all(), f"{label}: live slots are not a prefix"
    if gc is not None:
        assert (gc == n_live).all(), f"{label}: cnt differs from the number of live slots at {int((gc != n_live).sum())} pixels"
    assert (gi[~live] == -1).all(), f"{label}: a dead slot's index is not -1"
    for name_, x_ in (("len", gl), ("act", ga), ("dsd", gd)):
        assert x_ is None or np.isfinite(x_[live]).all(), f"{label}: a live slot's {name_} is not finite"
    both = live[:, 1:]
    assert not (both & (gl[:, 1:] < gl[:, :-1])).any(), f"{label}: lens decrease along a list"
    assert not (both & (gl[:, 1:] == gl[:, :-1]) & (gi[:, 1:] <= gi[:, :-1])).any(), f"{label}: bit-equal lens not in ascending index order"
    srt = np.sort(np.where(live, gi, -1 - np.arange(K)[None, :]), axis=1)
    assert not (srt[:, 1:] == srt[:, :-1]).any(), f"{label}: an index twice in one list"
    if n_per_batch is not None:
        b_of = (np.arange(P) // (P // B))[:, None]
        assert (~live | ((gi >= b_of * n_per_batch) & (gi < (b_of + 1) * n_per_batch))).all(), f"{label}: an index outside the pixel's batch element"
    sent = ~live
    s32 = np.float32(1e10)
    assert (gl[sent] == s32).all(), f"{label}: a dead slot's len is not the sentinel"
    if ga is not None:
        assert (ga[sent] == s32).all() and (gd[sent] == 0).all(), f"{label}: a dead slot's act / dsd is not the sentinel"

    # ---- decided pixels
    D = np.nonzero(decided)[0]
    BIG = np.int64(1) << 40
    key_o = np.where(o_live[D, :K], oi[D, :K], BIG)
    key_g = np.where(live[D], gi[D], BIG)
    ord_o, ord_g = np.argsort(key_o, axis=1, kind="stable"), np.argsort(key_g, axis=1, kind="stable")
    set_o, set_g = np.take_along_axis(key_o, ord_o, 1), np.take_along_axis(key_g, ord_g, 1)
    bad = (set_o != set_g).any(1)
    if bad.any():
        p = int(D[np.nonzero(bad)[0][0]])
        raise AssertionError(f"{label}: {int(bad.sum())} of {D.size} decided pixels have another index set; pixel {p}: kernel "
                             f"{gi[p].tolist()} {gl[p].tolist()}, oracle {oi[p].tolist()} {ol[p].tolist()}")
    assert (n_live[D] == np.minimum(nh[D], K)).all(), f"{label}: hit counts differ on decided pixels"
    member = set_o < BIG
    pix = np.broadcast_to(D[:, None], set_o.shape)[member]
    ids = set_o[member]
    use = {}

    def measure(name, res_sorted, check):
        b = bounds(pix, ids) if bounds is not None else None
        shares = []
        for q, (g_, r_) in enumerate(res_sorted):
            if g_ is None:
                shares.append(float("nan"))
                continue
            err = np.abs(g_[member].astype(np.float64) - r_[member])
            if b is None:
                shares.append(float("nan"))
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                sh = np.where(err == 0, 0.0, err / b[q])
            shares.append(float(sh.max(initial=0.0)))
            if check:
                w = int(np.argmax(sh)) if sh.size else 0
                assert (sh <= 1.0).all(), (f"{label}: {('len', 'act', 'dsd')[q]} off by {shares[-1]:.2f} x its bound at pixel "
                                              f"{int(pix[w])}, Gaussian {int(ids[w])}: {g_[member][w]!r} vs {r_[member][w]!r}")
        use[name] = tuple(shares)

    o_sorted = [np.take_along_axis(x[D, :K].astype(np.float64), ord_o, 1) for x in lo[1:]]
    g_sorted = [None if x is None else np.take_along_axis(x[D], ord_g, 1) for x in (gl, ga, gd)]
    measure("kernel", list(zip(g_sorted, o_sorted)), True)
    # positions: the oracle's run label at the member's oracle slot and at its kernel slot
    run = _runs(ol[D, :K], o_live[D, :K], delta)
    run_at_o, run_at_g = np.take_along_axis(run, ord_o, 1), np.take_along_axis(run, ord_g, 1)
    assert (run_at_o == run_at_g)[member].all(), f"{label}: a member sits outside its run of near-equal lens"
    for name, res in (also or {}).items():
        ri = np.asarray(res[0]).reshape(P, K).astype(np.int64)[D]
        key_r = np.where(ri >= 0, ri, BIG)
        ord_r = np.argsort(key_r, axis=1, kind="stable")
        okr = (np.take_along_axis(key_r, ord_r, 1) == set_o).all(1)
        keep = member & okr[:, None]
        r_sorted = [np.take_along_axis(np.asarray(x).reshape(P, K)[D], ord_r, 1) for x in res[1:]]
        saved = member
        member, pix, ids = keep, np.broadcast_to(D[:, None], set_o.shape)[keep], set_o[keep]
        measure(name, list(zip(r_sorted, o_sorted)), False)
        member, pix, ids = saved, np.broadcast_to(D[:, None], set_o.shape)[saved], set_o[saved]

    # ---- undecided pixels
    U = np.nonzero(~decided)[0]
    if U.size:
        wide = np.asarray(oracle_fn(K + 4, thr_act * (1.0 + delta))[0]).reshape(P, K + 4).astype(np.int64)
        for p in U:
            mine = set(gi[p][live[p]].tolist())
            extra = mine - set(wide[p][wide[p] >= 0].tolist())
            assert not extra, f"{label}: pixel {p} (undecided) holds {sorted(extra)}, not among the oracle's first {K + 4}"
            kth_g = float(gl[p, K - 1]) if n_live[p] == K else np.inf
            for m, lm in zip(oi[p][o_live[p]].tolist(), ol[p][o_live[p]].tolist()):
                front = lm < kth_g - delta * max(1.0, abs(lm), abs(kth_g) if np.isfinite(kth_g) else 0.0)
                assert (not front) or m in mine, f"{label}: pixel {p} (undecided) misses {m} at len {lm}, in front of its K-th {kth_g}"
    log_line(f"[trace bounds] {label}: {U.size} of {P} pixels undecided ({100 * und:.2f} %, cap {100 * cap:.0f} %), delta {delta:.2e}; "
             + "; ".join(f"{k} uses {v[0]:.2f} / {v[1]:.2f} / {v[2]:.2f} of the len / act / dsd bound" for k, v in use.items()))
    assert und <= cap, f"{label}: {100 * und:.2f} % of the pixels undecided, cap {100 * cap:.0f} %"
    return dict(undecided=und, use=use, decided=decided)


def cuboid_scene():
    """BASELINE config 1 (Readme.md:81-97): 866 cuboid-surface Gaussians, isotropic."""
    g = np.load(os.path.join(GOLDEN, "misc_api.npz"))
    verts, isig = g["cuboid_verts"], g["cuboid_isigma"]
    return dict(verts=verts, sigmas=isig, colors=((verts + 1) / 3).astype(np.float32), focal=300.0,
                principal=(128.0, 128.0), image_size=(256, 256), dist=6.0, elev=10.0, azim=70.0, K=20)


def bunny_scene():
    """BASELINE config 2 (demo/RenderBunny.py:17-41): 8171 Gaussians, 256x256, f=2000, K=40."""
    g = np.load(os.path.join(GOLDEN, "bunny_gaussians.npz"))
    return dict(verts=g["verts"], sigmas=g["isigma"], colors=g["colors"], focal=2000.0, principal=(128.0, 128.0),
                image_size=(256, 256), dist=6.0, elev=0.0, azim=10.0, K=40)


def random_scene(n, seed=0, aniso=False, lo=0.02, hi=0.04, extent=1.0):
    """SURVEY.md §8d synthetic scene: centres uniform in a cube, radius-derived Sigma^-1 scale."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    r = rng.uniform(lo, hi, n)
    s = 1.0 / (r * r / (2 * np.log(1 / 0.6)))
    if aniso:
        L = np.tril(rng.uniform(-1, 1, (n, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.3
        L = L * np.sqrt(s)[:, None, None]
        sig = (L @ L.transpose(0, 2, 1)).astype(np.float32)
    else:
        sig = s.astype(np.float32)
    colors = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    return verts, sig, colors
