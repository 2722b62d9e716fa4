"""Each case of tests/trace_bound_cases.py is what it claims -- in fp64 numpy and with the oracle alone, no GPU: the cones the
kernels would make of its rays, where its centres sit against depth_key's tests, what the oracle yields, that its membership is
decided on >= 95 % of the pixels at its delta <= 1e-4, and that util.compare_trace_strict accepts a correct result and refuses one
with a candidate missing just in front of the K-th."""
import numpy as np
import pytest

import oracle
import trace_bound_cases as tb
from util import compare_trace_strict, log_line

IDS = tb.case_ids()


def _ids(v):
    return f"{v[0]}-{v[1]}"


def block_cone(rays):
    """(axis, cmin, all finite) of a block of rays as the kernels make it: axis = the normalised sum of the finite rays."""
    d = rays.reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        n2 = (d * d).sum(1)
        fin = (n2 > 1e-30) & (n2 < 1e30)
    s = d[fin].sum(0)
    ax = s / np.linalg.norm(s)
    cmin = float(((d[fin] @ ax) / np.sqrt(n2[fin])).min())
    return ax, cmin, bool(fin.all()), float(np.linalg.norm(s) / max(fin.sum(), 1))


def cones_of_level(rays, edge):
    H, W = rays.shape[1:3]
    return [block_cone(rays[0, y:y + edge, x:x + edge]) for y in range(0, H, edge) for x in range(0, W, edge)]


def usable(c):
    """cone_finish's test (voge_common.h): every ray finite, n > 1e-3, cmin > 0.05."""
    return c[2] and c[3] > 1e-3 and c[1] > 0.05


@pytest.mark.parametrize("cs", IDS, ids=_ids)
def test_undecided_share_and_delta(cs):
    case = tb.build(*cs)
    delta, d_len, d_act, outside = tb.case_delta(*cs)
    log_line(f"[trace bounds] {case.name}/{case.size}: N {case.N}, delta {delta:.2e} (len {d_len:.2e}, act {d_act:.2e}), outside-band ratio {outside:.2e}")
    assert delta <= 1e-4
    assert outside < 1.0, "a pair far from the threshold has an act bound that reaches it"
    fn = tb.case_oracle(*cs)
    K = case.K
    got = [np.asarray(x) for x in fn(K, case.thr_act)]
    res = compare_trace_strict(tuple(got), fn, K,
                               case.thr_act, delta, tb.CAP, f"oracle as its own result, {case.name}/{case.size}", n_per_batch=case.N)
    assert res["undecided"] <= tb.CAP
    if case.exit_case:
        full = (got[0] >= 0).all(-1).mean()
        assert full > 0.5, f"lists are full on only {full:.2f} of the pixels"
    for (y, x) in case.empty_pixels:
        assert (got[0][0, y, x] == -1).all(), f"the oracle has hits at the degenerate ray ({y}, {x})"


@pytest.mark.parametrize("cs", [("nonunit_one_pixel", "binned"), ("front_4r", "small"), ("twins", "binned")], ids=_ids)
def test_strict_comparison_refuses_a_candidate_dropped_in_front_of_the_kth(cs):
    """What compare_trace forgives: on a decided pixel with a full list, drop the (K-1)-th member and let the (K+1)-th take the
    last slot -- 'an early exit that dropped a candidate'."""
    case = tb.build(*cs)
    delta = tb.case_delta(*cs)[0]
    fn = tb.case_oracle(*cs)
    K = case.K
    ok = compare_trace_strict(tuple(np.asarray(x) for x in fn(K, case.thr_act)), fn, K, case.thr_act, delta, tb.CAP, "self", n_per_batch=case.N)
    wide = [np.array(x).reshape(-1, K + 1) for x in fn(K + 1, case.thr_act * (1 - delta))]
    p = int(np.nonzero(ok["decided"] & (wide[0] >= 0).all(1))[0][0])
    bad = [np.array(x).reshape(-1, K) for x in fn(K, case.thr_act)]
    for b, w in zip(bad, wide):
        b[p, K - 2:] = w[p, K - 1:]
    with pytest.raises(AssertionError, match="another index set"):
        compare_trace_strict(tuple(x.reshape(1, *case.rays.shape[1:3], K) for x in bad), fn, K, case.thr_act, delta, tb.CAP, "dropped", n_per_batch=case.N)


@pytest.mark.parametrize("size", ["small", "binned"])
def test_near_unit_candidates_lie_between_the_unit_bound_and_the_scaled_one(size):
    """Rays of length s: len = mu . u / s.  The bins' bound of a front candidate is a depth along a UNIT direction: its bucket's lower
    edge less 4e-6 span, 1e-5 |edge| and 1.13 Rmax (Rmax with the 2e-5 |mu| of iso_cull_record; 1e-5 |mu| on the general entry).
    binB orders a quad's entries by bucket only, and every entry of a bucket carries the bucket's edge.  Proved here per 16x16 quad:
    all near candidates share bucket 0 (510 buckets over the span the far Gaussians stretch), whose edge is the quad's nearest key;
    at s - 1 = 4e-5 and 4.9e-5 EVERY near candidate's fp64 len lies below that bound with all its margins while its ray holds a
    same-bucket candidate of larger len -- a tile that exits on the bound once its lists are full loses whichever member arrives
    late, which is what the kernels did while `unit` allowed |dn2 - 1| < 1e-4 -- and at s - 1 = 1.9e-5 (inside the 4e-5 it allows
    now) and at s < 1 every len lies above the bound, on both entries."""
    for name, s1 in (("near_unit_plus", tb.NEAR_UNIT_S), ("near_unit_edge", tb.NEAR_UNIT_EDGE), ("near_unit_inside", tb.NEAR_UNIT_INSIDE),
                     ("near_unit_minus", -tb.NEAR_UNIT_S)):
        case = tb.build(name, size)
        H, W = case.rays.shape[1:3]
        d = case.rays.astype(np.float64).reshape(-1, 3)
        assert np.abs(np.linalg.norm(d, axis=1) - (1 + s1)).max() < 2e-7
        assert (np.abs((d * d).sum(1) - 1.0) < 1e-4).all() and ((np.abs((d * d).sum(1) - 1.0) < 4e-5).all() == (abs(s1) < 2e-5))
        idx, ln, _, _ = (x.reshape(H, W, case.K + 1) for x in tb.case_oracle(name, size)(case.K + 1, case.thr_act))
        assert (idx >= 0).all(), "every ray holds K + 1 candidates"
        key = tb.fp32_norm(case.mus).astype(np.float64)
        reach = np.sqrt(case.thr_act / case.a.astype(np.float64))
        assert (reach < 1e-4 * key).all()
        far = key > tb.NEAR_UNIT_D * 1.005
        below = above = 0
        for y0 in range(0, H, 16):
            for x0 in range(0, W, 16):
                qi, ql = idx[y0:y0 + 16, x0:x0 + 16].reshape(-1, case.K + 1), ln[y0:y0 + 16, x0:x0 + 16].reshape(-1, case.K + 1)
                near = np.unique(qi)
                assert not far[near].any()
                # the quad's keys: its rays' candidates and the far Gaussians of its four tiles (on the rays of pixels (4, 4) of a tile)
                u = d.reshape(H, W, 3)[y0 + 4:y0 + 16:8, x0 + 4:x0 + 16:8].reshape(-1, 3) / (1 + s1)
                mf = case.mus.astype(np.float64)[far]
                qfar = np.nonzero(far)[0][(np.linalg.norm(mf[:, None] / np.linalg.norm(mf, axis=1)[:, None, None] - u[None], axis=2) < 1e-4).any(1)]
                assert qfar.size == u.shape[0] >= 2
                lo, hi = key[near].min(), key[qfar].max()
                span = hi - lo
                assert (np.floor((key[near] - lo) * 510 / span) == 0).all(), "the near candidates do not share a bucket"
                for pad in (2e-5, 1e-5):      # the scalar entry's reach, the general entry's
                    rmax = max((reach[near] * (1 + 2e-5) + pad * key[near]).max(), (reach[qfar] * (1 + 2e-5) + pad * key[qfar]).max())
                    edge = lo - 4e-6 * span
                    bound = edge - 1.13 * rmax * (1 + 1e-5) - 1e-5 * edge
                    if s1 >= tb.NEAR_UNIT_S:
                        # every candidate but a ray's farthest has a same-bucket candidate of larger len on its ray; all lie below the bound
                        assert (ql < bound).all()
                        below += ql[:, :-1].size
                    else:
                        assert (ql > bound).all()
                        above += ql.size
        log_line(f"[trace bounds] {name}/{size}: {below} (pixel, candidate) pairs below the bound with all margins beside a same-bucket "
                 f"candidate of larger len; {above} above it")
        assert (below > 0) == (s1 >= tb.NEAR_UNIT_S)


def test_nonunit_bundles():
    r = tb.build("nonunit_random", "binned").rays.astype(np.float64)
    n = np.linalg.norm(r, axis=-1)
    assert n.min() >= 0.25 - 1e-6 and n.max() <= 4.0 + 1e-6 and (np.abs(n * n - 1) >= 1e-4).mean() > 0.99
    r = tb.build("nonunit_one_pixel", "binned").rays.astype(np.float64)[0]
    off = np.abs((r * r).sum(-1) - 1.0) >= 1e-4
    per_tile = off.reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(64, 64).sum(1)
    assert (per_tile[0::2] == 1).all() and (per_tile[1::2] == 0).all()
    for size in tb.SIZES:
        c9, c12 = tb.build("nonunit_1e-9", size), tb.build("nonunit_1e-12", size)
        l9 = tb.case_oracle("nonunit_1e-9", size)(c9.K, c9.thr_act)[1]
        hit = l9 < 1e10
        assert hit.any() and l9[hit].max() > 6e9, "no hit near the sentinel"
        # some Gaussians the rays do hit are dropped by len < 1e10 alone
        unit = tb.pinhole(64, 64, 64.0)
        l_unit = oracle.trace_fwd(c9.mus, c9.isigmas(), unit, c9.K, c9.thr_act)[1]
        assert ((l_unit < 1e10) & (l_unit > 10.5)).any()
        assert (tb.case_oracle("nonunit_1e-12", size)(c12.K, c12.thr_act)[0] == -1).all()


def test_wide_angle_cones():
    r6, r2 = tb.build("wide_6px", "binned").rays, tb.build("wide_2px", "binned").rays
    st6 = cones_of_level(r6, 32)
    assert all(usable(c) for c in st6) and min(c[1] for c in st6) < 0.5, [c[1] for c in st6]      # ok, but cs < 0.5: keys are -|mu|
    region = block_cone(r2[0])
    assert region[1] <= 0.05, region[1]                      # the region's cone fails cmin > 0.05 ...
    tiles = cones_of_level(r2, 8)
    assert min(c[1] for c in tiles) > 0.05, min(c[1] for c in tiles)      # ... while every tile's holds
    log_line(f"[trace bounds] wide_6px super-tile cmin {[round(c[1], 3) for c in st6]}; wide_2px region cmin {region[1]:.4f}, "
             f"smallest tile cmin {min(c[1] for c in tiles):.3f}")


def test_scrambled_cones():
    r = tb.build("scrambled", "small").rays
    for edge in (8, 16, 32, 64):
        assert not any(usable(c) for c in cones_of_level(r, edge)), f"a usable cone at edge {edge}"
    ln = tb.case_oracle("scrambled", "small")(6, tb.THR_ACT)
    live = ln[0] >= 0
    assert (ln[1][live] < 0).any() and (ln[1][live] > 0).any()
    r = tb.build("scrambled_supertiles", "binned").rays
    assert all(usable(c) for c in cones_of_level(r, 32))
    H, W = r.shape[1:3]
    rows = [block_cone(r[0, y:y + 32]) for y in range(0, H, 32)]
    # the region's cone is !ok, so binA sets use_rows (trace_bin.h: `!cn.ok || cn.sn > 1.6 widest_row`) and tests the rows' cones;
    # the rows are pairs of unrelated super-tiles: wide or !ok themselves (logged), while every super-tile's own cone is tight
    assert not usable(block_cone(r[0]))
    assert max(c[1] for c in rows) < min(c[1] for c in cones_of_level(r, 32))
    log_line(f"[trace bounds] scrambled_supertiles: region cmin {block_cone(r[0])[1]:.3f}, rows' cmin {[round(c[1], 3) for c in rows]}")


def test_centres_against_depth_keys_tests():
    for size in tb.SIZES:
        c = tb.build("front_4r", size)
        nm = np.linalg.norm(c.mus.astype(np.float64), axis=1)
        # the reach as iso_cull_record pads it: r (1 + 2e-5) + 2e-5 |mu|
        reach = np.sqrt(c.thr_act / c.a.astype(np.float64)) * (1 + 2e-5) + 2e-5 * nm
        kind = c.notes["kind"]
        edge = kind == 1
        above, below = (nm[edge] > 4 * reach[edge]).mean(), (nm[edge] <= 4 * reach[edge]).mean()
        assert above > 0.25 and below > 0.25 and np.abs(nm[edge] / reach[edge] - 4).max() < 2e-3
        assert (nm[kind == 2] < reach[kind == 2]).all() and np.abs(nm[kind == 3] / reach[kind == 3] - 1).max() < 2e-3
        idx, ln, _, _ = tb.case_oracle("front_4r", size)(c.K, c.thr_act)
        assert (ln[idx >= 0] < 0).mean() > 0.3, "hits behind the camera"
        for k in (1, 2, 3):
            assert np.isin(np.nonzero(kind == k)[0], idx).any(), f"no Gaussian of kind {k} is anybody's member"
        log_line(f"[trace bounds] front_4r/{size}: {above:.2f} of the boundary centres beyond 4 R, {below:.2f} inside")
        c = tb.build("shell_one", size)
        assert np.unique(tb.fp32_norm(c.mus)).size == 1      # span == 0 in fp32
        c = tb.build("shell_two", size)
        assert sorted(np.unique(tb.fp32_norm(c.mus)).tolist()) == [np.float32(1e-2), np.float32(1e3)]
        hit = tb.case_oracle("shell_two", size)(c.K, c.thr_act)[1]
        assert ((hit < 1) & (hit > 0)).any() and ((hit > 100) & (hit < 1e10)).any()


def test_mixed_reach_and_invalid_forms_and_needles_and_twins():
    for size in tb.SIZES:
        for name in ("mixed_reach_behind", "mixed_reach_front"):
            c = tb.build(name, size)
            fn = tb.case_oracle(name, size)
            delta = tb.case_delta(name, size)[0]
            res = compare_trace_strict(tuple(np.asarray(x) for x in fn(c.K, c.thr_act)), fn, c.K, c.thr_act, delta, tb.CAP, "self", n_per_batch=c.N)
            idx = fn(c.K, c.thr_act)[0].reshape(-1, c.K)[res["decided"]]
            assert np.isin(c.notes["big"], idx).all(), f"{name}: a big Gaussian is nobody's member"
        c = tb.build("invalid_scalar", size)
        idx = tb.case_oracle("invalid_scalar", size)(c.K, c.thr_act)[0]
        w = c.notes["where"]
        neg = [g for g in w[:12] if c.a[g] == -1.0]
        assert np.isin(neg, idx).all() and not np.isin([g for g in w if g not in neg], idx).any()
        c = tb.build("invalid_general", size)
        assert np.array_equal(c.A, c.A.transpose(0, 2, 1))
        ev = np.linalg.eigvalsh(c.A.astype(np.float64)[c.notes["where"]])
        assert (ev[0::2, 0] < 0).all() and (ev[1::2, 0] == 0).all()
        c = tb.build("needles", size)
        m = c.mus.astype(np.float64)
        inside = np.einsum("ni,nij,nj->n", m, c.A.astype(np.float64), m) < c.thr_act
        assert np.array_equal(np.nonzero(inside)[0], c.notes["where"]), "the needles, and only they, contain the camera"
        assert np.isin(c.notes["where"], tb.case_oracle("needles", size)(c.K, c.thr_act)[0]).mean() > 0.5
        c = tb.build("twins", size)
        idx, ln, _, _ = (x.reshape(-1, c.K) for x in tb.case_oracle("twins", size)(c.K, c.thr_act))
        pair = (idx[:, 1:] == idx[:, :-1] + c.N // 2) & (idx[:, :-1] >= 0)
        assert pair.sum() > 1000 and (ln[:, 1:][pair] == ln[:, :-1][pair]).all()
