"""The composite walks' erfc evaluator without a range clamp (composite_core.h: h_pair, degree 5) on lists built to reach
everything the clamp used to cover, against the fp64 oracle:

  * window ends INSIDE a row pair: the walk takes the pair for its nearer row, the partner row sits x = 3.6 .. 1e6 outside;
  * K = 5: the back sentinels are +3e38, and lists with s > 1 multiply that gap to x' = +inf;
  * exact ties (x = 0), dead slots inside a lane's group, an empty and a full pixel;
  * one unsorted pixel and one with a NaN len: the cold K x K scan, which keeps the clamped degree-6 evaluator and must give
    the bits it gave before the walks changed (tests/golden/erfc_walks_cold.npz, written by the parent commit's build).

96 pixels; K = 40 takes the flagship forms (four slots per lane forward, two backward), K = 5 the odd-K forms.

Weight bound per slot, derived: |dw| <= w occ eps sum_j E_j + 1e-6 max w, eps = 7.5e-7 + 3.7e-7 -- the fit's 6.0e-7, at most
1.2e-7 for two ulp of the hardware exp2 at values <= 0.5, rounded up to 7.5e-7, plus the 3.7e-7 = erfc(3.5)/2 a window drops per
column; the second term is the fp32 summation over <= K terms.  Gradients: the project's TOL = 1e-4 of scale.
Measured on MI355X (max of |dw| / bound over the slots; largest gradient error of scale over g_act, g_len, g_dsd):
  K = 40: weights 0.28 (max |dw| 5.7e-7), counted from idx or given; gradients 1.1e-6 with the forward's weights and recomputed,
          fused (g_mus / g_isigmas) 1.1e-6 / 8.2e-7
  K = 5:  weights 0.34 (max |dw| 6.8e-7); gradients 1.2e-6 both ways, fused 2.2e-7 / 1.8e-7"""
import os

import numpy as np
import pytest
import torch

import oracle
from util import GOLDEN, TOL, grad_close, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NPIX, H, W = 96, 8, 12
OCC = 0.9
P_GAUSS = 300
KSAT = 3.5                      # composite_core.h: kSat, the window of a column in units of 1 / s
EPS = 7.5e-7 + 3.7e-7
MARGIN = 1e-3                   # every window decision of the reference is at least this far (in x) from its switch
JUMPS = (3.6, 4.5, 7.0, 30.0, 1e3, 1e6)
UNSORTED, NAN_LEN = NPIX - 2, NPIX - 1      # the two cold pixels
COLD_FILE = os.path.join(GOLDEN, "erfc_walks_cold.npz")


def _pixel(rng, K, nv, s_pix, jump):
    """One sorted list of nv live slots (fp32 values): steps of a tie / a fraction of a window / a jump far outside it, the jumps
    placed BEHIND EVEN slots so that the aligned row pair (2t, 2t + 1) straddles them (jump: where in JUMPS this list starts)."""
    s = (s_pix * rng.uniform(0.7, 1.4, K)).astype(np.float32)
    dsd = (s.astype(np.float64) ** 2).astype(np.float32)
    s = np.sqrt(dsd.astype(np.float64))
    ln = np.empty(K, np.float64)
    cur = float(np.float32(rng.uniform(1.0, 2.0)))
    for k in range(K):
        ln[k] = cur
        r = rng.uniform()
        if k % 2 == 0 and r < 0.35:
            step = JUMPS[jump % len(JUMPS)] * rng.uniform(1.0, 1.2) / min(s[k], s[min(k + 1, K - 1)])
            jump += 1
        elif r < 0.5:
            step = 0.0
        else:
            step = rng.uniform(0.05, 2.0) / s[k]
        cur = float(np.float32(cur + step))
    act = rng.uniform(0.0, 4.0, K).astype(np.float32)
    idx = rng.permutation(P_GAUSS)[:K].astype(np.int32)
    ln, act, dsd = ln.astype(np.float32), act, dsd
    ln[nv:], act[nv:], dsd[nv:], idx[nv:] = 1e10, 1e10, 0.0, -1      # what the trace leaves in the slots it did not fill
    return idx, act, ln, dsd


def _conditioned(ln, dsd, nv):
    """The reference's own window decisions: |x_mj| = |len_m - len_j| s_j against kSat for every live (row, column), and the
    steps of the sort -- an exact tie (deliberate) or a clear step."""
    l, s = ln[:nv].astype(np.float64), np.sqrt(dsd[:nv].astype(np.float64) + 1e-10)
    x = np.abs(l[:, None] - l[None, :]) * s[None, :]
    if x.size and np.abs(x - KSAT).min() < MARGIN:
        return False
    step = np.diff(l) * np.maximum(s[1:], s[:-1]) if nv > 1 else np.zeros(0)
    return bool(((step == 0.0) | (step >= MARGIN)).all())


def build_lists(K, cold=None):
    """-> idx [NPIX,K] int32, act, ln, dsd fp32, nv [NPIX].  cold: the golden file's inputs of the two cold pixels (None: made here,
    which is how the golden file itself was written)."""
    rng = np.random.default_rng(1400 + K)
    counts = [0, K] + [[K, K - 1, max(K - 3, 1), K // 2 + 1, 3, 2, 1][p % 7] for p in range(2, NPIX)]
    out = [np.empty((NPIX, K), t) for t in (np.int32, np.float32, np.float32, np.float32)]
    for p in range(NPIX):
        nv = min(counts[p], K)
        if p in (UNSORTED, NAN_LEN):
            nv = counts[p] = K
        s_pix = float(np.exp(rng.uniform(np.log(0.3), np.log(1e3)))) if p % 3 else float(rng.uniform(1.5, 40.0))      # (every third: s > 1)
        for _ in range(200):
            px = _pixel(rng, K, nv, s_pix, p)
            if _conditioned(px[2], px[3], nv):
                break
        else:
            raise AssertionError("no conditioned list found")
        for o, v in zip(out, px):
            o[p] = v
    idx, act, ln, dsd = out
    ln[UNSORTED, [1, K - 2]] = ln[UNSORTED, [K - 2, 1]]
    if ln[UNSORTED, 1] == ln[UNSORTED, K - 2]:
        ln[UNSORTED, 1] += 1.0
    ln[NAN_LEN, 2] = np.nan
    if cold is not None:
        for name, o in zip(("idx", "act", "len", "dsd"), out):
            o[[UNSORTED, NAN_LEN]] = cold[f"in_{name}_k{K}"]
    return idx, act, ln, dsd, np.array(counts)


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def n(x):
    return x.detach().cpu().numpy()


def run_gpu(K, idx, act, ln, dsd, nv, gw):
    """Everything the GPU computes for one K: forward (counted from idx / from the given counts), backward with the forward's
    weights and with recomputed ones, each [NPIX,K]."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ti, ta, tl, td, tg = t(idx, torch.int32), t(act), t(ln), t(dsd), t(gw)
    tc = t(nv, torch.int32)
    res = {}
    for name, cnt in (("idx", None), ("cnt", tc)):
        w = torch.full_like(ta, -7.0)
        vn = torch.full((NPIX,), -7, dtype=torch.int64, device=DEV)
        rc = lib.voge_composite_fwd(ti.data_ptr(), None if cnt is None else cnt.data_ptr(), ta.data_ptr(), tl.data_ptr(), td.data_ptr(), OCC,
                                    NPIX, K, w.data_ptr(), vn.data_ptr(), st)
        assert rc == 0
        res["w_" + name], res["vn_" + name] = w, vn
    for name, wt in (("given", res["w_idx"]), ("recomputed", None)):
        outs = [torch.full_like(ta, -7.0) for _ in range(3)]
        rc = lib.voge_composite_bwd(ta.data_ptr(), tl.data_ptr(), td.data_ptr(), None if wt is None else wt.data_ptr(), None, tg.data_ptr(), OCC,
                                    NPIX, K, *[o.data_ptr() for o in outs], st)
        assert rc == 0
        res["g_" + name] = outs
    torch.cuda.synchronize()
    return {k: ([n(x) for x in v] if isinstance(v, list) else n(v)) for k, v in res.items()}


COLD_KEYS = ("w_idx", "w_cnt", "g_given", "g_recomputed")


def cold_rows(res):
    """The cold pixels' rows of run_gpu's results, as bit patterns (a NaN compares by its bits)."""
    out = {}
    for k in COLD_KEYS:
        v = np.stack(res[k]) if isinstance(res[k], list) else res[k][None]
        out[k] = np.ascontiguousarray(v[:, [UNSORTED, NAN_LEN]]).view(np.uint32)
    return out


@pytest.fixture(scope="module")
def cold():
    return np.load(COLD_FILE)


@pytest.fixture(scope="module", params=[40, 5])
def case(request, cold, hip_lib):
    K = request.param
    idx, act, ln, dsd, nv = build_lists(K, cold)
    gw = np.random.default_rng(77 + K).normal(size=(NPIX, K)).astype(np.float32)
    res = run_gpu(K, idx, act, ln, dsd, nv, gw)
    warm = np.ones(NPIX, bool)
    warm[[UNSORTED, NAN_LEN]] = False
    wr, vr = oracle.composite_fwd(idx[warm], act[warm], ln[warm], dsd[warm], OCC)
    gr = oracle.composite_bwd(act[warm], ln[warm], dsd[warm], gw[warm], OCC)
    return dict(K=K, idx=idx, act=act, ln=ln, dsd=dsd, nv=nv, gw=gw, res=res, warm=warm, wr=wr, vr=vr, gr=gr)


def test_reference_is_conditioned(case):
    """The oracle alone: no window decision of a walked pixel within 1e-3 of its switch, every kind of list present."""
    K, nv, ln, dsd = case["K"], case["nv"], case["ln"], case["dsd"]
    far, ties, inf = 0, 0, 0
    for p in np.nonzero(case["warm"])[0]:
        assert _conditioned(ln[p], dsd[p], nv[p]), p
        l, s = ln[p, :nv[p]].astype(np.float64), np.sqrt(dsd[p, :nv[p]].astype(np.float64))
        ties += int((np.diff(l) == 0).sum())
        for e in range(0, nv[p] - 1, 2):      # the aligned pair (e, e + 1): columns whose window holds one row and not the other
            for j in range(nv[p]):
                if j in (e, e + 1):
                    continue
                xa, xb = abs(l[e] - l[j]) * s[j], abs(l[e + 1] - l[j]) * s[j]
                far += int(min(xa, xb) < KSAT <= max(xa, xb))
        if K % 2 and nv[p] == K and (s[K - 2:] * np.sqrt(np.log2(np.e)) > 1.2).all():
            inf += 1      # the last row shares its pair with +3e38: x' = (3e38 - len) s' overflows
    assert nv[0] == 0 and nv[1] == K and far >= 20 and ties >= 20 and (inf >= 3 or K % 2 == 0), (far, ties, inf)
    assert ((nv % 4 != 0) & (nv > 0)).sum() >= 20 and ((nv % 2 == 1) & (nv > 1)).sum() >= 10      # dead slots inside a lane's group


@pytest.mark.parametrize("counted", ["idx", "cnt"])
def test_weights_within_the_derived_bound(case, counted):
    warm, wr = case["warm"], case["wr"]
    w = case["res"]["w_" + counted][warm].astype(np.float64)
    assert (case["res"]["vn_" + counted][warm] == case["vr"]).all()
    E = np.where(case["idx"][warm] >= 0, np.exp(-case["act"][warm].astype(np.float64)), 0.0)
    bound = wr * OCC * EPS * E.sum(-1, keepdims=True) + 1e-6 * wr.max()
    ratio = np.abs(w - wr) / bound
    log_line(f"[erfc walks] K={case['K']} weights ({counted}): max |dw| {np.abs(w - wr).max():.3e}, max |dw| / bound {ratio.max():.3f}, "
             f"max w {wr.max():.3f}")
    assert np.isfinite(w).all() and (w[case["idx"][warm] < 0] == 0).all()
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("weights", ["given", "recomputed"])
def test_gradients_within_tol(case, weights):
    for name, got, ref in zip(("g_act", "g_len", "g_dsd"), case["res"]["g_" + weights], case["gr"]):
        assert np.isfinite(got[case["warm"]]).all()
        grad_close(f"erfc walks K={case['K']} {weights} weights {name}", got[case["warm"]], ref, TOL)


def test_fused_backward_within_tol(case):
    """voge_fragment_bwd: the same composite backward inside the fused kernel (sorted lists only: it takes the trace's own), then the
    trace's chain rule -- against the oracle's composite_bwd -> trace_bwd."""
    from voge_amd import ops
    K, warm = case["K"], case["warm"]
    rng = np.random.default_rng(5 + K)
    mus = rng.uniform(-1, 1, (P_GAUSS, 3)).astype(np.float32) + np.array([0, 0, 4], np.float32)
    L = np.tril(rng.uniform(-1, 1, (P_GAUSS, 3, 3)))
    L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
    isg = (L @ L.transpose(0, 2, 1)).astype(np.float32)
    rays = rng.normal(size=(NPIX, 3)) * 0.2 + np.array([0, 0, 1.0])
    rays = (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    idx, act, ln, dsd, nv = (case[k].copy() for k in ("idx", "act", "ln", "dsd", "nv"))
    idx[~warm], act[~warm], ln[~warm], dsd[~warm], nv[~warm] = -1, 1e10, 1e10, 0.0, 0      # the cold pixels: empty here
    weight = case["res"]["w_idx"].copy()
    weight[~warm] = 0.0
    tm, ts = t(mus), t(isg)
    g_mus, g_isg = ops._fragment_bwd(0, tm, ts, None, False, 0, t(rays).reshape(1, H, W, 3), t(idx, torch.int32).reshape(1, H, W, K),
                                     t(nv, torch.int32), 1, P_GAUSS, (tm, ts), t(weight), t(act), t(ln), t(dsd), t(case["gw"]), None, OCC)
    torch.cuda.synchronize()
    ga, gl, gd = (np.zeros((NPIX, K)) for _ in range(3))
    ga[warm], gl[warm], gd[warm] = case["gr"]
    _, rm, rs = oracle.trace_bwd(mus, isg, rays, idx, gl, ga, gd)
    assert np.abs(rm).max() > 0 and np.abs(rs).max() > 0
    grad_close(f"erfc walks K={K} fused g_mus", n(g_mus), rm, TOL)
    grad_close(f"erfc walks K={K} fused g_isigmas", n(g_isg).reshape(P_GAUSS, 3, 3), rs, TOL)


def test_cold_pixels_keep_their_bits(case, cold):
    """The unsorted pixel and the NaN-len pixel: the full K x K scan with the clamped evaluator, bit for bit what the build before
    the degree-5 walks gave for the same inputs."""
    K = case["K"]
    for name, a in (("idx", case["idx"]), ("act", case["act"]), ("len", case["ln"]), ("dsd", case["dsd"])):
        assert np.array_equal(a[[UNSORTED, NAN_LEN]].view(np.uint32), cold[f"in_{name}_k{K}"].view(np.uint32))
    ln = case["ln"]
    assert not (np.diff(ln[UNSORTED]) >= 0).all() and np.isnan(ln[NAN_LEN]).sum() == 1
    for k, bits in cold_rows(case["res"]).items():
        want = cold[f"{k}_k{K}"]
        assert np.array_equal(bits, want), (k, int((bits != want).sum()))
    # (and the unsorted pixel's weights are right: the oracle sorts nothing either)
    p = [UNSORTED]
    wr, _ = oracle.composite_fwd(case["idx"][p], case["act"][p], ln[p], case["dsd"][p], OCC)
    assert np.abs(case["res"]["w_idx"][p] - wr).max() < TOL
