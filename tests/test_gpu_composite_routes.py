"""Every route of the stand-alone composite (composite.hip: launch_composite picks the instantiation from K alone), K = 1 .. 256,
against the fp64 oracle at a derived bound.  The routes, the lists and the bound are stated and checked without a GPU in
tests/test_composite_routes_cpu.py; this file runs them.

Per K, 193 pixels (a prime: every route's last workgroup is partial), six launches through the C ABI: the forward counted from
idx and with the counts given, the backward with the forward's weights and with recomputed ones (the one-slot kernel), each
without and with the counts.  Pixels 64 .. 127 are empty (whole waves and workgroups take the early-out), pixels 130 and 191 are
unsorted (the K x K scan beside windowed walks in one workgroup), six pixels repeat six others elsewhere in their workgroup.

Checked: valid_num exact; weights 0 in dead slots, finite, and within the derived bound of test_composite_routes_cpu.py
(|dw| <= w occ [EPS_COL sum_near E_j + 2^-24 (n_pre sum_front E_j + n_h / 2 sum_near E_j)] + 1e-6 max w, the chains counted per
route); six pixels carry a column 3.02 .. 3.3 windows behind a row with weight, where a window cut short shows; gradients within the project's
TOL = 1e-4 of scale; a repeated pixel has its original's bits; a second run has the first one's bits; every output element is
written.  Then the alignment precondition of the wide routes (include/voge_hip.h): ops.composite copies what is off the boundary,
the C entries refuse it, odd K takes anything.

Measured on MI355X (max over the slots and both count modes of |dw| / bound, largest |dw|, largest gradient error of scale over
g_act, g_len, g_dsd and the four backward launches):
  stand-alone entries, K: weights max |dw| / bound (unsorted pixels), max |dw|; gradients of scale (unsorted pixels)
      1: 0.233 (0.000), 4.9e-07; 1.4e-05 (0.0e+00)
      2: 0.252 (0.046), 5.0e-07; 8.2e-07 (9.5e-09)
      3: 0.272 (0.035), 6.1e-07; 8.2e-07 (8.7e-08)
      4: 0.236 (0.099), 6.2e-07; 2.1e-06 (1.7e-06)
      5: 0.260 (0.045), 6.1e-07; 1.5e-06 (2.7e-07)
      6: 0.293 (0.046), 6.2e-07; 1.2e-06 (9.8e-08)
      8: 0.240 (0.039), 5.9e-07; 1.1e-06 (1.5e-07)
     63: 0.145 (0.022), 7.1e-07; 2.2e-06 (1.5e-07)
     64: 0.136 (0.023), 6.0e-07; 9.6e-07 (2.0e-07)
     65: 0.146 (0.025), 7.2e-07; 1.4e-06 (3.6e-08)
     66: 0.136 (0.029), 5.9e-07; 9.5e-07 (5.5e-07)
    126: 0.121 (0.013), 6.3e-07; 1.6e-06 (2.3e-07)
    127: 0.125 (0.010), 6.8e-07; 1.8e-06 (3.7e-07)
    128: 0.106 (0.017), 6.5e-07; 2.3e-06 (2.3e-07)
    129: 0.154 (0.027), 7.5e-07; 1.2e-06 (4.0e-07)
    130: 0.146 (0.012), 7.1e-07; 1.5e-06 (6.8e-07)
    131: 0.135 (0.012), 7.8e-07; 2.7e-06 (1.4e-07)
    132: 0.101 (0.009), 7.3e-07; 1.6e-06 (1.9e-07)
    170: 0.133 (0.016), 8.7e-07; 1.1e-06 (3.7e-07)
    171: 0.130 (0.009), 6.0e-07; 1.3e-06 (8.5e-08)
    253: 0.108 (0.011), 6.5e-07; 2.4e-06 (2.0e-07)
    254: 0.102 (0.008), 6.4e-07; 1.3e-06 (1.6e-07)
    255: 0.118 (0.008), 6.1e-07; 1.8e-06 (1.0e-07)
    256: 0.075 (0.007), 7.4e-07; 9.9e-07 (2.3e-07)
  one-pass entries, K: largest |dw| on the matched pixels; largest gradient error of scale over the five consumers
      1: 2.8e-06; 6.0e-06
      2: 3.5e-06; 4.5e-06
      3: 2.9e-06; 4.8e-06
      5: 3.7e-06; 3.8e-06
      6: 3.6e-06; 6.0e-06
      7: 3.5e-06; 6.8e-06
    125: 6.2e-06; 1.3e-05
    126: 6.1e-06; 1.0e-05
    127: 5.0e-06; 8.8e-06
    128: 4.2e-06; 7.6e-06"""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import camera_np
from test_composite_routes_cpu import COPIES, K_LIST, K_ONEPASS, NPIX, UNSORTED, build_lists, route, weight_bound
from test_gpu_erfc_walks import OCC
from util import TOL, grad_close, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -7.0
FWD = ("w_idx", "w_cnt")
BWD = ("g_given", "g_given_cnt", "g_recomputed", "g_recomputed_cnt")
BAD_ARG = -1


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def n(x):
    return x.detach().cpu().numpy()


def run_gpu(K, idx, act, ln, dsd, nv, gw):
    """The six launches for one K (test_gpu_erfc_walks.run_gpu's set-up), every output pre-filled with -7."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ti, ta, tl, td, tg, tc = t(idx, torch.int32), t(act), t(ln), t(dsd), t(gw), t(nv, torch.int32)
    res = {}
    for name, cnt in (("idx", None), ("cnt", tc)):
        w = torch.full_like(ta, FILL)
        vn = torch.full((NPIX,), int(FILL), dtype=torch.int64, device=DEV)
        rc = lib.voge_composite_fwd(ti.data_ptr(), None if cnt is None else cnt.data_ptr(), ta.data_ptr(), tl.data_ptr(), td.data_ptr(), OCC,
                                    NPIX, K, w.data_ptr(), vn.data_ptr(), st)
        assert rc == 0
        res["w_" + name], res["vn_" + name] = w, vn
    for name, wt in (("given", res["w_idx"]), ("recomputed", None)):
        for suffix, cnt in (("", None), ("_cnt", tc)):
            outs = [torch.full_like(ta, FILL) for _ in range(3)]
            rc = lib.voge_composite_bwd(ta.data_ptr(), tl.data_ptr(), td.data_ptr(), None if wt is None else wt.data_ptr(),
                                        None if cnt is None else cnt.data_ptr(), tg.data_ptr(), OCC, NPIX, K, *[o.data_ptr() for o in outs], st)
            assert rc == 0
            res["g_" + name + suffix] = outs
    torch.cuda.synchronize()
    return {k: (np.stack([n(x) for x in v]) if isinstance(v, list) else n(v)) for k, v in res.items()}


@pytest.fixture(scope="module", params=K_LIST)
def case(request, hip_lib):
    K = request.param
    idx, act, ln, dsd, nv, _ = build_lists(K)
    gw = np.random.default_rng(77 + K).normal(size=(NPIX, K)).astype(np.float32)
    gw[list(COPIES)] = gw[list(COPIES.values())]
    res = run_gpu(K, idx, act, ln, dsd, nv, gw)
    again = run_gpu(K, idx, act, ln, dsd, nv, gw)
    wr, vr = oracle.composite_fwd(idx, act, ln, dsd, OCC)
    gr = np.stack(oracle.composite_bwd(act, ln, dsd, gw, OCC))
    uns = UNSORTED + tuple(d for d, s in COPIES.items() if s in UNSORTED) if K >= 2 else ()
    bound = weight_bound(K, idx, act, ln, dsd, wr, uns)
    return dict(K=K, idx=idx, act=act, ln=ln, dsd=dsd, nv=nv, gw=gw, res=res, again=again, wr=wr, vr=vr, gr=gr, uns=uns, bound=bound)


def _routes(K):
    f, b, r = (route(K, w) for w in ("fwd", "bwd_given", "bwd_recomputed"))
    return (f"fwd {f['NS']} slots {'wave' if f['wave'] else 'workgroup'} {'wide' if f['wide'] else 'by slot'} {f['ppw']} px; "
            f"bwd {'wave' if b['wave'] else 'workgroup'} {b['ppw']} px; one-slot {r['ppw']} px")


def test_every_output_element_is_written(case):
    for k, v in case["res"].items():
        assert (v != FILL).all(), (case["K"], k, int((v == FILL).sum()))


@pytest.mark.parametrize("counted", ["idx", "cnt"])
def test_valid_num_and_dead_slots(case, counted):
    assert (case["res"]["vn_" + counted] == case["vr"]).all() and (case["vr"] == case["nv"]).all()
    dead = case["idx"] < 0
    w = case["res"]["w_" + counted]
    assert np.isfinite(w).all() and (w[dead] == 0).all() and (w[~dead] >= 0).all()


@pytest.mark.parametrize("counted", ["idx", "cnt"])
def test_weights_within_the_derived_bound(case, counted):
    K, wr = case["K"], case["wr"]
    w = case["res"]["w_" + counted].astype(np.float64)
    uns, bound = case["uns"], case["bound"]
    dw = np.abs(w - wr)
    ratio = dw / bound
    sorted_rows = np.ones(NPIX, bool)
    sorted_rows[list(uns)] = False
    log_line(f"[composite routes] K={K} weights ({counted}): max |dw| {dw.max():.3e}, max |dw| / bound {ratio.max():.3f} "
             f"(sorted {ratio[sorted_rows].max():.3f}, unsorted {ratio[~sorted_rows].max() if len(uns) else 0.0:.3f}), max w {wr.max():.3f}; {_routes(K)}")
    assert ratio.max() <= 1.0, (K, counted, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


@pytest.mark.parametrize("launch", BWD)
def test_gradients_within_tol(case, launch):
    got = case["res"][launch]
    assert np.isfinite(got).all() and (got[:, case["idx"] < 0] == 0).all()
    uns = list(UNSORTED) if case["K"] >= 2 else []
    for name, g, ref in zip(("g_act", "g_len", "g_dsd"), got, case["gr"]):
        grad_close(f"composite routes K={case['K']} {launch} {name}", g, ref, TOL)
        if uns:
            grad_close(f"composite routes K={case['K']} {launch} {name} (unsorted pixels)", g[uns], ref[uns], TOL)


def test_a_pixel_does_not_depend_on_where_it_sits(case):
    """composite_core.h: the association of every scan is a function of the slot alone -- row bands equal to the whole frame and
    fused equal to stand-alone rest on it."""
    dst, src = list(COPIES), list(COPIES.values())
    for k in FWD + BWD:
        v = case["res"][k]
        a, b = np.ascontiguousarray(v[..., dst, :]).view(np.uint32), np.ascontiguousarray(v[..., src, :]).view(np.uint32)
        assert np.array_equal(a, b), (case["K"], k, int((a != b).sum()))
    assert (case["res"]["vn_idx"][dst] == case["res"]["vn_idx"][src]).all()


def test_a_second_run_gives_the_same_bits(case):
    for k, v in case["res"].items():
        assert np.array_equal(v.view(np.uint32 if v.dtype == np.float32 else np.int64), case["again"][k].view(np.uint32 if v.dtype == np.float32 else np.int64)), (case["K"], k)


# ---- alignment of the wide routes ------------------------------------------------------------------------------------------------

def _off4(a, dtype=torch.float32):
    """the same values in a contiguous view that starts 4 bytes into a larger buffer"""
    a = t(a, dtype)
    buf = torch.empty(a.numel() + 1, dtype=dtype, device=DEV)
    v = buf[1:].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 8 == 4 and a.data_ptr() % 16 == 0
    return v


def _ops_composite(idx, act, ln, dsd, gw):
    from voge_amd import ops
    act, ln, dsd = (x.requires_grad_(True) for x in (act, ln, dsd))
    w, vn = ops.composite(idx, act, ln, dsd, OCC)
    w.backward(gw)
    torch.cuda.synchronize()
    return [n(x).view(np.uint32) for x in (w, act.grad, ln.grad, dsd.grad)] + [n(vn)]


@pytest.mark.parametrize("K", [8, 6, 5])
def test_ops_composite_takes_views_off_the_boundary(hip_lib, K):
    """K = 8 (16-byte accesses forward, 8 backward), 6 (8 both ways), 5 (slot by slot: nothing to copy): every input and the
    incoming gradient 4 bytes into a larger buffer -> the bits of the aligned tensors."""
    idx, act, ln, dsd, nv, _ = build_lists(K)
    gw = np.random.default_rng(3 + K).normal(size=(NPIX, K)).astype(np.float32)
    want = _ops_composite(t(idx, torch.int32), t(act), t(ln), t(dsd), t(gw))
    got = _ops_composite(_off4(idx, torch.int32), _off4(act), _off4(ln), _off4(dsd), _off4(gw))
    for name, a, b in zip(("weight", "g_act", "g_len", "g_dsd", "valid_num"), got, want):
        assert np.array_equal(a, b), (K, name)
    assert (want[4] == nv).all() and want[0].any() and want[1].any()


@pytest.mark.parametrize("K", [8, 6])
def test_c_entries_refuse_pointers_off_the_boundary(hip_lib, K):
    """One array at a time off its boundary: VOGE_ERR_BAD_ARG, nothing launched -- the pre-filled outputs keep their fill."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    idx, act, ln, dsd, nv, _ = build_lists(K)
    ti, vn = t(idx, torch.int32), torch.full((NPIX,), int(FILL), dtype=torch.int64, device=DEV)
    good = dict(act=t(act), len=t(ln), dsd=t(dsd), weight=torch.full((NPIX, K), FILL, device=DEV))
    for name in good:
        a = dict(good)
        a[name] = _off4(n(good[name]))
        rc = lib.voge_composite_fwd(ti.data_ptr(), None, a["act"].data_ptr(), a["len"].data_ptr(), a["dsd"].data_ptr(), OCC, NPIX, K,
                                    a["weight"].data_ptr(), vn.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == BAD_ARG, (K, name, rc)
        assert (a["weight"] == FILL).all() and (good["weight"] == FILL).all() and (vn == int(FILL)).all(), (K, name)
    good = dict(act=t(act), len=t(ln), dsd=t(dsd), weight=t(np.abs(act) * 0 + 0.5), g_weight=t(act * 0 + 1),
                g_act=torch.full((NPIX, K), FILL, device=DEV), g_len=torch.full((NPIX, K), FILL, device=DEV), g_dsd=torch.full((NPIX, K), FILL, device=DEV))
    for name in good:
        a = dict(good)
        a[name] = _off4(n(good[name]))
        rc = lib.voge_composite_bwd(a["act"].data_ptr(), a["len"].data_ptr(), a["dsd"].data_ptr(), a["weight"].data_ptr(), None, a["g_weight"].data_ptr(),
                                    OCC, NPIX, K, a["g_act"].data_ptr(), a["g_len"].data_ptr(), a["g_dsd"].data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == BAD_ARG, (K, name, rc)
        for o in ("g_act", "g_len", "g_dsd"):
            assert (a[o] == FILL).all() and (good[o] == FILL).all(), (K, name, o)


def test_c_entries_take_any_pointer_at_odd_k(hip_lib):
    """K = 5 goes slot by slot both ways: every array 4 bytes off -> accepted, and the aligned arrays' bits."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    K = 5
    idx, act, ln, dsd, nv, _ = build_lists(K)
    gw = np.random.default_rng(8).normal(size=(NPIX, K)).astype(np.float32)
    out = []
    for mk in (lambda a, d=torch.float32: t(a, d), _off4):
        ti, ta, tl, td, tg = mk(idx, torch.int32), mk(act), mk(ln), mk(dsd), mk(gw)
        w, vn = mk(np.full((NPIX, K), FILL, np.float32)), torch.full((NPIX,), int(FILL), dtype=torch.int64, device=DEV)
        gs = [mk(np.full((NPIX, K), FILL, np.float32)) for _ in range(3)]
        assert lib.voge_composite_fwd(ti.data_ptr(), None, ta.data_ptr(), tl.data_ptr(), td.data_ptr(), OCC, NPIX, K, w.data_ptr(), vn.data_ptr(), st) == 0
        assert lib.voge_composite_bwd(ta.data_ptr(), tl.data_ptr(), td.data_ptr(), w.data_ptr(), None, tg.data_ptr(), OCC, NPIX, K,
                                      *[g.data_ptr() for g in gs], st) == 0
        torch.cuda.synchronize()
        out.append([n(x).view(np.uint32) for x in [w] + gs] + [n(vn)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert (out[0][4] == nv).all() and (out[0][0] != np.float32(FILL).view(np.uint32)).all()


# ---- the one-pass entries on lists that are really full ---------------------------------------------------------------------------
# composite_shade_fwd_impl / voge_frame_depth_fwd_iso put four slots on a lane whatever K is, so K % 4 != 0 leaves the last group
# short (`has[a]`, `lead`) -- except voge_composite_fwd_iso (scalar sigmas, vert_weight read directly), which goes through
# launch_composite and takes the stand-alone forward's choice: two slots for K % 4 != 0, from the records.  act / dsd come from the records, so they run on frames, through the public renderer: 16 x 12 pixels, a
# cube of Gaussians dense enough that some lists hold exactly K hits and some K - 1 .. K - 3, with empty pixels around it.
ONE_H, ONE_W = 12, 16
FORMS = ("scalar", "diag", "full")
CONSUMERS = ("white3", "white4", "attr_sil", "depth", "weight")
# (N, seed) per (form, K): found on the CPU with the oracle alone, so that the lists meet test_one_pass_*'s conditions
SCENES = {("scalar", 1): (45, 103), ("scalar", 2): (44, 203), ("scalar", 3): (56, 300), ("scalar", 5): (45, 505), ("scalar", 6): (52, 600),
          ("scalar", 7): (59, 702), ("scalar", 125): (1520, 12500), ("scalar", 126): (1532, 12603), ("scalar", 127): (1544, 12701),
          ("scalar", 128): (1556, 12800), ("diag", 1): (45, 103), ("diag", 2): (44, 203), ("diag", 3): (56, 301), ("diag", 5): (45, 507),
          ("diag", 6): (52, 600), ("diag", 7): (59, 702), ("diag", 125): (1520, 12500), ("diag", 126): (1532, 12600), ("diag", 127): (1544, 12700),
          ("diag", 128): (1556, 12801), ("full", 1): (17, 102), ("full", 2): (9, 211), ("full", 3): (11, 311), ("full", 5): (16, 503),
          ("full", 6): (19, 601), ("full", 7): (34, 700), ("full", 125): (885, 12500), ("full", 126): (892, 12600), ("full", 127): (899, 12700),
          ("full", 128): (906, 12800)}
ONE_PASS_ENTRIES = ("voge_composite_fwd_iso", "voge_composite_shade_fwd_iso", "voge_frame_shade_fwd_iso", "voge_frame_shade_fwd_rec",
                    "voge_frame_depth_fwd_iso", "voge_composite_fwd_rec", "voge_composite_shade_fwd_rec")
OTHER_ENTRIES = ("voge_composite_fwd", "voge_merge_fwd", "voge_silhouette_fwd", "voge_depth_fwd")


def one_pass_cases():
    """Every K with every consumer; the sigma forms dealt round-robin over the K list (get_depth's one-pass form: scalar sigmas)."""
    out = []
    for c, consumer in enumerate(CONSUMERS):
        for i, K in enumerate(K_ONEPASS):
            out.append((K, "scalar" if consumer == "depth" else FORMS[(i + c) % 3], consumer))
    return out


def expected_entry(form, consumer):
    """ops._composite_fwd / ops._CompositeDepth: the general forms' records have one entry; scalar sigmas one per consumer."""
    if form != "scalar":
        return "voge_frame_shade_fwd_rec"
    return {"white3": "voge_frame_shade_fwd_iso", "white4": "voge_frame_shade_fwd_iso", "attr_sil": "voge_frame_shade_fwd_iso",
            "depth": "voge_frame_depth_fwd_iso", "weight": "voge_composite_fwd_iso"}[consumer]


def _one_scene(K, form):
    N, seed = SCENES[(form, K)]
    rng = np.random.default_rng(seed)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.45).astype(np.float32)
    r = rng.uniform(0.07, 0.11, N)
    s = (1.0 / (r * r / (2 * np.log(1 / 0.6)))).astype(np.float32)
    if form == "scalar":
        sig = s
    elif form == "diag":
        sig = (s[:, None] * rng.uniform(0.6, 1.6, (N, 3))).astype(np.float32)
    else:
        L = np.tril(rng.uniform(-1, 1, (N, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
        L = L * np.sqrt(s)[:, None, None] * 0.8
        sig = (L @ L.transpose(0, 2, 1)).astype(np.float32)
    cols = np.random.default_rng(seed + 1).uniform(0, 1, (N, 4)).astype(np.float32)
    return dict(verts=verts, sigmas=sig, colors=cols, focal=30.0, principal=(ONE_W / 2.0, ONE_H / 2.0), image_size=(ONE_H, ONE_W), dist=4.0,
                elev=10.0, azim=70.0, K=K)


@functools.lru_cache(maxsize=None)
def _one_frame(K, form):
    """One oracle frame per (K, form), shared by its consumers (trace + composite; the colour stages are added per consumer)."""
    import test_gpu_configs as cfg
    sc = _one_scene(K, form)
    R, T = camera_np.look_at_view_transform(sc["dist"], sc["elev"], sc["azim"])
    ref = cfg._oracle_frame(dict(sc, colors=sc["colors"][:, :3]), R, T)
    ref["occ"] = 1.0
    return sc, ref


def _with_colors(sc, ref, C):
    sc = dict(sc, colors=np.ascontiguousarray(sc["colors"][:, :C]))
    ref = dict(ref, colsB=sc["colors"])
    ref["rgb"] = oracle.merge_fwd(ref["colsB"], ref["idx"], ref["weight"], ref["valid_num"])
    ref["image"], ref["silhouette"] = oracle.blend_fwd(ref["rgb"], ref["weight"], bg=(1.0,) * C)
    return sc, ref


@pytest.mark.parametrize("K,form,consumer", one_pass_cases())
def test_one_pass_entries_on_full_lists(hip_lib, monkeypatch, K, form, consumer):
    import test_gpu_configs as cfg
    import test_gpu_depth as dpt
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import get_depth, get_silhouette, interpolate_attr, to_colored_background, to_white_background
    sc, ref = _one_frame(K, form)
    label = f"one-pass K={K} {form} {consumer}"
    # the oracle's lists alone: really full, nearly full, empty
    vn = ref["valid_num"].ravel()
    assert (vn == K).any() and np.isin(vn, [k for k in (K - 1, K - 2, K - 3) if k >= 0]).any() and (vn == 0).any(), label
    calls = dpt.count_calls(monkeypatch, ONE_PASS_ENTRIES + OTHER_ENTRIES)
    renderer = dpt.renderer_for(ONE_H, ONE_W, K, sc["focal"])
    gm = GaussianMeshes(cfg.t(sc["verts"]), cfg.t(sc["sigmas"])).to(DEV)
    R, T = camera_np.look_at_view_transform(sc["dist"], sc["elev"], sc["azim"])
    frag = renderer(gm, R=cfg.t(R), T=cfg.t(T))
    rng = np.random.default_rng(9 + K)
    colors = None
    if consumer in ("white3", "white4"):
        C = int(consumer[-1])
        sc_c, ref_c = _with_colors(sc, ref, C)
        colors = cfg.t(sc_c["colors"], rg=True)
        # (four channels: to_white_background's (1, 1, 1) does not broadcast -- the same white through to_colored_background)
        out = to_white_background(frag, colors) if C == 3 else to_colored_background(frag, colors, background_color=(1.0,) * C)
    elif consumer == "attr_sil":
        sc_c, ref_c = _with_colors(sc, ref, 3)
        colors = cfg.t(sc_c["colors"], rg=True)
        out = interpolate_attr(frag, colors)
        sil = get_silhouette(frag)
    elif consumer == "depth":
        out = get_depth(frag, normalize=True, background=dpt.BG)
    else:
        out = frag.vert_weight
    got = {k: v for k, v in calls.items() if v}
    assert got == {expected_entry(form, consumer): 1}, (label, got)
    idx = n(frag.vert_index)
    same = (idx == np.where(ref["idx"] < 0, 0, ref["idx"])).all(-1) | (idx == ref["idx"]).all(-1)
    assert same.mean() >= 0.9, f"{label}: only {same.mean():.3f} of the pixels have the oracle's index list"
    assert (n(frag.valid_num)[same] == ref["valid_num"][same]).all()
    dw = np.abs(n(frag.vert_weight)[same] - ref["weight"][same]).max()
    assert dw < TOL, (label, dw)
    if consumer in ("white3", "white4"):
        err = np.abs(n(out)[same] - ref_c["image"][same]).max()
        assert err < TOL, (label, err)
        g_img = rng.normal(size=ref_c["image"].shape) * same[..., None]
        (out * cfg.t(g_img)).sum().backward()
        want = cfg._oracle_grads(sc_c, ref_c, g_img)
        cfg._check_grads(label, (colors.grad, gm.verts.grad, gm.sigmas.grad), want, mult=1)
    elif consumer == "attr_sil":
        s_ref = np.minimum(ref["weight"].sum(-1), 1.0)
        err = max(np.abs(n(out)[same] - ref_c["rgb"][same]).max(), np.abs(n(sil)[same] - s_ref[same]).max())
        assert err < TOL, (label, err)
        g_rgb = rng.normal(size=ref_c["rgb"].shape) * same[..., None]
        g_s = rng.normal(size=s_ref.shape) * same
        ((out * cfg.t(g_rgb)).sum() + (sil * cfg.t(g_s)).sum()).backward()
        g_attr, g_w = oracle.merge_bwd(ref_c["colsB"], ref["idx"], ref["weight"], ref["valid_num"], g_rgb)
        g_w = g_w + (g_s * (ref["weight"].sum(-1) < 1))[..., None]
        g_mu, g_sig = dpt.oracle_param_grads(ref, sc["sigmas"], g_w)
        cfg._check_grads(label, (colors.grad, gm.verts.grad, gm.sigmas.grad), (g_attr.reshape(-1, 3), g_mu, g_sig), mult=1)
    elif consumer == "depth":
        D_ref, S_ref, live = dpt.depth_ref(ref["weight"], ref["len"], ref["valid_num"], True, dpt.BG)
        assert dpt.close(n(out)[same], D_ref[same]).all(), (label, dpt.max_rel(n(out)[same], D_ref[same]))
        assert (n(out)[(ref["valid_num"] == 0) & same] == np.float32(dpt.BG)).all()
        g = rng.normal(size=D_ref.shape) * same
        (out * cfg.t(g)).sum().backward()
        g_w, g_h = dpt.depth_grads_ref(ref["weight"], ref["len"], ref["valid_num"], g, True)
        g_mu, g_sig = dpt.oracle_param_grads(ref, sc["sigmas"], g_w, g_h)
        grad_close(f"{label} verts", n(gm.verts.grad), g_mu, 0.25 * TOL)
        grad_close(f"{label} sigmas", n(gm.sigmas.grad), g_sig, 0.25 * TOL)
    else:
        g_w = rng.normal(size=ref["weight"].shape) * same[..., None]
        (out * cfg.t(g_w)).sum().backward()
        g_mu, g_sig = dpt.oracle_param_grads(ref, sc["sigmas"], g_w)
        grad_close(f"{label} verts", n(gm.verts.grad), g_mu, TOL)
        grad_close(f"{label} sigmas", n(gm.sigmas.grad), g_sig, TOL)
    log_line(f"[composite routes] {label}: {int((vn == K).sum())} full pixels, {int((vn == 0).sum())} empty, {int((~same).sum())} flipped, "
             f"max |dw| {dw:.2e}, entry {expected_entry(form, consumer)}")
