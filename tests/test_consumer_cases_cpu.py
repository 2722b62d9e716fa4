"""CPU proof of what tests/test_gpu_consumers.py relies on (nothing here measures a kernel): in every case of
tests/consumer_cases.py no decision is near its edge, so the lists, the clamps and the signs are the reference's on any correct
fp32 evaluation; a lost or doubled term of any of the nine consumers moves a leaf's gradient by at least 10 TOL of its scale; the
composition evaluated in fp32 on the host stays within TOL / 4 of the fp64 one; and the orders are what they claim."""
import numpy as np
import pytest
import torch

import consumer_cases as C
import oracle
import trace_bound_cases as TB
from consumer_cases import H, HIDDEN, N, W
from util import TOL, close, grad_close, log_line

KEYS = sorted({C.case_key(name) for name in C.CASES}, key=str)
MARGIN = 1e-3      # |sum_k w_k - 1|, |M|, the images' clamp at 1, the normals' signs


def key_id(key):
    return f"{key[0]}-B{key[1]}-K{key[2]}" + ("-inverse" if key[3] else "")


def test_every_case_has_a_reference_and_the_cases_are_the_issues_ten():
    assert len(C.CASES) == 10 and len(KEYS) == 7
    assert {C.case_key(n) for n in ("frame", "frame_nodirect", "bundle", "bundle_kept")} == {("scalar", 1, 5, False)}
    assert (H, W, N, HIDDEN) == (7, 10, 40, 3) and W % 4 and H % 3 and W % 8 and H % 2


def test_the_orders_do_what_they_claim():
    orders = C.ORDERS
    assert len(orders) == 12 and len(set(orders.values())) == 12
    for name, seq in orders.items():
        assert sorted(seq) == sorted(C.CONSUMERS), name
        assert seq.index("depth") < seq.index("n_depth"), name
    rot = [seq for name, seq in orders.items() if name.startswith("rot")]
    assert len(rot) == 9
    # rotation i begins with consumer i; n_depth reads no fragments -- it is made from depth's output --, so in its rotation the
    # two change places: depth reads first and n_depth is made last, after every other consumer
    firsts = [seq[0] for seq in rot]
    for i, (name, seq) in enumerate(zip(C.CONSUMERS, rot)):
        if name == "n_depth":
            assert seq[0] == "depth" and seq[-1] == "n_depth"
        else:
            assert seq[0] == name and firsts.count(name) == (2 if name == "depth" else 1)
    assert set(firsts) == set(C.CONSUMERS) - {"n_depth"}
    assert orders["reversed"][0] == "image_bg" and orders["reversed"][-1] == "image"


def trace_margins(key):
    """The delta rule of tests/trace_bound_cases.py over ALL (pixel, Gaussian) pairs of every view -> (delta_len, delta_act, the
    smallest |act - thr| / thr, the smallest gap of consecutive hit lens / max(1, |len|)).  delta_len = max 2 |d len| / max(1, |len|):
    two lens this far apart cannot swap; delta_act = max |d act| / thr: a pair this far from thr cannot cross it; |d .| the forward
    error bounds of the sweep's evaluation (pair_terms).  Every hit of a pixel is looked at, kept or not: the K-th against the
    (K+1)-th is one of the gaps."""
    x = C.inputs(key)
    thr = C.THR_ACT
    d_len = d_act = outside = 0.0
    act_margin = len_margin = np.inf
    for b in range(key[1]):
        case = C.pair_case(key, b)
        d = x["rays"][b].astype(np.float64).reshape(-1, 3)
        T = TB.pair_terms(case, d[:, None, :], np.arange(N)[None, :])
        hit = np.isfinite(T["len"]) & np.isfinite(T["act"])
        assert hit.all()
        near = T["act"] < 2 * thr
        band = near & (T["act"] > thr / 2)
        d_len = max(d_len, float((2 * T["b_len"][near] / np.maximum(1.0, np.abs(T["len"][near]))).max()))
        if band.any():
            d_act = max(d_act, float((T["b_act"][band] / thr).max()))
        outside = max(outside, float((T["b_act"][~band] / (np.abs(T["act"][~band] - thr) / 2)).max()))
        act_margin = min(act_margin, float((np.abs(T["act"] - thr) / thr).min()))
        ln = np.sort(np.where(T["act"] < thr, T["len"], np.inf), axis=1)
        a, c = ln[:, :-1], ln[:, 1:]
        both = np.isfinite(c)
        gap = (c[both] - a[both]) / np.maximum(1.0, np.maximum(np.abs(a[both]), np.abs(c[both])))
        len_margin = min(len_margin, float(gap.min()))
    assert outside < 1.0
    return max(d_len, 2.0 ** -20), max(d_act, 2.0 ** -20), act_margin, len_margin


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_no_decision_is_near_its_edge(key):
    form, B, K, inverse = key
    x = C.inputs(key)
    ref = C.evaluate(key)
    d_len, d_act, act_margin, len_margin = trace_margins(key)
    log_line(f"[consumer cases] {key_id(key)} seed {C.SEED}: delta_act {d_act:.2e}, |act - thr| / thr >= {act_margin:.2e}; "
             f"delta_len {d_len:.2e}, consecutive hit lens apart by >= {len_margin:.2e} of max(1, |len|)")
    assert act_margin > d_act and len_margin > d_len, "change the seed (consumer_cases.SEED), not the margin"
    # ... so the fp32 oracle returns exactly the fp64 lists, which are the reference's, on every pixel
    mus = np.stack([x["verts"] - x["origin"][b][None].astype(np.float32) for b in range(B)])
    pc = C.pair_case(key, 0)      # (the forms A = 2 S, the same for every view)
    isg = np.stack([pc.A if form != "scalar" else pc.a[:, None, None] * np.eye(3)] * B)
    i64 = oracle.trace_fwd(mus, isg, x["rays"], K, C.THR_ACT)[0].reshape(B, H * W, K)
    i32 = oracle.trace_fwd(mus, isg, x["rays"], K, C.THR_ACT, precision="f32")[0].reshape(B, H * W, K)
    assert (i32 == i64).all(), int((i32 != i64).any(-1).sum())
    assert (i64 == ref["idx"]).all()
    # the scene: nothing hidden is hit; empty, partly filled and (K < N) full lists
    idx, vn, w = ref["idx"], ref["vn"], ref["w"]
    assert ((idx < 0) | (idx % N < N - HIDDEN)).all() and ((idx >= 0) == (np.arange(K)[None, None] < vn[..., None])).all()
    assert (vn == 0).any() and ((vn > 0) & (vn < min(K, N - HIDDEN))).any() and ((vn == K).any() or K > N)
    live = idx >= 0
    wl = np.where(live, w, 0.0)
    s = wl.sum(-1)
    m_sum = float(np.abs(s - 1).min())
    assert (s < 1).any() and (s > 1).any()
    # the rendered normal's |M| wherever a pixel is hit
    table = x["table"].astype(np.float64) if form != "ori" else None
    if table is None:
        from voge_amd.Aggregation import camera_centres, gaussian_normals
        t64 = lambda a: torch.tensor(a, dtype=torch.float64)
        centres = camera_centres(t64(x["R"]), t64(x["T"]))
        table = gaussian_normals(t64(x["sig"]), t64(x["quats"]), t64(x["verts"]), centres).numpy()
        # (the table's own decisions: the thinnest axis and the side that faces the camera, on the Gaussians that are hit)
        sc = np.sort(x["sig"].astype(np.float64), -1)
        seen = np.unique(idx[live] % N)
        assert ((sc[:, 2] - sc[:, 1]) / sc[:, 2])[seen].min() > MARGIN
        delta_v = x["verts"].astype(np.float64)[None] - centres.numpy()[:, None]
        tdot = np.abs((table.reshape(B, N, 3) * delta_v).sum(-1)) / np.linalg.norm(delta_v, axis=-1)
        assert tdot[:, seen].min() > MARGIN
    M = (table[np.maximum(idx, 0)] * wl[..., None]).sum(-2)
    m_M = float(np.linalg.norm(M, axis=-1)[vn > 0].min())
    # the images' clamp at 1, plain and learnable background
    cols = np.tile(x["colors"].astype(np.float64), (B, 1))
    rgb = (cols[np.maximum(idx, 0)] * wl[..., None]).sum(-2)
    m_img = min(float(np.abs(rgb + (1 - np.minimum(s, 1.0))[..., None] * np.asarray(bg, np.float64) - 1).min()) for bg in (C.BG_PLAIN, x["bg"]))
    # the depth's normals: hit or no hit is the only decision in the stencil, and the side that faces the camera
    nd = ref["out"]["n_depth"]
    rays = x["rays"].astype(np.float64)
    has = (nd != 0).any(-1)
    assert (ref["out"]["depth"].reshape(B, -1)[vn > 0] > 1.0).all() and (ref["out"]["depth"].reshape(B, -1)[vn == 0] == 0).all()
    assert has.any() and (has <= (vn.reshape(B, H, W) > 0)).all()
    m_side = float(np.abs((nd * rays).sum(-1))[has].min())
    log_line(f"[consumer cases] {key_id(key)}: |sum w - 1| >= {m_sum:.2e}, |M| >= {m_M:.2e}, |image - 1| before the clamp >= {m_img:.2e}, "
             f"|n_depth . ray| >= {m_side:.2e}; {int(has.sum())} of {has.size} pixels have a depth normal")
    assert min(m_sum, m_M, m_img, m_side) > MARGIN, "change the seed (consumer_cases.SEED), not the margin"


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_a_lost_or_doubled_term_fails(key):
    ref = C.evaluate(key)
    names = C.leaf_names(key[0])
    scale = {k: max(1.0, float(np.abs(ref["grad"][k]).max())) for k in names}
    for k in names:
        assert np.abs(ref["grad"][k]).max() > 0, k
    rows = []
    for term in C.CONSUMERS:
        ratio = {k: float(np.abs(ref["term"][term][k]).max()) / (TOL * scale[k]) for k in names}
        best = max(ratio, key=ratio.get)
        rows.append(f"{term} {ratio[best]:.0f} on {best}")
        assert ratio[best] >= 10, (f"{key_id(key)}: term {term} moves no leaf by 10 TOL of the total's scale: "
                                   + ", ".join(f"{k} {v:.1f}" for k, v in ratio.items()))
    log_line(f"[consumer cases] {key_id(key)}: largest own gradient of each term, in TOL x the total's scale: " + "; ".join(rows))
    # the Gaussians outside every view get exactly nothing, and bg only from image_bg
    assert (ref["grad"]["verts"][N - HIDDEN:] == 0).all()
    assert all((ref["term"][t]["bg"] == 0).all() for t in C.CONSUMERS if t != "image_bg")


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_the_reference_alone_stays_inside_the_tolerance(key):
    """The same composition in fp32 torch on the host against the fp64 one, at TOL / 4.  The hits' act is evaluated as the kernels
    evaluate it (v = mu - len d, act = v^T A v: consumer_cases.hit_forms); torch_ref.trace_dense's own mu^T A mu - (mu^T A d)^2 / dsd
    cancels -- in fp32 its error scales with a |mu|^2, 4e3 here, and no kernel uses it -- and is measured and logged only."""
    ref = C.evaluate(key)
    k64 = C.evaluate(key, torch.float64, None, None, "kernel")
    for name in C.CONSUMERS:      # (in fp64 the two forms are the same numbers, outputs and gradients)
        assert np.abs(k64["out"][name] - ref["out"][name]).max() <= 1e-9 * max(1.0, np.abs(ref["out"][name]).max())
    for k in C.leaf_names(key[0]):
        assert np.abs(k64["grad"][k] - ref["grad"][k]).max() <= 1e-9 * max(1.0, np.abs(ref["grad"][k]).max()), k
    label = f"[consumer cases] {key_id(key)} fp32 on the host"
    for forms in ("dense", "kernel"):
        got = C.evaluate(key, torch.float32, None, None, forms)
        assert (got["idx"] == ref["idx"]).all(), forms
        worst = {}
        for name in C.CONSUMERS:
            a, b = got["out"][name], ref["out"][name]
            worst[name] = float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
        for k in C.leaf_names(key[0]):
            a, b = got["grad"][k], ref["grad"][k]
            worst["d " + k] = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
        log_line(f"{label}, {forms} form, error of scale: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        if forms == "kernel":
            for name in C.CONSUMERS:
                assert close(got["out"][name], ref["out"][name], TOL / 4).all(), (name, worst[name])
            for k in C.leaf_names(key[0]):
                grad_close(f"{label} {k}", got["grad"][k], ref["grad"][k], TOL / 4)
