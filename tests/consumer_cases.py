"""Nine consumers of ONE Fragments in one backward: the cases, the call orders and the fp64 reference that tests/test_gpu_consumers.py
holds the renderer to (numpy and torch on the host, no GPU; tests/test_consumer_cases_cpu.py proves the cases are what that test needs).

Scene: tests/test_gpu_fragment_bwd_entries.py's -- 40 Gaussians, three of them outside every view, a 10 x 7 image (the fused
backward's pixel group is 4 x 3, the stand-alone kernels' tile 8 x 2: partial groups on both edges), one view or two views of a
shared set.  Consumers, each with its own seeded standard-normal upstream gradient g_i; the loss is sum_i <g_i, out_i>:

    image      to_colored_background(frag, colors [N,3], (0.2, 0.3, 0.4))
    sil        get_silhouette(frag)
    depth      get_depth(frag, normalize=True)
    n_depth    get_normals(depth, cameras, edge=None) of THAT depth
    n_hat      get_rendered_normals(frag, table [B*N,3]); form "ori": table = gaussian_normals(scales, quats, verts, centres)
    dist       get_distortion(frag, normalize=False)
    hit        frag.vert_hit_length (g zero on the slots at or past valid_num: the 1e10 sentinels carry no gradient)
    feat       interpolate_attr(frag, features [N,4])
    image_bg   to_colored_background(frag, colors, bg) with bg a [3] leaf that requires grad

The reference is fp64 autograd on the fp32 inputs, composed from oracle/torch_ref.py (trace_dense, aggregation, merge_final,
to_colored_background, through the entries test's reference()), voge_amd/Aggregation.py (distortion, depth_normals, gaussian_normals,
oriented_sigma, camera_centres) and the depth / rendered-normal formulas of voge_amd/Renderer.py's docstrings."""
import functools
import types

import numpy as np
import torch

import oracle
from oracle import camera_np, torch_ref
from test_gpu_fragment_bwd_entries import FOCAL, H, HIDDEN, N, VIEWS, W, reference, scene

CONSUMERS = ("image", "sil", "depth", "n_depth", "n_hat", "dist", "hit", "feat", "image_bg")
BG_PLAIN = (0.2, 0.3, 0.4)
THR_ACT = oracle.thr_act_of(0.01)

# case -> Gaussians' form, views, K, inverse_sigma, route knobs (frame / direct / keep: as tests/test_gpu_fragment_bwd_entries.py)
CASES = {
    "frame": dict(form="scalar", B=1, K=5),
    "frame_shared": dict(form="scalar", B=2, K=5),
    "frame_inverse": dict(form="scalar", B=1, K=5, inverse=True),
    "frame_nodirect": dict(form="scalar", B=1, K=5, direct=False),
    "bundle": dict(form="scalar", B=1, K=5, frame=False),
    "bundle_kept": dict(form="scalar", B=1, K=5, frame=False, keep=True),
    "diag": dict(form="diag", B=2, K=5),
    "full": dict(form="full", B=1, K=5),
    "ori": dict(form="ori", B=1, K=5),
    "K130": dict(form="scalar", B=1, K=130),
}
# the seed of the scene and of the tables: the first one from the entries test's 5 upwards at which, in every case, every decision
# keeps its margin and the fp32 evaluation on the host stays within TOL / 4 (tests/test_consumer_cases_cpu.py: a seed that fails
# is replaced, never the margin -- 5 fails on the rendered normals, whose weighted unit vectors nearly cancel at one pixel)
SEED = 6


def case_key(name):
    c = CASES[name]
    return (c["form"], c["B"], c["K"], bool(c.get("inverse", False)))


# ---- orders ---------------------------------------------------------------------------------------------------------------------------------
def _with_depth_first(seq):
    """n_depth is made from depth's output: where a sequence names it before depth, the two change places."""
    seq = list(seq)
    i, j = seq.index("n_depth"), seq.index("depth")
    if i < j:
        seq[i], seq[j] = seq[j], seq[i]
    return tuple(seq)


def _orders():
    out = {}
    for i, name in enumerate(CONSUMERS):
        out[f"rot{i}_{name}"] = _with_depth_first(CONSUMERS[i:] + CONSUMERS[:i])
    out["reversed"] = _with_depth_first(CONSUMERS[::-1])
    rng = np.random.default_rng(0)
    for j in range(2):
        out[f"perm{j}"] = _with_depth_first([CONSUMERS[i] for i in rng.permutation(len(CONSUMERS))])
    return out


# 12: the nine rotations (rotation i begins with consumer i; n_depth's begins with depth and ends with n_depth), the reversed list and
# two permutations
ORDERS = _orders()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(key):
    """The fp32 arrays a case's Gaussians, tables and cameras are made of, and the upstream gradients g[consumer] [B,H,W,..] (fp64)."""
    form, B, K, inverse = key
    seed = SEED
    verts, sig, quats, cols = scene(form, seed)
    if inverse:      # (the renderer inverts: it is handed 1 / s, so the scene is the same one)
        sig = (1.0 / sig.astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(1000 + seed)
    features = rng.uniform(-1, 1, (N, 4)).astype(np.float32)
    table = rng.normal(size=(B * N, 3))
    table = (table / np.linalg.norm(table, axis=-1, keepdims=True)).astype(np.float32)
    bg = np.array([0.35, 0.15, 0.25], np.float32)
    R, T = camera_np.look_at_view_transform(*VIEWS[B])
    rays, origin = camera_np.pixel_rays(R, T, FOCAL, (W / 2.0, H / 2.0), (H, W))
    shapes = dict(image=(3,), sil=(), depth=(), n_depth=(3,), n_hat=(3,), dist=(), hit=(K,), feat=(4,), image_bg=(3,))
    g = {name: np.random.default_rng(100 + i).normal(size=(B, H, W) + shapes[name]) for i, name in enumerate(CONSUMERS)}
    out = dict(verts=verts, sig=sig, quats=quats, colors=np.ascontiguousarray(cols[:, :3]), features=features, table=table, bg=bg,
               R=R, T=T, rays=rays, origin=origin, g=g)
    for v in list(out.values()) + list(g.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def leaf_names(form):
    return ("verts",) + (("scales", "quats") if form == "ori" else ("sigmas",)) + ("colors", "features") + (() if form == "ori" else ("table",)) + ("bg",)


# ---- the traced and composited fragments, per view ----------------------------------------------------------------------------------------
def hit_forms(m, A, rays, idx):
    """len, act, dsd of the kept hits in the kernels' own, non-cancelling form (tests/trace_bound_cases.py): with v = mu - len d,
        act = v^T A v + len * sum_ij (A_ij - A_ji) d_i mu_j ,
    which IS torch_ref.trace_dense's mu^T A mu - (mu^T A d)^2 / dsd as a function of any A, symmetric or not (expand v; len =
    mu^T A d / dsd), so the gradients of the two are the same too -- the second term is exactly zero on the symmetric forms and
    only carries the reference's convention for d act / d A_ij.  In fp32 trace_dense's form is off by a |mu|^2 2^-24, this one by
    a |mu| |v| 2^-24."""
    live = idx >= 0
    g = idx.clamp(min=0)
    mk, Ak = m[g], A[g]
    Ad = torch.einsum("pkij,pj->pki", Ak, rays)
    dsd = torch.einsum("pki,pi->pk", Ad, rays)
    ln = torch.einsum("pki,pki->pk", mk, Ad) / dsd
    v = mk - ln[..., None] * rays[:, None, :]
    act = torch.einsum("pki,pkij,pkj->pk", v, Ak, v) + ln * torch.einsum("pkij,pi,pkj->pk", Ak - Ak.transpose(-1, -2), rays, mk)
    S = torch_ref.SENT
    return (torch.where(live, ln, torch.full_like(ln, S)), torch.where(live, act, torch.full_like(ln, S)),
            torch.where(live, dsd, torch.zeros_like(dsd)))


def _traced(key, dtype, forms):
    """-> dict(verts, p1, quats: leaves; idx, len, w, vn: per view [H*W, K]).  fp64: the entries test's reference() itself."""
    from voge_amd.Aggregation import oriented_sigma
    form, B, K, inverse = key
    x = inputs(key)
    if dtype == torch.float64 and forms == "dense":
        sig = 1.0 / x["sig"].astype(np.float64) if inverse else x["sig"]
        return reference(form, B, K, x["verts"], sig, x["quats"])
    v = torch.tensor(x["verts"], dtype=dtype, requires_grad=True)
    p1 = torch.tensor(x["sig"], dtype=dtype, requires_grad=True)
    q = None if x["quats"] is None else torch.tensor(x["quats"], dtype=dtype, requires_grad=True)
    eye = torch.eye(3, dtype=dtype)
    s = 1.0 / p1 if inverse else p1
    S = {"scalar": lambda: s[:, None, None] * eye, "diag": lambda: torch.diag_embed(s), "full": lambda: s, "ori": lambda: oriented_sigma(s, q)}[form]()
    out = dict(verts=v, p1=p1, quats=q, idx=[], len=[], w=[], vn=[])
    for b in range(B):
        m = v - torch.tensor(x["origin"][b], dtype=dtype)[None]
        rays = torch.tensor(x["rays"][b], dtype=dtype).reshape(-1, 3)
        idx, ln, act, dsd = torch_ref.trace_dense(m, 2 * S, rays, K, THR_ACT)
        if forms == "kernel":
            ln, act, dsd = hit_forms(m, 2 * S, rays, idx)
        w, vn = torch_ref.aggregation(idx, act, ln, dsd, 1.0)
        for k, t_ in zip(("idx", "len", "w", "vn"), (idx, ln, w, vn)):
            out[k].append(t_)
    return out


def compose(tr, lv, key, dtype, views, rows):
    """Every consumer's output [len(views), r1 - r0, W, ..] from the per-view fragments tr and the leaves lv."""
    from voge_amd.Aggregation import depth_normals, distortion
    form, B, K, _ = key
    x = inputs(key)
    r0, r1 = rows
    one = torch.ones((), dtype=dtype)
    colsB, featB = torch.cat([lv["colors"]] * B), torch.cat([lv["features"]] * B)
    per = {k: [] for k in CONSUMERS if k != "n_depth"}
    for b in views:
        px = slice(r0 * W, r1 * W)
        idx, ln, w, vn = (tr[k][b][px] for k in ("idx", "len", "w", "vn"))
        idx = torch.where(idx >= 0, idx + b * N, idx)      # (row b * N + i of a table is what view b's fragments index)
        rgb = torch_ref.merge_final(colsB, w, vn, idx)
        per["image"].append(torch_ref.to_colored_background(rgb, w, torch.tensor(BG_PLAIN, dtype=dtype)))
        per["sil"].append(torch.minimum(w.sum(-1), one))
        # get_depth: A = sum w len, S = sum w over the live slots; A / S where S > 0, else the background (0)
        live = torch.arange(K)[None] < vn[:, None]
        wl = w * live
        A, S = (wl * torch.where(live, ln, torch.zeros_like(ln))).sum(-1), wl.sum(-1)
        per["depth"].append(torch.where(S > 0, A / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S)))
        # get_rendered_normals: M = sum_k w_k n_k; M / |M| where |M| > 0, else (0, 0, 0)
        M = torch_ref.merge_final(lv["table"], w, vn, idx)
        n2 = (M * M).sum(-1, keepdim=True)
        ok = n2 > 0
        per["n_hat"].append(torch.where(ok, M / torch.sqrt(torch.where(ok, n2, torch.ones_like(n2))), torch.zeros_like(M)))
        per["dist"].append(distortion(w, ln, vn, False))
        per["hit"].append(ln)
        per["feat"].append(torch_ref.merge_final(featB, w, vn, idx))
        per["image_bg"].append(torch_ref.to_colored_background(rgb, w, lv["bg"]))
    out = {k: torch.stack(v).reshape((len(views), r1 - r0, W) + tuple(v[0].shape[1:])) for k, v in per.items()}
    rays = torch.tensor(x["rays"][list(views), r0:r1], dtype=dtype)
    out["n_depth"] = depth_normals(out["depth"], rays, None)
    return out


@functools.lru_cache(maxsize=None)
def evaluate(key, dtype=torch.float64, views=None, rows=None, forms="dense"):
    """The composition in `dtype` on the host, on `views` (default: all) and the pixel rows `rows` (default: all) -> dict(
    out {consumer: [V,h,W,..]}, grad {leaf: total gradient}, term {consumer: {leaf: its own gradient}}, idx [B,H*W,K] (global rows,
    -1 empty), vn [B,H*W], w [B,H*W,K]), numpy fp64."""
    from voge_amd.Aggregation import camera_centres, gaussian_normals
    form, B, K, inverse = key
    x = inputs(key)
    views = tuple(range(B)) if views is None else tuple(views)
    rows = (0, H) if rows is None else tuple(rows)
    tr = _traced(key, dtype, forms)
    lv = {k: torch.tensor(x[k], dtype=dtype, requires_grad=True) for k in ("colors", "features", "bg")}
    if form == "ori":
        centres = camera_centres(torch.tensor(x["R"], dtype=dtype), torch.tensor(x["T"], dtype=dtype))
        lv["table"] = gaussian_normals(tr["p1"], tr["quats"], tr["verts"], centres)
    else:
        lv["table"] = torch.tensor(x["table"], dtype=dtype, requires_grad=True)
    out = compose(tr, lv, key, dtype, views, rows)
    names = leaf_names(form)
    leaves = [dict(verts=tr["verts"], sigmas=tr["p1"], scales=tr["p1"], quats=tr["quats"], **lv)[k] for k in names]
    term = {}
    for name in CONSUMERS:
        g = torch.tensor(x["g"][name][list(views), rows[0]:rows[1]], dtype=dtype)
        if name == "hit":      # (the sentinels carry no gradient)
            vn = torch.stack([tr["vn"][b] for b in views]).reshape(len(views), H, W)[:, rows[0]:rows[1]]
            g = g * (torch.arange(K)[None, None, None] < vn[..., None])
        gr = torch.autograd.grad((out[name] * g).sum(), leaves, retain_graph=True, allow_unused=True)
        term[name] = {k: (np.zeros(tuple(l.shape)) if t_ is None else t_.detach().numpy().astype(np.float64)) for k, l, t_ in zip(names, leaves, gr)}
    if inverse and dtype == torch.float64 and forms == "dense":
        # reference() was handed s = 1 / sigma in fp64: its leaf is s, the renderer's is sigma -- ds / dsigma = -1 / sigma^2
        f = -1.0 / x["sig"].astype(np.float64) ** 2
        for name in CONSUMERS:
            term[name]["sigmas"] = term[name]["sigmas"] * f
    grad = {k: sum(term[name][k] for name in CONSUMERS) for k in names}
    idx = np.stack([np.where(tr["idx"][b].numpy() >= 0, tr["idx"][b].numpy() + b * N, -1) for b in range(B)])
    res = dict(out={k: out[k].detach().numpy().astype(np.float64) for k in CONSUMERS}, grad=grad, term=term, idx=idx,
               vn=np.stack([tr["vn"][b].numpy() for b in range(B)]), w=np.stack([tr["w"][b].detach().numpy().astype(np.float64) for b in range(B)]),
               len=np.stack([tr["len"][b].detach().numpy().astype(np.float64) for b in range(B)]))
    return res


def reference_of(name, views=None, rows=None):
    """The fp64 reference of a case (computed once per (form, B, K, inverse) and selection, shared and left unchanged)."""
    return evaluate(case_key(name), torch.float64, None if views is None else tuple(views), None if rows is None else tuple(rows))


def upstream(key, name, vn=None):
    """g of a consumer [B,H,W,..]; `hit`: zero on the slots at or past vn [B,H,W]."""
    g = inputs(key)["g"][name]
    if name == "hit":
        g = g * (np.arange(key[2])[None, None, None] < np.asarray(vn).reshape(g.shape[:3])[..., None])
    return g


# ---- margins --------------------------------------------------------------------------------------------------------------------------------
def pair_case(key, b):
    """View b's (centres, forms) as tests/trace_bound_cases.pair_terms takes them, in fp64 of the fp32 inputs."""
    from voge_amd.Aggregation import oriented_sigma
    form, B, K, inverse = key
    x = inputs(key)
    mus = x["verts"].astype(np.float64) - x["origin"][b][None]
    s = x["sig"].astype(np.float64)
    s = 1.0 / s if inverse else s
    if form == "scalar":
        return types.SimpleNamespace(mus=mus, a=2 * s, A=None)
    if form == "diag":
        S = s[:, :, None] * np.eye(3)[None]
    elif form == "full":
        S = s
    else:
        S = oriented_sigma(torch.tensor(s), torch.tensor(x["quats"], dtype=torch.float64)).numpy()
    return types.SimpleNamespace(mus=mus, a=None, A=2 * S)
