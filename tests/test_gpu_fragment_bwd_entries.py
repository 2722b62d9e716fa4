"""The fused backward's eleven C entries at the smallest shapes at which their shared host launcher can go wrong, each reached
through the public route that selects it and compared with fp64 autograd through oracle/torch_ref.py.

Shapes: 40 Gaussians (three of them out of every view), a 10 x 7 image (the kernel's pixel group is 4 x 3: partial groups on both
edges), one view and two views of a shared set (the finishing pass's sum over the views), K = 5 and, for the weights' own gradient,
K = 130 (four slots on a lane), 3 and 4 channels -- and 1 where a public route lets it through --, an attribute table with fewer
and with more rows than B * N, with and without kept act / dsd, per-axis and full 3x3 records, an accumulator that arrives zeroed
and one that is zeroed by the entry.  Every case states which entry it must reach and with which of those arguments; a spy on the
loaded library checks that it did.  The tolerances are those of the nearest existing test of each route: TOL of scale
(tests/test_gpu_composite_routes.py, tests/test_gpu_oriented.py), a quarter of it for get_depth's one-pass form.

The empty cases (no pixels, no Gaussians) cannot be reached through the renderer on the frame path -- it does not take that path
for an empty set or an empty band -- so those call the entries directly and check which outputs are zero-filled and which are left
alone.  The 64-bit-offset instantiations need nrows * W * K >= 2^30 (or, with K <= 3, more
pixels than the rays' or the rgb's 32-bit byte offsets reach): tests/test_gpu_large_shapes.py runs them."""
import numpy as np
import pytest
import torch

import oracle
from oracle import camera_np, torch_ref
from test_fragment_bwd_args_cpu import ARGS, base
from util import TOL, grad_close, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N, HIDDEN, FOCAL = 7, 10, 40, 3, 30.0
VIEWS = {1: ([4.0], [10.0], [70.0]), 2: ([4.0, 3.7], [10.0, -20.0], [70.0, 200.0])}


def t(a, dtype=torch.float32, rg=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def n(x):
    return x.detach().cpu().numpy()


def scene(form, seed=5):
    """40 Gaussians in a cube of side 0.9 around the origin, the last HIDDEN of them far above every camera's field of view (an
    attribute table may then stop short of them); sigmas as scalars, per axis, full L L^T, or scales + quaternions."""
    rng = np.random.default_rng(seed)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.45).astype(np.float32)
    verts[N - HIDDEN:, 1] += 40.0
    r = rng.uniform(0.07, 0.11, N)
    s = (1.0 / (r * r / (2 * np.log(1 / 0.6)))).astype(np.float32)
    quats = None
    if form == "scalar":
        sig = s
    elif form in ("diag", "ori"):
        sig = (s[:, None] * rng.uniform(0.6, 1.6, (N, 3))).astype(np.float32)
        if form == "ori":
            quats = (rng.normal(size=(N, 4)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    else:
        L = np.tril(rng.uniform(-1, 1, (N, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
        L = L * np.sqrt(s)[:, None, None] * 0.8
        sig = (L @ L.transpose(0, 2, 1)).astype(np.float32)
    cols = np.random.default_rng(seed + 1).uniform(0, 1, (N, 4)).astype(np.float32)
    return verts, sig, quats, cols


def reference(form, B, K, verts, sig, quats):
    """fp64 torch_ref on the CPU: leaves (verts, sigmas | scales, quats | None) and per view the trace and the weights."""
    from voge_amd.Aggregation import oriented_sigma
    R, T = camera_np.look_at_view_transform(*VIEWS[B])
    rays, origin = camera_np.pixel_rays(R, T, FOCAL, (W / 2.0, H / 2.0), (H, W))
    v = torch.tensor(verts, dtype=torch.float64, requires_grad=True)
    p1 = torch.tensor(sig, dtype=torch.float64, requires_grad=True)
    q = None if quats is None else torch.tensor(quats, dtype=torch.float64, requires_grad=True)
    eye = torch.eye(3, dtype=torch.float64)
    S = {"scalar": lambda: p1[:, None, None] * eye, "diag": lambda: torch.diag_embed(p1), "full": lambda: p1,
         "ori": lambda: oriented_sigma(p1, q)}[form]()
    out = dict(verts=v, p1=p1, quats=q, R=R, T=T, idx=[], len=[], w=[], vn=[])
    for b in range(B):
        idx, ln, act, dsd = torch_ref.trace_dense(v - torch.tensor(origin[b])[None], 2 * S, torch.tensor(rays[b], dtype=torch.float64).reshape(-1, 3),
                                                  K, oracle.thr_act_of(0.01))
        w, vn = torch_ref.aggregation(idx, act, ln, dsd, 1.0)
        for k, x in zip(("idx", "len", "w", "vn"), (idx, ln, w, vn)):
            out[k].append(x)
    return out


def spy_on(monkeypatch, cut_rows=0):
    """[(entry, {argument name: value})] of every call of a fused-backward entry from here on.  cut_rows: the attribute table the
    entries are told of is that many rows shorter than the one the caller handed in (below)."""
    from voge_amd import _lib
    lib = _lib.load()
    calls = []
    for name, spec in ARGS.items():
        def wrap(*a, _real=getattr(lib, name), _name=name, _names=spec.split()):
            if cut_rows and "Nattr" in _names:
                a = tuple(v - cut_rows if k == "Nattr" else v for k, v in zip(_names, a))
            calls.append((_name, dict(zip(_names, a))))
            return _real(*a)
        monkeypatch.setattr(lib, name, wrap, raising=True)
    return calls


# (entry, Gaussians' form, consumer, B, K, C, attribute rows: "=" B * N | "<" | ">", route knobs, arguments the entry must see)
#   knobs: frame = the camera-input frame path; direct = its forward zeroes the backward's accumulator; keep = the fragments keep
#   act / dsd (scalar sigmas: VOGE_FRAGMENTS_KEEP_ACT_DSD=1, the eager fragments; general forms: VOGE_GENERAL_KEEP_ACT_DSD, on by default)
def _c(entry, gauss, consumer, B, K=5, C=3, rows="=", frame=True, direct=True, keep=None, **see):
    return (entry, gauss, consumer, B, K, C, rows, frame, direct, keep, see)


CASES = [
    # the frame path's record forms: the accumulator arrives zeroed, no act / dsd
    _c("voge_frame_shade_bwd_iso", "scalar", "white", 1, C=3, rows=">"),
    _c("voge_frame_shade_bwd_iso", "scalar", "white", 2, C=4, rows="<"),
    _c("voge_frame_merge_bwd_iso", "scalar", "attr_sil", 1, C=4, rows="<", g_wsum=True),
    _c("voge_frame_merge_bwd_iso", "scalar", "attr_sil", 2, C=3, rows=">", g_wsum=True),
    _c("voge_frame_merge_bwd_iso", "scalar", "attr", 2, C=3, g_wsum=False),
    _c("voge_frame_depth_bwd_iso", "scalar", "depth_norm", 1, normalize=1, g=True, g_sil=False),
    _c("voge_frame_depth_bwd_iso", "scalar", "depth_raw", 2, normalize=0, g=True, g_sil=False),
    _c("voge_frame_depth_bwd_iso", "scalar", "depth_sil_only", 2, g=False, g_sil=True),
    _c("voge_frame_depth_bwd_iso", "scalar", "depth_and_sil", 1, normalize=1, g=True, g_sil=True),
    # the record forms on a workspace that the entry zeroes: the ray-bundle chain, and the frame path without its zeroed accumulator
    _c("voge_fragment_shade_bwd_iso", "scalar", "white", 1, C=4, rows=">", frame=False, act=False),
    _c("voge_fragment_shade_bwd_iso", "scalar", "white", 2, C=3, rows="<", direct=False, act=False),
    _c("voge_fragment_shade_bwd_iso", "scalar", "white", 1, C=1, frame=False, keep=True, act=True),
    _c("voge_fragment_shade_bwd_iso", "scalar", "white", 2, C=3, frame=False, keep=True, act=True),
    _c("voge_fragment_merge_bwd_iso", "scalar", "attr_sil", 1, C=3, rows="<", frame=False, act=False, g_wsum=True),
    _c("voge_fragment_merge_bwd_iso", "scalar", "attr", 2, C=4, rows=">", direct=False, act=False, g_wsum=False),
    _c("voge_fragment_bwd_iso", "scalar", "weight", 2, K=5, act=False),
    _c("voge_fragment_bwd_iso", "scalar", "weight", 1, K=130, frame=False, act=False),
    _c("voge_fragment_bwd_iso", "scalar", "weight", 1, K=5, frame=False, keep=True, act=True),
    _c("voge_fragment_bwd_iso", "scalar", "weight", 2, K=130, frame=False, keep=True, act=True),
    # the general 3x3 forms: records packed by the entry
    _c("voge_fragment_shade_bwd", "full", "white", 1, C=3, rows=">", frame=False, act=True),
    _c("voge_fragment_shade_bwd", "full", "white", 2, C=4, rows="<", frame=False, keep=False, act=False),
    _c("voge_fragment_merge_bwd", "full", "attr_sil", 2, C=4, rows=">", frame=False, act=True, g_wsum=True),
    _c("voge_fragment_merge_bwd", "full", "attr", 1, C=3, rows="<", frame=False, keep=False, act=False, g_wsum=False),
    _c("voge_fragment_bwd", "full", "weight", 2, K=5, frame=False, act=True),
    _c("voge_fragment_bwd", "full", "weight", 1, K=130, frame=False, keep=False, act=False),
    _c("voge_fragment_bwd", "full", "weight", 1, K=130, frame=False, act=True),
    # the general forms on the frame path: per-axis (kind 1, never act / dsd) and full 3x3 (kind 2) records
    _c("voge_frame_bwd_gen", "diag", "white", 1, C=3, rows=">", form=0, kind=1, act=False, acc_is_zero=1),
    _c("voge_frame_bwd_gen", "diag", "attr_sil", 2, C=4, rows="<", direct=False, form=1, kind=1, act=False, acc_is_zero=0),
    _c("voge_frame_bwd_gen", "diag", "weight", 1, K=5, form=2, kind=1, act=False),
    _c("voge_frame_bwd_gen", "diag", "weight", 2, K=130, form=2, kind=1, act=False),
    _c("voge_frame_bwd_gen", "full", "white", 2, C=4, rows="<", form=0, kind=2, act=True, acc_is_zero=1),
    _c("voge_frame_bwd_gen", "full", "white", 1, C=3, direct=False, keep=False, form=0, kind=2, act=False, acc_is_zero=0),
    _c("voge_frame_bwd_gen", "full", "attr", 1, C=3, rows=">", form=1, kind=2, act=True, acc_is_zero=1),
    _c("voge_frame_bwd_gen", "full", "attr_sil", 2, C=3, keep=False, form=1, kind=2, act=False, acc_is_zero=1),
    _c("voge_frame_bwd_gen", "full", "weight", 2, K=5, form=2, kind=2, act=True),
    _c("voge_frame_bwd_gen", "full", "weight", 1, K=130, keep=False, form=2, kind=2, act=False),
    # the oriented form
    _c("voge_frame_bwd_ori", "ori", "white", 1, C=3, rows="<", form=0, act=True, acc_is_zero=1),
    _c("voge_frame_bwd_ori", "ori", "attr_sil", 2, C=4, rows=">", direct=False, keep=False, form=1, act=False, acc_is_zero=0),
    _c("voge_frame_bwd_ori", "ori", "weight", 2, K=5, form=2, act=True),
    _c("voge_frame_bwd_ori", "ori", "weight", 1, K=130, keep=False, form=2, act=False),
]


def case_id(c):
    entry, form, consumer, B, K, C, rows, frame, direct, keep, _ = c
    return (f"{entry[5:]}-{form}-{consumer}-B{B}-K{K}-C{C}-rows{rows}" + ("" if frame else "-bundle") + ("" if direct else "-fill")
            + ("" if keep is None else "-keep" if keep else "-nokeep"))


def consume(consumer, frag, colsB, C):
    """-> the consumer's outputs on the GPU, in the order of reference_outputs."""
    from voge_amd.Renderer import get_depth, get_silhouette, interpolate_attr, to_colored_background
    if consumer == "white":
        return [to_colored_background(frag, colsB, background_color=(1.0,) * C)]
    if consumer == "attr":
        return [interpolate_attr(frag, colsB)]
    if consumer == "attr_sil":
        return [interpolate_attr(frag, colsB), get_silhouette(frag)]
    if consumer == "weight":
        return [frag.vert_weight]
    depth = get_depth(frag, normalize=consumer != "depth_raw", background=0.0)
    if consumer == "depth_sil_only":
        return [get_silhouette(frag)]
    return [depth, get_silhouette(frag)] if consumer == "depth_and_sil" else [depth]


def reference_outputs(consumer, ref, b, colors):
    idx, ln, w, vn = (ref[k][b] for k in ("idx", "len", "w", "vn"))
    K = idx.shape[-1]
    sil = torch.minimum(w.sum(-1), torch.ones((), dtype=w.dtype))
    if consumer == "weight":
        return [w]
    if consumer == "white":
        rgb = torch_ref.merge_final(colors, w, vn, idx)
        return [torch_ref.to_colored_background(rgb, w, torch.ones(colors.shape[1], dtype=w.dtype))]
    if consumer in ("attr", "attr_sil"):
        return [torch_ref.merge_final(colors, w, vn, idx)] + ([sil] if consumer == "attr_sil" else [])
    # get_depth (Renderer.get_depth's definition): A = sum w len, S = sum w over the live slots; A / S where S > 0, else the background
    live = torch.arange(K)[None] < vn[:, None]
    wl = w * live
    A, S = (wl * torch.where(live, ln, torch.zeros_like(ln))).sum(-1), wl.sum(-1)
    depth = A if consumer == "depth_raw" else torch.where(S > 0, A / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S))
    return {"depth_sil_only": [sil], "depth_and_sil": [depth, sil]}.get(consumer, [depth])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_entry_through_its_public_route_vs_fp64_autograd(hip_lib, monkeypatch, c):
    import test_gpu_depth as dpt
    from voge_amd import ops
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes
    entry, form, consumer, B, K, C, rows, frame, direct, keep, see = c
    label = case_id(c)
    verts, sig, quats, cols = scene(form)
    ref = reference(form, B, K, verts, sig, quats)
    monkeypatch.setattr(ops, "FRAME_PATH", frame)
    monkeypatch.setattr(ops, "FRAME_DIRECT_BWD", direct)
    if keep is not None:
        monkeypatch.setenv("VOGE_FRAGMENTS_KEEP_ACT_DSD" if form == "scalar" else "VOGE_GENERAL_KEEP_ACT_DSD", "1" if keep else "0")
    # (rows "<": ops refuses a table with fewer rows than B * N before it looks at the indices, so the public call hands in B * N
    #  rows, the last HIDDEN of them constants that no fragment indexes, and the entry is told of the rows before those)
    calls = spy_on(monkeypatch, cut_rows=HIDDEN if rows == "<" else 0)
    gm = (OrientedGaussianMeshes(t(verts), t(sig), t(quats)) if form == "ori" else GaussianMeshes(t(verts), t(sig))).to(DEV)
    frag = dpt.renderer_for(H, W, K, FOCAL)(gm, R=t(ref["R"]), T=t(ref["T"]))
    colors = t(cols[:, :C], rg=True)
    # the attribute table: one copy of the colours per view (row b * N + i is what view b's fragments index); "<" ends at the
    # last view's hidden Gaussians, ">" has seven rows more that nothing indexes
    parts = [colors] * B
    if rows == "<":
        parts[-1] = torch.cat([colors[:N - HIDDEN], torch.full((HIDDEN, C), 0.5, device=DEV)])
    if rows == ">":
        parts.append(torch.full((7, C), 0.5, device=DEV))
    colsB = torch.cat(parts)
    got = consume(consumer, frag, colsB, C)
    assert not calls, (label, "a backward entry ran in the forward")
    # the pixels whose index lists are the reference's (the selection is discrete: a flipped pixel is left out of the loss)
    idx = n(frag.vert_index).reshape(B, H * W, K)
    assert ((idx < 0) | (idx % N < N - HIDDEN)).all(), (label, "a hidden Gaussian was hit")
    ridx = np.stack([np.where(n(ref["idx"][b]) >= 0, n(ref["idx"][b]) + b * N, -1) for b in range(B)])
    same = (idx == np.where(ridx < 0, 0, ridx)).all(-1) | (idx == ridx).all(-1)
    assert same.mean() >= 0.9, f"{label}: only {same.mean():.3f} of the pixels have the reference's index list"
    vn = np.stack([n(ref["vn"][b]) for b in range(B)])
    assert (vn[same] == K).any() or K > N, (label, "no full list")
    assert (vn == 0).any() and ((vn > 0) & (vn < min(K, N - HIDDEN))).any(), (label, "no empty or no partly filled pixel")
    rng = np.random.default_rng(17)
    colors64 = torch.tensor(cols[:, :C], dtype=torch.float64, requires_grad=True)
    loss_gpu, loss_ref = 0.0, 0.0
    for j, out in enumerate(got):
        shape = (B, H * W) + tuple(out.shape[3:])
        G = rng.normal(size=shape) * same.reshape((B, H * W) + (1,) * (len(shape) - 2))
        loss_gpu = loss_gpu + (out.reshape(shape) * t(G)).sum()
        for b in range(B):
            r = reference_outputs(consumer, ref, b, colors64)[j]
            err = np.abs(n(out.reshape(shape)[b]) - n(r))[same[b]].max(initial=0.0)
            assert err <= TOL * max(1.0, float(r.detach().abs().max())), (label, "forward", j, err)
            loss_ref = loss_ref + (r * torch.tensor(G[b])).sum()
    loss_gpu.backward()
    torch.cuda.synchronize()
    loss_ref.backward()
    # the route: one call of the entry this case is about (and none of another entry), with the arguments it is about
    assert [name for name, _ in calls] == [entry], (label, [name for name, _ in calls])
    a = calls[0][1]
    P = B * N
    assert a["K"] == K and a["W"] == W and a["nrows"] == B * H and a.get("P", a.get("B", 0) * a.get("N", 0)) == P, (label, a)
    if "Nattr" in a and consumer != "weight":
        assert a["C"] == C and {"=": a["Nattr"] == P, "<": a["Nattr"] < P, ">": a["Nattr"] > P}[rows], (label, a["C"], a["Nattr"])
    if "shared" in a:
        assert a["shared"] == 1
    for k, v in see.items():
        assert (a[k] is not None) == v if isinstance(v, bool) else a[k] == v, (label, k, a[k], v)
    tol = 0.25 * TOL if entry == "voge_frame_depth_bwd_iso" else TOL
    pairs = [("verts", gm.verts.grad, ref["verts"].grad), ("scales" if form == "ori" else "sigmas", (gm.scales if form == "ori" else gm.sigmas).grad,
                                                            ref["p1"].grad)]
    if form == "ori":
        pairs.append(("quats", gm.quats.grad, ref["quats"].grad))
    if consumer in ("white", "attr", "attr_sil"):
        pairs.append(("colors", colors.grad, colors64.grad))
    for name, g, want in pairs:
        assert g is not None and want is not None and float(want.abs().max()) > 0, (label, name)
        grad_close(f"[fragment_bwd entries] {label} {name}", n(g), n(want), tol)
    assert np.abs(n(gm.verts.grad)[N - HIDDEN:]).max() == 0.0, (label, "a Gaussian that no pixel sees got a gradient")


# ---- the empty cases, called directly: which outputs the launcher zero-fills, and which it leaves alone ---------------------------
ATTR_ONLY = ("voge_fragment_shade_bwd_iso", "voge_fragment_merge_bwd_iso", "voge_frame_shade_bwd_iso", "voge_frame_merge_bwd_iso",
             "voge_fragment_shade_bwd", "voge_fragment_merge_bwd")      # zero g_attr, leave the Gaussians' gradients unwritten
OWN = ("voge_fragment_bwd_iso", "voge_fragment_bwd", "voge_frame_depth_bwd_iso")      # insist on both outputs and zero them


def zero_filled(entry, B, Ng, nrows, form=0):
    """{output: floats that must be zero} of an empty call on a shared set of Ng Gaussians (the general forms: P = B * Ng of their own)."""
    P, C, Nattr = B * Ng, 3, 11
    if entry in ATTR_ONLY:
        return {"g_attr": Nattr * C}
    if entry == "voge_fragment_bwd":
        return {} if P == 0 else {"g_verts": 3 * P, "g_sigmas": 9 * P}
    if entry in OWN:
        return {"g_verts": 3 * Ng, "g_sigmas": Ng}
    out = {"g_verts": 3 * Ng, "g_sigmas": (3 if entry == "voge_frame_bwd_ori" else 9) * Ng}
    if entry == "voge_frame_bwd_ori":
        out["g_quats"] = 4 * Ng
    if form != 2:
        out["g_attr"] = Nattr * C
    return out


@pytest.mark.parametrize("what", ["no pixels", "no Gaussians"])
@pytest.mark.parametrize("entry", list(ARGS))
def test_empty_calls_zero_fill_what_they_always_did(hip_lib, entry, what):
    B, Ng, nrows = (2, 5, 0) if what == "no pixels" else (0, 5, 14)
    dummy = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    for form in ((0, 2) if "form" in ARGS[entry].split() else (0,)):
        call = base(entry)
        outs = {k: torch.full((256,), 7.0, device=DEV) for k in ("g_verts", "g_sigmas", "g_quats", "g_attr") if k in call}
        for k, v in call.items():
            if v == 4096 and k != "ws_bytes":      # (base()'s placeholder pointer)
                call[k] = outs[k].data_ptr() if k in outs else dummy.data_ptr()
        sizes = dict(nrows=nrows, W=10, K=5, C=3, Nattr=11, ws_bytes=dummy.numel() * 4, acc_is_zero=0, B=B, N=Ng, P=B * Ng, shared=1,
                     shared_verts=1, shared_sigmas=1, form=form, kind=2)
        call.update({k: v for k, v in sizes.items() if k in call})
        rc = getattr(hip_lib, entry)(*call.values())
        torch.cuda.synchronize()
        assert rc == 0, (entry, what, form, rc)
        want = zero_filled(entry, B, Ng, nrows, form)
        for k, buf in outs.items():
            m = want.get(k, 0)
            assert torch.equal(buf[:m], torch.zeros(m, device=DEV)) and torch.equal(buf[m:], torch.full((256 - m,), 7.0, device=DEV)), \
                (entry, what, form, k, m, buf[:m + 2].tolist())
        assert float(dummy.abs().max()) == 0.0
    log_line(f"[fragment_bwd entries] {entry} {what}: zero-filled {zero_filled(entry, B, Ng, nrows)}")
