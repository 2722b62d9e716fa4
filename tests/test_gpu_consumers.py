"""Every consumer of one Fragments together, in any order, against fp64 autograd (tests/consumer_cases.py; what it relies on is
proven on the host by tests/test_consumer_cases_cpu.py).

One render, nine consumers -- image, silhouette, depth, normals from depth, rendered normals, distortion, hit length, a second
attribute table, an image on a learnable background -- called in twelve orders, so that each of them is the first reader of the
deferred composite once, then ONE backward of the sum of <g_i, out_i>.  The first reader decides which node makes the weights
(_CompositeShade / _CompositeMerge / _CompositeDepth / _CompositeLean); every later reader takes another route (_ShadeThrough, _Merge,
_Depth, _Distortion, _Silhouette, the cached weight sum or the silhouette the first node wrote), and in the backward the image or
merge gradient, the weights' own gradient and the silhouette's meet inside that node.  A contribution that is dropped or doubled
there, a stale weight sum or silhouette, or an accumulator used twice moves some leaf's gradient by at least 10 TOL of its scale
(proven per term on the host); everything here is held to TOL, over every element, with no pixel left out."""
import time
import types

import numpy as np
import pytest
import torch

import consumer_cases as C
from consumer_cases import FOCAL, H, HIDDEN, N, W
from test_gpu_fragment_bwd_entries import DEV, n, spy_on, t
from util import TOL, close, grad_close, log_line

pytestmark = pytest.mark.gpu
NODES = ("_CompositeShadeBackward", "_CompositeMergeBackward", "_CompositeDepthBackward", "_CompositeLeanBackward")
T0 = [None]      # (wall time of the file: from its first test to the end of each, logged)


def render(name, monkeypatch, rows=None):
    """A case's Gaussians, tables and renderer on the device, its route knobs set, and the Fragments of one render."""
    import test_gpu_depth as dpt
    from voge_amd import ops
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes
    from voge_amd.Renderer import gaussian_normals
    if T0[0] is None:
        T0[0] = time.perf_counter()
    c, key = C.CASES[name], C.case_key(name)
    form, B, K, inverse = key
    x = C.inputs(key)
    monkeypatch.setattr(ops, "FRAME_PATH", c.get("frame", True))
    monkeypatch.setattr(ops, "FRAME_DIRECT_BWD", c.get("direct", True))
    if c.get("keep") is not None:
        monkeypatch.setenv("VOGE_FRAGMENTS_KEEP_ACT_DSD", "1" if c["keep"] else "0")
    gm = (OrientedGaussianMeshes(t(x["verts"]), t(x["sig"]), t(x["quats"])) if form == "ori" else GaussianMeshes(t(x["verts"]), t(x["sig"]))).to(DEV)
    renderer = dpt.renderer_for(H, W, K, FOCAL, inverse=inverse)
    frag = renderer(gm, R=t(x["R"]), T=t(x["T"]), **({} if rows is None else dict(rows=rows)))
    st = types.SimpleNamespace(name=name, key=key, gm=gm, frag=frag, cameras=renderer.cameras, rows=rows,
                               colors=t(x["colors"], rg=True), features=t(x["features"], rg=True), bg=t(x["bg"], rg=True))
    # the tables the fragments index: row b * N + i is what view b's fragments read
    st.colsB, st.featB = torch.cat([st.colors] * B), torch.cat([st.features] * B)
    st.leaves = dict(verts=gm.verts, colors=st.colors, features=st.features, bg=st.bg)
    if form == "ori":
        st.leaves.update(scales=gm.scales, quats=gm.quats)
        st.table = gaussian_normals(gm.scales, gm.quats, gm.verts, t(x["origin"]))
    else:
        st.table = st.leaves["table"] = t(x["table"], rg=True)
        st.leaves["sigmas"] = gm.sigmas
    return st


def consume(st, order, frag=None, cameras=None):
    """The nine forward calls in the order given -> {consumer: output}."""
    from voge_amd.Renderer import (get_depth, get_distortion, get_normals, get_rendered_normals, get_silhouette, interpolate_attr,
                                   to_colored_background)
    frag = st.frag if frag is None else frag
    outs = {}
    for name in order:
        if name == "image":
            outs[name] = to_colored_background(frag, st.colsB, C.BG_PLAIN)
        elif name == "sil":
            outs[name] = get_silhouette(frag)
        elif name == "depth":
            outs[name] = get_depth(frag, normalize=True)
        elif name == "n_depth":
            outs[name] = get_normals(outs["depth"], st.cameras if cameras is None else cameras, rows=st.rows, edge=None)
        elif name == "n_hat":
            outs[name] = get_rendered_normals(frag, st.table)
        elif name == "dist":
            outs[name] = get_distortion(frag, normalize=False)
        elif name == "hit":
            outs[name] = frag.vert_hit_length
        elif name == "feat":
            outs[name] = interpolate_attr(frag, st.featB)
        else:
            outs[name] = to_colored_background(frag, st.colsB, st.bg)
    st.weight_node = type(frag._vert_weight.grad_fn).__name__
    return outs


def check_forward(label, frag, outs, ref, views):
    """Lists and outputs against the fp64 reference's, every pixel and element -> the largest output error of scale per consumer."""
    form, B, K, _ = ref["key"]
    r0, r1 = ref["rows"]
    want = ref["idx"][list(views)].reshape(len(views), H, W, K)[:, r0:r1]
    idx = n(frag.vert_index).reshape(want.shape)
    # (empty slots are -1, or 0 once a merge has rewritten the pixel's list: tests/test_gpu_distortion.py's same_lists)
    same = (idx == want).all(-1) | (idx == np.where(want < 0, 0, want)).all(-1)
    assert same.all(), f"{label}: {int((~same).sum())} of {same.size} pixels have another index list than the reference"
    errs = {}
    for name in C.CONSUMERS:
        got, exp = n(outs[name]).astype(np.float64).reshape(ref["out"][name].shape), ref["out"][name]
        errs[name] = float((np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max())
        print(f"{label} {name}: output error {errs[name]:.2e} of scale")
        assert close(got, exp, TOL).all(), f"{label}: {name} off by {errs[name]:.2e} of scale (TOL {TOL:.0e})"
    return errs


def total_loss(outs, ref, views):
    form, B, K, _ = ref["key"]
    r0, r1 = ref["rows"]
    vn = ref["vn"].reshape(B, H, W)
    loss = 0.0
    for name in C.CONSUMERS:
        g = C.upstream(ref["key"], name, vn)[list(views), r0:r1]
        loss = loss + (outs[name].reshape(g.shape) * t(g)).sum()
    return loss


def check_gradients(label, st, ref, times=1):
    """Every leaf's gradient against `times` x the fp64 total -> the error of scale per leaf."""
    errs = {}
    for k in C.leaf_names(st.key[0]):
        g = st.leaves[k].grad
        assert g is not None, (label, k)
        got, want = n(g).astype(np.float64), times * ref["grad"][k]
        errs[k] = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
        grad_close(f"{label} {k}", got, want, TOL)
    for k in ("verts", "sigmas", "scales", "quats", "colors", "features"):
        if k in st.leaves:
            assert np.abs(n(st.leaves[k].grad)[N - HIDDEN:N]).max() == 0.0, (label, k, "a Gaussian that no pixel sees got a gradient")
    return errs


def reference(name, views=None, rows=None):
    key = C.case_key(name)
    ref = dict(C.reference_of(name, views, rows))
    ref.update(key=key, rows=(0, H) if rows is None else rows)
    return ref


@pytest.mark.parametrize("order", list(C.ORDERS))
@pytest.mark.parametrize("case", list(C.CASES))
def test_every_order_gives_the_fp64_gradients(hip_lib, monkeypatch, case, order):
    label = f"[consumers] {case} {order}"
    ref = reference(case)
    views = range(ref["key"][1])
    st = render(case, monkeypatch)
    calls = spy_on(monkeypatch)
    outs = consume(st, C.ORDERS[order])
    assert not calls, (label, "a backward entry ran in the forward")
    out_errs = check_forward(label, st.frag, outs, ref, views)
    total_loss(outs, ref, views).backward()
    torch.cuda.synchronize()
    # measurements: the routes taken and what the kernels deliver (nothing below TOL is asserted)
    log_line(f"{label}: weights by {st.weight_node}; " + ", ".join(f"{k} {type(outs[k].grad_fn).__name__}" for k in C.CONSUMERS)
             + "; fused-backward entries " + (" ".join(name[5:] for name, _ in calls) or "none")
             + f"; largest output error {max(out_errs.values()):.1e} ({max(out_errs, key=out_errs.get)})")
    errs = check_gradients(label, st, ref)
    log_line(f"{label}: largest gradient error of scale per leaf: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items())
             + f"; {time.perf_counter() - T0[0]:.1f} s into the file")


# the composite nodes a case's orders must reach between them.  frame: all four.  full (a general form on the frame path, lz.gen set)
# and bundle (the ray-bundle chain, lz.frame unset): ops.composite_depth takes scalar-sigma fragments of the frame path only, so
# get_depth reads vert_weight and the lean composite makes it; composite_shade and composite_merge take both (K <= 128, 3 or 4 channels)
EXPECTED_NODES = {"frame": set(NODES), "full": set(NODES) - {"_CompositeDepthBackward"}, "bundle": set(NODES) - {"_CompositeDepthBackward"}}
FIRST_READER_NODE = dict(image="_CompositeShadeBackward", sil="_CompositeLeanBackward", depth="_CompositeDepthBackward",
                         n_hat="_CompositeMergeBackward", dist="_CompositeLeanBackward", feat="_CompositeMergeBackward",
                         image_bg="_CompositeMergeBackward")


@pytest.mark.parametrize("case", list(EXPECTED_NODES))
def test_the_orders_reach_all_four_composite_nodes(hip_lib, monkeypatch, case):
    seen = {}
    for order, seq in C.ORDERS.items():
        st = render(case, monkeypatch)
        consume(st, seq)
        seen[order] = st.weight_node
        first = next(name for name in seq if name != "hit")      # (vert_hit_length is the trace's: reading it composites nothing)
        want = FIRST_READER_NODE[first]
        if want not in EXPECTED_NODES[case]:
            want = "_CompositeLeanBackward"
        assert st.weight_node == want, (case, order, first, st.weight_node)
    log_line(f"[consumers] {case}: the node that made vert_weight, per order: " + ", ".join(f"{k} {v}" for k, v in seen.items()))
    assert set(seen.values()) == EXPECTED_NODES[case], (case, seen)


@pytest.mark.parametrize("case", list(C.CASES))
def test_second_backward_adds_the_same_gradients(hip_lib, monkeypatch, case):
    """retain_graph=True and two backward passes: the accumulators that the forwards zeroed are good for ONE backward each, and
    several nodes hold one at once -- the second pass must add the same gradient again."""
    ref = reference(case)
    views = range(ref["key"][1])
    for order in ("rot0_image", "reversed"):
        label = f"[consumers] {case} {order} two backwards"
        st = render(case, monkeypatch)
        outs = consume(st, C.ORDERS[order])
        loss = total_loss(outs, ref, views)
        loss.backward(retain_graph=True)
        first = {k: v.grad.clone() for k, v in st.leaves.items()}
        loss.backward()
        torch.cuda.synchronize()
        errs = check_gradients(label, st, ref, times=2)
        for k, g in first.items():      # (and the first pass alone was the reference's, once)
            grad_close(f"{label} {k}, first pass", n(g), ref["grad"][k], TOL)
        log_line(f"{label}: largest gradient error of scale per leaf: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))


@pytest.mark.parametrize("view", ["frag[1]", "frag[1] after a merge on the batch", "rows=(2, 6)", "squeeze"])
def test_views_of_the_fragments_behave_the_same(hip_lib, monkeypatch, view):
    """One view of two, a row band, and the reshaped view of a one-view batch (Fragments._map carries _lazy and _lead; the cached
    weight sum and the silhouette must follow the view): the nine consumers against the matching slice of the reference."""
    from voge_amd.Renderer import interpolate_attr
    from voge_amd.cameras import PerspectiveCameras
    label = f"[consumers] {view}"
    case = "frame" if view == "squeeze" else "frame_shared"
    x = C.inputs(C.case_key(case))
    for order in ("rot0_image", "rot2_depth", "rot7_feat", "reversed"):
        cameras = None
        if view == "rows=(2, 6)":
            ref, views = reference(case, rows=(2, 6)), (0, 1)
            st = render(case, monkeypatch, rows=(2, 6))
            frag = st.frag
        elif view == "squeeze":
            ref, views = reference(case), (0,)
            st = render(case, monkeypatch)
            frag = st.frag.squeeze()
            assert frag._lazy is not None and frag._lead is not None      # (still deferred: the one-pass forms stay open to it)
        else:
            ref, views = reference(case, views=(1,)), (1,)
            st = render(case, monkeypatch)
            if "after" in view:
                interpolate_attr(st.frag, st.featB)      # (leaves the batch's weight sum and silhouette on st.frag)
            frag = st.frag[1]
            cameras = PerspectiveCameras(focal_length=FOCAL, principal_point=((W / 2.0, H / 2.0),), image_size=((H, W),),
                                         R=np.array(x["R"][1:2]), T=np.array(x["T"][1:2]), device=DEV)
        outs = consume(st, C.ORDERS[order], frag, cameras)
        check_forward(f"{label} {order}", frag, outs, ref, views)
        total_loss(outs, ref, views).backward()
        torch.cuda.synchronize()
        errs = check_gradients(f"{label} {order}", st, ref)
        log_line(f"{label} {order}: weights by {st.weight_node}; largest gradient error of scale per leaf: "
                 + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
