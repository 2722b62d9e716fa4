"""Dirty scratch, dirty fresh tensors and leftovers between calls (tests/dirty.py; DESIGN.md "State between calls" names, for every
buffer poisoned here, the kernel that writes every byte later read).

Every entry point below runs with its scratch (ops._WS) and every torch.empty / empty_like / new_empty result of voge_amd byte-filled
with 0x00, 0x7F (floats 3.39e38, ints 2139062143) and 0xFF (NaN, -1, a full counter), and once behind another entry point with no
fill at all ("leftovers").  Nothing new is tolerated: the harnesses are the existing tests' own -- tests/test_gpu_consumers.py's
render / consume / check_forward / check_gradients against consumer_cases' fp64 reference at util.TOL, and each geometry module's
check against its module's reference at its own bound -- and no expected value comes from a clean run of the code under test.  What
the existing tests assert to be the same bits on every run (index lists, lens, weights, images, depth; mesh_reg; chamfer's and
point-mesh's fixed-point sums; knn and nearest-point indices) must be the same bits under all four patterns."""
import time

import numpy as np
import pytest
import torch

import consumer_cases as C
import dirty as D
import test_gpu_consumers as TC
from consumer_cases import FOCAL, H, HIDDEN, N, W
from test_gpu_fragment_bwd_entries import DEV, n, t
from util import TOL, grad_close, log_line

pytestmark = pytest.mark.gpu
PATTERNS = list(D.PATTERNS)
GROW = 1 << 25      # 32 MiB: the trace's scratch of these frames is 8.6 MiB (its list pool is never below 2^20 entries)
ORDERS = ("rot0_image", "reversed")
T0 = [None]


def clock():
    if T0[0] is None:
        T0[0] = time.perf_counter()
    return time.perf_counter() - T0[0]


def roomy(d):
    """No call under test outgrew the poisoned buffer (it would have got a fresh allocation in its place)."""
    assert all(asked <= GROW for asked, _ in d.taken), max(d.taken)
    return len(d.taken)


# ---- the other entry point that runs right before, for "leftovers" ----------------------------------------------------------------
def leftover_geometry():
    """chamfer forward + backward and a knn search on small clouds: fixed-point accumulators, grid cells and counters."""
    from knn_clouds import surface
    from voge_amd import Losses
    from voge_amd.Converter import Converters
    x = surface(24).to(DEV).requires_grad_(True)
    y = (surface(24)[:400] * 1.1).to(DEV)
    Losses.chamfer_distance(x, y)[0].backward()
    Converters.knn_points(y, 8)


def leftover_render():
    """One frame forward + backward: the trace's lists and counters, then the backward's accumulator at the scratch's head."""
    x = C.inputs(C.case_key("diag"))
    import test_gpu_depth as dpt
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import to_white_background
    gm = GaussianMeshes(t(x["verts"]), t(x["sig"])).to(DEV)
    frag = dpt.renderer_for(H, W, 5, FOCAL)(gm, R=t(x["R"]), T=t(x["T"]))
    to_white_background(frag, torch.cat([t(x["colors"], rg=True)] * 2)).sum().backward()


def sentinels(label, frag, ref, views):
    """Dead slots keep what the contract gives them: index -1 (0 once a merge rewrote the list: check_forward), len 1e10, weight 0."""
    K = ref["key"][2]
    r0, r1 = ref["rows"]
    vn = ref["vn"].reshape(-1, H, W)[list(views), r0:r1]
    dead = np.arange(K)[None, None, None] >= vn[..., None]
    ln, w = n(frag.vert_hit_length).reshape(dead.shape), n(frag.vert_weight).reshape(dead.shape)
    assert (ln[dead] == np.float32(1e10)).all(), (label, "a dead slot's len is not 1e10")
    assert (w[dead] == 0).all(), (label, "a dead slot's weight is not 0")
    assert (n(frag.valid_num).reshape(vn.shape) == vn).all(), (label, "valid_num")


# ---- the renderer: ten cases, nine consumers, two orders, one backward each ---------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS, ids=D.pattern_id)
@pytest.mark.parametrize("case", list(C.CASES))
def test_consumers_on_dirty_state(hip_lib, monkeypatch, case, pattern):
    ref = TC.reference(case)
    views = range(ref["key"][1])
    for order in ORDERS:
        label = f"[dirty {D.pattern_id(pattern)}] {case} {order}"
        with D.dirty(pattern, grow=GROW, before=leftover_geometry) as d:
            st = TC.render(case, monkeypatch)
            outs = TC.consume(st, C.ORDERS[order])
            loss = TC.total_loss(outs, ref, views)
            d.refill()
            loss.backward()
            torch.cuda.synchronize()
            taken = roomy(d)
        TC.check_forward(label, st.frag, outs, ref, views)
        sentinels(label, st.frag, ref, views)
        errs = TC.check_gradients(label, st, ref)
        log_line(f"{label}: {d.filled} fresh tensors and {taken} scratch hand-overs poisoned; largest gradient error of scale "
                 f"{max(errs.values()):.1e} ({max(errs, key=errs.get)}); {clock():.1f} s into the file")


@pytest.mark.parametrize("pattern", PATTERNS, ids=D.pattern_id)
@pytest.mark.parametrize("case", list(C.CASES))
def test_second_backward_on_dirty_state(hip_lib, monkeypatch, case, pattern):
    """The second pass over a retained graph finds the forward's accumulator used: it takes the scratch form, which is poisoned."""
    ref = TC.reference(case)
    views = range(ref["key"][1])
    label = f"[dirty {D.pattern_id(pattern)}] {case} two backwards"
    with D.dirty(pattern, grow=GROW, before=leftover_geometry) as d:
        st = TC.render(case, monkeypatch)
        outs = TC.consume(st, C.ORDERS["rot0_image"])
        loss = TC.total_loss(outs, ref, views)
        loss.backward(retain_graph=True)
        first = {k: v.grad.clone() for k, v in st.leaves.items()}
        d.refill()
        loss.backward()
        torch.cuda.synchronize()
        roomy(d)
    TC.check_gradients(label, st, ref, times=2)
    for k, g in first.items():
        grad_close(f"{label} {k}, first pass", n(g), ref["grad"][k], TOL)


def forward_bits(case, monkeypatch, pattern):
    with D.dirty(pattern, grow=GROW, before=leftover_geometry) as d:
        st = TC.render(case, monkeypatch)
        outs = TC.consume(st, C.ORDERS["rot0_image"])
        torch.cuda.synchronize()
        roomy(d)
    frag = st.frag
    out = dict(index=frag.vert_index, len=frag.vert_hit_length, weight=frag.vert_weight, valid_num=frag.valid_num)
    out.update({k: outs[k] for k in ("image", "image_bg", "depth")})
    return {k: n(v).tobytes() for k, v in out.items()}


@pytest.mark.parametrize("case", list(C.CASES))
def test_forward_outputs_have_the_same_bits_under_every_pattern(hip_lib, monkeypatch, case):
    got = {p: forward_bits(case, monkeypatch, p) for p in PATTERNS}
    for p in PATTERNS[1:]:
        for k, v in got[p].items():
            assert v == got[PATTERNS[0]][k], (case, k, D.pattern_id(p), "differs from", D.pattern_id(PATTERNS[0]))
    log_line(f"[dirty] {case}: {len(got[PATTERNS[0]])} forward outputs bit-equal under {len(PATTERNS)} patterns; {clock():.1f} s into the file")


# ---- the accumulator's two zeroing routes -----------------------------------------------------------------------------------------
# composite.hip, comp_plan(K = 5, npix = 70, forward, onepass): NS = 4 slots a lane -> lanes = ceil(5 / 4) = 2 a pixel, one-wave
# workgroups of threads = 64 -> ppw = 64 / 2 = 32 pixels each, grid = ceil(70 / 32) = 3: grid x threads = 192 float4.  comp_zero_rider
# lets the forward's launch zero the accumulator on its way while n4 = B N per / 16 <= 192 and takes voge_fill_async beyond.
# One view, per bytes a Gaussian -> n4 = N per / 16: the rider's last float4 is used at n4 = 192 exactly.
#   per 32 (scalar sigmas, image first):  N = 95 (190), 96 (192), 97 (194: the fill)
#   per 48 ([N,3] sigmas, image first):   N = 63 (189), 64 (192), 65 (195: the fill)
#   per 64 ([N,3,3] sigmas, image first): N = 47 (188), 48 (192), 49 (196: the fill)
#   per 16 (scalar sigmas, depth first):  N = 191, 192, 193 (the fill)
GRID_X_THREADS = 192
ACC_CASES = [(form, order, per, GRID_X_THREADS * 16 // per + dn)
             for form, order, per in (("scalar", "rot0_image", 32), ("diag", "rot0_image", 48), ("full", "rot0_image", 64), ("scalar", "rot2_depth", 16))
             for dn in (-1, 0, 1)]


def render_padded(key, n_total, monkeypatch):
    """TC.render for a key of consumer_cases with n_total - N more Gaussians outside every view (copies of the scene's last hidden
    one, moved further up): index lists, outputs and the first N rows of every gradient are the case's own, the other rows zero."""
    import types
    import test_gpu_depth as dpt
    from voge_amd import ops
    from voge_amd.Meshes import GaussianMeshes
    form, B, K, inverse = key
    assert B == 1 and n_total > N
    x = C.inputs(key)
    extra = n_total - N
    monkeypatch.setattr(ops, "FRAME_PATH", True)
    monkeypatch.setattr(ops, "FRAME_DIRECT_BWD", True)
    rng = np.random.default_rng(n_total)

    def pad(a, rows):
        return np.concatenate([a, rows.astype(np.float32)])
    verts = pad(x["verts"], x["verts"][-1:] + np.stack([rng.uniform(-1, 1, extra), rng.uniform(1, 9, extra), rng.uniform(-1, 1, extra)], 1))
    sig = pad(x["sig"], np.repeat(x["sig"][-1:], extra, 0))
    gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
    renderer = dpt.renderer_for(H, W, K, FOCAL, inverse=inverse)
    frag = renderer(gm, R=t(x["R"]), T=t(x["T"]))
    st = types.SimpleNamespace(name=str(key), key=key, gm=gm, frag=frag, cameras=renderer.cameras, rows=None,
                               colors=t(pad(x["colors"], rng.uniform(0, 1, (extra, 3))), rg=True),
                               features=t(pad(x["features"], rng.uniform(-1, 1, (extra, 4))), rg=True), bg=t(x["bg"], rg=True),
                               table=t(pad(x["table"], np.repeat(x["table"][-1:], extra, 0)), rg=True))
    st.colsB, st.featB = st.colors, st.features
    st.leaves = dict(verts=gm.verts, sigmas=gm.sigmas, colors=st.colors, features=st.features, bg=st.bg, table=st.table)
    return st


@pytest.mark.parametrize("pattern", PATTERNS, ids=D.pattern_id)
@pytest.mark.parametrize("form,order,per,n_total", ACC_CASES, ids=lambda v: str(v))
def test_accumulator_zeroing_routes_at_the_launchs_last_float4(hip_lib, monkeypatch, form, order, per, n_total, pattern):
    from voge_amd import ops
    key = (form, 1, 5, False)
    ref = dict(C.evaluate(key))
    ref.update(key=key, rows=(0, H))
    label = f"[dirty {D.pattern_id(pattern)}] accumulator {per} B a Gaussian, N = {n_total} (n4 = {n_total * per // 16} against {GRID_X_THREADS})"
    made = []
    real_acc = ops._frame_acc

    def spy_acc(lz, need, per_=None):
        acc = real_acc(lz, need, per_)
        made.append(None if acc is None else acc.numel())
        return acc
    monkeypatch.setattr(ops, "_frame_acc", spy_acc)
    with D.dirty(pattern, grow=GROW, before=leftover_geometry) as d:
        st = render_padded(key, n_total, monkeypatch)
        outs = TC.consume(st, C.ORDERS[order])
        TC.total_loss(outs, ref, (0,)).backward()
        torch.cuda.synchronize()
        roomy(d)
    assert n_total * per in made, (label, made, "the first reader did not make the accumulator this case is about")
    TC.check_forward(label, st.frag, outs, ref, (0,))
    sentinels(label, st.frag, ref, (0,))
    for k in C.leaf_names(form):
        got, want = n(st.leaves[k].grad).astype(np.float64), ref["grad"][k]
        if got.shape != want.shape:
            assert (got[N:] == 0).all(), (label, k, "a Gaussian that no pixel sees got a gradient: the accumulator was not zero")
            got = got[:N]
        grad_close(f"{label} {k}", got, want, TOL)
        if k not in ("bg", "table"):
            assert np.abs(got[N - HIDDEN:N]).max() == 0.0, (label, k)
    log_line(f"{label}: accumulators made {made}; {clock():.1f} s into the file")


# ---- the ray-bundle API and the geometry: each module's own check, on dirty state ---------------------------------------------------
def _rays(lib):
    import test_gpu_parity as m
    m.test_pixel_rays_fwd_bwd(lib)


def _packed_trace_bwd(lib):
    import test_gpu_parity as m
    m.test_trace_bwd_vs_oracle(lib, False)
    m.test_trace_bwd_vs_oracle(lib, True)


def _nearest_k(lib):
    import test_gpu_attr_routes as a
    import test_gpu_next_rows as m
    m.test_find_nearest_and_farest_k(lib, 5)
    a.test_nearest_and_farthest_k_are_exact_copies_in_oracle_order(lib, 129, 9, 4, False)
    m.test_dense_ray_trace_fwd_bwd(lib)


def _scatter_max(lib):
    import test_gpu_attr_routes as a
    a.test_scatter_max_is_the_exact_maximum_under_heavy_collisions(lib)


def _knn(lib):
    import test_gpu_knn as m
    from knn_clouds import lattice
    m.same_as_definition(lattice(), 4)
    m.same_as_definition(lattice()[:777], 8, include_self=True, cell_size=8 / 1024)
    m.test_frames_against_fp64_eigh(lib, 24, 8)


def _nearest_points(lib):
    import test_gpu_chamfer as m
    from knn_clouds import lattice
    m.same_as_definition(lattice()[:1400], lattice()[1400:], routes=("brute", "grid"))


def _chamfer(lib):
    import test_gpu_chamfer as m
    from chamfer_clouds import surface_pair
    x, y = surface_pair()
    for route in ("brute", "grid"):
        m.test_loss_is_the_fp64_reduction_of_the_definitions_d2(lib, route)
        m.check_grads("surfaces, dirty", x, y, route)
        m.check_grads("surfaces single, dirty", x, y, route, single_directional=True)


def _mesh_sample(lib):
    import test_gpu_mesh_sample as m
    m.test_tetrahedron(lib, True)
    m.test_areas_are_the_definitions_bits(lib)


def _point_mesh(lib):
    import point_mesh_cases as cases
    import test_gpu_point_mesh as m
    verts, faces = cases.soup(65)
    m.check_both_directions("soup F=65, dirty", verts, faces, cases.points_around(verts, faces, 65, seed=130))
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 700, seed=4)
    m.check_grads("sphere, dirty", verts, faces, points)
    m.check_grads("sphere single, dirty", verts, faces, points, single_directional=True)


def _mesh_reg(lib):
    import test_gpu_mesh_reg as m
    from test_mesh_reg_cpu import noisy_sphere
    for name in ("hexagon_hub", "zero_area"):
        m.test_hand_cases(lib, name)
    v, f = noisy_sphere(1, 0.15)
    m.compare("sphere1", v, m.topology(f), m.T)


MESHING_REF = {}


def _meshing(lib):
    """TSDF integrate -> marching tetrahedra: tests/test_gpu_meshing.py's two comparisons (the fp64 definition is made once)."""
    import meshing_cases as mc
    import test_gpu_meshing as m
    from voge_amd import Aggregation
    m.check_extraction("random 5x7x9, dirty", m.bordered_noise((9, 7, 5), 5), lo=(0.3, -2.0, 1.0), h=(0.1, 0.2, 0.3))
    values, weight = mc.holes_field()
    m.check_extraction("holes, dirty", values, weight)
    depth, R, T, focal, pp = mc.three_views()
    trunc = 2 * mc.GRID_H
    if not MESHING_REF:
        MESHING_REF["ref"] = mc.definition_fp64(depth, R, T, focal, pp, trunc, mark=(2.0 ** -10, 2.0 ** -18))
    ref_t, ref_w, marked = MESHING_REF["ref"]
    vol = m.device_volume().integrate(depth.to(DEV), m.device_cams(R, T, focal, pp), trunc)
    keep = ~marked
    bound = mc.tsdf_bound(Aggregation.camera_centres(R.double(), T.double()), float(np.float32(trunc)), 3, float(depth[torch.isfinite(depth)].max()))
    assert torch.equal(vol.weight.cpu().double()[keep], ref_w[keep])
    assert float((vol.tsdf.cpu().double() - ref_t)[keep].abs().max()) <= bound
    m.test_end_to_end_on_the_device()      # (integrate -> extract -> the mesh side of the project)


ENTRIES = dict(pixel_rays=_rays, packed_trace_bwd=_packed_trace_bwd, nearest_k=_nearest_k, scatter_max=_scatter_max, knn=_knn,
               nearest_points=_nearest_points, chamfer=_chamfer, mesh_sample=_mesh_sample, point_mesh=_point_mesh, mesh_reg=_mesh_reg,
               meshing=_meshing)


@pytest.mark.parametrize("pattern", PATTERNS, ids=D.pattern_id)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_points_on_dirty_state(hip_lib, entry, pattern):
    t0 = time.perf_counter()
    with D.dirty(pattern, grow=GROW, before=leftover_render) as d:
        ENTRIES[entry](hip_lib)
        torch.cuda.synchronize()
        taken = roomy(d)
    log_line(f"[dirty {D.pattern_id(pattern)}] {entry}: its module's checks passed with {d.filled} fresh tensors and {taken} scratch "
             f"hand-overs poisoned; {time.perf_counter() - t0:.1f} s; {clock():.1f} s into the file")


# ---- the same bits under every pattern ---------------------------------------------------------------------------------------------
def _bits(*tensors):
    return tuple(None if x is None else x.detach().cpu().numpy().tobytes() for x in tensors)


def bits_knn():
    from knn_clouds import lattice
    from voge_amd import ops
    from voge_amd.Converter import Converters
    q, p = lattice()[:1400].to(DEV), lattice()[1400:].to(DEV)
    out = _bits(*Converters.knn_points(lattice().to(DEV), 4))
    for route in ("brute", "grid"):
        out += _bits(*ops.nearest_points(q, p, route=route))
    return out


def bits_chamfer():
    from chamfer_clouds import surface_pair
    from voge_amd import ops
    out = ()
    for route in ("brute", "grid"):
        x, y = (a.to(DEV).requires_grad_(True) for a in surface_pair())
        loss, nn_x, nn_y = ops.chamfer(x, y, False, False, route)
        (loss * -1.75).backward()
        out += _bits(loss, nn_x, nn_y, x.grad, y.grad)
    return out


def bits_point_mesh():
    import point_mesh_cases as cases
    from voge_amd import ops
    verts, faces = cases.level2_sphere()
    points = cases.points_around(verts, faces, 700, seed=4)
    v, p = verts.to(DEV).requires_grad_(True), points.to(DEV).requires_grad_(True)
    loss, face_idx, bary_p, point_idx, bary_f = ops.point_mesh(v, faces.int().to(DEV), p)
    (loss * -1.75).backward()
    return _bits(loss, face_idx, bary_p, point_idx, bary_f, v.grad, p.grad)


def bits_mesh_reg():
    import test_gpu_mesh_reg as m
    from test_mesh_reg_cpu import noisy_sphere
    v, f = noisy_sphere(2, 0.15)
    got, grads, _ = m.run_kernel(v, m.topology(f), m.T)
    return (got.tobytes(),) + tuple(g.tobytes() for g in grads)


BITS = dict(knn_and_nearest_points=bits_knn, chamfer=bits_chamfer, point_mesh=bits_point_mesh, mesh_reg=bits_mesh_reg)


@pytest.mark.parametrize("what", list(BITS))
def test_reproducible_outputs_have_the_same_bits_under_every_pattern(hip_lib, what):
    got = {}
    for p in PATTERNS:
        with D.dirty(p, grow=GROW, before=leftover_render) as d:
            got[p] = BITS[what]()
            torch.cuda.synchronize()
            roomy(d)
    for p in PATTERNS[1:]:
        assert len(got[p]) == len(got[PATTERNS[0]])
        for i, (a, b) in enumerate(zip(got[p], got[PATTERNS[0]])):
            assert a == b, (what, i, D.pattern_id(p), "differs from", D.pattern_id(PATTERNS[0]))
    log_line(f"[dirty] {what}: {len(got[PATTERNS[0]])} outputs bit-equal under {len(PATTERNS)} patterns; {clock():.1f} s into the file")


# ---- cross-talk: the entry points are each other's leftovers -------------------------------------------------------------------------
def test_interleaved_entry_points_on_one_stream(hip_lib, monkeypatch):
    """render forward -> chamfer -> render backward -> knn -> point-mesh -> second render backward, nothing filled in between; every
    result to its reference."""
    import point_mesh_cases as cases
    import test_gpu_chamfer as tch
    import test_gpu_knn as tknn
    import test_gpu_point_mesh as tpm
    from chamfer_clouds import surface_pair
    from knn_clouds import lattice
    for case in ("frame", "full", "bundle"):
        label = f"[cross-talk] {case}"
        ref = TC.reference(case)
        views = range(ref["key"][1])
        st = TC.render(case, monkeypatch)
        outs = TC.consume(st, C.ORDERS["rot0_image"])
        loss = TC.total_loss(outs, ref, views)
        x, y = surface_pair()
        tch.check_grads("cross-talk", x, y, "grid")
        loss.backward(retain_graph=True)
        first = {k: v.grad.clone() for k, v in st.leaves.items()}
        tknn.same_as_definition(lattice()[:777], 8)
        verts, faces = cases.soup(65)
        tpm.check_both_directions("cross-talk", verts, faces, cases.points_around(verts, faces, 65, seed=130))
        tpm.check_grads("cross-talk", verts, faces, cases.points_around(verts, faces, 65, seed=131))
        loss.backward()
        torch.cuda.synchronize()
        TC.check_forward(label, st.frag, outs, ref, views)
        TC.check_gradients(label, st, ref, times=2)
        for k, g in first.items():
            grad_close(f"{label} {k}, first pass", n(g), ref["grad"][k], TOL)
    log_line(f"[cross-talk] three cases interleaved with chamfer, knn and point-mesh; {clock():.1f} s into the file")
