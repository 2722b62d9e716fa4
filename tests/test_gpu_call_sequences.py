"""One GaussianRenderer, many frames, one thing changed per step: every memo that outlives a call (GaussianRenderer._frame_memo,
cameras._INTR, Renderer._BG_CACHE, ops._WS, the lazy composite's version tags) must answer for the state it is asked about.

At every step the index lists and the image are BIT-EQUAL to the same frame from fresh state (a new renderer and cameras,
cameras._INTR.clear(), ops.release_workspaces()), the image differs from the previous step's where the change must show (two stale
results would agree otherwise), and every distinct camera configuration is compared once with the fp64 oracle (oracle/torch_ref.py:
trace_dense, aggregation, merge_final, to_colored_background, as tests/consumer_cases.py composes them) at util.TOL, every pixel.
The sequence runs first and the fresh frames afterwards, so that clearing the memos for them does not disturb what is under test.
Scene: tests/test_gpu_fragment_bwd_entries.py's 40 Gaussians on a 10 x 7 image, as scalar, [N,3] and oriented Gaussians (the three
call sites of _frame_camera).  The CPU half is tests/test_call_sequences_cpu.py."""
import time

import numpy as np
import pytest
import torch

import consumer_cases as C
from oracle import camera_np, torch_ref
from test_gpu_fragment_bwd_entries import DEV, FOCAL, H, HIDDEN, N, W, n, scene, t
from util import TOL, close, log_line

pytestmark = pytest.mark.gpu
K = 5
FORMS = {"scalar": "scalar", "per_axis": "diag", "oriented": "ori"}
ORACLE = {}


def look(dist, elev, azim):
    R, T = camera_np.look_at_view_transform(dist, elev, azim)
    return R.astype(np.float32), T.astype(np.float32)


def arrays(form, copies=1):
    """The scene's fp32 arrays; copies > 1: that many copies side by side (a larger N for a larger frame)."""
    verts, sig, quats, cols = scene(form, C.SEED)
    cols = np.ascontiguousarray(cols[:, :3])
    if copies > 1:
        shift = np.linspace(-0.5, 0.5, copies)
        verts = np.concatenate([verts + np.float32([s, 0.0, 0.0]) for s in shift]).astype(np.float32)
        sig, cols = np.concatenate([sig] * copies), np.concatenate([cols] * copies)
        quats = None if quats is None else np.concatenate([quats] * copies)
    return dict(form=form, verts=verts, sig=sig, quats=quats, cols=cols)


def meshes(a):
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes
    if a["form"] == "ori":
        return OrientedGaussianMeshes(t(a["verts"]), t(a["sig"]), t(a["quats"])).to(DEV)
    return GaussianMeshes(t(a["verts"]), t(a["sig"])).to(DEV)


def oracle_frame(a, cam):
    """fp64 index lists [B,h,W,K] and white-background image [B,h,W,3] of a configuration, made once."""
    from voge_amd.Aggregation import oriented_sigma
    key = (a["form"], len(a["verts"]), cam["R"].tobytes(), cam["T"].tobytes(), cam["focal"].tobytes(), cam["pp"].tobytes(), cam["size"],
           str(cam["rows"]))
    if key not in ORACLE:
        Hh, Ww = cam["size"]
        rays, origin = camera_np.pixel_rays(cam["R"], cam["T"], cam["focal"], cam["pp"], (Hh, Ww))
        rows = cam["rows"]
        if rows is not None:
            rays = rays[:, rows.image_rows().numpy()] if hasattr(rows, "stripe_h") else rays[:, rows[0]:rows[1]]
        v = torch.tensor(a["verts"], dtype=torch.float64)
        s = torch.tensor(a["sig"], dtype=torch.float64)
        S = {"scalar": lambda: s[:, None, None] * torch.eye(3, dtype=torch.float64), "diag": lambda: torch.diag_embed(s),
             "ori": lambda: oriented_sigma(s, torch.tensor(a["quats"], dtype=torch.float64))}[a["form"]]()
        cols = torch.tensor(a["cols"], dtype=torch.float64)
        idxs, imgs = [], []
        for b in range(rays.shape[0]):
            r = torch.tensor(rays[b], dtype=torch.float64).reshape(-1, 3)
            idx, ln, act, dsd = torch_ref.trace_dense(v - torch.tensor(origin[b])[None], 2 * S, r, K, C.THR_ACT)
            w, vn = torch_ref.aggregation(idx, act, ln, dsd, 1.0)
            rgb = torch_ref.merge_final(cols, w, vn, idx)
            imgs.append(torch_ref.to_colored_background(rgb, w, torch.ones(3, dtype=torch.float64)).numpy())
            idxs.append(torch.where(idx >= 0, idx + b * len(a["verts"]), idx).numpy())
        shape = rays.shape[:3]
        ORACLE[key] = (np.stack(idxs).reshape(shape + (K,)), np.stack(imgs).reshape(shape + (3,)))
    return ORACLE[key]


def renderer_of(cam, requires_grad=False):
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras
    cams = PerspectiveCameras(focal_length=t(cam["focal"]), principal_point=torch.tensor(cam["pp"], dtype=torch.float64), R=cam["R"],
                              T=cam["T"], image_size=(cam["size"],), device=DEV)
    if requires_grad:
        cams.R = cams.R.clone().requires_grad_(True)
    return GaussianRenderer(cams, GaussianRenderSettings(image_size=cam["size"], max_assign=K, max_point_per_bin=-1)).to(DEV)


def shot(renderer, gm, cols, rows=None):
    """One frame -> (index lists after the image's merge, image), on the host."""
    from voge_amd.Renderer import to_white_background
    frag = renderer(gm) if rows is None else renderer(gm, rows=rows)
    img = to_white_background(frag, torch.cat([cols] * frag.vert_index.shape[0]))
    return n(frag.vert_index).copy(), n(img).copy()


def snapshot(renderer, a, rows, requires_grad=False):
    c = renderer.cameras
    B = max(c.R.shape[0], c.T.shape[0])
    f = np.broadcast_to(n(c.focal_length).astype(np.float32).reshape(-1, 1), (B, 2)) if c.focal_length.numel() == B or c.focal_length.numel() == 1 \
        else n(c.focal_length).astype(np.float32).reshape(B, 2)
    return dict(a=a, requires_grad=requires_grad,
                cam=dict(R=n(c.R).copy(), T=n(c.T).copy(), focal=np.ascontiguousarray(f), pp=np.ascontiguousarray(np.broadcast_to(
                    n(c.principal_point).astype(np.float32).reshape(-1, 2), (B, 2))), size=tuple(renderer.render_settings.image_size), rows=rows))


def run_sequence(form, monkeypatch):
    """The steps -> [(label, snapshot of the state, index lists, image, must the image differ from the step before)]."""
    import voge_amd.Renderer as RM
    from voge_amd import ops
    from voge_amd.distributed import Stripes
    a, big = arrays(form), arrays(form, copies=3)
    gm, gm_big = meshes(a), meshes(big)
    cols, cols_big = t(a["cols"]), t(big["cols"])
    R0, T0_ = look([4.0], [10.0], [70.0])
    R1, T1 = look([3.7], [-20.0], [200.0])
    R2, T2 = look([4.3], [25.0], [130.0])
    RB, TB = look([4.0, 3.7], [10.0, -20.0], [70.0, 200.0])
    size = (H, W)
    r = renderer_of(dict(R=R0, T=T0_, focal=np.float32([FOCAL]), pp=np.float64([[W / 2.0, H / 2.0]]), size=size))
    cams = r.cameras
    rebuilt = []
    real = RM.camera_tensors
    monkeypatch.setattr(RM, "camera_tensors", lambda *x, **k: (rebuilt.append(1), real(*x, **k))[1])
    steps = []

    def take(label, differs, gmesh=gm, colours=cols, arr=a, rows=None, rg=False):
        idx, img = shot(r, gmesh, colours, rows)
        steps.append((label, snapshot(r, arr, rows, rg), idx, img, differs))

    take("0 the first frame", False)
    before = len(rebuilt)
    take("1 the same frame again", False)
    assert len(rebuilt) == before, "the second identical call rebuilt the camera tensors: the test is not on the memo path"
    cams.R.copy_(t(R1)); cams.T.copy_(t(T1))
    take("2 R / T overwritten in place", True)
    assert len(rebuilt) == before, "an in-place pose update left the memo path (the pose is read on every call, not remembered)"
    cams.R, cams.T = t(R2), t(T2)
    take("3 R / T replaced by new tensors", True)
    cams.focal_length.mul_(1.25)
    take("4 focal_length edited in place", True)
    seen = {cams.focal_length.data_ptr()}
    recycled = 0
    for i, value in enumerate((24.0, 33.0, 27.0)):
        cams.focal_length = None      # (the renderer's memo still holds the old tensor until the next frame replaces it)
        cams.focal_length = torch.full((1,), value, device=DEV)
        recycled += cams.focal_length.data_ptr() in seen
        seen.add(cams.focal_length.data_ptr())
        take(f"5.{i} focal_length replaced by a new tensor of value {value}", True)
    cams.principal_point[0, 0] += 1.5
    take("6 principal_point edited in place", True)
    seen_p = {cams.principal_point.data_ptr()}
    for i, value in enumerate(((4.0, 3.0), (6.0, 4.5), (5.0, 3.5))):
        cams.principal_point = None
        cams.principal_point = torch.tensor([value], dtype=torch.float64, device=DEV)
        recycled += cams.principal_point.data_ptr() in seen_p
        seen_p.add(cams.principal_point.data_ptr())
        take(f"6.{i} principal_point replaced by a new tensor {value}", True)
    log_line(f"[sequences] {form}: {recycled} of 6 replaced intrinsics came back at an address seen before")
    r.render_settings.image_size = (H + 2, W + 2)
    take("7 image_size replaced by another tuple", True)
    r.render_settings.image_size = (H, W)
    take("7 ... and back (an equal tuple, another object)", True)
    take("8 rows=(2, 6)", True, rows=(2, 6))
    take("8 rows=Stripes(H, 1, 2, 2)", True, rows=Stripes(H, 1, 2, 2))
    take("8 rows=None again", True)
    cams.R, cams.T = t(RB), t(TB)
    take("9 two views", True)
    cams.R, cams.T = t(R2), t(T2)
    take("9 one view again", True)
    cams.R = t(R0).requires_grad_(True)
    cams.T = t(T0_)
    take("10 a camera whose R requires grad (off the frame path)", True, rg=True)
    cams.R = t(R0)
    take("10 ... and back on it", False)
    r.render_settings.image_size = (2 * H + 2, 2 * W)
    cams.principal_point = torch.tensor([[W * 1.0, H + 1.0]], dtype=torch.float64, device=DEV)
    cams.focal_length = torch.full((1,), 2 * FOCAL, device=DEV)
    take("11 a larger N and frame", True, gmesh=gm_big, colours=cols_big, arr=big)
    r.render_settings.image_size = size
    cams.principal_point = torch.tensor([[W / 2.0, H / 2.0]], dtype=torch.float64, device=DEV)
    cams.focal_length = torch.full((1,), FOCAL, device=DEV)
    take("11 the small one again (the scratch shrank logically, not physically)", True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        take("12 the same on a side stream", False)
    side.synchronize()
    ops.release_workspaces()
    take("13 after release_workspaces()", False)
    return steps


@pytest.mark.parametrize("form", list(FORMS))
def test_one_renderer_many_frames(hip_lib, monkeypatch, form):
    from voge_amd import cameras, ops
    t0 = time.perf_counter()
    steps = run_sequence(FORMS[form], monkeypatch)
    monkeypatch.undo()
    checked = set()
    prev = None
    for label, snap, idx, img, differs in steps:
        label = f"[sequences] {form} step {label}"
        cam = snap["cam"]
        # fresh state
        cameras._INTR.clear()
        ops.release_workspaces()
        fi, fimg = shot(renderer_of(cam, snap["requires_grad"]), meshes(snap["a"]), t(snap["a"]["cols"]), cam["rows"])
        assert idx.shape == fi.shape and (idx == fi).all(), (label, "index lists differ from the fresh frame's")
        assert img.tobytes() == fimg.tobytes(), (label, "the image differs from the fresh frame's", float(np.abs(img - fimg).max()))
        # the change shows
        if differs:
            assert prev.shape != img.shape or not (prev == img).all(), (label, "the image is the previous step's")
        prev = img
        # the oracle, once per configuration
        want_idx, want_img = oracle_frame(snap["a"], cam)
        key = (len(snap["a"]["verts"]), cam["R"].tobytes(), cam["T"].tobytes(), cam["focal"].tobytes(), cam["pp"].tobytes(), cam["size"], str(cam["rows"]))
        if key not in checked:
            checked.add(key)
            same = (idx == want_idx).all(-1) | (idx == np.where(want_idx < 0, 0, want_idx)).all(-1)
            assert same.all(), (label, f"{int((~same).sum())} of {same.size} pixels have another index list than the fp64 oracle")
            err = float((np.abs(img - want_img) / np.maximum(1.0, np.abs(want_img))).max())
            assert close(img, want_img, TOL).all(), (label, f"image off by {err:.2e} of scale")
            assert (want_idx >= 0).any() and (want_idx < 0).any(), (label, "a frame without hits or without empty slots")
    log_line(f"[sequences] {form}: {len(steps)} steps, {len(checked)} camera configurations against the fp64 oracle; {time.perf_counter() - t0:.1f} s")


def test_background_cache_and_two_lazy_composites_alive(hip_lib):
    """_BG_CACHE: (1, 1, 1), (1.0, 1.0, 1.0), [1, 1, 1] and a second colour, alternating; then the Fragments of frame i consumed
    after frame i + 1 was rendered, backward in both orders: every image and gradient is the one of its own frame."""
    from voge_amd.Renderer import to_colored_background
    a = arrays("scalar")
    R0, T0_ = look([4.0], [10.0], [70.0])
    R1, T1 = look([3.7], [-20.0], [200.0])
    cam0 = dict(R=R0, T=T0_, focal=np.float32([[FOCAL, FOCAL]]), pp=np.float32([[W / 2.0, H / 2.0]]), size=(H, W), rows=None)
    cam1 = dict(cam0, R=R1, T=T1)
    r = renderer_of(cam0)
    gm = meshes(a)
    white_idx, white = oracle_frame(a, cam0)
    other = (0.2, 0.3, 0.4)
    cols = t(a["cols"])
    imgs = {}
    for rnd in range(2):
        for name, bg in (("ints", (1, 1, 1)), ("other", other), ("floats", (1.0, 1.0, 1.0)), ("other again", other), ("list", [1, 1, 1])):
            img = n(to_colored_background(r(gm), cols, bg))[0]
            imgs.setdefault(name, img)
            assert img.tobytes() == imgs[name].tobytes(), (name, rnd)
    for name in ("ints", "floats", "list"):
        assert imgs[name].tobytes() == imgs["ints"].tobytes() and close(imgs[name], white[0], TOL).all(), name
    assert imgs["other"].tobytes() == imgs["other again"].tobytes()
    want_other = oracle_colored(a, cam0, other)
    assert close(imgs["other"], want_other[0], TOL).all() and not (imgs["other"] == imgs["ints"]).all()
    # two lazy composites alive at once
    ref = {}
    for name, cam in (("i", cam0), ("i + 1", cam1)):
        ref[name] = fp64_image_grads(a, cam)
    for order in (("i", "i + 1"), ("i + 1", "i")):
        gm = meshes(a)
        cols = t(a["cols"], rg=True)
        frag = {"i": r(gm, R=t(R0), T=t(T0_))}
        frag["i + 1"] = r(gm, R=t(R1), T=t(T1))
        img = {name: to_colored_background(frag[name], cols, (1, 1, 1)) for name in ("i", "i + 1")}      # (frame i is consumed after i + 1 was rendered)
        for name in ("i", "i + 1"):
            assert close(n(img[name]), ref[name]["img"], TOL).all(), (order, name)
        for name in order:
            gm.zero_grad()
            cols.grad = None
            (img[name] * t(ref[name]["g"])).sum().backward()
            for k, got in (("verts", gm.verts.grad), ("sig", gm.sigmas.grad), ("cols", cols.grad)):
                want = ref[name][k]
                err = float(np.abs(n(got) - want).max())
                assert err <= TOL * max(1.0, float(np.abs(want).max())), (order, name, k, err)
                assert np.abs(n(got)[N - HIDDEN:]).max() == 0.0, (order, name, k)


def oracle_colored(a, cam, bg):
    out = fp64_image_grads(a, cam, bg)
    return out["img"]


GRADS = {}


def fp64_image_grads(a, cam, bg=(1.0, 1.0, 1.0)):
    """fp64 autograd of <g, image> of one scalar-sigma frame -> dict(img [1,H,W,3], g, verts, sig, cols)."""
    key = (cam["R"].tobytes(), cam["T"].tobytes(), tuple(bg))
    if key not in GRADS:
        rays, origin = camera_np.pixel_rays(cam["R"], cam["T"], cam["focal"], cam["pp"], cam["size"])
        v = torch.tensor(a["verts"], dtype=torch.float64, requires_grad=True)
        s = torch.tensor(a["sig"], dtype=torch.float64, requires_grad=True)
        cols = torch.tensor(a["cols"], dtype=torch.float64, requires_grad=True)
        S = s[:, None, None] * torch.eye(3, dtype=torch.float64)
        idx, ln, act, dsd = torch_ref.trace_dense(v - torch.tensor(origin[0])[None], 2 * S, torch.tensor(rays[0], dtype=torch.float64).reshape(-1, 3), K, C.THR_ACT)
        w, vn = torch_ref.aggregation(idx, act, ln, dsd, 1.0)
        img = torch_ref.to_colored_background(torch_ref.merge_final(cols, w, vn, idx), w, torch.tensor(bg, dtype=torch.float64)).reshape(1, H, W, 3)
        g = np.random.default_rng(7).normal(size=(1, H, W, 3))
        (img * torch.tensor(g)).sum().backward()
        GRADS[key] = dict(img=img.detach().numpy(), g=g, verts=v.grad.numpy(), sig=s.grad.numpy(), cols=cols.grad.numpy())
    return GRADS[key]


# ---- Losses._checked_faces on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["point_mesh_face_distance", "point_mesh_edge_distance", "closest_faces"])
def test_a_new_device_faces_tensor_at_a_recycled_address_is_checked(hip_lib, name):
    """tests/test_call_sequences_cpu.py's loop with the faces on the device (whichever way it goes no kernel is at risk: they skip a
    face that names a vertex out of range, and with the check in place none is launched)."""
    import test_call_sequences_cpu as cpu
    from voge_amd import Losses
    verts, points = cpu.VERTS.to(DEV), cpu.POINTS.to(DEV)
    width, check = {"point_mesh_face_distance": (3, lambda f: Losses.point_mesh_face_distance(verts, f, points)),
                    "point_mesh_edge_distance": (2, lambda f: Losses.point_mesh_edge_distance(verts, f, points)),
                    "closest_faces": (3, lambda f: Losses.closest_faces(points, verts, f))}[name]
    reused = cpu.recycled_faces(check, width, device=DEV)
    log_line(f"[faces memo] {name} on the device: the bad table had the freed table's address in {reused} of 8 rounds")
    assert reused >= 1, "the allocator never handed the address back: the test did not reach the case it is about"


def test_faces_are_read_once_and_never_under_capture(hip_lib, monkeypatch):
    """One read-back per tensor and version; inside a stream capture none at all, also for a tensor never seen before."""
    import point_mesh_cases as cases
    from voge_amd import Losses
    reads = []
    real_min = torch.Tensor.min
    monkeypatch.setattr(torch.Tensor, "min", lambda self, *a, **k: (reads.append(id(self)), real_min(self, *a, **k))[1])
    verts, faces = cases.level2_sphere()
    v, f = verts.to(DEV), faces.int().to(DEV)
    p = cases.points_around(verts, faces, 300, seed=3).to(DEV)
    unseen = f.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = Losses.point_mesh_face_distance(v, f, p)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert reads.count(id(f)) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = Losses.point_mesh_face_distance(v, unseen, p)
    assert id(unseen) not in reads, "a read-back inside a stream capture"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager)
    Losses.point_mesh_face_distance(v, unseen, p)      # (outside the capture it is checked, once)
    Losses.point_mesh_face_distance(v, unseen, p)
    assert reads.count(id(unseen)) == 1 and reads.count(id(f)) == 1
