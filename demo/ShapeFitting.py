"""Multi-view shape fitting with the Gaussian renderer: the counterpart of the reference's
demo/ShapeFitting.py (BASELINE.json config 5; structure of ShapeFitting.py:125-296).

Same loop as the reference: 20 views on a spiral (`elev = linspace(0, 360)`, `azim = linspace(-180, 180)`,
dist 2.7, f = 126, 128 x 128; :125-133), an ico-sphere of level 4 (2562 vertices) converted with
`naive_vertices_converter` and only its vertices trainable (`gradianted_args=[True, False, False]`, :239),
a per-vertex colour parameter initialised to 0.5 (:242), `max_assign=25, max_point_per_bin=-1` (:226),
5 random views per iteration (:231), SGD lr 0.8 momentum 0.9 (:245), loss = silhouette MSE, plus rgb MSE
from iteration 400 on (:247,:276-277).  The edge / normal / laplacian entries of the reference's loss table
(weights 1.0 / 0 / 0.1) are never filled in its loop (:255-280); here they are off by default and --regularise adds them
(VoGE.Losses.mesh_regularisers over the sphere's faces: one autograd node, HIP kernels) with the table's weights.
--w-chamfer W (default 0: nothing is computed) adds W * chamfer_distance(vertices, ground-truth vertices), the 3-D supervision a
fit has when target points exist; it runs inside the captured iteration.  --chamfer-samples S (default 0: the vertices, as above)
puts that term on S points drawn afresh every iteration from the SURFACE of the fitted mesh and S from the ground-truth surface
(VoGE.Losses.sample_points_from_meshes, area-weighted, gradients to the three vertices of every sampled face) -- what PyTorch3D's
tutorial does: a coarse region is pulled too, and faces that cut through the target no longer score zero.

What differs, and why: the reference renders its TARGET images with PyTorch3D's mesh rasteriser from
data/cow.obj (:110-182); neither is available here, so the targets are rendered by this renderer from a
ground-truth Gaussian set (a bumpy, coloured closed surface).  There are therefore no reference numbers to
match; the run is pinned by the loss going down (tests/test_gpu_parity.py::test_shape_fitting_loop_converges)
and by the gradient checks of the kernels it uses.

usage: python demo/ShapeFitting.py [--iters 2000] [--level 4] [--size 128] [--save DIR]
                                   [--regularise [--w-edge 1.0] [--w-laplacian 0.1] [--w-normal 0.0]] [--w-chamfer 0.0 [--chamfer-samples 0]]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from VoGE.Converter import Converters                                                  # noqa: E402
from VoGE.Losses import MeshTopology, SurfaceSampler, chamfer_distance, mesh_regularisers, sample_points_from_meshes  # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_silhouette, interpolate_attr  # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform               # noqa: E402


def ico_sphere(level):
    """Unit icosphere: (verts [V,3] float32, faces [F,3] int64); level 4 has 2562 vertices
    (what pytorch3d.utils.ico_sphere(4) returns, ShapeFitting.py:216)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    verts = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = [tuple(x) for x in f]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64)


def ground_truth_shape(level):
    """The stand-in for the cow: a closed bumpy surface inside the unit ball with position-dependent colours."""
    v, f = ico_sphere(level)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    r = 0.62 + 0.16 * np.sin(3.0 * x) * np.cos(2.0 * y) + 0.12 * np.cos(4.0 * z + 1.0) * x
    verts = (v * r[:, None] * np.float32([1.0, 0.75, 1.2])).astype(np.float32)
    colors = np.stack([0.5 + 0.45 * np.sin(4 * x + 1), 0.5 + 0.45 * np.cos(3 * y), 0.5 + 0.45 * np.sin(5 * z)], -1)
    return verts, f, colors.astype(np.float32)


def make_views(num_views, dist, device):
    elev = torch.linspace(0, 360, num_views)
    azim = torch.linspace(-180, 180, num_views)
    return look_at_view_transform(dist=dist, elev=elev, azim=azim, device=device)


REGULARISER_WEIGHTS = {"edge": 1.0, "laplacian": 0.1, "normal": 0.0}      # the reference's loss table (ShapeFitting.py:247)


def regulariser_loss(verts, regularisers):
    """sum_k w_k term_k of the mesh regularisers: regularisers = {"topo": MeshTopology, "edge": w, "laplacian": w, "normal": w}
    (a missing weight is the table's); a term whose weight is 0 is not computed."""
    w = {k: float(regularisers.get(k, REGULARISER_WEIGHTS[k])) for k in REGULARISER_WEIGHTS}
    on = tuple(k for k in w if w[k] != 0.0)
    terms = dict(zip(REGULARISER_WEIGHTS, mesh_regularisers(verts, regularisers["topo"], terms=on)))
    return sum(w[k] * terms[k] for k in on)


def chamfer_loss(verts, chamfer):
    """weight * chamfer_distance of the fit against its target.  chamfer = (weight, target points [M,3]): between the vertices
    and the points; chamfer = (weight, target vertices, S, SurfaceSampler of the fit, SurfaceSampler of the target): between S
    fresh surface samples of each mesh (the target's carry no gradient)."""
    if len(chamfer) == 2:
        return chamfer[0] * chamfer_distance(verts, chamfer[1])[0]
    weight, target, S, src_sampler, tgt_sampler = chamfer
    x = sample_points_from_meshes(verts, src_sampler, S)
    with torch.no_grad():
        y = sample_points_from_meshes(target, tgt_sampler, S)
    return weight * chamfer_distance(x, y)[0]


def gauss_renderer(render, gmesh, R, T, color):
    """[H, W, 4] = interpolated colour + silhouette (ShapeFitting.py:219-222)."""
    frag = render(gmesh, R=R, T=T)
    return torch.cat((interpolate_attr(frag, color).squeeze(0), get_silhouette(frag).squeeze(0).unsqueeze(-1)), dim=-1)


class BatchedIteration:
    """One SGD iteration of the loop (ShapeFitting.py:250-296) with its `views_per_iter` views rendered as ONE batched
    renderer call: rays, trace, composite, interpolate_attr, get_silhouette, the two MSE losses, backward and the
    optimizer step are each ONE launch chain over B views instead of B chains, and -- with `graph=True` -- the whole
    iteration is captured once into a HIP graph and replayed (the views of an iteration are gathered ON THE DEVICE
    from the stacked cameras / targets by an index tensor, so nothing about an iteration depends on the host).
    The mean over a [B,H,W(,3)] batch equals the reference's sum over views of per-view means / B.
    regularisers (see regulariser_loss; default None: nothing is added) puts the weighted mesh regularisers of gsrc.verts
    into the loss, inside the same graph; chamfer = (weight, target points [M,3]) (default None) adds
    weight * chamfer_distance(gsrc.verts, target points) the same way, and the five-entry form of chamfer_loss the chamfer
    distance between fresh surface samples of both meshes (torch.rand under capture: every replay draws new samples)."""

    def __init__(self, render, gsrc, vert_color, optimizer, R_all, T_all, target_rgb, target_silhouette, views_per_iter,
                 graph=False, regularisers=None, chamfer=None):
        self.render, self.gsrc, self.vert_color, self.optimizer = render, gsrc, vert_color, optimizer
        self.regularisers, self.chamfer = regularisers, chamfer
        self.R_all, self.T_all = R_all.contiguous(), T_all.contiguous()
        self.tgt_rgb, self.tgt_sil = torch.stack(list(target_rgb)), torch.stack(list(target_silhouette))
        dev, B = self.R_all.device, views_per_iter
        self.B = B
        self.sel = torch.zeros(B, dtype=torch.long, device=dev)            # this iteration's views
        self.w_rgb = torch.zeros((), device=dev)                            # the rgb loss' weight (0 until rgb_on)
        self.losses = torch.zeros(2, device=dev)                            # (silhouette, rgb) of the last iteration
        self.graph = None
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                state = [p.detach().clone() for p in self._params()]
                for _ in range(3):                                          # momentum buffers, allocator pools, code objects
                    self._iteration()
                for p, q in zip(self._params(), state):                     # the warm-up must not move the optimisation
                    p.data.copy_(q)
                for st in optimizer.state.values():
                    if "momentum_buffer" in st and st["momentum_buffer"] is not None:
                        st["momentum_buffer"].zero_()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(self.graph):
                self._iteration()

    def _params(self):
        return [p for g in self.optimizer.param_groups for p in g["params"]]

    def _iteration(self):
        B, N = self.B, self.vert_color.shape[0]
        self.optimizer.zero_grad(set_to_none=True)
        R, T = self.R_all.index_select(0, self.sel), self.T_all.index_select(0, self.sel)
        frag = self.render(self.gsrc, R=R, T=T)
        rgb = interpolate_attr(frag, self.vert_color.repeat(B, 1))          # indices address rows b * N + n (RayTracing.py:24-30)
        sil = get_silhouette(frag)
        l_sil = ((sil - self.tgt_sil.index_select(0, self.sel)) ** 2).mean()
        l_rgb = ((rgb - self.tgt_rgb.index_select(0, self.sel)) ** 2).mean()
        loss = l_sil + self.w_rgb * l_rgb
        if self.regularisers is not None:
            loss = loss + regulariser_loss(self.gsrc.verts, self.regularisers)
        if self.chamfer is not None:
            loss = loss + chamfer_loss(self.gsrc.verts, self.chamfer)
        loss.backward()
        self.optimizer.step()
        self.losses.copy_(torch.stack((l_sil.detach(), l_rgb.detach())))

    def __call__(self, views, rgb_weight):
        """views: LongTensor [B] on the device (or a list of ints: one small host-to-device copy)."""
        if not torch.is_tensor(views):
            views = torch.tensor(views, dtype=torch.long)
        self.sel.copy_(views, non_blocking=True)
        self.w_rgb.fill_(float(rgb_weight))
        if self.graph is not None:
            self.graph.replay()
        else:
            self._iteration()
        return self.losses


def fit(iters=2000, level=4, size=128, num_views=20, views_per_iter=5, max_assign=25, rgb_on=400, seed=0,
        device="cuda:0", log_every=100, save=None, quiet=False, per_view=False, graph=False, timed_from=0, regularise=None,
        w_chamfer=0.0, chamfer_samples=0):
    """Runs the optimisation; returns {"silhouette": [...], "rgb": [...], "sec_per_iter": s}.
    per_view=True renders the views of an iteration one at a time, as the reference's loop is written (:258-259);
    the default renders them as one batch (BatchedIteration; graph=True replays the iteration as a HIP graph).
    regularise: None, or the weights {"edge": w, "laplacian": w, "normal": w} of the mesh regularisers over the sphere's faces
    (a missing one is REGULARISER_WEIGHTS').  w_chamfer: the weight of chamfer_distance(vertices, ground-truth vertices); 0 (the
    default) computes nothing.  chamfer_samples S > 0 puts that term on S fresh surface samples of both meshes instead (two
    SurfaceSamplers built once, here); 0 (the default) is the vertex form."""
    device = torch.device(device)
    rng = np.random.RandomState(seed)
    focal, pp = 126.0 * size / 128.0, (size / 2.0, size / 2.0)
    R, T = make_views(num_views, 2.7, device)
    camera = PerspectiveCameras(device=device, R=R[None, 1, ...], T=T[None, 1, ...], image_size=((size, size),),
                                principal_point=(pp,), focal_length=focal, in_ndc=False)
    settings = GaussianRenderSettings(batch_size=-1, image_size=(size, size), principal=pp, max_assign=max_assign,
                                      max_point_per_bin=-1)
    render = GaussianRenderer(cameras=camera, render_settings=settings).to(device)

    # targets: the ground-truth Gaussians seen from every view (the reference uses a mesh rasteriser here)
    gv, gf, gc = ground_truth_shape(level)
    gt = Converters.to_gaussian_meshes(Converters.naive_vertices_converter)(
        torch.from_numpy(gv), torch.from_numpy(gf), device=device, gradianted_args=[False, False, False])
    gt_color = torch.from_numpy(gc).to(device)
    with torch.no_grad():
        targets = [gauss_renderer(render, gt, R[None, j, ...], T[None, j, ...], gt_color) for j in range(num_views)]
    target_rgb = [t[..., :3] * t[..., 3:4] for t in targets]          # black background, like the reference's targets
    target_silhouette = [t[..., 3] for t in targets]

    # source: a unit sphere whose vertices (and colours) are optimised
    sv, sf = ico_sphere(level)
    gsrc = Converters.to_gaussian_meshes(Converters.naive_vertices_converter)(
        torch.from_numpy(sv), torch.from_numpy(sf), device=device, gradianted_args=[True, False, False])
    vert_color = torch.nn.Parameter(torch.ones((gsrc.verts.shape[0], 3), device=device) * 0.5, requires_grad=True)
    optimizer = torch.optim.SGD(list(gsrc.grad_parameters()) + [vert_color], lr=0.8, momentum=0.9)
    regularisers = None if regularise is None else dict(regularise, topo=MeshTopology(faces=sf, num_verts=sv.shape[0], device=device))
    chamfer = None if not w_chamfer else (float(w_chamfer), torch.from_numpy(gv).to(device))
    if chamfer is not None and chamfer_samples:
        chamfer = chamfer + (int(chamfer_samples), SurfaceSampler(sf, num_verts=sv.shape[0], device=device),
                             SurfaceSampler(gf, num_verts=gv.shape[0], device=device))
    weights = {"rgb": 0.0, "silhouette": 1.0}
    history = {"rgb": [], "silhouette": []}
    step = None if per_view else BatchedIteration(render, gsrc, vert_color, optimizer, R, T, target_rgb, target_silhouette,
                                                  views_per_iter, graph=graph, regularisers=regularisers, chamfer=chamfer)
    trace = torch.zeros((iters, 2), device=device)                     # losses stay on the device: no per-iteration sync

    # the views of every iteration, drawn up front and kept on the device: an iteration then needs nothing from the host
    # (no host-to-device copy, no synchronisation) and consecutive iterations queue back to back
    schedule = np.stack([rng.permutation(num_views)[:views_per_iter] for _ in range(max(iters, 1))])
    schedule_dev = torch.from_numpy(schedule).to(device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for i in range(iters):
        if i == timed_from and i > 0:      # (benchmarks: the first iterations settle clocks and pools, untimed)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
        if i == rgb_on:
            weights["rgb"] = 1.0
        views = schedule[i].tolist()
        if step is not None:
            trace[i].copy_(step(schedule_dev[i], weights["rgb"]))
        else:
            optimizer.zero_grad()
            loss = {k: torch.zeros((), device=device) for k in weights}
            for j in views:
                pred = gauss_renderer(render, gsrc, R[None, j, ...], T[None, j, ...], vert_color)
                loss["silhouette"] = loss["silhouette"] + ((pred[..., 3] - target_silhouette[j]) ** 2).mean() / views_per_iter
                loss["rgb"] = loss["rgb"] + ((pred[..., :3] - target_rgb[j]) ** 2).mean() / views_per_iter
            total = sum(loss[k] * weights[k] for k in weights)
            if regularisers is not None:
                total = total + regulariser_loss(gsrc.verts, regularisers)
            if chamfer is not None:
                total = total + chamfer_loss(gsrc.verts, chamfer)
            total.backward()
            optimizer.step()
            trace[i].copy_(torch.stack((loss["silhouette"].detach(), loss["rgb"].detach())))
        if not quiet and (i % log_every == 0 or i == iters - 1):
            sl, rl = trace[i].tolist()
            print(f"iter {i:5d}  silhouette {sl:.6f}  rgb {rl:.6f}", flush=True)
    torch.cuda.synchronize(device)
    history["sec_per_iter"] = (time.perf_counter() - t0) / max(iters - max(timed_from, 0), 1)
    tr = trace.cpu().numpy()
    history["silhouette"], history["rgb"] = tr[:, 0].tolist(), tr[:, 1].tolist()
    history["final_verts"] = gsrc.verts.detach().cpu().numpy()
    history["final_colors"] = vert_color.detach().cpu().numpy()
    history["sigmas"] = gsrc.sigmas.detach().cpu().numpy()
    if save:
        os.makedirs(save, exist_ok=True)
        with torch.no_grad():
            final = gauss_renderer(render, gsrc, R[None, 1, ...], T[None, 1, ...], vert_color)
        np.savez(os.path.join(save, "shape_fitting.npz"), final=final.cpu().numpy(), target=targets[1].cpu().numpy(),
                 verts=gsrc.verts.detach().cpu().numpy(), colors=vert_color.detach().cpu().numpy(),
                 silhouette_loss=np.asarray(history["silhouette"]), rgb_loss=np.asarray(history["rgb"]))
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rgb-on", type=int, default=400)
    ap.add_argument("--save", default=None)
    ap.add_argument("--per-view", action="store_true", help="one renderer call per view, as the reference's loop is written")
    ap.add_argument("--graph", action="store_true", help="replay the batched iteration as a HIP graph")
    ap.add_argument("--regularise", action="store_true", help="add the mesh regularisers (edge, laplacian, normal) to the loss")
    ap.add_argument("--w-edge", type=float, default=REGULARISER_WEIGHTS["edge"])
    ap.add_argument("--w-laplacian", type=float, default=REGULARISER_WEIGHTS["laplacian"])
    ap.add_argument("--w-normal", type=float, default=REGULARISER_WEIGHTS["normal"])
    ap.add_argument("--w-chamfer", type=float, default=0.0, help="weight of the chamfer distance to the ground-truth vertices (0: off)")
    ap.add_argument("--chamfer-samples", type=int, default=0,
                    help="with --w-chamfer: compare this many fresh surface samples of both meshes instead of the vertices (0: vertices)")
    a = ap.parse_args()
    reg = {"edge": a.w_edge, "laplacian": a.w_laplacian, "normal": a.w_normal} if a.regularise else None
    h = fit(iters=a.iters, level=a.level, size=a.size, rgb_on=a.rgb_on, save=a.save, per_view=a.per_view, graph=a.graph,
            regularise=reg, w_chamfer=a.w_chamfer, chamfer_samples=a.chamfer_samples)
    n = max(1, len(h["silhouette"]) // 20)
    print(f"silhouette loss {np.mean(h['silhouette'][:n]):.5f} -> {np.mean(h['silhouette'][-n:]):.5f}; "
          f"rgb loss {np.mean(h['rgb'][:n]):.5f} -> {np.mean(h['rgb'][-n:]):.5f}; "
          f"{h['sec_per_iter'] * 1e3:.2f} ms per iteration of 5 views ({5 / h['sec_per_iter']:.0f} frames/s fwd+bwd)")
