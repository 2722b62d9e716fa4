"""Fit a triangle mesh to depth maps (an extension: the reference has no such demo).

A few depth maps of the Stanford bunny's Gaussians are rendered with Renderer.get_depth (demo/ExtractMesh.py's cameras); an
icosphere inside the bunny is then deformed with Adam on

    mean |rasterize_mesh(verts, faces, cameras).depth - get_depth| over the pixels both cover
        + w_edge * edge + w_laplacian * laplacian + w_normal * normal.

Meshing.rasterize_mesh speaks get_depth's convention -- the distance along the unit pixel ray -- so the two maps are compared as
they are; its depth is differentiable to the vertices (one face a pixel, no soft silhouette: a pixel pulls the three corners of
the face it sees along its ray).  The brute route is two launches with nothing read back, so with --graph the whole iteration
(rasterisation, loss, both backwards, the regularisers and the Adam step) is captured once into a HIP graph and replayed.

usage: python demo/FitMeshToDepth.py [--iters 300] [--level 4] [--views 6] [--image 128] [--graph] [--save fit.off]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Losses import MeshTopology, mesh_regularisers                               # noqa: E402
from VoGE.Meshes import GaussianMeshesNaive                                            # noqa: E402
from VoGE.Meshing import rasterize_mesh                                                # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_silhouette   # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform               # noqa: E402

WEIGHTS = {"edge": 1.0, "laplacian": 0.1, "normal": 0.01}      # PyTorch3D's mesh-fitting tutorial


def ico_sphere(level):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ShapeFitting_for_FitMeshToDepth", os.path.join(ROOT, "demo", "ShapeFitting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ico_sphere(level)


def target_depths(views, image, device):
    """(depth [views,image,image] -- 0 where the silhouette covers less than half a pixel --, cameras of all the views)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
    meshes = GaussianMeshesNaive(torch.from_numpy(g["verts"]), torch.from_numpy(g["isigma"]), None).to(device)
    focal, half = 2000.0 * image / 256, image / 2
    settings = GaussianRenderSettings(image_size=(image, image), max_assign=40, absorptivity=1, principal=(half, half), inverse_sigma=False)
    cameras = PerspectiveCameras(focal_length=focal, principal_point=((half, half),), image_size=(settings['image_size'],), device=device,
                                 in_ndc=False)
    renderer = GaussianRenderer(cameras=cameras, render_settings=settings)
    R, T = look_at_view_transform([6.0] * views, [25.0 if k % 2 == 0 else -25.0 for k in range(views)], [360.0 * k / views for k in range(views)],
                                  degrees=True)
    depths = []
    with torch.no_grad():
        for k in range(views):
            cameras.R, cameras.T = R[k:k + 1].to(device), T[k:k + 1].to(device)
            frag = renderer(meshes)
            depth = get_depth(frag, normalize=True, background=0.0)
            depths.append(torch.where(get_silhouette(frag) > 0.5, depth, torch.zeros_like(depth)))
    cameras.R, cameras.T = R.to(device), T.to(device)
    return torch.cat(depths), cameras


def fit(iters=300, level=4, views=6, image=128, lr=2e-3, radius=0.12, graph=False, device="cuda:0", quiet=False, save=None, weights=None,
        log_every=50):
    w = dict(WEIGHTS, **(weights or {}))
    target, cameras = target_depths(views, image, device)
    seen = target > 0
    sv, sf = ico_sphere(level)
    verts = torch.from_numpy(sv * np.float32(radius)).to(device).requires_grad_(True)
    faces = torch.from_numpy(sf).to(device=device, dtype=torch.int32)
    topo = MeshTopology(faces=sf, device=device)
    on = tuple(k for k in w if w[k] != 0.0)
    opt = torch.optim.Adam([verts], lr=lr, capturable=bool(graph))
    losses = torch.zeros(3, device=device)

    def iteration():
        opt.zero_grad(set_to_none=True)
        frags = rasterize_mesh(verts, faces, cameras, (image, image), route="brute")
        both = (frags.pix_to_face >= 0) & seen
        err = torch.where(both, (frags.depth - target).abs(), torch.zeros_like(target)).sum() / both.sum().clamp(min=1)
        terms = dict(zip(("edge", "laplacian", "normal"), mesh_regularisers(verts, topo, terms=on)))
        reg = sum(w[k] * terms[k] for k in on)
        (err + reg).backward()
        opt.step()
        losses.copy_(torch.stack((err.detach(), torch.as_tensor(reg, device=device).detach(), both.float().mean())))

    def reset(start):
        with torch.no_grad():
            verts.copy_(start)
            for st in opt.state.values():
                for t in st.values():
                    if torch.is_tensor(t):
                        t.zero_()

    replay = iteration
    if graph:
        start = verts.detach().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):                                   # Adam's buffers, allocator pools, code objects
                iteration()
            reset(start)                                         # the warm-up must not move the optimisation
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g):
            iteration()
        reset(start)
        replay = g.replay
    history = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        replay()
        if it % log_every == 0 or it == iters - 1:
            history.append((it, *losses.tolist()))
            if not quiet:
                print(f"iteration {it:5d}: mean |depth error| {history[-1][1]:.6f} over {history[-1][3] * 100:.1f} % of the pixels, "
                      f"regularisers {history[-1][2]:.6f}")
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    if not quiet:
        print(f"{iters} iterations in {sec:.2f} s ({sec / max(iters, 1) * 1e3:.3f} ms each, {'graph replay' if graph else 'eager'}); "
              f"{views} views of {image}^2, {len(faces)} faces")
    if save:
        from VoGE.Converter import IO
        IO.save_off(save, verts.detach().cpu().numpy(), sf)
    return {"history": history, "sec_per_iter": sec / max(iters, 1), "final_verts": verts.detach().cpu().numpy(), "faces": sf,
            "target_covered": float(seen.float().mean()), "replay": replay}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--graph", action="store_true", help="replay the iteration as a HIP graph")
    ap.add_argument("--save", default=None, help="write the fitted mesh as an OFF file")
    a = ap.parse_args()
    fit(iters=a.iters, level=a.level, views=a.views, image=a.image, lr=a.lr, graph=a.graph, save=a.save)
