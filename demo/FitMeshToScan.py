"""Fit a triangle mesh to a scanned point cloud -- no rendering involved (an extension: the reference has no such demo).

An icosphere is deformed towards the bunny's points (the centres of tests/golden/bunny_gaussians.npz, scaled into the unit
ball) with Adam on

    point_mesh_face_distance(verts, faces, points) + w_edge * edge + w_laplacian * laplacian + w_normal * normal,

the exact distance between the mesh and the cloud -- every point to its nearest triangle, every triangle to its nearest point --
plus the mesh regularisers.  Unlike a chamfer distance between surface samples the first term is 0 on a perfect fit, does not
change with a draw and pulls no vertex along the surface.  With --graph the whole iteration (both searches, the loss, the
backward, the regularisers and the Adam step) is captured once into a HIP graph and replayed: nothing in it is read back on the
host.  closest_faces scores the fit before and after: the distance from every scanned point to the mesh.  --route brute | grid
chooses the search of both (default: by the number of pairs); the two return the same bits, and both can be captured.

usage: python demo/FitMeshToScan.py [--iters 500] [--level 4] [--points 8171] [--graph] [--route grid] [--save fit.off]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from VoGE.Losses import MeshTopology, closest_faces, mesh_regularisers, point_mesh_face_distance  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WEIGHTS = {"edge": 1.0, "laplacian": 0.1, "normal": 0.01}      # PyTorch3D's mesh-fitting tutorial


def ico_sphere(level):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ShapeFitting_for_FitMeshToScan", os.path.join(ROOT, "demo", "ShapeFitting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ico_sphere(level)


def scan_points(n=None, seed=0):
    """The bunny's points [n,3] fp32 inside the unit ball (n None: all 8171)"""
    v = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))["verts"].astype(np.float64)
    v = (v - v.mean(0)) / np.abs(v - v.mean(0)).max()
    if n is not None and n < len(v):
        v = v[np.random.default_rng(seed).choice(len(v), n, replace=False)]
    return v.astype(np.float32)


def score(points, verts, faces, route=None):
    """(mean, median, largest) distance from the points to the mesh"""
    d = closest_faces(points, verts.detach(), faces, route=route)[0].sqrt()
    return float(d.mean()), float(d.median()), float(d.max())


def fit(iters=500, level=4, points=None, lr=5e-3, graph=False, device="cuda:0", quiet=False, save=None, weights=None, log_every=100,
        route=None):
    w = dict(WEIGHTS, **(weights or {}))
    sv, sf = ico_sphere(level)
    verts = torch.from_numpy(sv * np.float32(0.6)).to(device).requires_grad_(True)
    faces = torch.from_numpy(sf).to(device=device, dtype=torch.int32)
    pts = torch.from_numpy(scan_points(points)).to(device)
    topo = MeshTopology(faces=sf, device=device)
    on = tuple(k for k in w if w[k] != 0.0)
    opt = torch.optim.Adam([verts], lr=lr, capturable=bool(graph))
    losses = torch.zeros(2, device=device)

    def iteration():
        opt.zero_grad(set_to_none=True)
        dist = point_mesh_face_distance(verts, faces, pts, route=route)
        terms = dict(zip(("edge", "laplacian", "normal"), mesh_regularisers(verts, topo, terms=on)))
        reg = sum(w[k] * terms[k] for k in on)
        (dist + reg).backward()
        opt.step()
        losses.copy_(torch.stack((dist.detach(), torch.as_tensor(reg, device=device).detach())))

    before = score(pts, verts, faces, route)
    replay = iteration
    if graph:
        start = verts.detach().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):                                   # Adam's buffers, allocator pools, code objects
                iteration()
            with torch.no_grad():                                # the warm-up must not move the optimisation
                verts.copy_(start)
                for st in opt.state.values():
                    for t in st.values():
                        if torch.is_tensor(t):
                            t.zero_()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g):
            iteration()
        with torch.no_grad():                                    # (the capture launches nothing, but leaves no doubt either)
            verts.copy_(start)
            for st in opt.state.values():
                for t in st.values():
                    if torch.is_tensor(t):
                        t.zero_()
        replay = g.replay
    history = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        replay()
        if (it % log_every == 0 or it == iters - 1):
            history.append((it, *losses.tolist()))
            if not quiet:
                print(f"iteration {it:5d}: point-mesh distance {history[-1][1]:.6f}, regularisers {history[-1][2]:.6f}")
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    after = score(pts, verts, faces, route)
    if not quiet:
        for label, s in (("before", before), ("after", after)):
            print(f"closest_faces {label}: mean distance {s[0]:.5f}, median {s[1]:.5f}, largest {s[2]:.5f} ({len(pts)} points, {len(faces)} faces)")
        print(f"{iters} iterations in {sec:.2f} s ({sec / max(iters, 1) * 1e3:.3f} ms each, {'graph replay' if graph else 'eager'})")
    if save:
        from VoGE.Converter import IO
        IO.save_off(save, verts.detach().cpu().numpy(), sf)
    return {"before": before, "after": after, "history": history, "sec_per_iter": sec / max(iters, 1),
            "final_verts": verts.detach().cpu().numpy(), "faces": sf}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--points", type=int, default=None, help="a random subset of the scan (default: all 8171 points)")
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--graph", action="store_true", help="replay the iteration as a HIP graph")
    ap.add_argument("--route", choices=("brute", "grid"), default=None, help="the search of the distance term (default: by the number of pairs)")
    ap.add_argument("--save", default=None, help="write the fitted mesh as an OFF file")
    a = ap.parse_args()
    fit(iters=a.iters, level=a.level, points=a.points, lr=a.lr, graph=a.graph, save=a.save, route=a.route)
