"""Two overlapping translucent shells of Gaussians (radii 0.85 and 1.15) fitted to the depth map of ONE shell of radius 1, with
and without Renderer.get_distortion -- an extension, the reference has no such term.

The target depth lies between the two shells, so the depth loss alone is satisfied from the start by weight smeared along the
ray: nothing pulls the shells together.  The distortion term sum_i sum_j w_i w_j |t_i - t_j| (normalize=True: of the weights
rescaled to sum to 1) does.  Printed before and after each fit: the depth error and the per-pixel spread of the ray's mass about
its own depth, sum_k w_k (t_k - D)^2 / sum_k w_k, averaged over the covered pixels.

usage: python demo/DistortionRegulariser.py [--steps 200] [--lam 0.5]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Meshes import GaussianMeshes                                                              # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_distortion      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--lam", type=float, default=0.5, help="weight of the distortion term")
a = ap.parse_args()
device = "cuda:0"
H = W = 96
K = 24


def shell(radius, n=1500):
    """n points spread evenly over a sphere (a Fibonacci lattice)."""
    i = np.arange(n) + 0.5
    z, phi = 1 - 2 * i / n, i * math.pi * (3 - math.sqrt(5))
    r = np.sqrt(1 - z * z)
    return torch.tensor(radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], -1), dtype=torch.float32)


def sigmas(n, footprint=0.09):      # (the inverse-variance scale of scenes.random_gaussians for a Gaussian of that radius)
    return torch.full((n,), 2 * math.log(1 / 0.6) / footprint ** 2, dtype=torch.float32)


cameras = PerspectiveCameras(focal_length=110.0, principal_point=((W / 2, H / 2),), image_size=((H, W),), device=device)
renderer = GaussianRenderer(cameras, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(device)
R, T = look_at_view_transform(dist=3.5, elev=10.0, azim=30.0, device=device)


def spread(frag, depth):
    w, t = frag.vert_weight, frag.vert_hit_length
    live = torch.arange(K, device=device) < frag.valid_num[..., None]
    w = torch.where(live, w, torch.zeros_like(w))
    d2 = torch.where(live, (t - depth[..., None]) ** 2, torch.zeros_like(t))
    s = w.sum(-1)
    return ((w * d2).sum(-1) / s.clamp(min=1e-12))[s > 0].mean().item()


with torch.no_grad():
    one = shell(1.0)
    target = get_depth(renderer(GaussianMeshes(one, sigmas(len(one))).to(device), R=R, T=T))
    covered = target > 0
start = torch.cat([shell(0.85), shell(1.15)])
for lam in (0.0, a.lam):
    gm = GaussianMeshes(start.clone(), sigmas(len(start)), gradianted_args=[True, False, False]).to(device)
    opt = torch.optim.Adam([gm.verts], lr=2e-3)
    for it in range(a.steps + 1):
        frag = renderer(gm, R=R, T=T)
        depth = get_depth(frag)
        err = (((depth - target) ** 2) * covered).sum() / covered.sum()
        if it in (0, a.steps):
            with torch.no_grad():
                print(f"lambda = {lam:4.2f}  step {it:4d}: depth error {err.item():.3e}, spread of the mass along the ray {spread(frag, depth):.3e}")
        if it == a.steps:
            break
        loss = err + lam * get_distortion(frag, normalize=True).mean() if lam > 0 else err
        opt.zero_grad()
        loss.backward()
        opt.step()
