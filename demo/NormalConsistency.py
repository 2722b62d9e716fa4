"""Flat oriented Gaussians on a tilted plane patch, their orientations fitted with the normal-consistency term of 2D Gaussian
splatting -- Renderer.gaussian_normals and get_rendered_normals, extensions the reference has no counterpart of.

The centres lie on the plane and stay fixed; every Gaussian is a disc five times thinner along its axis 0 than across, and starts
tilted away from the plane's normal by 10 to 35 degrees about a random axis.  The loss is 1 - n_rendered . n_depth, averaged over
the pixels where both normals exist: n_rendered = normalise(sum_k w_k n_k) of the Gaussians' own normals
(get_rendered_normals(fragments, gaussian_normals(...))) and n_depth the normal of the rendered depth
(get_normals(get_depth(fragments), cameras)).  The discs overlap, so the rendered depth blends several of them and follows the
plane through their centres; the term turns each disc towards it.  Only the quaternions are optimised (Adam).  Printed: the loss
and the mean angle between the Gaussians' normals and the plane's normal, before and after.

usage: python demo/NormalConsistency.py [--steps 200]"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Meshes import OrientedGaussianMeshes                                                                     # noqa: E402
from VoGE.Renderer import (GaussianRenderer, GaussianRenderSettings, gaussian_normals, get_depth, get_normals,   # noqa: E402
                           get_rendered_normals)
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform                                           # noqa: E402


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) quaternions [.., 4]: the rotation b followed by the rotation a."""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def plane_scene(side, seed, normal=(0.35, 0.25, 1.0), extent=0.8, overlap=1.6, thin=5.0):
    """side x side discs on the plane through the origin with that normal -> verts [N,3], scales [N,3] (axis 0 the thin one:
    renderer with inverse_sigma=False, where a LARGER scale is a thinner extent), quats [N,4] tilted off the plane, the normal."""
    rng = np.random.default_rng(seed)
    p = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    e1 = np.cross(p, (0.0, 1.0, 0.0))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(p, e1)
    u = np.linspace(-extent, extent, side)
    verts = (u[:, None, None] * e1 + u[None, :, None] * e2).reshape(-1, 3)
    N = len(verts)
    footprint = overlap * (u[1] - u[0])
    s = 2 * math.log(1 / 0.6) / footprint ** 2      # (the inverse-variance scale of scenes.random_gaussians for that radius)
    scales = np.tile([s * thin * thin, s, s], (N, 1))
    a = np.array([1.0, 0.0, 0.0])      # the rotation that takes axis 0 to the plane's normal ...
    on_plane = np.concatenate([[1 + a @ p], np.cross(a, p)])
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = np.deg2rad(rng.uniform(10.0, 35.0, (N, 1))) / 2      # ... followed by a tilt of 10 to 35 degrees about a random axis
    quats = quat_mul(np.concatenate([np.cos(half), np.sin(half) * axis], -1), on_plane[None])
    return verts.astype(np.float32), scales.astype(np.float32), quats.astype(np.float32), p.astype(np.float32)


def run(iters=200, size=96, side=16, K=12, lr=0.02, seed=0, device="cuda:0", log=print):
    verts, scales, quats, p = plane_scene(side, seed)
    cameras = PerspectiveCameras(focal_length=1.5 * size, principal_point=((size / 2, size / 2),), image_size=((size, size),),
                                 device=device)
    R, T = look_at_view_transform(dist=3.0, elev=0.0, azim=0.0, device=device)
    cameras.R, cameras.T = R, T
    renderer = GaussianRenderer(cameras, GaussianRenderSettings(image_size=(size, size), max_assign=K, max_point_per_bin=-1,
                                                                inverse_sigma=False)).to(device)
    gm = OrientedGaussianMeshes(torch.from_numpy(verts), torch.from_numpy(scales), torch.from_numpy(quats),
                                gradianted_args=[False, False, True]).to(device)
    centres = cameras.get_camera_center()      # (fixed cameras: computed once)
    plane = torch.from_numpy(p).to(device)
    plane = torch.where((plane * (0 - centres[0])).sum() > 0, -plane, plane)      # the side that faces the camera
    opt = torch.optim.Adam([gm.quats], lr=lr)

    def step():
        table = gaussian_normals(gm.scales, gm.quats, gm.verts, centres)      # [N, 3], one launch
        frag = renderer(gm, R=R, T=T)
        n_depth = get_normals(get_depth(frag), cameras)
        n_hat = get_rendered_normals(frag, table)
        both = (n_hat != 0).any(-1) & (n_depth != 0).any(-1)
        loss = (1 - (n_hat * n_depth).sum(-1))[both].mean()
        with torch.no_grad():
            angle = torch.rad2deg(torch.acos((table * plane).sum(-1).clamp(-1, 1))).mean()
        return loss, float(angle)

    losses, angles = [], []
    for it in range(iters + 1):
        loss, angle = step()
        losses.append(float(loss.detach()))
        angles.append(angle)
        if it in (0, iters):
            log(f"step {it:4d}: normal-consistency loss {losses[-1]:.4e}, mean angle to the plane's normal {angle:.2f} deg")
        if it == iters:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return dict(loss=np.array(losses), angle=np.array(angles))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    run(iters=ap.parse_args().steps)
