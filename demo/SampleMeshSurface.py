"""Mesh surface -> points with normals -> oriented Gaussians (an extension; the reference has no counterpart).

Samples the ground-truth shape of demo/ShapeFitting.py with VoGE.Losses.sample_points_from_meshes (area-weighted, with the face
normals), turns the samples into oriented Gaussians with Converters.point_cloud_converter(oriented=True) -- discs flattened along
the local PCA normal of the cloud -- and renders them.  Printed: how well the PCA normals of the cloud agree with the normals of
the faces the points were drawn from (mean |cos|), and the share of covered pixels.

usage: python demo/SampleMeshSurface.py [--samples 20000] [--level 4] [--size 256] [--out PREFIX]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ShapeFitting import ground_truth_shape                                               # noqa: E402
from VoGE import Aggregation                                                              # noqa: E402
from VoGE.Converter import Converters                                                     # noqa: E402
from VoGE.Losses import SurfaceSampler, sample_points_from_meshes                         # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, to_white_background   # noqa: E402
from voge_amd.Meshes import OrientedGaussianMeshes                                       # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform                   # noqa: E402


def run(samples=20000, level=4, size=256, out=None, device="cuda", seed=0, log=print):
    gv, gf, _ = ground_truth_shape(level)
    verts = torch.from_numpy(gv).to(device)
    sampler = SurfaceSampler(gf, num_verts=gv.shape[0], device=device)
    gen = torch.Generator(device=device).manual_seed(seed)
    points, normals, face_idx, bary = sample_points_from_meshes(verts, sampler, samples, return_normals=True, generator=gen,
                                                                return_faces=True)
    R, T = look_at_view_transform(2.7, 10, 30, device=device)
    eye = -torch.matmul(R[0], T[0])                                                       # the camera centre: the discs face it
    pts, scales, quats = Converters.point_cloud_converter(points, percentage=0.75, oriented=True, toward=eye)
    pca = Aggregation.quaternion_to_matrix(quats)[..., 2]                                 # the third axis of R(q): the PCA normal
    agree = float((pca * normals).sum(-1).abs().mean())
    colors = (0.5 + 0.5 * normals).clamp(0, 1)                                            # coloured by the sampled normal
    focal = 126.0 * size / 128.0
    cameras = PerspectiveCameras(focal_length=focal, principal_point=((size / 2, size / 2),), image_size=((size, size),),
                                 device=device, in_ndc=False)
    renderer = GaussianRenderer(cameras=cameras, render_settings=GaussianRenderSettings(image_size=(size, size),
                                                                                         principal_point=(size / 2, size / 2)))
    with torch.no_grad():
        frag = renderer(OrientedGaussianMeshes(pts, scales, quats).to(device), R=R, T=T)
        img = to_white_background(frag, colors).clamp(0, 1).squeeze(0)
    covered = float((frag.valid_num > 0).float().mean())
    log(f"{samples} samples of {gf.shape[0]} faces ({int(torch.unique(face_idx).numel())} of them hit): PCA normals agree with the "
        f"faces' to a mean |cos| of {agree:.4f}; {size} x {size}: {covered * 100:.1f} % of the pixels covered")
    if out:
        np.save(out + ".npy", img.cpu().numpy())
    return {"image": img, "points": points, "normals": normals, "face_idx": face_idx, "bary": bary, "agree": agree, "covered": covered}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.samples, a.level, a.size, a.out)
