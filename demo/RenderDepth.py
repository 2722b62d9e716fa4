"""Depth map of the Stanford bunny (the Gaussians of demo/RenderBunny.py: tests/golden/bunny_gaussians.npz, f = 2000, 256 x 256,
max_assign = 40, look_at(6, 0, 10)) with Renderer.get_depth -- an extension, the reference has no depth output.

get_depth is the expected hit distance along each pixel's UNIT ray from the camera centre, sum_k w_k len_k / sum_k w_k, and
`background` where nothing was hit.  `--z` turns it into view-space z by the ray's cosine to the view axis.  The map goes to
PREFIX.npy, and to PREFIX.png (near = bright, background black) when PIL is present.

usage: python demo/RenderDepth.py [--out PREFIX] [--z] [--raw]      (--raw: the un-normalised sum, normalize=False)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Meshes import GaussianMeshesNaive                                            # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_silhouette   # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform, pixel_rays   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="bunny_depth")
ap.add_argument("--z", action="store_true", help="view-space z instead of the distance along the ray")
ap.add_argument("--raw", action="store_true", help="the accumulated sum_k w_k len_k (normalize=False)")
a = ap.parse_args()
device = "cuda:0"
g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
verts, sigmas = (torch.from_numpy(g[k]) for k in ("verts", "isigma"))
meshes = GaussianMeshesNaive(verts, sigmas, None).to(device)
settings = GaussianRenderSettings(image_size=(256, 256), max_assign=40, absorptivity=1, principal=(128, 128), inverse_sigma=False)
cameras = PerspectiveCameras(focal_length=2000.0, principal_point=((128, 128),), image_size=(settings['image_size'],), device=device,
                             in_ndc=False)
renderer = GaussianRenderer(cameras=cameras, render_settings=settings)
R, T = look_at_view_transform([6], [0], [10], degrees=True)
cameras.R, cameras.T = R.to(device), T.to(device)
with torch.no_grad():
    frag = renderer(meshes)
    depth = get_depth(frag, normalize=not a.raw, background=0.0)      # [1, H, W]; weights, depth and silhouette in one launch
    hit = get_silhouette(frag) > 0                                    # (free after get_depth)
    if a.z:
        rays, _ = pixel_rays(cameras, settings['image_size'])          # unit directions, world space [1, H, W, 3]
        axis = cameras.R.to(torch.float32)[:, :, 2]                     # the view axis in world space (row-vector convention)
        depth = depth * (rays * axis[:, None, None, :]).sum(-1)
arr, mask = depth[0].cpu().numpy(), hit[0].cpu().numpy()
np.save(a.out + ".npy", arr)
near, far = float(arr[mask].min()), float(arr[mask].max())
print("depth", arr.shape, f"covered pixels {int(mask.sum())}, nearest {near:.4f}, farthest {far:.4f} ->", a.out + ".npy")
try:
    from PIL import Image
    shade = np.where(mask, 255.0 - 215.0 * (arr - near) / max(far - near, 1e-12), 0.0)
    Image.fromarray(shade.astype(np.uint8)).save(a.out + ".png")
    print("->", a.out + ".png")
except ImportError:
    pass
