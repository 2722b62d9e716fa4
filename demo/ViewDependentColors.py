"""View-dependent colours fitted by gradient descent (no counterpart in the reference, which has one colour per Gaussian).

The Stanford bunny's Gaussians (tests/golden/bunny_gaussians.npz, the scene of demo/RenderBunny.py: f = 2000, 256 x 256,
max_assign = 40, distance 6) get a fixed random "ground truth" of degree-2 spherical-harmonic colour coefficients -- the
constant term from the bunny's own colours, the eight direction-dependent terms ~ N(0, 0.3^2) -- and are rendered from eight
views around the object in ONE batch.  A second set of coefficients, started at zero (mid-grey from everywhere), is then
fitted to those eight images with Adam through
    renderer -> sh_to_colors -> to_white_background
with the geometry fixed: the [8 * N, 3] table of per-view colours comes from one HIP launch, and its gradient goes back to the
[N, 9, 3] coefficients in one more.  The camera centres are computed once, in front of the loop.

usage: python demo/ViewDependentColors.py [--iters 300] [--degree 2] [--save DIR]      (--save: PNGs of view 0, needs PIL)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Meshes import GaussianMeshesNaive                                                            # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, sh_to_colors, to_white_background  # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform                               # noqa: E402

VIEWS = 8
Y0 = 0.28209479177387814      # the constant basis function: colour = Y0 * sh[:, 0] + 0.5 when nothing else is set


def save_png(img, path):
    from PIL import Image
    a = img.clamp(min=0, max=1)[0, ..., :3].detach().cpu().numpy() * 255
    Image.fromarray(a.astype(np.uint8)).save(path)


def run(iters=300, degree=2, device="cuda", save=None, log=print):
    """-> {"loss": [...], "sh": the fitted coefficients [N, (degree+1)^2, 3], "sh_true": the ground truth, "sec_per_iter": s}"""
    size = (256, 256)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
    verts, sigmas, base = (torch.from_numpy(g[k]).to(device) for k in ("verts", "isigma", "colors"))
    N, M = verts.shape[0], (degree + 1) ** 2
    rng = np.random.default_rng(7)
    sh_true = torch.from_numpy(rng.normal(0.0, 0.3, (N, M, 3)).astype(np.float32)).to(device)
    sh_true[:, 0] = (base - 0.5) / Y0
    R, T = look_at_view_transform(dist=[6.0] * VIEWS, elev=[20.0 * (-1) ** i for i in range(VIEWS)],
                                  azim=[10.0 + 360.0 * i / VIEWS for i in range(VIEWS)], device=device)
    cams = PerspectiveCameras(focal_length=2000.0, principal_point=((128, 128),), image_size=(size,), device=device, R=R, T=T)
    settings = GaussianRenderSettings(image_size=size, max_assign=40, absorptivity=1, principal=(128, 128), inverse_sigma=False)
    renderer = GaussianRenderer(cameras=cams, render_settings=settings).to(device)
    meshes = GaussianMeshesNaive(verts, sigmas, None)
    centres = cams.get_camera_center()      # (once: the cameras do not move)

    def images(sh):
        return to_white_background(renderer(meshes, R=R, T=T), sh_to_colors(sh, verts, centres, degree=degree))

    with torch.no_grad():
        target = images(sh_true)
    sh = torch.zeros_like(sh_true, requires_grad=True)
    opt = torch.optim.Adam([sh], lr=0.05)
    if save:
        os.makedirs(save, exist_ok=True)
        with torch.no_grad():
            save_png(target, os.path.join(save, "target.png"))
            save_png(images(sh), os.path.join(save, "before.png"))
    losses = []
    warm = min(10, iters // 2)      # (the first iterations load the library and make the first allocations: not timed)
    t_start = time.perf_counter()
    for it in range(iters):
        if it == warm:
            torch.cuda.synchronize()
            t_start = time.perf_counter()
        loss = torch.nn.functional.mse_loss(images(sh), target)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach())
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t_start) / max(iters - warm, 1)
    losses = [float(x) for x in losses]
    log(f"{VIEWS} views of {N} Gaussians, degree {degree}: {iters} iterations, {sec * 1e3:.2f} ms each: image loss {losses[0]:.5f} -> "
        f"{losses[-1]:.2e} ({100 * losses[-1] / losses[0]:.2f} % of the start)")
    if save:
        with torch.no_grad():
            save_png(images(sh), os.path.join(save, "after.png"))
    return {"loss": losses, "sh": sh.detach(), "sh_true": sh_true, "sec_per_iter": sec}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--save", default=None)
    a = ap.parse_args()
    run(a.iters, degree=a.degree, save=a.save)
