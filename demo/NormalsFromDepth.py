"""Diffuse shading WITHOUT a mesh: normals from the rendered depth map (Renderer.get_normals, an extension -- the reference has
neither a depth nor a normal output).

demo/LightDiffusion.py can shade the bunny because the mesh comes with faces and per-vertex normals to interpolate.  A point
cloud, a fitted or an oriented set of Gaussians has none, and the Gaussians cannot supply one: at a slot's hit point, the density
maximum along the ray, the density gradient is perpendicular to the ray.  What can be shaded is the RENDERED surface:

    frag = renderer(meshes);  depth = get_depth(frag);  normals = get_normals(depth, cameras, edge=0.01)

-- finite differences of the back-projected depth map, cut where the depth jumps by more than 1 % between neighbours (0.06 at
distance 6, twenty pixel footprints: the ears against the body), facing the camera.  The bunny's Gaussians only are used (tests/golden/bunny_gaussians.npz: f = 2000, 256 x 256,
max_assign = 40, look_at(6, 0, 10)), lit by demo/LightDiffusion.py's directional light and diffuse term.  The image goes to
PREFIX.npy and, when PIL is present, PREFIX.png.  As a sanity value the script also prints the median angle between these
normals and the ones interpolate_attr gives from the mesh's vertex normals, over the pixels where both exist.

usage: python demo/NormalsFromDepth.py [--out PREFIX] [--edge 0.01] [--coverage 0.5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Meshes import GaussianMeshesNaive                                            # noqa: E402
from VoGE.Renderer import (GaussianRenderer, GaussianRenderSettings, get_depth, get_normals, get_silhouette,  # noqa: E402
                           interpolate_attr)
from voge_amd.cameras import PerspectiveCameras, camera_position_from_spherical_angles, look_at_view_transform  # noqa: E402


def vertex_normals(verts, faces):
    """Unit vertex normals: the area-weighted sum of the adjacent faces' normals (for the comparison only)."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, f[:, c], fn)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)).astype(np.float32)


def diffuse(normals_map, direction, color):
    """colour * max(<n, l>, 0) with n and l normalised (demo/LightDiffusion.py's diffuse term)."""
    n = torch.nn.functional.normalize(normals_map, p=2, dim=-1, eps=1e-6)
    l = torch.nn.functional.normalize(direction, p=2, dim=-1, eps=1e-6)
    return color * torch.relu((n * l).sum(-1))[..., None]


def run(out=None, edge=0.01, coverage=0.5, device="cuda:0", log=print):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
    meshes = GaussianMeshesNaive(torch.from_numpy(g["verts"]), torch.from_numpy(g["isigma"]), None).to(device)
    settings = GaussianRenderSettings(image_size=(256, 256), max_assign=40, absorptivity=1, principal=(128, 128), inverse_sigma=False)
    cameras = PerspectiveCameras(focal_length=2000.0, principal_point=((128, 128),), image_size=(settings['image_size'],),
                                 device=device, in_ndc=False)
    renderer = GaussianRenderer(cameras=cameras, render_settings=settings)
    R, T = look_at_view_transform([6], [0], [10], degrees=True)
    cameras.R, cameras.T = R.to(device), T.to(device)
    with torch.no_grad():
        frag = renderer(meshes)
        depth = get_depth(frag, background=0.0)                          # [1, H, W]: distance along the unit ray, 0 where nothing was hit
        covered = get_silhouette(frag) > coverage                         # (free after get_depth)
        depth = torch.where(covered, depth, torch.zeros_like(depth))      # the thin rim of half-covered pixels is no surface
        normals = get_normals(depth, cameras, edge=edge)                  # [1, H, W, 3], one launch; (0, 0, 0) where undefined
        direction = camera_position_from_spherical_angles(1, 30 + abs(100 - 5) * 0.5, 10, device=device)
        img = diffuse(normals, direction, torch.ones((1, 3), device=device))
        # the sanity value: against the mesh's interpolated vertex normals, which this path never saw
        mesh_map = interpolate_attr(frag, torch.from_numpy(vertex_normals(g["verts"], g["faces"])).to(device))
        both = (normals.abs().sum(-1) > 0) & (mesh_map.norm(dim=-1) > 0.5) & covered
        cos = (normals * torch.nn.functional.normalize(mesh_map, dim=-1)).sum(-1)[both].clamp(-1, 1)
        angle = float(torch.rad2deg(torch.acos(cos)).median()) if int(both.sum()) else float("nan")
    defined = int((normals.abs().sum(-1) > 0).sum())
    log(f"normals from depth: {defined} of {int(covered.sum())} covered pixels have a normal, lit pixels "
        f"{100 * float((img[0].sum(-1) > 0).float().mean()):.1f} %, median angle to the mesh's interpolated normals {angle:.2f} deg over "
        f"{int(both.sum())} pixels")
    if out:
        np.save(out + ".npy", img[0].cpu().numpy())
        try:
            from PIL import Image
            Image.fromarray((img[0].clamp(0, 1) * 255).cpu().numpy().astype(np.uint8)).save(out + ".png")
        except ImportError:
            pass
    return {"image": img, "normals": normals, "depth": depth, "median_angle_deg": angle, "defined": defined}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bunny_normals")
    ap.add_argument("--edge", type=float, default=0.01)
    ap.add_argument("--coverage", type=float, default=0.5)
    a = ap.parse_args()
    run(a.out, a.edge, a.coverage)
