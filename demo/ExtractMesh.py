"""A mesh of the Stanford bunny from its Gaussians (tests/golden/bunny_gaussians.npz, the ones demo/RenderBunny.py draws): depth
maps with Renderer.get_depth from views on a sphere around them, fused with Meshing.TSDFVolume.integrate, extracted with
Meshing.extract_mesh, written with save_off -- an extension, the reference has no mesh extraction.

get_depth is the distance along each pixel's UNIT ray, which is what integrate takes; pixels the silhouette covers by less than a
half are handed over as 0 ("no surface").  Neither step is differentiable: this is what one does AFTER a fit.  Prints V, F, the
Euler characteristic and the number of boundary edges (a bunny seen from a ring of views keeps holes where no view looks: under
the chin, between the ears).  --keep-largest K and / or --min-faces M run Meshing.clean_mesh on the extraction -- the floaters of a
fused volume go, the K largest components with at least M faces stay -- and print the report before and after.

usage: python demo/ExtractMesh.py [--resolution 128] [--views 24] [--image 256] [--out bunny_mesh.off] [--keep-largest K] [--min-faces M]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Converter.IO import save_off                                                 # noqa: E402
from VoGE.Meshes import GaussianMeshesNaive                                            # noqa: E402
from VoGE.Meshing import TSDFVolume, clean_mesh, connected_components, extract_mesh    # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_silhouette   # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform               # noqa: E402


def mesh_report(verts, faces):
    """(V, F, Euler characteristic over the used vertices, boundary edges) of a triangle mesh"""
    f = faces.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * max(len(verts), 1) + e[:, 1], return_counts=True)
    used = len(np.unique(f))
    return len(verts), len(f), used - len(counts) + len(f), int((counts == 1).sum())


def run(resolution=128, views=24, image=256, out="bunny_mesh.off", device="cuda:0", keep_largest=None, min_faces=None):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
    verts, sigmas = (torch.from_numpy(g[k]) for k in ("verts", "isigma"))
    meshes = GaussianMeshesNaive(verts, sigmas, None).to(device)
    focal, half = 2000.0 * image / 256, image / 2      # demo/RenderBunny.py's camera, scaled with the image
    settings = GaussianRenderSettings(image_size=(image, image), max_assign=40, absorptivity=1, principal=(half, half), inverse_sigma=False)
    cameras = PerspectiveCameras(focal_length=focal, principal_point=((half, half),), image_size=(settings['image_size'],), device=device,
                                 in_ndc=False)
    renderer = GaussianRenderer(cameras=cameras, render_settings=settings)
    azim = [360.0 * k / views for k in range(views)]
    elev = [25.0 if k % 2 == 0 else -25.0 for k in range(views)]
    R, T = look_at_view_transform([6.0] * views, elev, azim, degrees=True)
    depths = []
    with torch.no_grad():
        for k in range(views):      # one view a frame: the renderer's cameras are the frame's
            cameras.R, cameras.T = R[k:k + 1].to(device), T[k:k + 1].to(device)
            frag = renderer(meshes)
            depth = get_depth(frag, normalize=True, background=0.0)      # [1, H, W]
            depths.append(torch.where(get_silhouette(frag) > 0.5, depth, torch.zeros_like(depth)))
    cameras.R, cameras.T = R.to(device), T.to(device)
    vol = TSDFVolume((-0.36, -0.36, -0.36), hi=(0.36, 0.36, 0.36), resolution=resolution, device=device)
    vol.integrate(torch.cat(depths), cameras, trunc=4 * vol.voxel_size[0])
    mesh_verts, faces = extract_mesh(vol)
    V, F, chi, boundary = mesh_report(mesh_verts, faces)
    report = f"V {V}, F {F}, Euler characteristic {chi}, boundary edges {boundary}"
    print(f"bunny at {resolution}^3 from {views} views of {image}^2: {report}")
    if keep_largest is not None or min_faces is not None:
        before = connected_components(faces, len(mesh_verts))[2]
        mesh_verts, faces = clean_mesh(mesh_verts, faces, keep_largest=keep_largest, min_faces=1 if min_faces is None else min_faces)
        V, F, chi, boundary = mesh_report(mesh_verts, faces)
        report = f"V {V}, F {F}, Euler characteristic {chi}, boundary edges {boundary}"
        print(f"cleaned (keep_largest {keep_largest}, min_faces {min_faces}): {before} -> {connected_components(faces, V)[2]} components: {report}")
    if out:
        save_off(out, mesh_verts, faces)
        print("->", out)
    return mesh_verts, faces, report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--out", default="bunny_mesh.off")
    ap.add_argument("--keep-largest", type=int, default=None)
    ap.add_argument("--min-faces", type=int, default=None)
    a = ap.parse_args()
    run(a.resolution, a.views, a.image, a.out, keep_largest=a.keep_largest, min_faces=a.min_faces)
