"""A mesh of the Stanford bunny from its Gaussians (tests/golden/bunny_gaussians.npz, the ones demo/RenderBunny.py draws): depth
maps with Renderer.get_depth from views on a sphere around them, fused with Meshing.TSDFVolume.integrate, extracted with
Meshing.extract_mesh, written with save_off -- an extension, the reference has no mesh extraction.

get_depth is the distance along each pixel's UNIT ray, which is what integrate takes; pixels the silhouette covers by less than a
half are handed over as 0 ("no surface").  Neither step is differentiable: this is what one does AFTER a fit.  Prints V, F, the
Euler characteristic and the number of boundary edges (a bunny seen from a ring of views keeps holes where no view looks: under
the chin, between the ears).  --keep-largest K and / or --min-faces M run Meshing.clean_mesh on the extraction -- the floaters of a
fused volume go, the K largest components with at least M faces stay -- and print the report before and after.

--colour carries the Gaussians' colours through every step: a colour image (interpolate_attr of the colour table) is rendered beside
each depth map and fused with it (TSDFVolume(channels=3), integrate(attr=...)), extract_mesh(vol, attr=True) brings the colours to the
vertices, they follow clean_mesh through its vert_index, save_off writes them (a COFF file), and the mesh goes back into Gaussians
-- Converters.normal_mesh_converter(..., oriented=True) on Meshing.vertex_normals, the vertex colours as the colour table -- which
are rendered from the first camera: the report ends with "round trip", the mean absolute difference of that image from the first
colour image.  LAST then holds vert_attr, colour_range (the least and the greatest value of the fused images) and round_trip.

The extracted (and cleaned) mesh is then scored against the scene's own points, the Gaussians' centres, with the exact
point-to-mesh search in both roles: the mean distance from every point to the mesh (completeness: how much of the scene the mesh
covers) and from every face to its nearest point (accuracy: how far the mesh strays from the scene).  Both take route="grid",
which has no pair cap: the million faces of a 256^3 volume are scored whole, neither kept small nor sampled.  LAST holds both.

--simplify CELL runs Meshing.simplify_mesh after clean_mesh, with cells of CELL voxels and placement="quadric" (vertex clustering:
no target face count -- a count is reached by trying cell sizes -- and no promise of a manifold result); the colours go with it
through attr=.  It prints the faces before and after and the same two scores for both meshes; the simplified mesh is what is
saved and returned.  LAST then holds simplified = (F before, F after, the scores before, the scores after).

--depth-error closes the loop directly: the final mesh is rasterised under the fusion's own cameras (Meshing.rasterize_mesh, whose
depth is get_depth's) and compared with the depth maps it was fused from, pixel for pixel: per view the mean and the largest
|mesh depth - get_depth| over the pixels both cover, and the share of the pixels only one of the two covers.  LAST then holds
depth_error = [(mean, largest, share), ...].

usage: python demo/ExtractMesh.py [--resolution 128] [--views 24] [--image 256] [--out bunny_mesh.off] [--keep-largest K] [--min-faces M]
                                  [--colour] [--simplify CELL] [--depth-error]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from VoGE.Losses import closest_faces                                                  # noqa: E402
from VoGE.Converter.IO import save_off                                                 # noqa: E402
from VoGE.Meshes import GaussianMeshesNaive                                            # noqa: E402
from VoGE.Converter.Converters import normal_mesh_converter                            # noqa: E402
from VoGE.Meshing import TSDFVolume, clean_mesh, connected_components, extract_mesh, rasterize_mesh, simplify_mesh, vertex_normals    # noqa: E402
from VoGE.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_silhouette, interpolate_attr   # noqa: E402
from voge_amd.Meshes import OrientedGaussianMeshesNaive                                # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform               # noqa: E402


LAST = {}      # what the last run(colour=True) made beyond its return value


def mesh_report(verts, faces):
    """(V, F, Euler characteristic over the used vertices, boundary edges) of a triangle mesh"""
    f = faces.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * max(len(verts), 1) + e[:, 1], return_counts=True)
    used = len(np.unique(f))
    return len(verts), len(f), used - len(counts) + len(f), int((counts == 1).sum())


def score_mesh(mesh_verts, faces, points):
    """(completeness, accuracy): the mean distance from every point to the mesh and from every face to its nearest point, exact,
    by the grid route (Losses.closest_faces for the first, the node's second search for the second)"""
    from voge_amd import ops
    if len(faces) == 0 or len(points) == 0:
        return float("nan"), float("nan")
    d2 = closest_faces(points, mesh_verts, faces, route="grid")[0]
    _, _, _, point_idx, bary_f = ops.point_mesh(mesh_verts, faces.int(), points, route="grid")
    tri = mesh_verts[faces.long()]
    q = (bary_f[:, :, None] * tri).sum(1)                      # the closest point of every face to its nearest scene point
    return float(d2.sqrt().mean()), float((points[point_idx.long()] - q).norm(dim=-1).mean())


def round_trip(renderer, mesh_verts, faces, vert_attr, R, T, first, device):
    """The coloured mesh as oriented Gaussians, rendered under (R, T): the mean absolute difference from the colour image `first`"""
    normals = vertex_normals(mesh_verts, faces)
    flat = normals.norm(dim=-1) < 0.5      # (a vertex whose faces' normals cancel: any direction will do for one disc)
    normals = torch.where(flat[:, None], normals.new_tensor([0.0, 0.0, 1.0]), normals)
    gv, scales, quats = normal_mesh_converter(mesh_verts.cpu(), faces.cpu().long(), normals.cpu(), oriented=True)
    with torch.no_grad():
        frag = renderer(OrientedGaussianMeshesNaive(gv, scales, quats).to(device), R=R.to(device), T=T.to(device))
        back = interpolate_attr(frag, vert_attr.contiguous())
    return float((back - first).abs().mean())


def depth_errors(mesh_verts, faces, cameras, depths):
    """[(mean, largest |mesh depth - depth| over the pixels both cover, share of the pixels only one covers)] per view"""
    frags = rasterize_mesh(mesh_verts, faces, cameras, tuple(depths.shape[1:]))
    rows = []
    for mesh, ours, ref in zip(frags.depth, frags.pix_to_face >= 0, depths):
        theirs = ref > 0
        both = ours & theirs
        diff = (mesh - ref).abs()[both]
        rows.append((float(diff.mean()) if len(diff) else float("nan"), float(diff.max()) if len(diff) else float("nan"),
                     float((ours ^ theirs).float().mean())))
    return rows


def run(resolution=128, views=24, image=256, out="bunny_mesh.off", device="cuda:0", keep_largest=None, min_faces=None, colour=False, simplify=None,
        depth_error=False):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_gaussians.npz"))
    verts, sigmas = (torch.from_numpy(g[k]) for k in ("verts", "isigma"))
    colours = torch.from_numpy(g["colors"]).to(device) if colour else None
    meshes = GaussianMeshesNaive(verts, sigmas, None).to(device)
    focal, half = 2000.0 * image / 256, image / 2      # demo/RenderBunny.py's camera, scaled with the image
    settings = GaussianRenderSettings(image_size=(image, image), max_assign=40, absorptivity=1, principal=(half, half), inverse_sigma=False)
    cameras = PerspectiveCameras(focal_length=focal, principal_point=((half, half),), image_size=(settings['image_size'],), device=device,
                                 in_ndc=False)
    renderer = GaussianRenderer(cameras=cameras, render_settings=settings)
    azim = [360.0 * k / views for k in range(views)]
    elev = [25.0 if k % 2 == 0 else -25.0 for k in range(views)]
    R, T = look_at_view_transform([6.0] * views, elev, azim, degrees=True)
    depths, images = [], []
    with torch.no_grad():
        for k in range(views):      # one view a frame: the renderer's cameras are the frame's
            cameras.R, cameras.T = R[k:k + 1].to(device), T[k:k + 1].to(device)
            frag = renderer(meshes)
            depth = get_depth(frag, normalize=True, background=0.0)      # [1, H, W]
            depths.append(torch.where(get_silhouette(frag) > 0.5, depth, torch.zeros_like(depth)))
            if colour:
                images.append(interpolate_attr(frag, colours))      # [1, H, W, 3]
    cameras.R, cameras.T = R.to(device), T.to(device)
    vol = TSDFVolume((-0.36, -0.36, -0.36), hi=(0.36, 0.36, 0.36), resolution=resolution, device=device, channels=3 if colour else 0)
    if colour:
        images = torch.cat(images)
        vol.integrate(torch.cat(depths), cameras, trunc=4 * vol.voxel_size[0], attr=images)
        mesh_verts, faces, vert_attr = extract_mesh(vol, attr=True)
    else:
        vol.integrate(torch.cat(depths), cameras, trunc=4 * vol.voxel_size[0])
        mesh_verts, faces = extract_mesh(vol)
    V, F, chi, boundary = mesh_report(mesh_verts, faces)
    report = f"V {V}, F {F}, Euler characteristic {chi}, boundary edges {boundary}"
    print(f"bunny at {resolution}^3 from {views} views of {image}^2: {report}")
    if keep_largest is not None or min_faces is not None or colour:      # (with colours always: the vertices no face names go as well)
        before = connected_components(faces, len(mesh_verts))[2]
        mesh_verts, faces, vert_index, _ = clean_mesh(mesh_verts, faces, keep_largest=keep_largest, min_faces=1 if min_faces is None else min_faces,
                                                      return_index=True)
        if colour:
            vert_attr = vert_attr[vert_index.long()]      # the colours follow their vertices
        V, F, chi, boundary = mesh_report(mesh_verts, faces)
        report = f"V {V}, F {F}, Euler characteristic {chi}, boundary edges {boundary}"
        print(f"cleaned (keep_largest {keep_largest}, min_faces {min_faces}): {before} -> {connected_components(faces, V)[2]} components: {report}")
    if simplify is not None:
        fine = score_mesh(mesh_verts, faces, verts.to(device=device, dtype=torch.float32))
        faces_before = len(faces)
        cell = [simplify * h for h in vol.voxel_size]
        if colour:
            mesh_verts, faces, vert_attr = simplify_mesh(mesh_verts, faces, cell, placement="quadric", attr=vert_attr)
        else:
            mesh_verts, faces = simplify_mesh(mesh_verts, faces, cell, placement="quadric")
        coarse = score_mesh(mesh_verts, faces, verts.to(device=device, dtype=torch.float32))
        V, F, chi, boundary = mesh_report(mesh_verts, faces)
        report = f"V {V}, F {F}, Euler characteristic {chi}, boundary edges {boundary}"
        print(f"simplified (cells of {simplify:g} voxels, quadric placement): faces {faces_before} -> {F}: {report}; points -> mesh "
              f"{fine[0]:.5f} -> {coarse[0]:.5f}, faces -> points {fine[1]:.5f} -> {coarse[1]:.5f}")
        LAST.update(simplified=(faces_before, F, fine, coarse))
    completeness, accuracy = score_mesh(mesh_verts, faces, verts.to(device=device, dtype=torch.float32))
    report += f", points -> mesh {completeness:.5f}, faces -> points {accuracy:.5f}"
    print(f"scored against the scene's {len(verts)} points (closest_faces, route=\"grid\", {len(faces)} faces): mean distance points -> mesh "
          f"{completeness:.5f} (completeness), faces -> points {accuracy:.5f} (accuracy)")
    LAST.update(completeness=completeness, accuracy=accuracy)
    if colour:
        diff = round_trip(renderer, mesh_verts, faces, vert_attr, R[:1], T[:1], images[:1], device)
        report += f", round trip mean |dimage| {diff:.4f}"
        print(f"coloured mesh back as {len(mesh_verts)} oriented Gaussians, rendered from the first camera: round trip mean |dimage| {diff:.4f}")
        LAST.update(vert_attr=vert_attr, colour_range=(float(images.min()), float(images.max())), round_trip=diff)
    if depth_error:
        rows = depth_errors(mesh_verts, faces, cameras, torch.cat(depths))
        for k, (mean, largest, share) in enumerate(rows):
            print(f"view {k:2d}: |mesh depth - get_depth| mean {mean:.5f}, largest {largest:.5f} over the pixels both cover; "
                  f"{share * 100:.2f} % of the pixels covered by one of the two only")
        LAST.update(depth_error=rows)
    if out:
        save_off(out, mesh_verts, faces, vert_color=vert_attr if colour else None)
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
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL")
    ap.add_argument("--depth-error", action="store_true", help="rasterise the final mesh under the fusion's cameras and compare the depth maps")
    a = ap.parse_args()
    run(a.resolution, a.views, a.image, a.out, keep_largest=a.keep_largest, min_faces=a.min_faces, colour=a.colour, simplify=a.simplify,
        depth_error=a.depth_error)
