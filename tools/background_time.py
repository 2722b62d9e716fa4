"""Frame time of to_colored_background at cfg3 (50k Gaussians, 512^2, K = 40; forward + backward of img.sum()) for three
backgrounds: the constant colour (the one-pass route), a per-pixel [1,512,512,3] image and a learnable [3] colour (both
through interpolate_attr + get_silhouette + voge_blend_bg_fwd / _bwd).  Each variant eager and replayed from a captured graph;
times from device events around `steps` frames, the median of `reps` windows.
usage: python tools/background_time.py [steps] [reps]      (--ktrace: only run each variant eagerly, for rocprofv3)"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from voge_amd import scenes      # noqa: E402
from voge_amd.Meshes import GaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, to_colored_background      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
steps = int(args[0]) if args else 30
reps = int(args[1]) if len(args) > 1 else 5
ktrace = "--ktrace" in sys.argv
dev = torch.device("cuda", 0)
N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
verts, sig, cols = scenes.random_gaussians(N, seed=0)
gm = GaussianMeshes(torch.from_numpy(verts), torch.from_numpy(sig)).to(dev)
gm.verts.requires_grad_(True)
gm.sigmas.requires_grad_(True)
colors = torch.from_numpy(cols).to(dev).requires_grad_(True)
R, T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev)
renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
photo = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(0)).to(dev)
learnable = torch.ones(3, device=dev, requires_grad=True)
VARIANTS = {"constant colour (0.9, 1.0, 0.8)": (0.9, 1.0, 0.8), "per-pixel [1,512,512,3] image": photo,
            "learnable [3] colour": learnable}
params = [gm.verts, gm.sigmas, colors, learnable]


def frame(bg):
    for p in params:
        p.grad = None
    to_colored_background(renderer(gm, R=R, T=T), colors, bg).sum().backward()


def timed(fn):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out), min(out), max(out)


lines = [f"cfg3: {N} Gaussians, {H}x{W}, K = {K}; forward + backward of img.sum(); ms per frame, median (min - max) of {reps} "
         f"windows of {steps} frames"]
for name, bg in VARIANTS.items():
    for _ in range(5):
        frame(bg)
    torch.cuda.synchronize()
    if ktrace:
        for _ in range(steps):
            frame(bg)
        torch.cuda.synchronize()
        continue
    eager = timed(lambda: frame(bg))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            frame(bg)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frame(bg)
    replay = timed(graph.replay)
    del graph
    lines.append(f"{name:34s} eager {eager[0]:.4f} ({eager[1]:.4f} - {eager[2]:.4f})   graph {replay[0]:.4f} "
                 f"({replay[1]:.4f} - {replay[2]:.4f})")
print("\n".join(lines if not ktrace else ["ktrace run done"]))
