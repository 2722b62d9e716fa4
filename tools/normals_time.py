"""Step time of a normal-map loss at cfg3 (50k Gaussians, 512^2, K = 40; scenes.CONFIGS["cfg3_50k_512"]): forward + backward of
  (a) get_depth(frag).sum()                                    -- the depth-only step of tools/depth_time.py, the base;
  (b) get_normals(get_depth(frag), cameras, edge=0.1).sum()    -- ops._DepthNormals: voge_depth_normals_fwd / _bwd, one launch each way;
  (c) Aggregation.depth_normals(get_depth(frag), rays, 0.1).sum() with rays from cameras.pixel_rays -- the same stencil in torch.
What has to hold: (b) - (a) < (c) - (a).  Each variant is replayed from a captured graph; the variants ALTERNATE window by window
in one process (one graph alive at a time), times from device events around `steps` replays, the median of `reps` windows.  A
step keeps nothing of its autograd graph alive (tools/depth_time.py says why).
usage: python tools/normals_time.py [steps] [reps] [--out FILE]
       python tools/normals_time.py --eager VARIANT STEPS        (5 warm + STEPS eager steps: for a kernel trace)
       python tools/normals_time.py --summary DIR [--out FILE]   (of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
                                          python tools/normals_time.py --eager ...` run: launches per step -- the period of the trace's
                                          sequence of kernel names -- and the two kernels' durations with the bytes they have
                                          to move over that time: 4 + 12 B a pixel forward, 4 + 12 + 4 B backward)"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
EDGE = 0.1


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


if "--summary" in argv:
    d = argv[argv.index("--summary") + 1]
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    names = [r[2] for r in rows]
    # the steps are identical, so the names' sequence ends periodic: the shortest period of the trace's second half is one step
    tail = names[len(names) // 2:]
    period = next((p for p in range(1, len(tail) // 3 + 1) if tail[p:] == tail[:-p]), None)
    lines = [f"{d}: {len(rows)} launches in the trace",
             f"  launches per step: {period} (the shortest period of the kernel names over the second half of the trace)"]
    pixels = 512 * 512
    for key, nbytes in (("depth_normals_fwd", 16 * pixels), ("depth_normals_bwd", 20 * pixels)):
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            med = statistics.median(us)
            lines.append(f"  {key}_kernel: median {med:.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches); {nbytes / 1e6:.2f} MB "
                         f"to move -> {nbytes / med / 1e6:.3f} TB/s")
    emit(lines)
    sys.exit(0)

import torch      # noqa: E402
from voge_amd import scenes      # noqa: E402
from voge_amd.Aggregation import depth_normals      # noqa: E402
from voge_amd.Meshes import GaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_normals      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform, pixel_rays      # noqa: E402

dev = torch.device("cuda", 0)
N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
verts, sig, _ = scenes.random_gaussians(N, seed=0)
gm = GaussianMeshes(torch.from_numpy(verts), torch.from_numpy(sig)).to(dev)
gm.verts.requires_grad_(True)
gm.sigmas.requires_grad_(True)
R, T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev, R=R, T=T)
renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
params = [gm.verts, gm.sigmas]


def torch_normals(depth):      # (the rays are made inside the step: the frame path no longer materialises them for the user)
    return depth_normals(depth, pixel_rays(cams, (H, W))[0], EDGE)


VARIANTS = {"a": ("(a) get_depth only", lambda depth: depth),
            "b": ("(b) get_depth -> get_normals", lambda depth: get_normals(depth, cams, edge=EDGE)),
            "c": ("(c) get_depth -> Aggregation.depth_normals (torch)", torch_normals)}


def step(variant, keep=False):
    for p in params:
        p.grad = None
    out = VARIANTS[variant][1](get_depth(renderer(gm, R=R, T=T)))
    out.sum().backward()
    return out.detach().clone() if keep else None      # (never the map itself)


if "--eager" in argv:
    variant, steps = argv[argv.index("--eager") + 1], int(argv[argv.index("--eager") + 2])
    for _ in range(5 + steps):
        step(variant)
    torch.cuda.synchronize()
    print(f"eager run done: variant {variant}, {5 + steps} steps")
    sys.exit(0)

args = [a for a in argv if not a.startswith("--") and a != out_file]
steps = int(args[0]) if args else 30
reps = int(args[1]) if len(args) > 1 else 5


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def replay_window(variant):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(variant)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(variant)
    graph.replay()
    torch.cuda.synchronize()
    ms = window(graph.replay)
    del graph
    return ms


# (b) and (c) must be the same map and the same gradients, at the size that is timed
got = {}
for variant in ("b", "c"):
    for _ in range(3):
        out = step(variant, keep=True)
    torch.cuda.synchronize()
    got[variant] = [out] + [p.grad.clone() for p in params]
differ = int(((got["b"][0] != 0).any(-1) != (got["c"][0] != 0).any(-1)).sum())
print(f"  (b) against (c): the defined-masks differ at {differ} of {H * W} pixels", flush=True)
assert differ <= H * W // 1000
for x, y, what in zip(got["b"], got["c"], ("normals", "g_verts", "g_sigmas")):
    diff = (x - y).abs() / max(1.0, y.abs().max().item())
    err, most = diff.max().item(), torch.quantile(diff.flatten()[:1 << 24].float(), 0.999).item()
    print(f"  (b) against (c), {what}: max {err:.2e}, 99.9 % of the elements within {most:.2e} of scale", flush=True)
    # ((c) is the fp32 torch definition: the differences are its own floor, largest where the surface is seen at a grazing angle)
    assert most < 1e-3, (what, err, most)
for _ in range(3):
    step("a")
torch.cuda.synchronize()
res = {k: [] for k in VARIANTS}
for r in range(reps):
    for k in VARIANTS:
        res[k].append(replay_window(k))
        print(f"  window {r} ({k}): {res[k][-1]:.4f} ms", flush=True)
med = {k: statistics.median(v) for k, v in res.items()}
defined = float((got["b"][0] != 0).any(-1).float().mean())
lines = [f"cfg3: {N} Gaussians, {H}x{W}, K = {K}, edge = {EDGE}, {100 * defined:.1f} % of the pixels with a normal; forward + backward of "
         f"(...).sum(); graph replay, ms per step, median (min - max) of {reps} windows of {steps} steps, the variants alternating"]
for k, (name, _) in VARIANTS.items():
    lines.append(f"  {name:52s} {med[k]:.4f} ({min(res[k]):.4f} - {max(res[k]):.4f})")
lines.append(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):.1f} us, (c) - (a) = {1e3 * (med['c'] - med['a']):.1f} us; spread of the repeated (a) windows "
             f"{1e3 * (max(res['a']) - min(res['a'])):.1f} us")
emit(lines)
