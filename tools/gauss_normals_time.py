"""Step time of a cfg3-sized frame of oriented Gaussians (50 000 Gaussians, 512^2, K = 40, one view: scenes.CONFIGS["cfg3_50k_512"])
whose merged attribute is the Gaussians' own normals -- forward + backward of interpolate_attr(renderer(...), table).sum() -- for
three ways to the [B*N, 3] table:
  (a) a constant table, itself a parameter -- the frame alone;
  (b) Renderer.gaussian_normals (ops._GaussNormals: voge_gauss_normals_fwd / _bwd, one launch each way);
  (c) Aggregation.gaussian_normals, the same rules in torch, in its place.
No time is fixed in advance: what is measured is (b) - (a) against (c) - (a).  Each variant is replayed from a captured graph; the
variants ALTERNATE window by window in one process (one graph alive at a time), times from device events around `steps` replays,
the median of `reps` windows.  A step keeps nothing of its autograd graph alive (tools/depth_time.py says why).
usage: python tools/gauss_normals_time.py [steps] [reps] [--out FILE]
       python tools/gauss_normals_time.py --eager VARIANT STEPS      (5 warm + STEPS eager steps: for a kernel trace)
       python tools/gauss_normals_time.py --summary DIR [--out FILE] (of a `rocprofv3 --kernel-trace --stats --output-format csv
                                          -d DIR -- python tools/gauss_normals_time.py --eager ...` run: launches per step -- the
                                          period of the trace's sequence of kernel names -- and the two kernels' durations with
                                          the bytes they have to move over that time)"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
N_GAUSS, VIEWS = 50000, 1


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
    N, B = N_GAUSS, VIEWS
    # shared orientations and verts: scales + quats (28 N), verts (12 N), centres (12 B), the table (12 B N); the backward reads the
    # upstream gradient (12 B N) in the table's place and writes g_quats (16 N)
    need = {"gauss_normals_fwd": 28 * N + 12 * N + 12 * B + 12 * B * N, "gauss_normals_bwd": 28 * N + 12 * N + 12 * B + 12 * B * N + 16 * N}
    for key, nbytes in need.items():
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            med = statistics.median(us)
            lines.append(f"  {key}_kernel: median {med:.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches); {nbytes / 1e6:.2f} MB "
                         f"to move -> {nbytes / med / 1e6:.3f} TB/s")
    emit(lines)
    sys.exit(0)

import torch      # noqa: E402
import numpy as np      # noqa: E402
from voge_amd import scenes      # noqa: E402
from voge_amd.Aggregation import gaussian_normals as definition      # noqa: E402
from voge_amd.Meshes import OrientedGaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, gaussian_normals, interpolate_attr      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402

dev = torch.device("cuda", 0)


class Case:
    def __init__(self):
        N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
        assert N == N_GAUSS
        verts, sig, _ = scenes.random_gaussians(N, seed=0)
        rng = np.random.default_rng(1)
        scales = (sig[:, None] * rng.uniform(0.5, 2.0, (N, 3))).astype(np.float32)
        quats = (rng.normal(size=(N, 4)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
        self.R, self.T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
        self.gm = OrientedGaussianMeshes(torch.from_numpy(verts), torch.from_numpy(scales), torch.from_numpy(quats)).to(dev)
        cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev, R=self.R, T=self.T)
        self.renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
        self.centres = cams.get_camera_center()      # (once: the cameras are fixed)
        gen = torch.Generator(dev).manual_seed(0)
        self.table = torch.rand((VIEWS * N, 3), device=dev, generator=gen).requires_grad_(True)
        self.name = f"cfg3, oriented: {N} Gaussians, {H}x{W}, K = {K}, {VIEWS} view"

    def normals(self, variant):
        if variant == "a":
            return self.table
        return (gaussian_normals if variant == "b" else definition)(self.gm.scales, self.gm.quats, self.gm.verts, self.centres)

    def params(self):
        return [self.gm.quats, self.gm.verts, self.gm.scales]

    def step(self, variant, keep=False):
        for p in [self.table] + self.params():
            p.grad = None
        img = interpolate_attr(self.renderer(self.gm, R=self.R, T=self.T), self.normals(variant))
        img.sum().backward()
        return img.detach().clone() if keep else None      # (never the image itself)


VARIANTS = {"a": "(a) constant table", "b": "(b) gaussian_normals", "c": "(c) Aggregation.gaussian_normals (torch)"}

if "--eager" in argv:
    variant, steps = argv[argv.index("--eager") + 1], int(argv[argv.index("--eager") + 2])
    case = Case()
    for _ in range(5 + steps):
        case.step(variant)
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


def replay_window(case, variant):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            case.step(variant)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.step(variant)
    graph.replay()
    torch.cuda.synchronize()
    ms = window(graph.replay)
    del graph
    return ms


case = Case()
# (b) and (c) must be the same map and the same gradients, at the size that is timed
got = {}
for variant in ("b", "c"):
    for _ in range(3):
        img = case.step(variant, keep=True)
    torch.cuda.synchronize()
    got[variant] = [img] + [p.grad.clone() for p in case.params()]
for x, y, what in zip(got["b"], got["c"], ("map", "g_quats", "g_verts", "g_scales")):
    err = (x - y).abs().max().item() / max(1.0, y.abs().max().item())
    assert err < 1e-4, (what, err)
for _ in range(3):
    case.step("a")
torch.cuda.synchronize()
out = {k: [] for k in VARIANTS}
for r in range(reps):
    for k in VARIANTS:
        out[k].append(replay_window(case, k))
        print(f"  window {r} ({k}): {out[k][-1]:.4f} ms", flush=True)
med = {k: statistics.median(v) for k, v in out.items()}
lines = [f"{case.name}; forward + backward of interpolate_attr(...).sum(); graph replay, ms per step, median (min - max) of "
         f"{reps} windows of {steps} steps, the variants alternating"]
for k, name in VARIANTS.items():
    lines.append(f"  {name:42s} {med[k]:.4f} ({min(out[k]):.4f} - {max(out[k]):.4f})")
lines.append(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):.1f} us, (c) - (a) = {1e3 * (med['c'] - med['a']):.1f} us; spread of the repeated (a) windows "
             f"{1e3 * (max(out['a']) - min(out['a'])):.1f} us")
emit(lines)
