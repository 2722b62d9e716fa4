"""Step time of a frame with view-dependent colours (forward + backward of to_white_background(...).sum()) at two sizes:
  cfg3   50 000 Gaussians, 512^2, K = 40, one view (scenes.CONFIGS["cfg3_50k_512"]);
  demo   the eight-view batch of demo/ViewDependentColors.py (the bunny's 8171 Gaussians, 256^2, K = 40),
for three ways to the colours:
  (a) a constant [B*N, 3] colour table, itself a parameter -- the frame alone, what the parent commit measures;
  (b) Renderer.sh_to_colors at degree 3 (ops._ShColors: voge_sh_colors_fwd / _bwd, one launch each way);
  (c) Aggregation.sh_colors, the same polynomial in torch, in its place.
What has to hold: (b) - (a) < (c) - (a).  Each variant is replayed from a captured graph; the variants ALTERNATE window by window
in one process (one graph alive at a time), times from device events around `steps` replays, the median of `reps` windows.  A
step keeps nothing of its autograd graph alive (tools/depth_time.py says why).
usage: python tools/sh_colors_time.py [steps] [reps] [--out FILE]
       python tools/sh_colors_time.py --eager VARIANT CONFIG STEPS      (5 warm + STEPS eager steps: for a kernel trace)
       python tools/sh_colors_time.py --summary DIR CONFIG [--out FILE] (of a `rocprofv3 --kernel-trace --stats --output-format csv
                                          -d DIR -- python tools/sh_colors_time.py --eager ...` run: launches per step -- the
                                          period of the trace's sequence of kernel names -- and the two SH kernels' durations
                                          with the bytes they have to move over that time)"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
SIZES = {"cfg3": (50000, 1), "demo": (8171, 8)}      # (Gaussians, views)
M, C = 16, 3


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


if "--summary" in argv:
    d, config = argv[argv.index("--summary") + 1], argv[argv.index("--summary") + 2]
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    names = [r[2] for r in rows]
    # the steps are identical, so the names' sequence ends periodic: the shortest period of the trace's second half is one step
    # (a few equal names in a row at the very end must not pass for a period: every launch of that half is compared)
    tail = names[len(names) // 2:]
    period = next((p for p in range(1, len(tail) // 3 + 1) if tail[p:] == tail[:-p]), None)
    lines = [f"{d} ({config}): {len(rows)} launches in the trace",
             f"  launches per step: {period} (the shortest period of the kernel names over the second half of the trace)"]
    N, B = SIZES[config]
    need = {"sh_colors_fwd": 4 * (N * M * C + 3 * N + 3 * B + B * N * C), "sh_colors_bwd": 4 * (2 * N * M * C + 6 * N + 3 * B + B * N * C)}
    for key, nbytes in need.items():
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            med = statistics.median(us)
            lines.append(f"  {key}_kernel<{M}, {C}>: median {med:.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches); {nbytes / 1e6:.2f} MB "
                         f"to move -> {nbytes / med / 1e6:.3f} TB/s")
    emit(lines)
    sys.exit(0)

import torch      # noqa: E402
import numpy as np      # noqa: E402
from voge_amd import scenes      # noqa: E402
from voge_amd.Aggregation import sh_colors      # noqa: E402
from voge_amd.Meshes import GaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, sh_to_colors, to_white_background      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402

dev = torch.device("cuda", 0)


class Case:
    def __init__(self, config):
        if config == "cfg3":
            N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
            verts, sig, _ = scenes.random_gaussians(N, seed=0)
            self.R, self.T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
        else:
            g = np.load(os.path.join("tests", "golden", "bunny_gaussians.npz"))
            verts, sig = g["verts"], g["isigma"]
            N, (H, W), K, focal, pp = verts.shape[0], (256, 256), 40, 2000.0, (128.0, 128.0)
            self.R, self.T = look_at_view_transform(dist=[6.0] * 8, elev=[20.0 * (-1) ** i for i in range(8)],
                                                    azim=[10.0 + 45.0 * i for i in range(8)], device=dev)
        assert (N, self.R.shape[0]) == SIZES[config]
        B = self.R.shape[0]
        self.gm = GaussianMeshes(torch.from_numpy(verts), torch.from_numpy(sig)).to(dev)
        cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev, R=self.R, T=self.T)
        self.renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
        self.centres = cams.get_camera_center()      # (once: the cameras are fixed)
        gen = torch.Generator(dev).manual_seed(0)
        self.sh = (0.5 * torch.randn((N, M, C), device=dev, generator=gen)).requires_grad_(True)
        self.table = torch.rand((B * N, C), device=dev, generator=gen).requires_grad_(True)
        self.name = f"{config}: {N} Gaussians, {H}x{W}, K = {K}, {B} view{'s' if B > 1 else ''}"

    def colours(self, variant):
        if variant == "a":
            return self.table
        return (sh_to_colors if variant == "b" else sh_colors)(self.sh, self.gm.verts, self.centres)

    def params(self, variant):
        return [self.table if variant == "a" else self.sh, self.gm.verts, self.gm.sigmas]

    def step(self, variant, keep=False):
        for p in (self.table, self.sh, self.gm.verts, self.gm.sigmas):
            p.grad = None
        img = to_white_background(self.renderer(self.gm, R=self.R, T=self.T), self.colours(variant))
        img.sum().backward()
        return img.detach().clone() if keep else None      # (never the image itself)


VARIANTS = {"a": "(a) constant colour table", "b": "(b) sh_to_colors, degree 3", "c": "(c) Aggregation.sh_colors (torch)"}

if "--eager" in argv:
    variant, config, steps = argv[argv.index("--eager") + 1], argv[argv.index("--eager") + 2], int(argv[argv.index("--eager") + 3])
    case = Case(config)
    for _ in range(5 + steps):
        case.step(variant)
    torch.cuda.synchronize()
    print(f"eager run done: variant {variant}, {config}, {5 + steps} steps")
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


for config in SIZES:
    case = Case(config)
    # (b) and (c) must be the same image and the same gradients, at the size that is timed
    got = {}
    for variant in ("b", "c"):
        for _ in range(3):
            img = case.step(variant, keep=True)
        torch.cuda.synchronize()
        got[variant] = [img] + [p.grad.clone() for p in case.params(variant)]
    for x, y, what in zip(got["b"], got["c"], ("image", "g_sh", "g_verts", "g_sigmas")):
        err = (x - y).abs().max().item() / max(1.0, y.abs().max().item())
        assert err < 1e-4, (config, what, err)
    for _ in range(3):
        case.step("a")
    torch.cuda.synchronize()
    out = {k: [] for k in VARIANTS}
    for r in range(reps):
        for k in VARIANTS:
            out[k].append(replay_window(case, k))
            print(f"  {config} window {r} ({k}): {out[k][-1]:.4f} ms", flush=True)
    med = {k: statistics.median(v) for k, v in out.items()}
    lines = [f"{case.name}; forward + backward of to_white_background(...).sum(); graph replay, ms per step, median (min - max) of "
             f"{reps} windows of {steps} steps, the variants alternating"]
    for k, name in VARIANTS.items():
        lines.append(f"  {name:36s} {med[k]:.4f} ({min(out[k]):.4f} - {max(out[k]):.4f})")
    lines.append(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):.1f} us, (c) - (a) = {1e3 * (med['c'] - med['a']):.1f} us; spread of the repeated (a) windows "
                 f"{1e3 * (max(out['a']) - min(out['a'])):.1f} us")
    emit(lines)
    del case
