"""Times of the point-cloud kernels (Converters.knn_points -> voge_knn_points, point_cloud_frames -> voge_knn_frames) on one GPU.
No time is fixed in advance.  Clouds: the synthetic cloud of demo/RenderPointClouds.py (438 544 points on a wall over a ground
plane) and a uniform volume cloud of the same size.  A window is `steps` calls between two device events after a warm-up; the
variants ALTERNATE window by window in one process, the figure is the median (min - max) of `reps` windows.  A call includes the
host's read of the bounding box (one synchronisation), as a converter pays it.  The variants of one cloud and k (the default grid,
grids of twice and of half the cell, the latter as far as the cap of 8 N cells lets it) must return the same bits at the size timed: asserted.
Also: the frame kernel; naive_point_cloud_converter (cdist + topk over all pairs) against point_cloud_converter at 50 000 points,
where the former's chunks fit; the candidate distances a query evaluates, counted on the host from the grid and the k-th distances
(the search stops after ring r = ceil(sqrt(d2_k) / (cell (1 - 2^-20)) + 2^-10), or when the cube covers the grid), next to the
brute force's N; the demo's share of covered pixels for each form.
usage: python tools/knn_time.py [steps] [reps] [--out FILE] [--no-demo]
       python tools/knn_time.py --eager demo|uniform K STEPS      (3 warm + STEPS calls: for a kernel trace)
       python tools/knn_time.py --summary DIR [--out FILE]        (of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
                                          python tools/knn_time.py --eager ...` run: the knn kernels' durations per call)"""
import csv
import glob
import importlib.util
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
N_POINTS = 438544


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
    lines = [f"{d}: {len(rows)} launches in the trace; per kernel, the second half of its launches"]
    total = {}
    for key in ("voge_fill32", "knn_count", "knn_scan_partial", "knn_scan_sums", "knn_scan_final", "knn_fill", "knn_search", "knn_frames"):
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            total[key] = statistics.median(us)
            lines.append(f"  {key}_kernel: median {total[key]:.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches)")
    build = sum(v for k, v in total.items() if k not in ("knn_search", "knn_frames"))
    scan = sum(v for k, v in total.items() if "scan" in k)
    if "knn_search" in total:
        lines.append(f"  count + scan + fill (and the zero fill): {build:.2f} us, of which the scan {scan:.2f} us; the search: {total['knn_search']:.2f} us")
    emit(lines)
    sys.exit(0)

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd.Converter import Converters      # noqa: E402

dev = torch.device("cuda", 0)
spec = importlib.util.spec_from_file_location("RenderPointClouds", os.path.join("demo", "RenderPointClouds.py"))
demo = importlib.util.module_from_spec(spec)
spec.loader.exec_module(demo)


def cloud(name, n=N_POINTS):
    if name == "demo":
        return torch.from_numpy(demo.synthetic_cloud(n)[0]).to(dev)
    rng = np.random.default_rng(0)
    return torch.from_numpy((rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1))).to(dev)


if "--eager" in argv:
    i = argv.index("--eager")
    pts, k, steps = cloud(argv[i + 1]), int(argv[i + 2]), int(argv[i + 3])
    for _ in range(3 + steps):
        idx, d2 = Converters.knn_points(pts, k, include_self=True)
    quats, eig = Converters.point_cloud_frames(pts, idx)
    torch.cuda.synchronize()
    sys.exit(0)

nums = [a for a in argv if a.isdigit()]
steps, reps = (int(nums[0]) if nums else 10), (int(nums[1]) if len(nums) > 1 else 5)


def windows(variants):
    """{name: callable} -> {name: (median, min, max) ms per call}; the variants alternate window by window."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            got[name].append(a.elapsed_time(b) / steps)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def candidates(pts, d2, grid):
    """Mean / max number of candidate distances a query evaluates under `grid`, counted on the host."""
    cell, gx, gy, gz = grid
    p = pts.cpu().numpy()
    lo = p.min(0)
    inv = np.float32(1) / np.float32(cell)
    c = [np.clip(np.floor((p[:, a] - lo[a]) * inv), 0, g - 1).astype(np.int64) for a, g in enumerate((gx, gy, gz))]
    counts = np.zeros((gz, gy, gx), np.int64)
    np.add.at(counts, (c[2], c[1], c[0]), 1)
    summed = np.zeros((gz + 1, gy + 1, gx + 1), np.int64)
    summed[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)
    kth = np.sqrt(d2[:, -1].double().cpu().numpy())
    r = np.ceil(kth / (float(cell) * (1 - 2.0 ** -20)) + 2.0 ** -10).astype(np.int64)
    r = np.where(np.isfinite(kth), r, max(gx, gy, gz))
    x0, x1 = np.clip(c[0] - r, 0, gx), np.clip(c[0] + r + 1, 0, gx)
    y0, y1 = np.clip(c[1] - r, 0, gy), np.clip(c[1] + r + 1, 0, gy)
    z0, z1 = np.clip(c[2] - r, 0, gz), np.clip(c[2] + r + 1, 0, gz)
    n = (summed[z1, y1, x1] - summed[z0, y1, x1] - summed[z1, y0, x1] - summed[z1, y1, x0]
         + summed[z0, y0, x1] + summed[z0, y1, x0] + summed[z1, y0, x0] - summed[z0, y0, x0])
    return n.mean(), n.max(), r.mean()


lines = [f"knn_points, {N_POINTS} points, include_self=True; ms per call, median (min - max) of {reps} windows of {steps} calls, the variants alternating"]
for name in ("demo", "uniform"):
    pts = cloud(name)
    for k in (4, 16):
        idx, d2, grid = Converters.knn_points(pts, k, include_self=True, return_grid=True)
        idx2, d22, grid2 = Converters.knn_points(pts, k, include_self=True, cell_size=2 * grid[0], return_grid=True)
        assert torch.equal(idx, idx2) and torch.equal(d2, d22) and grid2[1:] != grid[1:], "the two grids disagree"
        idx3, d23, grid3 = Converters.knn_points(pts, k, include_self=True, cell_size=0.5 * grid[0], return_grid=True)      # (the cap of 8 N cells enlarges it)
        assert torch.equal(idx, idx3) and torch.equal(d2, d23) and grid3[1:] != grid[1:], "the two grids disagree"
        t = windows({"default": lambda: Converters.knn_points(pts, k, include_self=True),
                     "double": lambda: Converters.knn_points(pts, k, include_self=True, cell_size=2 * grid[0]),
                     "half": lambda: Converters.knn_points(pts, k, include_self=True, cell_size=0.5 * grid[0])})
        for variant, g in (("default", grid), ("double", grid2), ("half", grid3)):
            mean, most, rings = candidates(pts, d2, g)
            lines.append(f"  {name:8s} k={k:2d} {variant:8s} grid {g[1]}x{g[2]}x{g[3]} (cell {g[0]:.5f}): {t[variant][0]:.3f} ({t[variant][1]:.3f} - {t[variant][2]:.3f}) ms; "
                         f"candidates per query mean {mean:.0f}, max {most} (brute force: {N_POINTS}); rings mean {rings:.2f}")
    if name == "demo":
        idx16 = Converters.knn_points(pts, 16, include_self=True)[0]
        t = windows({"frames": lambda: Converters.point_cloud_frames(pts, idx16)})
        lines.append(f"  point_cloud_frames, k=16, demo cloud: {t['frames'][0]:.3f} ({t['frames'][1]:.3f} - {t['frames'][2]:.3f}) ms")
emit(lines)

small = cloud("demo", 50000)
new = Converters.point_cloud_converter(small)[1]
old = Converters.naive_point_cloud_converter(small)[1]
rel = ((new - old).abs() / old).max().item()
t = windows({"naive": lambda: Converters.naive_point_cloud_converter(small), "grid": lambda: Converters.point_cloud_converter(small)})
emit([f"converters at 50000 points of the demo cloud (n_nearest 4), ms per call: naive_point_cloud_converter (cdist + topk, on the device) "
      f"{t['naive'][0]:.2f} ({t['naive'][1]:.2f} - {t['naive'][2]:.2f}); point_cloud_converter {t['grid'][0]:.3f} ({t['grid'][1]:.3f} - {t['grid'][2]:.3f}); "
      f"isigma differs by at most {rel:.2e} relative (cdist's distances are not the definition's)"])

if "--no-demo" not in argv:
    for kw in ({}, {"adaptive": True}, {"oriented": True}):
        demo.run(out=None, log=lambda s: emit(["demo/RenderPointClouds.py " + " ".join("--" + k for k in kw) + ": " + s]), **kw)
