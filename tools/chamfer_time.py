"""Times of the chamfer distance (Losses.chamfer_distance -> ops._Chamfer -> voge_chamfer_fwd / _bwd) on one GPU.  No time is fixed
in advance.
  terms     forward + backward of the term alone, captured once and replayed `steps` times between two device events after a
            warm-up; the variants ALTERNATE window by window in one process, the figure is the median (min - max) of `reps`
            windows.  Variants: the kernels on the route the shapes choose, and Aggregation.chamfer_term (the chunked definition)
            on the device -- at 438 544 x 438 544 the definition is ONE eager call on a host clock (1.9e11 pairs).
            Shapes: the cfg5 sphere against its ground truth (2 562 x 2 562), uniform clouds of 50 000 x 50 000 and
            438 544 x 438 544.  Kernels and definition must agree at the sizes timed: asserted (loss to 1e-5, gradients to 1e-4 of
            their largest entry).
  sweep     the route threshold: forward + backward with route="brute" and route="grid" over square and lopsided shapes, the same
            windows; the two routes must give the same bits: asserted.
  launches  kernels of one eager forward + backward on each route, counted by torch.profiler.
  demo      the cfg5 shape-fitting iteration (demo.fit(graph=True), level 4, 128^2, 5 views) without the term, with the kernels,
            and with Aggregation.chamfer_term in the kernels' place: host clock from iteration 50 to a device synchronise after the
            last, the variants alternating.
usage: python tools/chamfer_time.py [reps] [--out FILE] [--no-demo] [--no-big-definition] [--launches-only]"""
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5
launches_only = "--launches-only" in argv

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd import Aggregation, ops      # noqa: E402

assert torch.cuda.is_available(), "chamfer_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)
spec = importlib.util.spec_from_file_location("ShapeFitting", os.path.join("demo", "ShapeFitting.py"))
demo = importlib.util.module_from_spec(spec)
spec.loader.exec_module(demo)


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


def fmt(us):
    return f"{statistics.median(us):10.2f} ({min(us):.2f} - {max(us):.2f})"


def uniform(n, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1)).to(dev)


class Replayed:
    """forward + backward of fn(x, y) captured into a graph; window(steps) -> us per step"""

    def __init__(self, fn, x, y):
        self.x, self.y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self.x.grad = self.y.grad = None
                fn(self.x, self.y).backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.x.grad = self.y.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = fn(self.x, self.y)
            self.loss.backward()
        self.graph.replay()
        torch.cuda.synchronize()

    def window(self, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(max(3, steps // 10)):
            self.graph.replay()
        a.record()
        for _ in range(steps):
            self.graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / steps


def alternate(variants, steps):
    """variants: {name: Replayed}, steps: an int or {name: int} -> {name: [us per step of each window]}"""
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, v in variants.items():
            out[k].append(v.window(steps[k] if isinstance(steps, dict) else steps))
    return out


def kernels(route=None):
    return lambda a, b: ops.chamfer(a, b, False, False, route)[0]


def definition(a, b):
    return Aggregation.chamfer_term(a, b)


def agree(label, u, v):
    dl = abs(float(u.loss) - float(v.loss)) / max(abs(float(v.loss)), 1e-30)
    dg = max(float((u.x.grad - v.x.grad).abs().max() / v.x.grad.abs().max()), float((u.y.grad - v.y.grad).abs().max() / v.y.grad.abs().max()))
    assert dl <= 1e-5 and dg <= 1e-4, (label, dl, dg)
    return f"loss differs by {dl:.1e} relative, gradients by {dg:.1e} of their largest entry"


# ---- terms --------------------------------------------------------------------------------------------------------------------
sv, gv = demo.ico_sphere(4)[0], demo.ground_truth_shape(4)[0]
HIP, TORCH = "ops._Chamfer (HIP)", "Aggregation.chamfer_term (torch, on the device)"
# (the definition at 50 000 x 50 000 is 300 chunks of a dozen launches over 16.7 M pairs each: three steps a window are 1 s)
shapes = [("cfg5 sphere against its ground truth", torch.from_numpy(sv).to(dev), torch.from_numpy(gv).to(dev), 2000, 500),
          ("uniform clouds", uniform(50000, 0), uniform(50000, 1), 200, 3),
          ("uniform clouds", uniform(438544, 2), uniform(438544, 3), 50, 0)]
for label, x, y, steps, def_steps in ([] if launches_only else shapes):
    with_definition = def_steps > 0
    variants = {HIP: Replayed(kernels(), x, y)}
    lines = [f"{label}: {len(x)} x {len(y)} points; forward + backward of the term alone; graph replay, us per step, median (min - max) of "
             f"{reps} windows of {steps} steps ({def_steps} for the definition), the variants alternating"]
    if with_definition:
        variants[TORCH] = Replayed(definition, x, y)
        lines.append("  " + agree(label, *variants.values()))
    for k, us in alternate(variants, {HIP: steps, TORCH: def_steps}).items():
        lines.append(f"  {k:50s} {fmt(us)}")
    if not with_definition:
        if "--no-big-definition" in argv:
            lines.append("  Aggregation.chamfer_term at this size: not measured")
        else:
            xd, yd = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = definition(xd, yd)
            loss.backward()
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            k = variants[HIP]
            dl = abs(float(loss) - float(k.loss)) / float(loss)
            assert dl <= 1e-5, dl
            lines.append(f"  Aggregation.chamfer_term (torch, on the device): ONE eager call, host clock, no warm-up: {sec:.2f} s "
                         f"(loss differs by {dl:.1e} relative)")
    emit(lines)
    del variants

# ---- the route threshold --------------------------------------------------------------------------------------------------------
SWEEP = ((162, 642), (1000, 1000), (2562, 2562), (4000, 4000), (5000, 5000), (6000, 6000), (8000, 8000), (12000, 12000),
         (16000, 16000), (24000, 24000), (500, 50000), (2562, 50000), (200, 438544))
if not launches_only:
    emit([f"route sweep: forward + backward, graph replay, us per step, median (min - max) of {reps} windows, brute and grid alternating; "
          "the crossing sets kChamferBruteMaxPairs of chamfer.hip"])
for nx, ny in (() if launches_only else SWEEP):
    x, y = uniform(nx, 10), uniform(ny, 11)
    v = {"brute": Replayed(kernels("brute"), x, y), "grid": Replayed(kernels("grid"), x, y)}
    b, g = v["brute"], v["grid"]
    assert torch.equal(b.loss, g.loss) and torch.equal(b.x.grad, g.x.grad) and torch.equal(b.y.grad, g.y.grad), (nx, ny)
    t = alternate(v, 1000 if nx * ny <= 4e7 else 200)
    mb, mg = statistics.median(t["brute"]), statistics.median(t["grid"])
    emit([f"  {nx:6d} x {ny:6d} = {nx * ny:.2e} pairs: brute {fmt(t['brute'])}   grid {fmt(t['grid'])}   -> {'brute' if mb < mg else 'grid'}"])
    del v, b, g

# ---- launches -------------------------------------------------------------------------------------------------------------------
try:
    from torch.profiler import ProfilerActivity, profile
    x, y = uniform(3000, 20), uniform(3000, 21)
    for route in ("brute", "grid"):
        xd, yd = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        for _ in range(2):
            ops.chamfer(xd, yd, False, False, route)[0].backward()
        torch.cuda.synchronize()
        counts = []
        for part in ("forward", "backward"):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                if part == "forward":
                    loss = ops.chamfer(xd, yd, False, False, route)[0]
                else:
                    loss.backward()
                torch.cuda.synchronize()
            # (device-side events only: the runtime's own calls are in the list too)
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                     and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            counts.append(f"{part} {len(names)} kernels ({sum('chamfer' in n or 'knn_scan' in n or 'voge_fill' in n for n in names)} of this library)")
        emit([f"launches of one eager call, route {route}: " + ", ".join(counts)])
except Exception as e:      # noqa: BLE001  (the profiler is optional: say so, do not guess)
    emit([f"launches: not measured ({type(e).__name__}: {e})"])

# ---- the demo's iteration -------------------------------------------------------------------------------------------------------
if "--no-demo" not in argv and not launches_only:
    iters = 1050
    hip_form = demo.chamfer_distance

    def run(variant):
        demo.chamfer_distance = hip_form if variant != "definition" else (lambda a, b: (Aggregation.chamfer_term(a, b), None))
        h = demo.fit(iters=iters, level=4, size=128, graph=True, quiet=True, timed_from=50, w_chamfer=0.0 if variant == "none" else 1.0)
        demo.chamfer_distance = hip_form
        return h["sec_per_iter"] * 1e3
    names = {"none": "(a) no chamfer term", "kernels": "(b) chamfer_distance (HIP node)", "definition": "(c) Aggregation.chamfer_term (torch)"}
    ms = {k: [] for k in names}
    for _ in range(reps):
        for k in names:
            ms[k].append(run(k))
    lines = [f"cfg5 iteration (level 4, 128^2, 5 views, SGD) replayed as a HIP graph, 2562 vertices against 2562 target points; ms per "
             f"iteration over iterations 50 .. {iters}, median (min - max) of {reps} runs, the variants alternating"]
    for k, label in names.items():
        lines.append(f"  {label:42s} {statistics.median(ms[k]):.4f} ({min(ms[k]):.4f} - {max(ms[k]):.4f})")
    a, b, c = (statistics.median(ms[k]) for k in names)
    lines.append(f"  (b) - (a) = {(b - a) * 1e3:.1f} us, (c) - (a) = {(c - a) * 1e3:.1f} us; spread of the repeated (a) runs {(max(ms['none']) - min(ms['none'])) * 1e3:.1f} us")
    emit(lines)
