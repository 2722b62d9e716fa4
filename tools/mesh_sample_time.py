"""Times of mesh surface sampling (Losses.sample_points_from_meshes -> ops._MeshSample -> voge_mesh_sample_fwd / _bwd) on one GPU.
No time is fixed in advance.
  terms     the forward alone, and forward + backward of sum(points^2) + sum(normals * points) with normals, captured once and
            replayed `steps` times between two device events after a warm-up, on a FIXED u; the variants ALTERNATE window by
            window in one process, the figure is the median (min - max) of `reps` windows.  Variants: the kernels, and
            Aggregation.mesh_surface_points (the definition) on the device.  Shapes: the cfg5 sphere (2 562 vertices, 5 120 faces,
            S = 5 000) and a grid mesh of about 1 M faces with S = 1 M.  Kernels and definition must agree at the sizes timed:
            asserted (at least 99.9 % of the faces equal, gradients to 1e-4 of their largest entry).
  launches  kernels of one eager forward and one backward of each variant, counted by torch.profiler.
  demo      the cfg5 shape-fitting iteration (demo.fit(graph=True), level 4, 128^2, 5 views) without a chamfer term, with the
            vertex chamfer term, and with the chamfer term on 5 000 fresh surface samples of both meshes: host clock from
            iteration 50 to a device synchronise after the last, the variants alternating.
usage: python tools/mesh_sample_time.py [reps] [--out FILE] [--no-demo] [--launches-only]"""
import importlib.util
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5
launches_only = "--launches-only" in argv

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd import Aggregation, Losses, ops      # noqa: E402

assert torch.cuda.is_available(), "mesh_sample_time.py measures on a GPU: none is visible"
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


def grid(n):
    """a height field of n x n cells: (verts [(n+1)^2,3], faces [2 n^2,3])"""
    xs, ys = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing="xy")
    v = np.stack([xs, ys, 0.2 * np.sin(3 * xs) * np.cos(2 * ys)], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)], 1).reshape(-1, 3)
    return v, f.astype(np.int64)


class Replayed:
    """fn(verts) -> (points, normals, face_idx), with or without the backward of a fixed functional, captured into a graph;
    window(steps) -> us per step"""

    def __init__(self, fn, verts, backward):
        self.v = verts.clone().requires_grad_(backward)
        self.fn, self.backward = fn, backward
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.v.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self.step()
        self.graph.replay()
        torch.cuda.synchronize()

    def step(self):
        self.v.grad = None
        p, n, idx = self.fn(self.v)
        if self.backward:
            ((p * p).sum() + (n * p).sum()).backward()
        return p.detach(), n.detach(), idx      # (nothing of a step's autograd graph stays alive: see tools/depth_time.py)

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
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, v in variants.items():
            out[k].append(v.window(steps[k]))
    return out


HIP, TORCH = "ops._MeshSample (HIP)", "Aggregation.mesh_surface_points (torch, on the device)"


def variants_of(verts, faces, u, backward):
    sampler = Losses.SurfaceSampler(faces, num_verts=verts.shape[0], device=dev)
    faces_dev = sampler.faces.long()
    return {HIP: Replayed(lambda v: ops.mesh_sample(v, sampler, u, True)[:3], verts, backward),
            TORCH: Replayed(lambda v: Aggregation.mesh_surface_points(v, faces_dev, u, True)[:3], verts, backward)}


# ---- terms --------------------------------------------------------------------------------------------------------------------
sv, sf = demo.ico_sphere(4)
gv, gf = grid(708)
# (steps a window: every window is 0.1 s of device time at the least, most of them 0.3 - 2 s)
shapes = [("cfg5 sphere", sv, sf, 5000, 20000, 1000), ("grid mesh", gv, gf, 1000000, 2000, 200)]
for label, v_np, f_np, S, steps, def_steps in ([] if launches_only else shapes):
    verts = torch.from_numpy(v_np).to(dev)
    u = torch.from_numpy(np.random.default_rng(0).random((S, 3), dtype=np.float32)).to(dev)
    for backward in (False, True):
        what = "forward + backward" if backward else "forward"
        lines = [f"{label}: {verts.shape[0]} vertices, {f_np.shape[0]} faces, S = {S}, with normals; {what}; graph replay, us per step, "
                 f"median (min - max) of {reps} windows of {steps} steps ({def_steps} for the definition), the variants alternating"]
        try:
            var = variants_of(verts, f_np, u, backward)
        except Exception as e:      # noqa: BLE001  (say what could not be measured, do not guess)
            emit(lines + [f"  not measured ({type(e).__name__}: {e})"])
            continue
        k, d = var[HIP], var[TORCH]
        same = float((k.out[2].long() == d.out[2]).float().mean())
        note = f"  {same * 100:.4f} % of the faces equal"
        assert same >= 0.999, same
        if backward:
            dg = float((k.v.grad - d.v.grad).abs().max() / d.v.grad.abs().max())
            assert dg <= 1e-4, dg
            note += f", gradients differ by {dg:.1e} of their largest entry"
        lines.append(note)
        for name, us in alternate(var, {HIP: steps, TORCH: def_steps}).items():
            lines.append(f"  {name:56s} {fmt(us)}")
        emit(lines)
        del var, k, d

# ---- launches -------------------------------------------------------------------------------------------------------------------
try:
    from torch.profiler import ProfilerActivity, profile
    verts = torch.from_numpy(sv).to(dev)
    u = torch.from_numpy(np.random.default_rng(1).random((5000, 3), dtype=np.float32)).to(dev)
    sampler = Losses.SurfaceSampler(sf, num_verts=sv.shape[0], device=dev)
    faces_dev = sampler.faces.long()
    forms = {HIP: lambda v: ops.mesh_sample(v, sampler, u, True), TORCH: lambda v: Aggregation.mesh_surface_points(v, faces_dev, u, True)}
    for name, fn in forms.items():
        vd = verts.clone().requires_grad_(True)
        for _ in range(2):
            vd.grad = None
            o = fn(vd)
            ((o[0] * o[0]).sum() + (o[1] * o[0]).sum()).backward()
        torch.cuda.synchronize()
        counts = []
        for part in ("forward", "backward"):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                if part == "forward":
                    o = fn(vd)
                    loss = (o[0] * o[0]).sum() + (o[1] * o[0]).sum()
                else:
                    loss.backward()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                     and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            counts.append(f"{part} {len(names)} kernels ({sum('ms_' in n or 'voge_fill' in n for n in names)} of this library)")
        emit([f"launches of one eager call, the functional's own included, {name}: " + ", ".join(counts)])
except Exception as e:      # noqa: BLE001  (the profiler is optional: say so, do not guess)
    emit([f"launches: not measured ({type(e).__name__}: {e})"])

# ---- the demo's iteration -------------------------------------------------------------------------------------------------------
if "--no-demo" not in argv and not launches_only:
    iters = 3050

    def run(variant):
        kw = {"none": {}, "vertices": {"w_chamfer": 1.0}, "samples": {"w_chamfer": 1.0, "chamfer_samples": 5000}}[variant]
        return demo.fit(iters=iters, level=4, size=128, graph=True, quiet=True, timed_from=50, **kw)["sec_per_iter"] * 1e3
    names = {"none": "(a) no chamfer term", "vertices": "(b) chamfer on the 2562 vertices", "samples": "(c) chamfer on 5000 + 5000 fresh surface samples"}
    ms = {k: [] for k in names}
    for _ in range(reps):
        for k in names:
            ms[k].append(run(k))
    lines = [f"cfg5 iteration (level 4, 128^2, 5 views, SGD) replayed as a HIP graph; ms per iteration over iterations 50 .. {iters}, "
             f"median (min - max) of {reps} runs, the variants alternating"]
    for k, label in names.items():
        lines.append(f"  {label:52s} {statistics.median(ms[k]):.4f} ({min(ms[k]):.4f} - {max(ms[k]):.4f})")
    a, b, c = (statistics.median(ms[k]) for k in names)
    lines.append(f"  (b) - (a) = {(b - a) * 1e3:.1f} us, (c) - (a) = {(c - a) * 1e3:.1f} us; spread of the repeated (a) runs "
                 f"{(max(ms['none']) - min(ms['none'])) * 1e3:.1f} us")
    emit(lines)
