"""Times of the point-to-mesh distance (Losses.point_mesh_face_distance -> ops._PointMesh -> voge_point_mesh_fwd / _bwd) on one
GPU.  No time is fixed in advance.
  terms     the forward alone and forward + backward of the term alone.  "kernels": captured once and replayed `steps` times
            between two device events after a warm-up (the launches without the host's share); "whole call": eager calls on a host
            clock that ends in a device synchronise.  The figure is the median (min - max) of `reps` windows.  Beside it
            Aggregation.point_mesh_term (the chunked definition) on the device, eager on the host clock -- its launches are in
            the thousands, a graph of them is not what a user would run.  Shapes: the cfg5 sphere (2 562 vertices, 5 120 faces)
            against 5 000 and against 50 000 points.  Kernels and definition must agree at the sizes timed: asserted (loss to
            1e-5, gradients to 1e-4 of their largest entry).
  cap       the two searches just below the pair cap ops.POINT_MESH_MAX_PAIRS, each alone between device events: points -> faces
            is voge_closest_faces, faces -> points the forward of both minus the single-directional one.  The slower must stay
            under one second: asserted.
  split     the searches with the candidates split over 16, 4 and 1 waves of a workgroup (the -DVOGE_AB build's switch; the
            product takes 16 below 1024 workgroups of queries, else 4), alternating, over small and large P and F; all must give
            the same bits: asserted.
  launches  kernels of one eager forward + backward of both forms, counted by torch.profiler.
usage: python tools/point_mesh_time.py [reps] [--out FILE] [--no-cap] [--no-split] [--no-definition]"""
import ctypes
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd import Aggregation, _lib, ops      # noqa: E402

assert torch.cuda.is_available(), "point_mesh_time.py measures on a GPU: none is visible"
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
    return f"{statistics.median(us):12.2f} ({min(us):.2f} - {max(us):.2f})"


def cloud(n, seed, scale=1.3):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(((rng.random((n, 3), dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)).to(dev)


def soup(F, seed):
    """F separate small triangles in the cube: 3 F vertices"""
    rng = np.random.default_rng(seed)
    centre = rng.random((F, 1, 3), dtype=np.float32) * 2 - 1
    v = (centre + (rng.random((F, 3, 3), dtype=np.float32) - 0.5) * np.float32(0.05)).reshape(-1, 3).astype(np.float32)
    return torch.from_numpy(v).to(dev), torch.arange(3 * F, dtype=torch.int32, device=dev).reshape(F, 3)


def events(fn, steps):
    """us per call of fn, `steps` calls between two device events after a warm-up"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(max(2, steps // 10)):
        fn()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def host_clock(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


class Term:
    """forward (+ backward) of fn(verts, points) eager, and captured into a graph"""

    def __init__(self, fn, verts, points, backward, graph=True):
        self.fn, self.backward = fn, backward
        self.v, self.p = verts.clone().requires_grad_(backward), points.clone().requires_grad_(backward)
        self.graph = None
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    self.eager()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.v.grad = self.p.grad = None
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.eager()
            self.graph.replay()
            torch.cuda.synchronize()

    def eager(self):
        self.v.grad = self.p.grad = None
        self.loss = self.fn(self.v, self.p)
        if self.backward:
            self.loss.backward()


def agree(label, u, v):
    dl = abs(float(u.loss) - float(v.loss)) / max(abs(float(v.loss)), 1e-30)
    dg = max(float((u.v.grad - v.v.grad).abs().max() / v.v.grad.abs().max()), float((u.p.grad - v.p.grad).abs().max() / v.p.grad.abs().max()))
    assert dl <= 1e-5 and dg <= 1e-4, (label, dl, dg)
    return f"loss differs by {dl:.1e} relative, gradients by {dg:.1e} of their largest entry"


# ---- terms --------------------------------------------------------------------------------------------------------------------
sv, sf = demo.ico_sphere(4)
verts, faces = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(device=dev, dtype=torch.int32)
HIP, TORCH = "ops._PointMesh (HIP)", "Aggregation.point_mesh_term (torch, on the device)"


def kernels(v, p):
    return ops.point_mesh(v, faces, p)[0]


def definition(v, p):
    return Aggregation.point_mesh_term(v, faces, p)


for P, steps, def_steps in ((5000, 500, 3), (50000, 100, 1)):
    points = cloud(P, P)
    lines = [f"cfg5 sphere ({len(verts)} vertices, {len(faces)} faces) against {P} points = {P * len(faces):.2e} pairs; us per call, median (min - max) "
             f"of {reps} windows of {steps} calls ({def_steps} for the definition)"]
    for backward in (False, True):
        k = Term(kernels, verts, points, backward)
        what = "forward + backward" if backward else "forward"
        lines.append(f"  {what:18s} {HIP:52s} kernels (graph replay) {fmt([events(k.graph.replay, steps) for _ in range(reps)])}")
        lines.append(f"  {what:18s} {HIP:52s} whole call (eager)     {fmt([host_clock(k.eager, steps) for _ in range(reps)])}")
        if "--no-definition" in argv:
            lines.append(f"  {what:18s} {TORCH}: not measured")
            continue
        d = Term(definition, verts, points, backward, graph=False)
        lines.append(f"  {what:18s} {TORCH:52s} whole call (eager)     {fmt([host_clock(d.eager, def_steps) for _ in range(reps)])}")
        if backward:
            k.eager()
            lines.append("  " + agree(P, k, d))
        del d, k
    emit(lines)

# ---- the pair cap ---------------------------------------------------------------------------------------------------------------
if "--no-cap" not in argv:
    cap = ops.POINT_MESH_MAX_PAIRS
    bits = cap.bit_length() - 1
    P = 1 << ((bits + 1) // 2)
    F = cap // P - 1
    cv, cf = soup(F, 7)
    cp = cloud(P, 8, 1.0)
    assert P * F <= cap < (P + 1) * (F + 1)
    t_points = [events(lambda: ops.closest_faces(cp, cv, cf), 2) for _ in range(reps)]
    t_single = [events(lambda: ops.point_mesh(cv, cf, cp, False, True), 2) for _ in range(reps)]
    t_both = [events(lambda: ops.point_mesh(cv, cf, cp, False, False), 2) for _ in range(reps)]
    t_faces = [b - s for b, s in zip(t_both, t_single)]
    slower = max(statistics.median(t_points), statistics.median(t_faces))
    emit([f"just below the pair cap 2^{bits}: {P} points x {F} faces = {P * F:.3e} pairs (separate small triangles, uniform points); us per call, "
          f"median (min - max) of {reps} windows of 2 calls between device events",
          f"  points -> faces (voge_closest_faces)                       {fmt(t_points)}",
          f"  forward, single-directional                                {fmt(t_single)}",
          f"  forward, both directions                                   {fmt(t_both)}",
          f"  faces -> points (both minus single-directional)            {fmt(t_faces)}",
          f"  the slower direction: {slower / 1e6:.3f} s at the cap ({slower / (P * F) * 1e6:.3f} ps a pair); twice the cap would take {2 * slower / 1e6:.3f} s "
          "by proportion (not measured: the entries refuse it)"])
    assert slower < 1e6, slower
    del cv, cf, cp

# ---- the split over the waves ---------------------------------------------------------------------------------------------------
if "--no-split" not in argv:
    with _lib.using(_lib.AB_LIB_PATH) as ab:
        ab.voge_debug_point_mesh_waves.restype, ab.voge_debug_point_mesh_waves.argtypes = ctypes.c_int, [ctypes.c_int]
        emit([f"the candidates split over 16, 4 and 1 waves of a workgroup (the A/B build's switch; the product: 16 below 1024 workgroups of queries, "
              f"else 4): forward, both directions, eager between device events, us per call, median (min - max) of {reps} windows, alternating; "
              "the same bits: asserted"])
        for P, F in ((500, 5120), (5000, 5120), (50000, 5120), (5000, 320), (5000, 81920), (65536, 65536), (100000, 100000), (200000, 20000)):
            v, f = (verts, faces) if F == 5120 else soup(F, F)
            p = cloud(P, P + 1)
            t, outs = {16: [], 4: [], 1: []}, {}
            steps = max(2, min(300, int(3e9 / (P * F))))
            for _ in range(reps):
                for w in (16, 4, 1):
                    assert ab.voge_debug_point_mesh_waves(w) == 0
                    t[w].append(events(lambda: ops.point_mesh(v, f, p), steps))
                    outs[w] = ops.point_mesh(v, f, p)
            assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(outs[1], outs[4], outs[16])), (P, F)
            emit([f"  {P:7d} points x {F:6d} faces: 16 waves {fmt(t[16])}   4 waves {fmt(t[4])}   1 wave {fmt(t[1])}"])
        ab.voge_debug_point_mesh_waves(0)

# ---- launches -------------------------------------------------------------------------------------------------------------------
try:
    from torch.profiler import ProfilerActivity, profile
    points = cloud(5000, 3)
    for name, fn in ((HIP, kernels), (TORCH, definition)):
        t = Term(fn, verts, points, True, graph=False)
        for _ in range(2):
            t.eager()
        torch.cuda.synchronize()
        counts = []
        for part in ("forward", "backward"):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                if part == "forward":
                    t.v.grad = t.p.grad = None
                    loss = fn(t.v, t.p)
                else:
                    loss.backward()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                     and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            counts.append(f"{part} {len(names)} kernels ({sum('pm_' in n or 'chamfer_loss' in n or 'voge_fill' in n for n in names)} of this library)")
        emit([f"launches of one eager call, 5000 points, {name}: " + ", ".join(counts)])
except Exception as e:      # noqa: BLE001  (the profiler is optional: say so, do not guess)
    emit([f"launches: not measured ({type(e).__name__}: {e})"])
