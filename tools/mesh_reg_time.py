"""What the mesh regularisers (VoGE.Losses.mesh_regularisers: edge 1.0, laplacian 0.1, normal 0.5 -- all three terms on) cost.
 1. The cfg5 shape-fitting iteration (demo/ShapeFitting.py: ico-sphere level 4 = 2562 vertices, 128^2, 5 views, replayed as a HIP
    graph) in three variants: (a) without regularisers, (b) with the HIP node (ops._MeshReg), (c) with the torch definitions of
    voge_amd/Aggregation.py on the device in its place.  Each variant is one demo.fit() run of `iters` iterations, timed by the
    host clock from iteration 50 to a device synchronise after the last; the variants ALTERNATE, `reps` runs each, the median.
 2. forward + backward of the three terms alone at the cfg5 mesh and at a 1000 x 1000 grid mesh (1 M vertices, 3 M edges, 3 M
    face pairs), (b) against (c): captured once, replayed `steps` times between device events, the variants alternating.
No ratio is fixed in advance.  (b) and (c) are checked against each other at the sizes that are timed before anything is timed.
usage: python tools/mesh_reg_time.py [reps] [--iters N] [--out FILE]
       python tools/mesh_reg_time.py --eager VARIANT SIZE STEPS   (VARIANT b | c, SIZE cfg5 | grid; 5 warm + STEPS eager forward +
                                                                   backward steps of the terms alone: for a kernel trace)
       python tools/mesh_reg_time.py --summary DIR [--out FILE]   (of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR
                                     -- python tools/mesh_reg_time.py --eager ...` run: launches per step -- the period of the
                                     trace's sequence of kernel names -- and the mesh_reg kernels' durations)"""
import csv
import glob
import importlib.util
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
WEIGHTS = {"edge": 1.0, "laplacian": 0.1, "normal": 0.5}


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
    for key in ("mesh_reg_fwd_kernel", "mesh_reg_sum_kernel", "mesh_reg_bwd_kernel"):
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            lines.append(f"  {key}: median {statistics.median(us):.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches)")
    emit(lines)
    sys.exit(0)

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd import Aggregation      # noqa: E402
from voge_amd.Losses import MeshTopology, mesh_regularisers      # noqa: E402

dev = torch.device("cuda", 0)
spec = importlib.util.spec_from_file_location("shape_fitting_demo", os.path.join("demo", "ShapeFitting.py"))
demo = importlib.util.module_from_spec(spec)
spec.loader.exec_module(demo)


def definitions(verts, topo, target_length=0.0, terms=("edge", "laplacian", "normal")):
    """mesh_regularisers through the torch definitions, whatever the device"""
    zero = verts.new_zeros(())
    return (Aggregation.mesh_edge_term(verts, topo.edges, target_length) if "edge" in terms else zero,
            Aggregation.mesh_laplacian_term(verts, topo.nbr_off, topo.nbr) if "laplacian" in terms else zero,
            Aggregation.mesh_normal_term(verts, topo.pairs) if "normal" in terms else zero)


def grid_mesh(n):
    """an n x n height field over the unit square: n^2 vertices, 2 (n - 1)^2 faces"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = 0.05 * np.sin(0.02 * x) * np.cos(0.03 * y) + 0.002 * np.random.default_rng(0).uniform(-1, 1, (n, n))
    verts = np.stack([x / (n - 1), y / (n - 1), z], -1).reshape(-1, 3).astype(np.float32)
    i = (y[:-1, :-1] * n + x[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([i, i + 1, i + n], -1), np.stack([i + 1, i + n + 1, i + n], -1)])
    return verts, faces


class Terms:
    """forward + backward of the weighted terms alone"""

    def __init__(self, size):
        verts, faces = demo.ico_sphere(4) if size == "cfg5" else grid_mesh(1000)
        self.topo = MeshTopology(faces=faces, num_verts=verts.shape[0], device=dev)
        self.verts = torch.tensor(verts, device=dev, requires_grad=True)
        self.name = (f"{size}: {self.topo.num_verts} vertices, {self.topo.num_edges} edges, {self.topo.num_pairs} face pairs, "
                     f"max degree {self.topo.max_degree}")

    def step(self, variant, keep=False):
        self.verts.grad = None
        out = (mesh_regularisers if variant == "b" else definitions)(self.verts, self.topo)
        sum(WEIGHTS[k] * o for k, o in zip(WEIGHTS, out)).backward()
        return [o.detach().clone() for o in out] + [self.verts.grad.clone()] if keep else None


if "--eager" in argv:
    variant, size, steps = argv[argv.index("--eager") + 1], argv[argv.index("--eager") + 2], int(argv[argv.index("--eager") + 3])
    case = Terms(size)
    for _ in range(5 + steps):
        case.step(variant)
    torch.cuda.synchronize()
    print(f"eager run done: variant {variant}, {case.name}, {5 + steps} steps")
    sys.exit(0)

args = [a for k, a in enumerate(argv) if not a.startswith("--") and (k == 0 or argv[k - 1] not in ("--out", "--iters"))]
reps = int(args[0]) if args else 5
iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 1050

# ---- 2. the terms alone ---------------------------------------------------------------------------------------------------------
def replay_window(case, variant, steps):
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
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    del graph
    return a.elapsed_time(b) / steps


for size, steps in (("cfg5", 2000), ("grid", 200)):
    case = Terms(size)
    got = {v: case.step(v, keep=True) for v in ("b", "c")}
    torch.cuda.synchronize()
    for x, y, what in zip(got["b"], got["c"], ("edge", "laplacian", "normal", "g_verts")):
        err = (x - y).abs().max().item() / max(y.abs().max().item(), 1e-30)
        assert err < 1e-4, (size, what, err)
    out = {"b": [], "c": []}
    for r in range(reps):
        for v in out:
            out[v].append(replay_window(case, v, steps))
    lines = [f"{case.name}; forward + backward of the three terms alone; graph replay, us per step, median (min - max) of {reps} "
             f"windows of {steps} steps, the variants alternating"]
    for v, name in (("b", "(b) ops._MeshReg (HIP)"), ("c", "(c) Aggregation definitions (torch, on the device)")):
        us = [1e3 * x for x in out[v]]
        lines.append(f"  {name:52s} {statistics.median(us):9.2f} ({min(us):.2f} - {max(us):.2f})")
    emit(lines)
    del case

# ---- 1. the cfg5 iteration ------------------------------------------------------------------------------------------------------
VARIANTS = {"a": "(a) no regularisers", "b": "(b) mesh_regularisers (HIP node)", "c": "(c) Aggregation definitions (torch)"}
kernel_route = demo.mesh_regularisers
out = {k: [] for k in VARIANTS}
for r in range(reps):
    for k in VARIANTS:
        demo.mesh_regularisers = definitions if k == "c" else kernel_route
        h = demo.fit(iters=iters, graph=True, timed_from=50, quiet=True, regularise=None if k == "a" else dict(WEIGHTS))
        out[k].append(1e3 * h["sec_per_iter"])
        print(f"  run {r} ({k}): {out[k][-1]:.4f} ms per iteration, silhouette {h['silhouette'][-1]:.5f}", flush=True)
demo.mesh_regularisers = kernel_route
med = {k: statistics.median(v) for k, v in out.items()}
lines = [f"cfg5 iteration (level 4, 128^2, 5 views, SGD) replayed as a HIP graph; ms per iteration over iterations 50 .. {iters}, "
         f"median (min - max) of {reps} runs, the variants alternating"]
for k, name in VARIANTS.items():
    lines.append(f"  {name:42s} {med[k]:.4f} ({min(out[k]):.4f} - {max(out[k]):.4f})")
lines.append(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):.1f} us, (c) - (a) = {1e3 * (med['c'] - med['a']):.1f} us; spread of the repeated (a) runs "
             f"{1e3 * (max(out['a']) - min(out['a'])):.1f} us")
emit(lines)
