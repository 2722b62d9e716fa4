"""Times of the two routes of the point-to-mesh distance (ops.closest_faces / ops.point_mesh, route "brute" against route "grid") in
one process on one GPU.  No time is fixed in advance.
  routes    closest_faces, the forward of both directions and forward + backward, each between two device events after a warm-up;
            the figure is the median (min - max) of `reps` windows, the routes alternating.  Both routes must return the same bits
            at every shape timed: asserted.  Shapes: the cfg5 sphere (5 120 faces) against 5 000 and 50 000 points; a ladder of
            spheres against clouds of two classes -- "box": uniform in the cube around the sphere, most points many cells from
            the surface; "near": within 0.02 of the surface, what a fit or a score sees --; lopsided pairs; a mesh of mostly large triangles; a 512 x 512 height field of
            524 287 faces against 524 288 points (just below the pair cap); the level set of the 256^3 sphere (1 011 492 faces)
            against 438 544 points -- demo/RenderPointClouds.py's cloud as it is, and as many points within 0.02 of the surface --,
            where the brute route refuses.
  work      per shape, from the grid the device chose (the workspace's head) and the d2 it returned: the length of the large list,
            the rings a point walked (the first ring at which the stopping rule could fire on its d2) and the pair evaluations
            a point made (the large list plus the small triangles of the cells in its cube; a 3-D prefix sum of the cell counts).
  crossover per class, the smallest P F of the ladder from which the grid route is faster in closest_faces AND in the faces'
            direction by more than the spread of the repeats at every larger shape, rounded up to a power of two.  kPmGridMinPairs
            is the larger of the two: the shapes of a call cannot tell the classes apart.
usage: python tools/point_mesh_grid_time.py [reps] [--out FILE] [--no-large]"""
import importlib.util
import math
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5

import numpy as np      # noqa: E402
import torch      # noqa: E402
from voge_amd import Meshing, ops      # noqa: E402

assert torch.cuda.is_available(), "point_mesh_grid_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join("demo", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


def fmt(us):
    return f"{statistics.median(us):11.1f} ({min(us):.1f} - {max(us):.1f})"


def events(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def sphere(level):
    v, f = load("ShapeFitting").ico_sphere(level)
    return torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(device=dev, dtype=torch.int32)


def cloud(n, seed, scale=1.3):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(((rng.random((n, 3), dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)).to(dev)


def shell(n, seed, radius=1.0, width=0.02):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * (radius + rng.uniform(-width, width, (n, 1)))
    return torch.from_numpy(d.astype(np.float32)).to(dev)


def work(v, f, p, d2):
    """(large-list length, mean and max rings a point walked, mean and max pair evaluations a point made) after a grid-route call"""
    head = next(iter(ops._WS.values()))[:64].clone()
    w = head.view(torch.int32).tolist()
    fl = head.view(torch.float32).tolist()
    lo, cell, inv, g, nlarge, H = fl[0:3], fl[3], fl[4], w[5:8], w[9], fl[10]
    lo_t = torch.tensor(lo, device=dev)

    def cells(x):
        return torch.minimum(torch.floor((x - lo_t) * inv).clamp(min=0), torch.tensor(g, device=dev) - 1.0).long()
    tri = v[f.long()]
    tlo, thi = tri.min(1).values, tri.max(1).values
    mid = 0.5 * tlo + 0.5 * thi
    h = torch.maximum(thi - mid, mid - tlo).max(1).values * (1 + 2.0 ** -22)
    small = torch.isfinite(h) & (h <= H)
    fc = cells(mid[small])
    counts = torch.zeros((g[2] * g[1] * g[0],), dtype=torch.int64, device=dev)
    counts.index_add_(0, (fc[:, 2] * g[1] + fc[:, 1]) * g[0] + fc[:, 0], torch.ones(len(fc), dtype=torch.int64, device=dev))
    S = torch.nn.functional.pad(counts.view(g[2], g[1], g[0]), (1, 0, 1, 0, 1, 0)).cumsum(0).cumsum(1).cumsum(2)      # S[z, y, x]: cells below
    pc = cells(p)
    # the first ring at which the rule can fire on the returned d2: b(r) >= sqrt(d2), b = (cell (r - 2^-10) - H)(1 - 2^-8) - 2^-7 H
    need = (d2.double().sqrt() + 2.0 ** -7 * H) / (1 - 2.0 ** -8) + H
    r = torch.ceil(need / cell + 2.0 ** -10).clamp(min=math.ceil(ops.POINT_MESH_GRID_BIG) + 1).long()
    gt = torch.tensor(g, device=dev)
    rmax = torch.maximum(pc, gt - 1 - pc).max(1).values
    r = torch.minimum(r, rmax) if bool(small.any()) else torch.zeros_like(rmax)
    a, b = (pc - r[:, None]).clamp(min=0), torch.minimum(pc + r[:, None], gt - 1) + 1

    def at(x, y, z):
        return S[z, y, x]
    box = (at(b[:, 0], b[:, 1], b[:, 2]) - at(a[:, 0], b[:, 1], b[:, 2]) - at(b[:, 0], a[:, 1], b[:, 2]) - at(b[:, 0], b[:, 1], a[:, 2])
           + at(a[:, 0], a[:, 1], b[:, 2]) + at(a[:, 0], b[:, 1], a[:, 2]) + at(b[:, 0], a[:, 1], a[:, 2]) - at(a[:, 0], a[:, 1], a[:, 2]))
    pairs = box + nlarge
    return (f"grid {g[0]} x {g[1]} x {g[2]}, cell {cell:.4g}; large list {nlarge} of {len(f)}; rings a point: mean {float(r.float().mean()):.1f}, "
            f"max {int(r.max())}; pairs a point: mean {float(pairs.float().mean()):.0f}, max {int(pairs.max())} (brute: {len(f)})")


ladder = {"box": [], "near": []}


def shape(label, v, f, p, brute=True, steps=None, in_ladder=None):
    P, F = len(p), len(f)
    pairs = P * F
    if steps is None:
        steps = 20 if pairs < 1 << 30 else (3 if pairs < 1 << 36 else 1)
    routes = ("brute", "grid") if brute else ("grid",)
    vg, pg = v.clone().requires_grad_(True), p.clone().requires_grad_(True)

    def both(route):
        vg.grad = pg.grad = None
        ops.point_mesh(vg, f, pg, route=route)[0].backward()
    fns = {"closest_faces": lambda r: ops.closest_faces(p, v, f, route=r), "forward, single": lambda r: ops.point_mesh(v, f, p, False, True, route=r),
           "forward, both": lambda r: ops.point_mesh(v, f, p, route=r), "forward + backward": both}
    t = {(k, r): [] for k in fns for r in routes}
    for _ in range(reps):
        for k, fn in fns.items():
            for r in routes:
                t[(k, r)].append(events(lambda: fn(r), steps))
    out = ops.point_mesh(v, f, p, route="grid")
    d2 = ops.closest_faces(p, v, f, route="grid")[0]
    lines = [f"{label}: {P} points x {F} faces = {pairs:.3g} pairs ({steps} calls a window, {reps} windows, us a call)", "  " + work(v, f, p, d2)]
    if brute:
        ref = ops.point_mesh(v, f, p, route="brute")
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, ref)), label
        assert torch.equal(d2, ops.closest_faces(p, v, f, route="brute")[0]), label
        lines[0] += "; the two routes agree bit for bit"
    for k in fns:
        row = f"  {k:18s}"
        for r in routes:
            row += f"  {r} {fmt(t[(k, r)])}"
        if brute:
            row += f"  brute / grid {statistics.median(t[(k, 'brute')]) / statistics.median(t[(k, 'grid')]):.2f}"
        lines.append(row)
    emit(lines)
    if in_ladder and brute:
        def faster(kb, kg):      # grid faster by more than the spread of either route's repeats
            return max(t[kg]) < min(t[kb])
        face_b = [b - s for b, s in zip(t[("forward, both", "brute")], t[("forward, single", "brute")])]
        face_g = [b - s for b, s in zip(t[("forward, both", "grid")], t[("forward, single", "grid")])]
        ladder[in_ladder].append((pairs, label, faster(("closest_faces", "brute"), ("closest_faces", "grid")) and max(face_g) < min(face_b)))


emit([f"point_mesh_grid_time.py on {torch.cuda.get_device_name(0)}: kPmGridBig {ops.POINT_MESH_GRID_BIG}, kPmGridFloor {ops.POINT_MESH_GRID_FLOOR}, "
      f"{ops.POINT_MESH_GRID_BLOCK} queries a workgroup, POINT_MESH_GRID_MIN_PAIRS {ops.POINT_MESH_GRID_MIN_PAIRS}"])
meshes = {level: sphere(level) for level in (2, 3, 4, 5, 6)}
for level, P in ((4, 5000), (4, 50000), (3, 2000), (4, 1000), (4, 2000), (4, 12000), (5, 5000), (5, 20000), (6, 20000), (6, 200000)):
    name = "cfg5 sphere" if level == 4 and P in (5000, 50000) else f"level-{level} sphere"
    shape(f"{name}, box cloud", *meshes[level], cloud(P, 10 + level + P), in_ladder="box")
    shape(f"{name}, near cloud", *meshes[level], shell(P, 20 + level + P), in_ladder="near")
shape("lopsided: level-2 sphere (320 faces), 1 000 000 points", *meshes[2], cloud(1000000, 3))
shape("lopsided: level-6 sphere (81 920 faces), 500 points", *meshes[6], cloud(500, 4))
rng = np.random.default_rng(5)
big_v = torch.from_numpy((rng.random((3 * 4000, 3)) * 2 - 1).astype(np.float32)).to(dev)      # 4 000 triangles as large as the box
shape("mostly large triangles: 4 000 of the box's size + level-4 sphere", torch.cat((meshes[4][0], big_v)),
      torch.cat((meshes[4][1], torch.arange(3 * 4000, dtype=torch.int32, device=dev).reshape(-1, 3) + len(meshes[4][0]))), cloud(50000, 6))
if "--no-large" not in argv:
    n = 512
    xs, ys = torch.meshgrid(torch.arange(n + 1, dtype=torch.float32) / n, torch.arange(n + 1, dtype=torch.float32) / n, indexing="xy")
    hv = torch.stack((xs, ys, 0.2 * torch.sin(3 * xs) * torch.cos(2 * ys)), -1).reshape(-1, 3).to(dev)
    i = (torch.arange(n)[:, None] * (n + 1) + torch.arange(n)[None, :]).reshape(-1)
    hf = torch.cat((torch.stack((i, i + 1, i + n + 2), 1), torch.stack((i, i + n + 2, i + n + 1), 1))).int().to(dev)[:524287]
    hp = torch.rand((524288, 3), device=dev) * torch.tensor([1.0, 1.0, 0.5], device=dev) - torch.tensor([0.0, 0.0, 0.25], device=dev)
    shape("height field just below the pair cap", hv, hf, hp, steps=1)
    N = 256
    ax = torch.arange(N, dtype=torch.float32, device=dev)
    c = (N - 1) / 2
    values = (((ax.view(1, 1, N) - c) ** 2 + (ax.view(1, N, 1) - c) ** 2 + (ax.view(N, 1, 1) - c) ** 2).sqrt() - 0.37 * N).contiguous()
    mv, mf = Meshing.extract_mesh(values, lo=(-1.0, -1.0, -1.0), voxel_size=2.0 / (N - 1))
    del values
    pts = torch.from_numpy(load("RenderPointClouds").synthetic_cloud(438544)[0]).to(dev)
    shape("256^3 sphere's level set, the demo's cloud as it is", mv, mf.int(), pts, brute=False, steps=1)
    shape("256^3 sphere's level set, points within 0.02 of it", mv, mf.int(), shell(438544, 7, 0.37 * N * 2.0 / (N - 1)), brute=False, steps=3)
firsts = {}
for cls, rows in ladder.items():
    rows = sorted(rows)
    lost = [pairs for pairs, _, ok in rows if not ok]
    firsts[cls] = min((pairs for pairs, _, ok in rows if ok and all(y < pairs for y in lost)), default=None)
    emit([f"crossover, {cls} clouds: " + ", ".join(f"{pairs:.3g} {'grid' if ok else 'brute'}" for pairs, _, ok in rows),
          f"  the smallest P F from which the grid route wins in both directions at every larger shape of the ladder: {firsts[cls]}"
          + (f" -> 2^{math.ceil(math.log2(firsts[cls]))}" if firsts[cls] else " -> never below the pair cap")])
emit([f"kPmGridMinPairs: {'the pair cap, 2^38 (a class never wins below it)' if None in firsts.values() else max(firsts.values())}"])
