"""Times of mesh depth maps (VoGE.Meshing.rasterize_mesh: voge_mesh_raster_fwd / _bwd) on one GPU, both routes at every shape.  No
time or ratio is fixed in advance: correctness is the bar, and the two routes must return the same bits wherever both run.
  cfg5 sphere   the level-4 icosphere (5 120 faces) under five 128^2 views: forward and forward + backward on both routes, and
                Aggregation.mesh_rasterize, the chunked definition, on the device in the same process (same faces required).
  crossover     icospheres of levels 2 .. 7 (320 .. 327 680 faces) under five 128^2 views and one 512^2 view, forward on both
                routes: the work B x tiles x F on either side of ops.MESH_RASTER_BINS_MIN_WORK, and where "bins" first wins.
  fit           one iteration of demo/FitMeshToDepth.py (level 4, six 128^2 views), eager and replayed as a HIP graph.
  large         the 256^3 sphere of tools/meshing_time.py (about 10^6 faces) under one and eight 512^2 views, forward, both routes.
  launches      NOT counted by a run: read from the entry points' stage masks in csrc/mesh_raster.hip -- brute 2 forward, bins 7
                (records, zero fill, count, two scans | list fill, raster), backward 4 (fill, largest term, scatter, finish).
Times: us a call, median (min - max) of `reps` samples; a sample is a window of as many calls as fill about 20 ms (at least one),
by the host clock around a synchronise (the bins route's read-back included), after warm-up calls.  Where two routes are compared
their samples alternate.
usage: python tools/mesh_raster_time.py [reps] [--out FILE] [--small] [--skip-large | --only-large]
       (--small: no large shape, levels 2 .. 4 -- a dry run; the large shape's brute calls take seconds: send it with its own time limit)"""
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 7
small = "--small" in argv
skip_large, only_large = "--skip-large" in argv or small, "--only-large" in argv

import torch            # noqa: E402
from voge_amd import Aggregation, Meshing, ops      # noqa: E402
from voge_amd.cameras import look_at_view_transform      # noqa: E402

assert torch.cuda.is_available(), "mesh_raster_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)


def load_demo(name):
    spec = importlib.util.spec_from_file_location(name + "_for_mesh_raster_time", os.path.join("demo", name + ".py"))
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
    return f"{statistics.median(us):10.1f} ({min(us):.1f} - {max(us):.1f})"


WINDOW_US = 20000.0


def window(fn, calls):
    """us a call over one window of `calls` calls, and the last result"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls, out


def timed_many(fns, n=None):
    """[(samples, last result)] of several functions whose samples ALTERNATE: two warm-up calls each, a window sized from the second"""
    calls = []
    for fn in fns:
        fn()
        calls.append(max(1, min(500, int(WINDOW_US / max(window(fn, 1)[0], 1.0)))))
    us, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(n or reps):
        for k, fn in enumerate(fns):
            t, outs[k] = window(fn, calls[k])
            us[k].append(t)
    return list(zip(us, outs))


def timed(fn, n=None):
    return timed_many([fn], n)[0]


class Cams:
    def __init__(self, views, image, dist, focal):
        R, T = look_at_view_transform([dist] * views, [25.0 if k % 2 == 0 else -25.0 for k in range(views)],
                                      [360.0 * k / views + 10.0 for k in range(views)], degrees=True)
        self.R, self.T = R.to(dev), T.to(dev)
        self.focal_length = torch.full((views, 2), float(focal), device=dev)
        self.principal_point = torch.full((views, 2), image / 2 + 0.37, device=dev)


def work(B, image, F):
    t = (image + ops.MESH_RASTER_TILE - 1) // ops.MESH_RASTER_TILE
    return B * t * t * F


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


ico = load_demo("ShapeFitting").ico_sphere
emit([f"mesh depth maps: us a call, median (min - max) of {reps} samples, a sample a window of calls of about 20 ms by the host clock around a "
      f"synchronise, after two warm-up calls; compared routes alternate; "
      f"ops.MESH_RASTER_BINS_MIN_WORK = {ops.MESH_RASTER_BINS_MIN_WORK}"])

outs = {}
if not only_large:
    # ---- the cfg5 sphere ------------------------------------------------------------------------------------------------------------
    sv, sf = ico(4)
    verts, faces = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(device=dev, dtype=torch.int32)
    cams = Cams(5, 128, 2.7, 150.0)
    g = torch.randn((5, 128, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for route in ("brute", "bins"):
        fwd, outs[route] = timed(lambda: Meshing.rasterize_mesh(verts, faces, cams, (128, 128), route=route))

        def both():
            v = verts.detach().requires_grad_(True)
            (Meshing.rasterize_mesh(v, faces, cams, (128, 128), route=route).depth * g).sum().backward()
            return v.grad

        fb, grad = timed(both)
        outs[route + " grad"] = grad
        emit([f"  cfg5 sphere ({len(faces)} faces, five 128^2 views, work {work(5, 128, len(faces)):.3g}), {route:5s}: forward {fmt(fwd)}   "
              f"forward + backward {fmt(fb)}"])
    assert same(outs["brute"], outs["bins"]) and torch.equal(outs["brute grad"], outs["bins grad"])
    covered = float((outs["brute"].pix_to_face >= 0).float().mean())
    define = lambda: Aggregation.mesh_rasterize(verts, faces, cams.R, cams.T, cams.focal_length, cams.principal_point, 128, 128)
    d_us, ref = timed(define, 1)
    differ = ref[0] != outs["brute"].pix_to_face.long()
    emit([f"  the definition (Aggregation.mesh_rasterize, chunked, on the device): {d_us[0]:.1f}; {int(differ.sum())} of {differ.numel()} pixels choose "
          f"another face, {covered * 100:.1f} % of the pixels covered; elsewhere depth differs by at most "
          f"{float((ref[2] - outs['brute'].depth).abs()[~differ].max()):.3e} (the device's torch kernels round their own way; the tests compare with the host)"])

    # ---- the crossover --------------------------------------------------------------------------------------------------------------
    emit(["  crossover: forward, both routes, icospheres of rising level; work = B x tiles x F"])
    for views, image, focal in ((5, 128, 150.0), (1, 512, 600.0)):
        cams = Cams(views, image, 2.7, focal)
        for level in range(2, 5 if small else 8):
            sv, sf = ico(level)
            v, f = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(device=dev, dtype=torch.int32)
            pair = timed_many([lambda: Meshing.rasterize_mesh(v, f, cams, (image, image), route="brute"),
                               lambda: Meshing.rasterize_mesh(v, f, cams, (image, image), route="bins")])
            rows = {"brute": pair[0][0], "bins": pair[1][0]}
            outs["brute"], outs["bins"] = pair[0][1], pair[1][1]
            assert same(outs["brute"], outs["bins"])
            wins = "bins" if statistics.median(rows["bins"]) < statistics.median(rows["brute"]) else "brute"
            emit([f"    {views} x {image}^2, {len(f):7d} faces, work {work(views, image, len(f)):10.3g}: brute {fmt(rows['brute'])}   bins {fmt(rows['bins'])}"
                  f"   -> {wins}"])

    # ---- one iteration of the fit ---------------------------------------------------------------------------------------------------
    demo = load_demo("FitMeshToDepth")
    for graph in (False, True):
        run = demo.fit(iters=3, level=4, views=6, image=128, graph=graph, quiet=True)
        us, _ = timed(run["replay"], max(reps, 20))
        emit([f"  demo/FitMeshToDepth.py, one iteration (5 120 faces, six 128^2 views, brute), {'graph replay' if graph else 'eager':12s}: {fmt(us)}"])

# ---- the large mesh -------------------------------------------------------------------------------------------------------------
if not skip_large:
    N = 256
    ax = torch.arange(N, device=dev, dtype=torch.float32)
    c = (N - 1) * torch.tensor([0.4913, 0.5107, 0.4989])
    values = (((ax.view(1, 1, N) - c[0]) ** 2 + (ax.view(1, N, 1) - c[1]) ** 2 + (ax.view(N, 1, 1) - c[2]) ** 2).sqrt() - 0.37 * N).contiguous()
    verts, faces = ops.marching_tets(values, None, 0.0, (0.0,) * 3, (1.0,) * 3)
    del values
    verts = ((verts - c.to(dev)) / (0.37 * N)).contiguous()      # the unit sphere about the origin
    for views in (1, 8):
        cams = Cams(views, 512, 2.7, 600.0)
        for route in ("bins", "brute"):
            us, outs[route] = timed(lambda: Meshing.rasterize_mesh(verts, faces, cams, (512, 512), route=route), 3)
            emit([f"  the 256^3 sphere ({len(faces)} faces), {views} x 512^2, work {work(views, 512, len(faces)):.3g}, {route:5s}: forward {fmt(us)} (3 runs)"])
        assert same(outs["brute"], outs["bins"])
emit(["  launches (read from the stage masks of csrc/mesh_raster.hip, not counted by this run): brute 2 forward; bins 7 forward and one read-back; backward 4"])
