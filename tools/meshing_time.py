"""Times of mesh extraction (VoGE.Meshing: voge_tsdf_integrate, voge_mtet_count / _scan / _emit) on one GPU.  No time is fixed in
advance.
  fusion      a 256^3 volume, 32 views of 512^2 analytic ray-sphere depth maps (r = 0.6, eyes at distance 3 on a spiral), trunc = 4 h:
              ops.tsdf_integrate (ONE launch a call) between two device events, `steps` calls a window, median (min - max) of `reps`
              windows; Aggregation.tsdf_integrate (the definition) in fp32 on the device, one call a window.  Both start from an empty
              volume for the comparison that is printed: the share of equal weights and the largest |tsdf| difference where they are.
  extraction  the 256^3 sphere's signed distance: count, scan and emit between device events of their own (the read-back of the two
              totals sits between scan and emit and is given as host time), and the whole of ops.marching_tets by the host clock;
              Aggregation.marching_tets in fp32 on the device, by the host clock around a synchronise.  Faces must be equal: asserted.
usage: python tools/meshing_time.py [reps] [--out FILE] [--small]      (--small: 64^3, 4 views of 128^2 -- a dry run of the tool)"""
import math
import statistics
import sys
import time

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5
small = "--small" in argv

import torch      # noqa: E402
from voge_amd import Aggregation, _lib, ops      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform, pixel_rays      # noqa: E402

assert torch.cuda.is_available(), "meshing_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)
N, B, IMG = (64, 4, 128) if small else (256, 32, 512)
RADIUS = 0.6


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


def fmt(us):
    return f"{statistics.median(us):10.1f} ({min(us):.1f} - {max(us):.1f})"


def events(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


# ---- fusion -------------------------------------------------------------------------------------------------------------------
k = torch.arange(B, dtype=torch.float32)
elev = (torch.asin(2 * (k + 0.5) / B - 1) * (180 / math.pi) * 0.8).tolist()
azim = ((k * 137.50776) % 360).tolist()
R, T = look_at_view_transform([3.0] * B, elev, azim, degrees=True)
focal = 150.0 * IMG / 96
cams = PerspectiveCameras(focal_length=focal, principal_point=((IMG / 2 - 0.37, IMG / 2 + 0.29),), R=R, T=T, device=dev)
rays, centres = pixel_rays(cams, (IMG, IMG))      # unit directions [B,H,W,3], centres [B,3]
bq = (rays * centres[:, None, None, :]).sum(-1)
disc = bq * bq - ((centres * centres).sum(-1)[:, None, None] - RADIUS ** 2)
depth = torch.where(disc > 0, -bq - disc.clamp(min=0).sqrt(), torch.full_like(bq, float("inf"))).contiguous()
del rays, bq, disc
lo, h = (-1.013,) * 3, (2.0 / (N - 1),) * 3
trunc = 4 * h[0]
Rd, Td = cams.R.contiguous(), cams.T.contiguous()
f2 = torch.full((B, 2), focal, device=dev)
p2 = torch.tensor([[IMG / 2 - 0.37, IMG / 2 + 0.29]], device=dev).expand(B, 2).contiguous()
cen = Aggregation.camera_centres(Rd.double(), Td.double()).float()
tsdf = torch.zeros((N, N, N), device=dev)
weight = torch.zeros((N, N, N), device=dev)
run = lambda: ops.tsdf_integrate(tsdf, weight, depth, Rd, Td, cen, f2, p2, lo, h, trunc)
run()
torch.cuda.synchronize()
k_t, k_w = tsdf.clone(), weight.clone()
zero = torch.zeros((N, N, N), device=dev)
define = lambda: Aggregation.tsdf_integrate(zero, zero, depth, Rd, Td, f2, p2, lo, h, trunc, centre=cen)
d_t, d_w = define()
same = d_w == k_w
lines = [f"fusion: {N}^3 grid points, {B} views of {IMG}^2 depth maps, trunc = 4 h; us per call, median (min - max) of {reps} windows, "
         f"device events",
         f"  weights equal at {float(same.float().mean()) * 100:.4f} % of the grid points (the others sit on a pixel or truncation boundary), "
         f"largest |tsdf| difference where they are {float((d_t - k_t)[same].abs().max()):.3e}; weights up to {int(k_w.max())}, "
         f"{float((k_w > 0).float().mean()) * 100:.1f} % of the grid points observed"]
del d_t, d_w, same
steps = 3 if small else 20
lines.append(f"  ops.tsdf_integrate (HIP, one launch, {steps} calls a window)       {fmt([events(run, steps) for _ in range(reps)])}")
lines.append(f"  Aggregation.tsdf_integrate (torch, on the device, 1 call a window)  {fmt([events(define, 1) for _ in range(min(reps, 3))])}")
moved = 16 * N ** 3
lines.append(f"  the kernel moves {moved / 1e6:.0f} MB a call and does {B * N ** 3 / 1e6:.0f} M projections")
emit(lines)
del depth, tsdf, weight, zero, k_t, k_w

# ---- extraction ---------------------------------------------------------------------------------------------------------------
ax = torch.arange(N, device=dev, dtype=torch.float32)
c = (N - 1) * torch.tensor([0.4913, 0.5107, 0.4989])
values = (((ax.view(1, 1, N) - c[0]) ** 2 + (ax.view(1, N, 1) - c[1]) ** 2 + (ax.view(N, 1, 1) - c[2]) ** 2).sqrt() - 0.37 * N).contiguous()
lib = _lib.load()
n = N ** 3
nb = (n + ops.MTET_BLOCK - 1) // ops.MTET_BLOCK


def staged():
    """ops.marching_tets' calls with events between them -> (count, scan, emit in us, read-back in us of host time, verts, faces)"""
    edge_mask = torch.empty((n,), dtype=torch.uint8, device=dev)
    face_count = torch.empty((n,), dtype=torch.uint8, device=dev)
    loc = torch.empty((2, n), dtype=torch.int16, device=dev)
    blocks = torch.empty((2, nb), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    st = ops._stream()
    p = lambda t_: t_.data_ptr()
    ev[0].record()
    _lib.check(lib.voge_mtet_count(p(values), None, N, N, N, 0.0, p(edge_mask), p(face_count), p(loc[0]), p(loc[1]), p(blocks[0]), p(blocks[1]), st),
               "voge_mtet_count")
    ev[1].record()
    _lib.check(lib.voge_mtet_scan(p(blocks[0]), p(blocks[1]), nb, p(totals), st), "voge_mtet_scan")
    ev[2].record()
    t0 = time.perf_counter()
    V, F = (int(x) for x in totals.tolist())
    back = (time.perf_counter() - t0) * 1e6
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    ev[3].record()
    _lib.check(lib.voge_mtet_emit(p(values), None, N, N, N, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, p(edge_mask), p(face_count), p(loc[0]), p(loc[1]),
                                  p(blocks[0]), p(blocks[1]), V, F, p(verts), p(faces), st), "voge_mtet_emit")
    ev[4].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3, ev[1].elapsed_time(ev[2]) * 1e3, ev[3].elapsed_time(ev[4]) * 1e3, back, verts, faces


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


staged()
rows = [staged() for _ in range(reps)]
verts, faces = rows[0][4], rows[0][5]
whole = [host_clock(lambda: ops.marching_tets(values, None, 0.0, (0.0,) * 3, (1.0,) * 3))[0] for _ in range(reps)]
host_clock(lambda: Aggregation.marching_tets(values))
ref_us, (ref_v, ref_f) = host_clock(lambda: Aggregation.marching_tets(values))
assert torch.equal(ref_f.to(torch.int32), faces)
dv = float((ref_v - verts).abs().max())
lines = [f"extraction: the signed distance of a sphere on {N}^3 grid points: V {len(verts)}, F {len(faces)}; us, median (min - max) of {reps} runs",
         f"  faces equal to the definition's on the device, vertices differ by at most {dv:.3e} (both fp32)",
         f"  voge_mtet_count (device events)                                  {fmt([r[0] for r in rows])}",
         f"  voge_mtet_scan  (device events)                                  {fmt([r[1] for r in rows])}",
         f"  the totals read back (host clock, includes waiting for the scan)  {fmt([r[3] for r in rows])}",
         f"  voge_mtet_emit  (device events)                                  {fmt([r[2] for r in rows])}",
         f"  ops.marching_tets, the whole call (host clock)                   {fmt(whole)}",
         f"  Aggregation.marching_tets (torch, on the device; host clock, 1 run) {ref_us:10.1f}"]
emit(lines)
