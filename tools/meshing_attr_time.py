"""Times of attributes through the mesh extraction (voge_tsdf_integrate_attr, voge_mtet_attr) on one GPU, beside the calls without
them.  No time is fixed in advance; the only number known beforehand is the traffic, (16 + 8 C) / 16 of the plain call's.
  fusion      tools/meshing_time.py's case: a 256^3 volume, 32 views of 512^2 analytic ray-sphere depth maps, trunc = 4 h, and a seeded
              uniform colour image [32,512,512,C] beside them, C = 3 unless --channels says otherwise.  ops.tsdf_integrate without and
              with attr= (ONE launch a call either way; the first is the kernel of the call without attributes, which this
              feature does not touch) between two device events, `steps` calls a window, the two ALTERNATING, median (min - max) of
              `reps` windows each; Aggregation.tsdf_integrate with attr= (the definition) in fp32 on the device, one call a window.
              Printed before any time: tsdf and weight of the two kernels are equal (asserted), and the largest |attr| difference
              from the definition where the weights agree.
  extraction  the 256^3 sphere's signed distance with a seeded [256,256,256,C] attribute: voge_mtet_emit and voge_mtet_attr between
              device events of their own, on the tables of one count and scan, alternating.
usage: python tools/meshing_attr_time.py [reps] [--channels C] [--out FILE] [--small]      (--small: 64^3, 4 views of 128^2 -- a dry run)"""
import math
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
C = int(argv[argv.index("--channels") + 1]) if "--channels" in argv else 3
reps = int(argv[0]) if argv and argv[0].isdigit() else 5
small = "--small" in argv

import torch      # noqa: E402
from voge_amd import Aggregation, _lib, ops      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform, pixel_rays      # noqa: E402

assert torch.cuda.is_available(), "meshing_attr_time.py measures on a GPU: none is visible"
assert 1 <= C <= ops.MTET_MAX_CHANNELS
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
image = torch.rand((B, IMG, IMG, C), generator=torch.Generator().manual_seed(0)).to(dev)
lo, h = (-1.013,) * 3, (2.0 / (N - 1),) * 3
trunc = 4 * h[0]
Rd, Td = cams.R.contiguous(), cams.T.contiguous()
f2 = torch.full((B, 2), focal, device=dev)
p2 = torch.tensor([[IMG / 2 - 0.37, IMG / 2 + 0.29]], device=dev).expand(B, 2).contiguous()
cen = Aggregation.camera_centres(Rd.double(), Td.double()).float()
grid = lambda *tail: torch.zeros((N, N, N) + tail, device=dev)
p_t, p_w = grid(), grid()
a_t, a_w, a_a = grid(), grid(), grid(C)
plain = lambda: ops.tsdf_integrate(p_t, p_w, depth, Rd, Td, cen, f2, p2, lo, h, trunc)
fused = lambda: ops.tsdf_integrate(a_t, a_w, depth, Rd, Td, cen, f2, p2, lo, h, trunc, attr=a_a, attr_image=image)
plain()
fused()
torch.cuda.synchronize()
assert torch.equal(p_t, a_t) and torch.equal(p_w, a_w), "the attribute kernel must leave tsdf and weight with the plain kernel's bits"
zero, zero_a = grid(), grid(C)
define = lambda: Aggregation.tsdf_integrate(zero, zero, depth, Rd, Td, f2, p2, lo, h, trunc, centre=cen, attr=zero_a, attr_image=image)
d_t, d_w, d_a = define()
same = d_w == a_w
lines = [f"fusion: {N}^3 grid points, {B} views of {IMG}^2 depth maps and [{B},{IMG},{IMG},{C}] colour images, trunc = 4 h; us per call, median "
         f"(min - max) of {reps} windows, device events, the two kernels in alternating windows",
         f"  tsdf and weight of the two kernels: equal bits; weights equal to the definition's at {float(same.float().mean()) * 100:.4f} % of the "
         f"grid points, largest |attr| difference where they are {float((d_a - a_a)[same].abs().max()):.3e}; weights up to {int(a_w.max())}, "
         f"{float((a_w > 0).float().mean()) * 100:.1f} % of the grid points observed"]
del d_t, d_w, d_a, same
steps = 3 if small else 20
t_plain, t_fused = [], []
for _ in range(reps):
    t_plain.append(events(plain, steps))
    t_fused.append(events(fused, steps))
t_def = [events(define, 1) for _ in range(min(reps, 3))]
ratio = statistics.median(t_fused) / statistics.median(t_plain)
lines += [f"  ops.tsdf_integrate (voge_tsdf_integrate, one launch, {steps} calls a window)                  {fmt(t_plain)}",
          f"  ops.tsdf_integrate(attr=) (voge_tsdf_integrate_attr, C = {C}, one launch, {steps} calls a window)  {fmt(t_fused)}",
          f"  Aggregation.tsdf_integrate(attr=) (torch, on the device, 1 call a window)                {fmt(t_def)}",
          f"  with attributes / without: {ratio:.3f} of the time for {(16 + 8 * C) / 16:.2f} of the traffic ({16 * N ** 3 / 1e6:.0f} MB -> "
          f"{(16 + 8 * C) * N ** 3 / 1e6:.0f} MB a call); the definition / the kernel: {statistics.median(t_def) / statistics.median(t_fused):.1f}"]
emit(lines)
del depth, image, p_t, p_w, a_t, a_w, a_a, zero, zero_a

# ---- extraction ---------------------------------------------------------------------------------------------------------------
ax = torch.arange(N, device=dev, dtype=torch.float32)
c = (N - 1) * torch.tensor([0.4913, 0.5107, 0.4989])
values = (((ax.view(1, 1, N) - c[0]) ** 2 + (ax.view(1, N, 1) - c[1]) ** 2 + (ax.view(N, 1, 1) - c[2]) ** 2).sqrt() - 0.37 * N).contiguous()
attr = torch.rand((N, N, N, C), generator=torch.Generator().manual_seed(1)).to(dev)
lib = _lib.load()
n = N ** 3
nb = (n + ops.MTET_BLOCK - 1) // ops.MTET_BLOCK
edge_mask = torch.empty((n,), dtype=torch.uint8, device=dev)
face_count = torch.empty((n,), dtype=torch.uint8, device=dev)
loc = torch.empty((2, n), dtype=torch.int16, device=dev)
blocks = torch.empty((2, nb), dtype=torch.int32, device=dev)
totals = torch.empty((2,), dtype=torch.int64, device=dev)
st = ops._stream()
p = lambda t_: t_.data_ptr()
_lib.check(lib.voge_mtet_count(p(values), None, N, N, N, 0.0, p(edge_mask), p(face_count), p(loc[0]), p(loc[1]), p(blocks[0]), p(blocks[1]), st),
           "voge_mtet_count")
_lib.check(lib.voge_mtet_scan(p(blocks[0]), p(blocks[1]), nb, p(totals), st), "voge_mtet_scan")
V, F = (int(x) for x in totals.tolist())
verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
vert_attr = torch.empty((V, C), dtype=torch.float32, device=dev)
emit_mesh = lambda: _lib.check(lib.voge_mtet_emit(p(values), None, N, N, N, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, p(edge_mask), p(face_count), p(loc[0]),
                                                  p(loc[1]), p(blocks[0]), p(blocks[1]), V, F, p(verts), p(faces), st), "voge_mtet_emit")
emit_attr = lambda: _lib.check(lib.voge_mtet_attr(p(values), N, N, N, 0.0, p(attr), C, p(edge_mask), p(loc[0]), p(blocks[0]), V, p(vert_attr), st),
                               "voge_mtet_attr")
emit_mesh()
emit_attr()
torch.cuda.synchronize()
ref = Aggregation.marching_tets(values, attr=attr)
assert torch.equal(ref[1].to(torch.int32), faces)
da = float((ref[2] - vert_attr).abs().max())
del ref
t_emit, t_attr = [], []
for _ in range(reps):
    t_emit.append(events(emit_mesh, 1))
    t_attr.append(events(emit_attr, 1))
emit([f"extraction: the signed distance of a sphere on {N}^3 grid points with a [{N},{N},{N},{C}] attribute: V {V}, F {F}; us, median (min - max) of "
      f"{reps} runs, device events, alternating",
      f"  vert_attr differs from the definition's on the device by at most {da:.3e} (both fp32)",
      f"  voge_mtet_emit                     {fmt(t_emit)}",
      f"  voge_mtet_attr (C = {C})              {fmt(t_attr)}"])
