"""Times of the mesh simplification (VoGE.Meshing.simplify_mesh: voge_mesh_simplify_scan / _emit / _attr) on one GPU.  No time or
ratio is fixed in advance: correctness is the bar.
  mesh        the 256^3 sphere of tools/meshing_time.py (ops.marching_tets of its signed distance, voxel 1) with C = 3 attribute
              channels.
  calls       simplify_mesh(..., attr=, return_index=True) at cells of 2, 4 and 8 voxels under both placements by the host clock
              around a synchronise (the call's own read-back included), median (min - max) of `reps` runs after a warm-up call;
              Aggregation.mesh_simplify, the definition, on the device in the same process the same way, one run after a warm-up.
              Faces and index tables must be equal; the largest position and attribute difference is reported.
  launches    every launch group of the three entry points between device events of its own (the `stages` masks of
              include/voge_hip.h), at every cell size, "quadric".
usage: python tools/mesh_simplify_time.py [reps] [--out FILE] [--small]      (--small: 64^3 -- a dry run of the tool)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
reps = int(argv[0]) if argv and argv[0].isdigit() else 5
small = "--small" in argv

import torch      # noqa: E402
from voge_amd import Aggregation, Meshing, _lib, ops      # noqa: E402

assert torch.cuda.is_available(), "mesh_simplify_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)
N = 64 if small else 256
CELLS = (2.0, 4.0, 8.0)
C = 3


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


def fmt(us):
    return f"{statistics.median(us):10.1f} ({min(us):.1f} - {max(us):.1f})"


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def staged(entry, masks):
    """us of every launch group of `masks`, between device events: entry(mask) launches the stages of one mask"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(masks) + 1)]
    ev[0].record()
    for k, mask in enumerate(masks):
        entry(mask)
        ev[k + 1].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(len(masks))]


# ---- the mesh -----------------------------------------------------------------------------------------------------------------
ax = torch.arange(N, device=dev, dtype=torch.float32)
c = (N - 1) * torch.tensor([0.4913, 0.5107, 0.4989])
values = (((ax.view(1, 1, N) - c[0]) ** 2 + (ax.view(1, N, 1) - c[1]) ** 2 + (ax.view(N, 1, 1) - c[2]) ** 2).sqrt() - 0.37 * N).contiguous()
verts, faces = ops.marching_tets(values, None, 0.0, (0.0,) * 3, (1.0,) * 3)
del values
attr = (0.5 + 0.5 * torch.sin(verts * 0.05)).contiguous()
V, F = len(verts), len(faces)
fl = faces.long()
emit([f"mesh simplification: the {N}^3 sphere: V {V}, F {F}, C = {C}; us, median (min - max) of {reps} runs, host clock around a synchronise "
      f"(the read-back included); the definition (Aggregation.mesh_simplify) on the device, 1 run after a warm-up"])

# ---- the calls and the definition -----------------------------------------------------------------------------------------------
for cell in CELLS:
    for placement in ("mean", "quadric"):
        call = lambda: Meshing.simplify_mesh(verts, faces, cell, placement, attr=attr, return_index=True)
        call()
        us = []
        for _ in range(reps):
            t, out = host_clock(call)
            us.append(t)
        define = lambda: Aggregation.mesh_simplify(verts, fl, cell, placement, attr)
        define()
        d_us, ref = host_clock(define)
        assert torch.equal(out[1].long(), ref[1]) and torch.equal(out[3].long(), ref[3]) and torch.equal(out[4].long(), ref[4])
        dv, da = float((out[0] - ref[0]).abs().max()), float((out[2] - ref[2]).abs().max())
        emit([f"  cell {cell:g} voxels, {placement:7s}: V' {len(out[0]):7d}, F' {len(out[1]):7d}   simplify_mesh {fmt(us)}   definition {d_us:12.1f}"
              f"   faces and index tables equal, positions differ by at most {dv:.3e}, attributes by {da:.3e}"])
        del ref, out

# ---- the launches ---------------------------------------------------------------------------------------------------------------
lib = _lib.load()
p = lambda t_: t_.data_ptr()
st = ops._stream()
nbytes = lib.voge_mesh_simplify_workspace_bytes(V, F)
ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
totals = torch.empty((3,), dtype=torch.int64, device=dev)
emit([f"  the launches, \"quadric\", device events, us, median (min - max) of {reps} runs; workspace {nbytes / 2 ** 20:.1f} MiB"])
for cell in CELLS:
    def scan_entry(mask):
        _lib.check(lib.voge_mesh_simplify_scan(p(verts), V, p(faces), F, cell, cell, cell, p(ws), nbytes, p(totals), mask, st), "voge_mesh_simplify_scan")

    scan_rows = [staged(scan_entry, (1, 2, 4, 8, 16, 32, 64, 128)) for _ in range(reps + 1)][1:]
    Vk, Fk, bad = (int(x) for x in totals.tolist())
    assert not bad
    acc_bytes = lib.voge_mesh_simplify_acc_bytes(Vk, 1)
    acc = torch.empty((acc_bytes // 8,), dtype=torch.int64, device=dev)
    out_v, out_f = torch.empty((Vk, 3), device=dev), torch.empty((Fk, 3), dtype=torch.int32, device=dev)
    vi, fi = torch.empty((V,), dtype=torch.int32, device=dev), torch.empty((Fk,), dtype=torch.int32, device=dev)

    def emit_entry(mask):
        _lib.check(lib.voge_mesh_simplify_emit(p(verts), V, p(faces), F, cell, cell, cell, 1, p(ws), nbytes, Vk, Fk, p(acc), acc_bytes, p(out_v),
                                               p(out_f), p(vi), p(fi), mask, st), "voge_mesh_simplify_emit")

    emit_rows = [staged(emit_entry, (1, 2, 4, 8)) for _ in range(reps + 1)][1:]
    abytes = lib.voge_mesh_simplify_attr_workspace_bytes(Vk)
    aws = torch.empty((abytes // 8,), dtype=torch.int64, device=dev)
    out_a = torch.empty((Vk, C), device=dev)

    def attr_entry(mask):
        _lib.check(lib.voge_mesh_simplify_attr(p(attr), V, F, C, 0, C, p(ws), nbytes, Vk, p(acc), 1, p(aws), abytes, p(out_a), mask, st),
                   "voge_mesh_simplify_attr")

    attr_rows = [staged(attr_entry, (1, 2, 4, 8)) for _ in range(reps + 1)][1:]
    want = Meshing.simplify_mesh(verts, faces, cell, "quadric", attr=attr)
    assert torch.equal(out_v, want[0]) and torch.equal(out_f, want[1]) and torch.equal(out_a, want[2])
    col = lambda rows, k: fmt([r[k] for r in rows])
    emit([f"    cell {cell:g} voxels: V' {Vk}, F' {Fk}",
          f"      voge_mesh_simplify_scan   fills + box {col(scan_rows, 0)}   cells {col(scan_rows, 1)}   labels {col(scan_rows, 2)}   triples "
          f"{col(scan_rows, 3)}",
          f"                                refill + faces {col(scan_rows, 4)}   flags {col(scan_rows, 5)}   local scan {col(scan_rows, 6)}   top scan "
          f"{col(scan_rows, 7)}",
          f"      voge_mesh_simplify_emit   fill {col(emit_rows, 0)}   indices + sums {col(emit_rows, 1)}   quadrics {col(emit_rows, 2)}   finish "
          f"{col(emit_rows, 3)}",
          f"      voge_mesh_simplify_attr   fill {col(attr_rows, 0)}   largest value {col(attr_rows, 1)}   scatter {col(attr_rows, 2)}   finish "
          f"{col(attr_rows, 3)}"])
