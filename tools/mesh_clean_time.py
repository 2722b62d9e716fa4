"""Times of the mesh clean-up (VoGE.Meshing: voge_mesh_components, voge_mesh_clean_scan / _emit, voge_vertex_normals) on one GPU.  No
time is fixed in advance.
  mesh        the 256^3 sphere of tools/meshing_time.py (ops.marching_tets of its signed distance) plus 4000 small tetrahedra
              scattered around it: the floaters of a fused volume.
  calls       connected_components, clean_mesh(keep_largest=1) and vertex_normals by the host clock around a synchronise, median
              (min - max) of `reps` runs; their Aggregation definitions on the device the same way, one run.  Labels, faces and index
              tables must be equal, the normals within 1e-5: asserted.
  launches    every launch of the three entry points between device events of its own (the `stages` masks of include/voge_hip.h).
usage: python tools/mesh_clean_time.py [reps] [--out FILE] [--small]      (--small: 64^3 and 200 tetrahedra -- a dry run of the tool)"""
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

assert torch.cuda.is_available(), "mesh_clean_time.py measures on a GPU: none is visible"
dev = torch.device("cuda", 0)
N, BLOBS = (64, 200) if small else (256, 4000)


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
sv, sf = ops.marching_tets(values, None, 0.0, (0.0,) * 3, (1.0,) * 3)
del values
g = torch.Generator().manual_seed(0)
tet = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
centres = torch.rand((BLOBS, 1, 3), generator=g) * (N - 1)
bv = (centres + tet[None] * (0.5 + torch.rand((BLOBS, 1, 1), generator=g))).reshape(-1, 3).to(dev)
bf = (torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])[None] + 4 * torch.arange(BLOBS)[:, None, None]).reshape(-1, 3)
verts = torch.cat([sv, bv]).contiguous()
faces = torch.cat([sf, (bf + len(sv)).to(torch.int32).to(dev)]).contiguous()
V, F = len(verts), len(faces)
del sv, sf, bv, bf

# ---- the calls and their definitions --------------------------------------------------------------------------------------------
cc_us, cl_us, vn_us = [], [], []
Meshing.connected_components(faces, V), Meshing.clean_mesh(verts, faces, keep_largest=1), Meshing.vertex_normals(verts, faces)
for _ in range(reps):
    t, comp = host_clock(lambda: Meshing.connected_components(faces, V))
    cc_us.append(t)
    t, cleaned = host_clock(lambda: Meshing.clean_mesh(verts, faces, keep_largest=1, return_index=True))
    cl_us.append(t)
    t, normals = host_clock(lambda: Meshing.vertex_normals(verts, faces))
    vn_us.append(t)
fl = faces.long()
d_cc_us, d_comp = host_clock(lambda: Aggregation.mesh_components(fl, V))
d_cl_us, d_clean = host_clock(lambda: Aggregation.mesh_clean(verts, fl, 1, 1))
d_vn_us, d_normals = host_clock(lambda: Aggregation.mesh_vertex_normals(verts, fl))
assert torch.equal(comp[0].long(), d_comp[0]) and torch.equal(comp[1].long(), d_comp[1]) and comp[2] == d_comp[2] == BLOBS + 1
assert torch.equal(cleaned[0], d_clean[0]) and all(torch.equal(a.long(), b) for a, b in zip(cleaned[1:], d_clean[1:]))
dn = float((normals - d_normals).abs().max())
assert dn < 1e-5, dn
lines = [f"mesh clean-up: the {N}^3 sphere plus {BLOBS} tetrahedra: V {V}, F {F}, {comp[2]} components; us, median (min - max) of {reps} runs, host "
         f"clock around a synchronise; the definitions on the device, 1 run",
         f"  labels, cleaned mesh and index tables equal to the definitions'; normals differ by at most {dn:.3e}; the largest component keeps "
         f"V {len(cleaned[0])}, F {len(cleaned[1])}",
         f"  Meshing.connected_components (3 launches, 1 synchronisation)        {fmt(cc_us)}      Aggregation.mesh_components     {d_cc_us:12.1f}",
         f"  Meshing.clean_mesh (components, ranking, 5 launches, 2 synchron.)   {fmt(cl_us)}      Aggregation.mesh_clean          {d_cl_us:12.1f}",
         f"  Meshing.vertex_normals (4 launches, nothing read back)              {fmt(vn_us)}      Aggregation.mesh_vertex_normals {d_vn_us:12.1f}"]
emit(lines)
del d_comp, d_clean, d_normals, fl

# ---- the launches ---------------------------------------------------------------------------------------------------------------
lib = _lib.load()
p = lambda t_: t_.data_ptr()
st = ops._stream()
i32 = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
parent, vert_label, face_label, count, meta = i32(V), i32(V), i32(F), i32(V), i32(4)


def cc_entry(mask):
    _lib.check(lib.voge_mesh_components(p(faces), F, V, p(parent), p(vert_label), p(face_label), p(count), p(meta), mask, st), "voge_mesh_components")


cc_rows = [staged(cc_entry, (1, 2, 4)) for _ in range(reps + 1)][1:]
keep = Aggregation.mesh_keep_roots(count, 1, 1).to(torch.uint8)
nb = (V + ops.MESH_CLEAN_BLOCK - 1) // ops.MESH_CLEAN_BLOCK + (F + ops.MESH_CLEAN_BLOCK - 1) // ops.MESH_CLEAN_BLOCK
vflag = torch.empty(((V + 3) // 4 * 4,), dtype=torch.uint8, device=dev)
loc = torch.empty((V + F,), dtype=torch.int16, device=dev)
blocks, err, totals = i32(nb), i32(1), torch.empty((3,), dtype=torch.int64, device=dev)


def scan_entry(mask):
    _lib.check(lib.voge_mesh_clean_scan(p(faces), F, V, p(face_label), p(keep), p(vflag), p(loc), p(blocks), p(err), p(totals), mask, st),
               "voge_mesh_clean_scan")


scan_rows = [staged(scan_entry, (1, 2, 4, 8)) for _ in range(reps + 1)][1:]
Vk, Fk, bad = (int(x) for x in totals.tolist())
assert not bad and (Vk, Fk) == (len(cleaned[0]), len(cleaned[1]))
out_v = torch.empty((Vk, 3), device=dev)
out_f, vert_index, face_index = torch.empty((Fk, 3), dtype=torch.int32, device=dev), i32(Vk), i32(Fk)


def emit_entry(_mask):
    _lib.check(lib.voge_mesh_clean_emit(p(verts), p(faces), F, V, p(face_label), p(keep), p(vflag), p(loc), p(blocks), Vk, Fk, p(out_v), p(out_f),
                                        p(vert_index), p(face_index), st), "voge_mesh_clean_emit")


emit_rows = [staged(emit_entry, (0,)) for _ in range(reps + 1)][1:]
assert torch.equal(out_f, cleaned[1]) and torch.equal(out_v, cleaned[0])
nbytes = lib.voge_vertex_normals_workspace_bytes(V)
ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
out_n = torch.empty((V, 3), device=dev)


def vn_entry(mask):
    _lib.check(lib.voge_vertex_normals(p(verts), V, p(faces), F, p(out_n), p(ws), nbytes, mask, st), "voge_vertex_normals")


vn_rows = [staged(vn_entry, (1, 2, 4, 8)) for _ in range(reps + 1)][1:]
assert torch.equal(out_n, normals)
col = lambda rows, k: fmt([r[k] for r in rows])
lines = [f"  the launches, device events, us, median (min - max) of {reps} runs",
         f"    voge_mesh_components   init {col(cc_rows, 0)}   link {col(cc_rows, 1)}   labels {col(cc_rows, 2)}",
         f"    voge_mesh_clean_scan   fill {col(scan_rows, 0)}   mark {col(scan_rows, 1)}   local scan {col(scan_rows, 2)}   top scan {col(scan_rows, 3)}",
         f"    voge_mesh_clean_emit   {col(emit_rows, 0)}",
         f"    voge_vertex_normals    fill {col(vn_rows, 0)}   largest component {col(vn_rows, 1)}   scatter {col(vn_rows, 2)}   finish {col(vn_rows, 3)}"]
emit(lines)
