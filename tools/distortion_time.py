"""Step time of a distortion-regulariser loss at cfg3 (50k Gaussians, 512^2, K = 40; scenes.CONFIGS["cfg3_50k_512"]): forward +
backward of (...).sum() on the renderer's fragments for
  (0) get_depth on the finished weights (ops._Depth)          -- tools/depth_time.py's (ii): a streaming pair over the same bytes, the base;
  (a) get_distortion(frag)                                      -- ops._Distortion: voge_distortion_fwd / _bwd, one launch each way;
  (b) Aggregation.distortion(w, len, valid_num)                 -- the definition in torch: stable sort, gathers, two cumsums;
  (c) the naive [.., K, K] expression, masked by valid_num      -- 1.7 GB of fp32 a temporary at this size; skipped if it does not fit.
Every variant reads frag.vert_weight first, so all of them sit behind the same deferred composite.  Each is replayed from a
captured graph; the variants ALTERNATE window by window in one process (one graph alive at a time), times from device events
around `steps` replays, the median of `reps` windows.  A step keeps nothing of its autograd graph alive (tools/depth_time.py
says why).
usage: python tools/distortion_time.py [steps] [reps] [--out FILE]
       python tools/distortion_time.py --eager VARIANT STEPS        (5 warm + STEPS eager steps: for a kernel trace)
       python tools/distortion_time.py --summary DIR [--out FILE]   (of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
                                          python tools/distortion_time.py --eager ...` run: launches per step -- the period of the
                                          trace's sequence of kernel names -- and the two kernels' durations with the bytes they
                                          have to move over that time: 8 B a slot forward, 8 read + 8 written backward)"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None


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
    slots = 512 * 512 * 40
    for key, nbytes in (("distortion_fwd", 8 * slots), ("distortion_bwd", 16 * slots)):
        us = [(e - s) / 1e3 for s, e, nm in rows if key in nm]
        if us:
            us = us[len(us) // 2:]
            med = statistics.median(us)
            lines.append(f"  {key}_kernel: median {med:.2f} us (min {min(us):.2f}, max {max(us):.2f}, {len(us)} launches); {nbytes / 1e6:.2f} MB "
                         f"to move -> {nbytes / med / 1e6:.3f} TB/s")
    emit(lines)
    sys.exit(0)

import torch      # noqa: E402
from voge_amd import scenes      # noqa: E402
from voge_amd.Aggregation import distortion      # noqa: E402
from voge_amd.Meshes import GaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth, get_distortion      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402

dev = torch.device("cuda", 0)
N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
verts, sig, _ = scenes.random_gaussians(N, seed=0)
gm = GaussianMeshes(torch.from_numpy(verts), torch.from_numpy(sig)).to(dev)
gm.verts.requires_grad_(True)
gm.sigmas.requires_grad_(True)
R, T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev)
renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
params = [gm.verts, gm.sigmas]
slots = torch.arange(K, device=dev)


def naive(frag):
    w, ln = frag.vert_weight, frag.vert_hit_length
    live = slots < frag.valid_num[..., None]
    w = torch.where(live, w, torch.zeros_like(w))
    ln = torch.where(live, ln, torch.zeros_like(ln))
    return (w[..., :, None] * w[..., None, :] * (ln[..., :, None] - ln[..., None, :]).abs()).sum((-1, -2))


def depth_node(frag):
    _ = frag.vert_weight
    return get_depth(frag)


VARIANTS = {"0": ("(0) get_depth on the finished weights (the base)", depth_node),
            "a": ("(a) get_distortion", get_distortion),
            "b": ("(b) Aggregation.distortion (torch: sort + cumsum)", lambda f: distortion(f.vert_weight, f.vert_hit_length, f.valid_num)),
            "c": ("(c) naive [.., K, K] expression (torch)", naive)}


def step(variant, keep=False):
    for p in params:
        p.grad = None
    out = VARIANTS[variant][1](renderer(gm, R=R, T=T))
    out.sum().backward()
    return out.detach().clone() if keep else None      # (never the map itself)


if "--eager" in argv:
    variant, steps = argv[argv.index("--eager") + 1], int(argv[argv.index("--eager") + 2])
    for _ in range(5 + steps):
        step(variant)
    torch.cuda.synchronize()
    print(f"eager run done: variant {variant}, {5 + steps} steps")
    sys.exit(0)

args = [a for a in argv if not a.startswith("--") and a != out_file]
steps = int(args[0]) if args else 30
reps = int(args[1]) if len(args) > 1 else 5


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def replay_window(variant):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(variant)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(variant)
    graph.replay()
    torch.cuda.synchronize()
    ms = window(graph.replay)
    del graph
    return ms


# (a), (b) and (c) must be the same map and the same gradients, at the size that is timed
got = {}
for variant in ("a", "b", "c"):
    try:
        for _ in range(3):
            out = step(variant, keep=True)
        torch.cuda.synchronize()
    except torch.cuda.OutOfMemoryError:
        print(f"  {VARIANTS[variant][0]}: does not fit into the device's memory, skipped", flush=True)
        del VARIANTS[variant]
        torch.cuda.empty_cache()
        continue
    got[variant] = [out] + [p.grad.clone() for p in params]
for variant in got:
    if variant == "a":
        continue
    for x, y, what in zip(got["a"], got[variant], ("distortion", "g_verts", "g_sigmas")):
        err = ((x - y).abs().max() / max(1.0, y.abs().max().item())).item()
        print(f"  (a) against ({variant}), {what}: max {err:.2e} of scale", flush=True)
        # ((c) differentiates |t_i - t_j| with sign(0) = 0: at exact ties its gradients are another subgradient, by definition)
        assert err < 1e-4 or (variant == "c" and what != "distortion"), (variant, what, err)
lit = float((got["a"][0] > 0).float().mean())
del got
torch.cuda.empty_cache()
res = {k: [] for k in VARIANTS}
notes = []
for r in range(reps):
    for k in list(VARIANTS):
        try:
            res[k].append(replay_window(k))
        except RuntimeError as e:      # (a torch expression that does not capture: reported, not timed)
            notes.append(f"  {VARIANTS[k][0]}: the step could not be captured and replayed ({str(e).splitlines()[0][:120]}), not timed")
            del VARIANTS[k], res[k]
            torch.cuda.synchronize()
            continue
        print(f"  window {r} ({k}): {res[k][-1]:.4f} ms", flush=True)
med = {k: statistics.median(v) for k, v in res.items()}
lines = [f"cfg3: {N} Gaussians, {H}x{W}, K = {K}, {100 * lit:.1f} % of the pixels with a positive distortion; forward + backward of "
         f"(...).sum(); graph replay, ms per step, median (min - max) of {reps} windows of {steps} steps, the variants alternating"]
for k, (name, _) in VARIANTS.items():
    lines.append(f"  {name:52s} {med[k]:.4f} ({min(res[k]):.4f} - {max(res[k]):.4f})")
lines.append("  " + ", ".join(f"({k}) - (0) = {1e3 * (med[k] - med['0']):.1f} us" for k in VARIANTS if k != "0")
             + f"; spread of the repeated (0) windows {1e3 * (max(res['0']) - min(res['0'])):.1f} us")
emit(lines + notes)
