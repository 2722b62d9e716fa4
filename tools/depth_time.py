"""Step time of a depth loss at cfg3 (50k Gaussians, 512^2, K = 40; forward + backward of depth.sum()) for three ways to the
same normalised depth map:
  (i)   the torch expression on the fragments' tensors, masked by valid_num -- what a user writes without get_depth;
  (ii)  get_depth on weights that already exist (ops._Depth: voge_depth_fwd / _bwd behind the deferred composite);
  (iii) get_depth on the renderer's fragments (ops._CompositeDepth: voge_frame_depth_fwd_iso / _bwd_iso, one pass each way).
Each variant eager and replayed from a captured graph; the variants ALTERNATE window by window in one process (one graph alive
at a time: a window's graph is captured in front of it and dropped behind it); times from device events around `steps` steps, the
median of `reps` windows.  A step keeps NOTHING of its autograd graph alive: a depth map held across steps keeps the parameters'
AccumulateGrad nodes of the eager warm-up -- and their stream, the default one -- in use, and a captured step whose two backward
nodes meet in such a node pulls the default stream into the capture (ending that capture crashed inside the HIP runtime).
usage: python tools/depth_time.py [steps] [reps]      (--ktrace [--only i|ii|iii]: run eagerly, for rocprofv3 --kernel-trace)"""
import faulthandler
import statistics
import sys

import torch

sys.path.insert(0, ".")
from voge_amd import scenes      # noqa: E402
from voge_amd.Meshes import GaussianMeshes      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, get_depth      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402

faulthandler.enable()
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in ("i", "ii", "iii")]
steps = int(args[0]) if args else 30
reps = int(args[1]) if len(args) > 1 else 5
ktrace = "--ktrace" in sys.argv
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
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


def torch_depth(frag):
    w, ln = frag.vert_weight, frag.vert_hit_length
    live = slots < frag.valid_num[..., None]
    w = torch.where(live, w, torch.zeros_like(w))
    a = (w * torch.where(live, ln, torch.zeros_like(ln))).sum(-1)
    s = w.sum(-1)
    return torch.where(s > 0, a / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))


def depth_node(frag):
    _ = frag.vert_weight      # (the composite runs now: get_depth finds finished weights)
    return get_depth(frag)


VARIANTS = {"i": ("(i)   torch expression, masked", torch_depth), "ii": ("(ii)  get_depth, ops._Depth", depth_node),
            "iii": ("(iii) get_depth, one pass", get_depth)}
if only is not None:
    VARIANTS = {only: VARIANTS[only]}


def step(fn, keep=False):
    for p in params:
        p.grad = None
    d = fn(renderer(gm, R=R, T=T))
    d.sum().backward()
    return d.detach().clone() if keep else None      # (never the map itself: see the docstring)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def replay_window(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(fn)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fn)
    graph.replay()
    torch.cuda.synchronize()
    ms = window(graph.replay)
    del graph
    return ms


def alternate(measure):
    out = {k: [] for k in VARIANTS}
    for r in range(reps):
        for k, (_, fn) in VARIANTS.items():
            out[k].append(measure(fn))
            print(f"  window {r} {k}: {out[k][-1]:.4f} ms", flush=True)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


ref = None
for key, (name, fn) in VARIANTS.items():
    for _ in range(5):
        d = step(fn, keep=True)
    torch.cuda.synchronize()
    if ktrace:
        for _ in range(steps):
            step(fn)
        torch.cuda.synchronize()
        continue
    # the three must be the same map and the same gradients, at the size that is timed
    cur = (d, gm.verts.grad.clone(), gm.sigmas.grad.clone())
    if ref is None:
        ref = cur
    for a, b, what in zip(cur, ref, ("depth", "g_verts", "g_sigmas")):
        err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
        assert err < 1e-4, (key, what, err)
if ktrace:
    print("ktrace run done")
    sys.exit(0)
print("eager windows", flush=True)
eager = alternate(lambda fn: window(lambda: step(fn)))
print("graph-replay windows", flush=True)
replay = alternate(replay_window)
print(f"cfg3: {N} Gaussians, {H}x{W}, K = {K}; forward + backward of depth.sum(), normalize=True; ms per step, median (min - max) "
      f"of {reps} windows of {steps} steps, the variants alternating")
for key, (name, _) in VARIANTS.items():
    e, g = eager[key], replay[key]
    print(f"{name:34s} eager {e[0]:.4f} ({e[1]:.4f} - {e[2]:.4f})   graph {g[0]:.4f} ({g[1]:.4f} - {g[2]:.4f})")
if "i" in replay:
    for key in ("ii", "iii"):
        if key in replay:
            print(f"{VARIANTS[key][0].split()[0]} / (i): eager {eager[key][0] / eager['i'][0]:.3f}, graph replay "
                  f"{replay[key][0] / replay['i'][0]:.3f}")
