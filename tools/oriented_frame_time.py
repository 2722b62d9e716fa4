"""Frame time of the three ways to render ORIENTED Gaussians (three scales + a quaternion each) at cfg3 (50k Gaussians, 512^2,
K = 40; forward + backward of to_white_background(...).sum(), HIP-graph replay as bench.py times it):
  (a) an [N,3,3] leaf parameter holding S = R diag(s) R^T -- the floor: no orientation parameters at all;
  (b) S composed in torch from (scales, quats) leaves in front of (a)'s route -- what a user writes without the oriented form
      (this file carries its own copy of the composition, so (a) and (b) run on a checkout that lacks the form);
  (c) Meshes.OrientedGaussianMeshes on the frame path (voge_frame_trace_fwd_ori / voge_frame_bwd_ori), when the package has it.
The legs are interleaved: `reps` rounds, each timing `steps` replays of every leg in turn (device events); the spread is the
range of a leg's rounds.
usage: python tools/oriented_frame_time.py [steps] [reps] [--out FILE]
       python tools/oriented_frame_time.py --eager LEG STEPS        (5 warm + STEPS eager steps of one leg: for a kernel trace)
       python tools/oriented_frame_time.py --launches [--out FILE]  (kernel launches per step of every leg, from
                                                                     `rocprofv3 --kernel-trace --stats` child runs of --eager;
                                                                     the first child that fails ends the run)
per-kernel times of a leg:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/oriented_frame_time.py --eager LEG 50
                            python tools/rocprof_summary.py DIR"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, ".")
argv = sys.argv[1:]
out_file = argv[argv.index("--out") + 1] if "--out" in argv else None
LEGS = ("a", "b", "c")


def emit(lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_file:
        with open(out_file, "a") as f:
            f.write(text)


def launches_of(leg, steps):
    """Kernel dispatches of one --eager run (a fresh child process under the profiler).  A child that does not end with status 0
    ends this program too, with the child's output shown: nothing more is started on the GPU after a failure."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__,
               "--eager", leg, str(steps)]
        try:
            child = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
            status, said = child.returncode, child.stdout
        except subprocess.TimeoutExpired as e:
            status, said = "timeout", (e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""))
        if status != 0:
            sys.stderr.write(f"leg ({leg}), {steps} steps: `{' '.join(cmd)}` ended with {status}; its output:\n{said}\n"
                             "stopping here: no further GPU run is started\n")
            sys.exit(1)
        rows = 0
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                rows += sum(1 for _ in csv.DictReader(fh))
        return rows


if "--launches" in argv:
    # (which legs this checkout has is read from the package, without a GPU run: a failing child is never taken for a missing leg)
    from voge_amd import Meshes as _meshes
    lines = ["kernel launches per step (rocprofv3 --kernel-trace --stats, eager steps; the difference of a 30-step and a 10-step run / 20):"]
    for leg in LEGS:
        if leg == "c" and not hasattr(_meshes, "OrientedGaussianMeshesNaive"):
            lines.append("  (c) this checkout has no oriented form")
            continue
        lines.append(f"  ({leg}) {(launches_of(leg, 30) - launches_of(leg, 10)) / 20:.2f}")
    emit(lines)
    sys.exit(0)

import torch      # noqa: E402
from voge_amd import Meshes, scenes      # noqa: E402
from voge_amd.Meshes import GaussianMeshesNaive      # noqa: E402
from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings, to_white_background      # noqa: E402
from voge_amd.cameras import PerspectiveCameras, look_at_view_transform      # noqa: E402


QUAT_TERMS = (((2, 2, -2.0), (3, 3, -2.0)), ((1, 2, 2.0), (0, 3, -2.0)), ((1, 3, 2.0), (0, 2, 2.0)),
              ((1, 2, 2.0), (0, 3, 2.0)), ((1, 1, -2.0), (3, 3, -2.0)), ((2, 3, 2.0), (0, 1, -2.0)),
              ((1, 3, 2.0), (0, 2, -2.0)), ((2, 3, 2.0), (0, 1, 2.0)), ((1, 1, -2.0), (2, 2, -2.0)))
QUAT_MAP = torch.zeros((16, 9))
for col, terms in enumerate(QUAT_TERMS):
    for qa, qb, coef in terms:
        QUAT_MAP[4 * qa + qb, col] = coef
QUAT_MAP = QUAT_MAP.to("cuda:0")
EYE = torch.eye(3, device="cuda:0")


def compose(scales, quats):
    """S = R(q / |q|) diag(scales) R^T in torch in front of the [N,3,3] renderer input: a copy of Aggregation.oriented_sigma
    (R - I as one constant [16,9] map of the products q_a q_b; the upper triangle of S mirrored), with its constants made once."""
    n2 = (quats * quats).sum(-1, keepdim=True)
    ok = (n2 > 0) & torch.isfinite(n2)
    unit = torch.zeros_like(quats)
    unit[..., 0] = 1
    qs = torch.where(ok, quats, unit)
    qh = qs / torch.sqrt((qs * qs).sum(-1, keepdim=True))
    outer = (qh[..., :, None] * qh[..., None, :]).reshape(quats.shape[:-1] + (16,))
    R = (outer @ QUAT_MAP).reshape(quats.shape[:-1] + (3, 3)) + EYE
    p = (scales[..., None, :] * R)[..., :, None, :] * R[..., None, :, :]
    S = (p[..., 0] + p[..., 1]) + p[..., 2]
    return torch.triu(S) + torch.triu(S, 1).transpose(-1, -2)


dev = torch.device("cuda", 0)
N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS["cfg3_50k_512"]
verts_np, sig_np, cols_np = scenes.random_gaussians(N, seed=0)
gen = torch.Generator().manual_seed(0)
scales0 = (torch.from_numpy(sig_np)[:, None] * (0.3 + 1.2 * torch.rand((N, 3), generator=gen))).to(dev)
quats0 = (torch.randn((N, 4), generator=gen) * (0.5 + 1.5 * torch.rand((N, 1), generator=gen))).to(dev)
verts = torch.from_numpy(verts_np).to(dev).requires_grad_(True)
colors = torch.from_numpy(cols_np).to(dev).requires_grad_(True)
R, T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev)
renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
one = torch.ones((), dtype=torch.float32, device=dev)

sigma_leaf = compose(scales0, quats0).detach().requires_grad_(True)
scales_b, quats_b = scales0.clone().requires_grad_(True), quats0.clone().requires_grad_(True)
scales_c, quats_c = scales0.clone().requires_grad_(True), quats0.clone().requires_grad_(True)
has_c = hasattr(Meshes, "OrientedGaussianMeshesNaive")
MESH = {"a": lambda: GaussianMeshesNaive(verts, sigma_leaf),
        "b": lambda: GaussianMeshesNaive(verts, compose(scales_b, quats_b))}
PARAMS = {"a": [verts, colors, sigma_leaf], "b": [verts, colors, scales_b, quats_b], "c": [verts, colors, scales_c, quats_c]}
if has_c:
    MESH["c"] = lambda: Meshes.OrientedGaussianMeshesNaive(verts, scales_c, quats_c)
NAMES = {"a": "(a) [N,3,3] leaf", "b": "(b) composed in torch + (a)'s route", "c": "(c) oriented frame path"}


def frame(leg):
    for p in PARAMS[leg]:
        p.grad = None
    to_white_background(renderer(MESH[leg](), R=R, T=T), colors).sum().backward(one)


if "--eager" in argv:
    leg, n_steps = argv[argv.index("--eager") + 1], int(argv[argv.index("--eager") + 2])
    if leg not in MESH:
        sys.exit(f"leg ({leg}) is not available on this checkout")
    for _ in range(5 + n_steps):
        frame(leg)
    torch.cuda.synchronize()
    sys.exit(0)

plain = [a for a in argv if not a.startswith("--") and a != out_file]
steps = int(plain[0]) if plain else 100
reps = int(plain[1]) if len(plain) > 1 else 7
graphs = {}
for leg in MESH:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            frame(leg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs[leg] = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs[leg]):
        frame(leg)
    for _ in range(10):
        graphs[leg].replay()
torch.cuda.synchronize()
times = {leg: [] for leg in graphs}
for _ in range(reps):
    for leg, g in graphs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        times[leg].append(a.elapsed_time(b) / steps)
lines = [f"cfg3: {N} Gaussians, {H}x{W}, K = {K}; forward + backward of to_white_background(...).sum(); HIP-graph replay, ms per step: "
         f"median (min - max) of {reps} interleaved rounds of {steps} replays"]
med = {}
for leg, v in times.items():
    med[leg] = statistics.median(v)
    lines.append(f"  {NAMES[leg]:38s} {med[leg]:.4f} ({min(v):.4f} - {max(v):.4f})")
spread = max(max(v) - min(v) for v in times.values())
lines.append(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):+.1f} us" + (f";  (c) - (a) = {1e3 * (med['c'] - med['a']):+.1f} us;  (c) - (b) = "
             f"{1e3 * (med['c'] - med['b']):+.1f} us" if has_c else "") + f";  largest spread of a leg's rounds {1e3 * spread:.1f} us")
if not has_c:
    lines.append("  (c): this checkout has no oriented form")
emit(lines)
