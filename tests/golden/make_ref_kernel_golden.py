#!/usr/bin/env python3
"""Record tests/golden/ref_kernels.npz: seeded inputs and what the REFERENCE'S OWN KERNELS return for them, from every one of
the nine entry points of oracle/_ref/voge_ref_C.so (built by oracle/build_ref.py).  Runs once on the MI355X:

    python tests/golden/make_ref_kernel_golden.py OUTDIR        # the run's output directory, where util.log_line keeps the parity log

and the file is then copied from OUTDIR into tests/golden/.  A fixture is data: inputs drawn here plus the kernels' outputs.
tests/test_oracle_cpu.py pins the fp64 oracle, the fp32 reference-order oracle, oracle/extras_np.py and oracle/coarse_np.py to it
on a machine without a GPU.

Sizes are around 16 x 20 pixels with K <= 12.  The fine-trace scenes are drawn until no decision of the selection lies within
TOL / 2 of its switch (ref_kernel_cases.decision_margins), so the recorded index lists are reproduced exactly by any evaluation
within TOL / 4 of fp64; the seeds found are stored beside the inputs.  The kernels are called through the checking wrappers of
tests/ref_kernels.py only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
import ref_kernel_cases as rc  # noqa: E402
from util import TOL  # noqa: E402

#              name    H   W  B   N   K  form    thr   lists   behind  list length
FIXTURE_FINE = [("fa", 16, 20, 1, 36, 12, "skew", 0.01, "holes", True, 30),
                ("fb", 20, 20, 2, 24, 5, "iso", 0.01, "full", False, 0),
                ("fc", 16, 20, 1, 10, 8, "sym", 0.0, "full", False, 0)]


def fine_inputs(spec, max_tries=20000):
    """The first seed from 9700 on whose scene keeps every decision TOL / 2 away from its switch."""
    name, H, W, B, N, K, form, thr, lists, behind, M = spec
    for seed in range(9700, 9700 + max_tries):
        rng = np.random.default_rng(seed)
        mus, isg = rc.gaussians_of(rng, B * N, form, 3.0, 12.0, behind)
        bins = rc.full_lists(B, H, W, N) if lists == "full" else rc.holed_lists(rng, B, H, W, N, M)
        c = dict(name=name, mus=mus, isg=isg, rays=rc.rays_of(B, H, W, 0.8 * max(H, W)), bins=bins, K=K, thr_act=oracle.thr_act_of(thr),
                 B=B, N=N, H=H, W=W, seed=seed)
        if min(rc.decision_margins(c)) > TOL / 2:
            g = rng.normal(size=(3, B, H, W, K)).astype(np.float32)
            g[2] *= 0.1
            c.update(g_len=g[0], g_act=g[1], g_dsd=g[2])
            return c
    raise RuntimeError(f"{name}: no seed keeps the decisions apart")


def dense_inputs():
    rng = np.random.default_rng(9800)
    mus, isg = rc.gaussians_of(rng, 12, "skew")
    rays = np.ascontiguousarray(rc.rays_of(1, 4, 5, 4.0).reshape(-1, 3))
    g = rng.normal(size=(3, rays.shape[0], 12)).astype(np.float32)
    g[2] *= 0.1
    return dict(mus=mus, isg=isg, rays=rays, g_len=g[0], g_act=g[1], g_dsd=g[2])


def sampler_inputs():
    rng = np.random.default_rng(9810)
    B, H, W, K, C, Nv = 1, 6, 7, 4, 3, 12
    cnt = rng.integers(1, K + 1, (B, H, W))
    idx = rng.integers(1, Nv - 2, (B, H, W, K)).astype(np.int32)
    idx[..., 0] = 0
    idx[np.arange(K) >= cnt[..., None]] = -1
    return dict(image=rng.uniform(0, 1, (B, H, W, C)).astype(np.float32), weight=rng.uniform(0, 1, (B, H, W, K)).astype(np.float32), idx=idx,
                n_vert=Nv, g_feat=rng.normal(size=(Nv, C)).astype(np.float32), g_wsum=rng.normal(size=Nv).astype(np.float32), C=C, K=K)


def coarse_inputs():
    """Two clouds of 40 and 25 points over a 16 x 20 image (2 x 2 bins of 10 pixels), every ninth point at z < 0."""
    H, W = 16, 20
    pts, rad = rc.coarse_points(np.random.default_rng(9820), 65, (H, W), 0.4)
    pts[::9, 2] *= -1
    return dict(points=pts, radius=rad, first=np.array([0, 40], np.int64), num=np.array([40, 25], np.int64), image_size=np.array([H, W]),
                bin_size=rc.BIN_SIZE, max_points_per_bin=40)


def inputs():
    """Everything the fixture holds that is not a kernel's output (no GPU needed)."""
    out = {}
    for spec in FIXTURE_FINE:
        c = fine_inputs(spec)
        for k in ("mus", "isg", "rays", "bins", "g_len", "g_act", "g_dsd"):
            out[f"{c['name']}_{k}"] = c[k]
        out[f"{c['name']}_meta"] = np.array([c["K"], c["seed"]], np.int64)
        out[f"{c['name']}_thr_act"] = np.float64(c["thr_act"])
    for prefix, d in (("dense", dense_inputs()), ("sampler", sampler_inputs()), ("coarse", coarse_inputs())):
        for k, v in d.items():
            out[f"{prefix}_{k}"] = np.asarray(v)
    return out


def main(outdir):
    import torch
    import ref_kernels as ref
    assert ref.available(), "oracle/_ref/voge_ref_C.so is absent: run oracle/build_ref.py where the reference sources are"
    assert torch.cuda.is_available()
    dev = "cuda:0"

    def t(a, dtype=torch.float32):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev)

    def n(x):
        return x.detach().cpu().numpy()

    fx = inputs()
    for spec in FIXTURE_FINE:
        nm = spec[0]
        mus, isg, rays = t(fx[nm + "_mus"]), t(fx[nm + "_isg"]), t(fx[nm + "_rays"])
        K = int(fx[nm + "_meta"][0])
        out = ref.ray_trace_voge_fine(mus, isg, rays, t(fx[nm + "_bins"], torch.int32), float(fx[nm + "_thr_act"]), rc.BIN_SIZE, K)
        for k, o in zip(("idx", "len", "act", "dsd"), out):
            fx[f"{nm}_out_{k}"] = n(o)
        valid = (n(out[0]) >= 0).astype(np.float32)
        g = [np.ascontiguousarray(fx[f"{nm}_{k}"] * valid) for k in ("g_len", "g_act", "g_dsd")]
        for k, o in zip(("g_ray", "g_mus", "g_isg"), ref.ray_trace_voge_fine_backward(mus, isg, rays, out[0], t(g[0]), t(g[1]), t(g[2]))):
            fx[f"{nm}_out_{k}"] = n(o)
    mus, isg, rays = t(fx["dense_mus"]), t(fx["dense_isg"]), t(fx["dense_rays"])
    dense = ref.ray_trace_voge_ray(mus, isg, rays)
    for k, o in zip(("len", "act", "dsd"), dense):
        fx["dense_out_" + k] = n(o)
    for k, o in zip(("g_ray", "g_mus", "g_isg"), ref.ray_trace_voge_ray_backward(mus, isg, rays, t(fx["dense_g_len"]), t(fx["dense_g_act"]),
                                                                                  t(fx["dense_g_dsd"]))):
        fx["dense_out_" + k] = n(o)
    fx["nearest_thr_act"] = np.float64(np.median(n(dense[1])))
    for K in (1, 5, 15):      # 15 > the 12 Gaussians
        for k, o in zip(("idx", "len", "act", "dsd"), ref.find_nearest_k(dense[0], dense[1], dense[2], float(fx["nearest_thr_act"]), K)):
            fx[f"nearest_k{K}_out_{k}"] = n(o)
    image, w, idx = t(fx["sampler_image"]), t(fx["sampler_weight"]), t(fx["sampler_idx"], torch.int32)
    Nv = int(fx["sampler_n_vert"])
    feat, wsum = ref.sample_voge(image, w, idx, Nv)
    g_img, g_w = ref.sample_voge_backward(image, w, idx, t(fx["sampler_g_feat"]), t(fx["sampler_g_wsum"]))
    fx.update(sampler_out_feat=n(feat), sampler_out_wsum=n(wsum), sampler_out_g_image=n(g_img), sampler_out_g_weight=n(g_w),
              sampler_out_max=n(ref.scatter_max(w, idx, Nv)))
    H, W = (int(v) for v in fx["coarse_image_size"])
    bins = ref.rasterize_points_coarse(t(fx["coarse_points"]), t(fx["coarse_first"], torch.int64), t(fx["coarse_num"], torch.int64), (H, W),
                                       t(fx["coarse_radius"]), int(fx["coarse_bin_size"]), int(fx["coarse_max_points_per_bin"]))
    fx["coarse_out_bins_sorted"] = rc.sorted_bins(n(bins))      # (the order inside a bin is the scheduler's)
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "ref_kernels.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
