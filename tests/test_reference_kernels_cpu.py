"""CPU side of the reference-kernel tests: the built extension is there and imports, and the inputs of
tests/test_gpu_reference_kernels.py are what that module's tolerances assume."""
import os

import numpy as np
import pytest

import oracle
import ref_kernel_cases as rc
import ref_kernels
from oracle import build_ref, extras_np
from util import TOL, max_rel


def test_build_left_the_reference_extension_and_it_imports():
    """Where the reference's sources exist, build() has left oracle/_ref/voge_ref_C.so; wherever the file exists it imports by path
    and exposes the reference's nine entry points.  (Neither sources nor file: nothing to check on this machine.)"""
    if build_ref.have_reference():
        assert os.path.exists(ref_kernels.SO_PATH), "the reference sources are here but build() left no oracle/_ref/voge_ref_C.so"
        assert os.path.exists(build_ref.INFO_PATH)
        left = set(os.listdir(build_ref.REF_DIR))
        assert left == {"voge_ref_C.so", "BUILD_INFO.json"}, f"oracle/_ref holds more than the binary and its record: {sorted(left)}"
    if ref_kernels.available():
        mod = ref_kernels.load()
        assert set(ref_kernels.NAMES) == set(build_ref.NAMES) and len(ref_kernels.NAMES) == 9
        for name in ref_kernels.NAMES:
            assert callable(getattr(mod, name)), name
    else:
        print(f"[ref-kernel] neither the reference sources ({build_ref.reference_csrc()}) nor {ref_kernels.SO_PATH} exist here: nothing checked")


def _conditioning(c, label):
    """The fp32 reference-order oracle against the fp64 oracle on pixels with equal lists: within TOL / 4."""
    out = {p: oracle.trace_fwd(c["mus"], c["isg"], c["rays"], c["K"], c["thr_act"], bin_points=c["bins"], bin_size=rc.BIN_SIZE, precision=p)
           for p in ("f32", "f64")}
    same = (out["f32"][0] == out["f64"][0]).all(-1)
    v = same[..., None] & (out["f64"][0] >= 0)
    assert v.sum() > 100
    for name, a, b in zip(("len", "act", "dsd"), out["f32"][1:], out["f64"][1:]):
        e = max_rel(a[v], b[v])
        print(f"[conditioning] {label} {name}: fp32 reference order vs fp64 {e:.2e} (TOL / 4 = {TOL / 4:.1e}); {int((~same).sum())} lists differ")
        assert e <= TOL / 4, f"{label} {name}: {e:.3e}"
    return int((~same).sum())


@pytest.mark.parametrize("name", rc.FINE_NAMES)
def test_fine_scenes_keep_the_fp32_reference_inside_a_quarter_of_the_tolerance(name):
    flips = _conditioning(rc.fine_case(name), name)
    assert rc.fine_flip_ceiling(name) == flips + 2


@pytest.mark.parametrize("name", rc.BWD_NAMES + ["twins_asc", "twins_desc"])
def test_backward_and_twin_scenes_keep_the_fp32_reference_inside_a_quarter_of_the_tolerance(name):
    c = rc.twin_case(name == "twins_desc") if name.startswith("twins") else rc.bwd_case(name)
    flips = _conditioning(c, name)
    if name.startswith("twins"):
        assert flips == 0      # the tie tests compare index lists exactly


def test_dense_scene_keeps_fp32_inside_a_quarter_of_the_tolerance():
    c = rc.dense_case()
    f64 = extras_np.ray_dense_fwd(c["mus"], c["isg"], c["rays"])
    mu, A, d = c["mus"], c["isg"], c["rays"]      # fp32, the reference's order of operations (voge_ray_tracing_ray.cu:10-37, :135-141)

    def form(a, b, cc):
        s = np.zeros(np.broadcast_shapes(a.shape[:-1], cc.shape[:-1]), np.float32)
        for i in range(3):
            for j in range(3):
                s = s + a[..., i] * b[..., i, j] * cc[..., j]
        return s
    ksk, msk, msm = form(d[:, None], A[None], d[:, None]), form(mu[None], A[None], d[:, None]), form(mu[None], A[None], mu[None])
    for name, a, b in zip(("len", "act", "dsd"), (msk / ksk, msm - msk * msk / ksk, ksk), f64):
        assert a.dtype == np.float32 and max_rel(a, b) <= TOL / 4, (name, max_rel(a, b))


@pytest.mark.parametrize("name", rc.BWD_NAMES)
def test_term_by_term_backward_equals_the_oracle(name):
    """ref_kernel_cases.trace_bwd_terms is a second fp64 evaluation of the backward, written from the kernel's atomicAdd list: it
    agrees with oracle.trace_bwd in all nine entries of grad_isigmas, and counts 3 terms per slot and output element."""
    c = rc.bwd_case(name)
    K = c["K"]
    idx = oracle.trace_fwd(c["mus"], c["isg"], c["rays"], K, c["thr_act"], bin_points=c["bins"], bin_size=rc.BIN_SIZE)[0]
    valid = idx >= 0
    assert (~valid).mean() > 0.05
    gl, ga, gd = (c[k] * valid for k in ("g_len", "g_act", "g_dsd"))
    want = oracle.trace_bwd(c["mus"], c["isg"], c["rays"], idx, gl, ga, gd)
    terms = rc.trace_bwd_terms(c["mus"], c["isg"], c["rays"].reshape(-1, 3), idx.reshape(-1, K), gl.reshape(-1, K), ga.reshape(-1, K),
                               gd.reshape(-1, K))
    for key, w in zip(("ray", "mus", "isg"), want):
        s, a, m = terms[key]
        assert np.abs(s - w.reshape(s.shape)).max() <= 1e-9 * max(1.0, np.abs(w).max())
        assert (a >= np.abs(s) - 1e-9).all()
    assert np.array_equal(terms["ray"][2], np.broadcast_to(3 * valid.reshape(-1, K).sum(1)[:, None], terms["ray"][2].shape))
    per = np.bincount(idx[valid], minlength=c["mus"].shape[0])
    assert np.array_equal(terms["mus"][2][:, 0], 3 * per) and np.array_equal(terms["isg"][2][:, 1, 2], 3 * per)
    # the fp32 oracle, one ordering of the same sums, sits inside the bound
    got32 = oracle.trace_bwd(c["mus"], c["isg"], c["rays"], idx, gl, ga, gd, precision="f32")
    for key, g in zip(("ray", "mus", "isg"), got32):
        s, a, m = terms[key]
        assert (np.abs(g.reshape(s.shape) - s) <= rc.atomic_bound(a, m, s)).all()


def test_term_by_term_dense_backward_equals_extras_np():
    """The dense backward is the fine one with every Gaussian in every ray's list; fp32 upstream gradients are summed in fp64."""
    c = rc.dense_case()
    N, M = rc.DENSE_RAYS, rc.DENSE_GAUSSIANS
    assert c["g_act"].dtype == np.float32 and N % 64 != 0
    every = np.ascontiguousarray(np.broadcast_to(np.arange(M, dtype=np.int32), (N, M)))
    terms = rc.trace_bwd_terms(c["mus"], c["isg"], c["rays"], every, c["g_len"], c["g_act"], c["g_dsd"])
    want = extras_np.ray_dense_bwd(c["mus"], c["isg"], c["rays"], c["g_len"], c["g_act"], c["g_dsd"])
    for key, w in zip(("ray", "mus", "isg"), want):
        assert np.abs(terms[key][0] - w).max() <= 1e-9 * max(1.0, np.abs(w).max()), key
    assert (terms["ray"][2] == 3 * M).all() and (terms["mus"][2] == 3 * N).all() and (terms["isg"][2] == 3 * N).all()


@pytest.mark.parametrize("C", rc.SAMPLER_C)
def test_sampler_terms_equal_the_oracle_and_the_case_has_its_edges(C):
    c = rc.sampler_case(C)
    Nv = c["n_vert"]
    t = rc.sampler_terms(c)
    feat, wsum = extras_np.sample_voge(c["image"], c["weight"], c["idx"], Nv)
    g_img, g_w = extras_np.sample_voge_bwd(c["image"], c["weight"], c["idx"], c["g_feat"], c["g_wsum"])
    for key, w in (("feat", feat), ("wsum", wsum), ("g_image", g_img), ("g_weight", g_w)):
        assert np.abs(t[key][0] - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
    idx = c["idx"]
    assert (idx[..., 0] == 0).all() and (idx == -1).any() and idx.max() < Nv - 2 and (c["weight"] >= 0).all()
    live = np.arange(c["K"]) < c["valid_num"][..., None]
    assert np.array_equal(idx >= 0, live)      # -1 exactly from valid_num on: ops.scatter_attr and the reference read the same slots


def test_coarse_case_keeps_every_box_edge_away_from_every_bin_edge():
    from oracle import coarse_np
    pts, rad, first, num = rc.coarse_case()
    assert rc.coarse_edge_gap(pts, rad).min() >= rc.COARSE_MARGIN
    # the fp64 edges are the fp32 ones the kernel computes, to rounding
    H, W = rc.COARSE_SIZE
    ex, ey = rc.coarse_bin_edges(rc.COARSE_SIZE)
    half_x = coarse_np.ndc_range(W, H) / 2 / W
    mine = [coarse_np.pix_to_ndc(b * rc.BIN_SIZE, W, H) - half_x for b in range(len(ex))]
    assert np.abs(np.array(mine, np.float64) - ex).max() < 1e-6
    assert (pts[:, 2] < 0).sum() > 20 and int(num.max()) >= 512 and first.tolist() == [0, 700]
