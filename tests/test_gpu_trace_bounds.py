"""The forward trace (binA -> binB -> sweep) on the ray bundles and Gaussian sets of tests/trace_bound_cases.py, held to the fp64
oracle by util.compare_trace_strict: wherever the oracle decides a pixel's membership the kernels' index SET must equal it, values
within the forward error bound derived in trace_bound_cases' docstring -- no share of differing pixels is forgiven, and the
undecided share is capped at 5 % by the case, not measured.  Every case runs through the general entry (ray_trace_fine) and, where
its forms are scalars, the scalar entry (_RayTraceVoGEIso); per-axis forms also through the fragments entry; at the small-set size
(N <= 4096, binA skipped) and the binned one.  Logged per test: the undecided share, the share of the bound the kernels use, the
share the reference's own formula in fp32 (oracle.trace_fwd(precision="f32")) uses on the same pixels, and the list pool's use.
"""
import numpy as np
import pytest
import torch

import trace_bound_cases as tb
from util import compare_trace_strict, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GENERAL_ONLY = ("invalid_general", "needles", "per_axis")
# cases whose quads hold more candidates than binB's in-LDS sort takes: their lists come from the pool (binB's long path)
POOLED = (("nonunit_1e-9", "binned"), ("nonunit_1e-12", "binned"), ("degenerate_rays", "binned"))


def _params():
    out = []
    for name, size in tb.case_ids():
        entries = ("general",) if name in GENERAL_ONLY else ("general", "scalar")
        if name == "per_axis":
            entries += ("fragments",)
        out += [(name, size, e) for e in entries]
    return out


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def n(x):
    return None if x is None else x.detach().cpu().numpy()


def _run(case, entry, rays):
    """-> (idx, len, act | None, dsd | None, cnt) as numpy."""
    from voge_amd import ops
    K = case.K
    if entry == "scalar":
        idx, ln, act, dsd = ops._RayTraceVoGEIso.apply(t(case.mus), t(case.a), rays, None, case.thr_act, K)
        return n(idx), n(ln), n(act), n(dsd), n(ops.hit_count_of(idx))
    if entry == "general":
        idx, ln, act, dsd = ops.ray_trace_fine(t(case.mus), t(case.isigmas()), rays, None, case.thr_act, 0, K)
        return n(idx), n(ln), n(act), n(dsd), n(ops.hit_count_of(idx))
    w, idx, vn, hl = ops.fragments(0, t(case.mus), t(case.isigmas()), None, rays, None, case.thr_act, K, 0, 1.0)
    return n(idx), n(hl), None, None, n(vn)


@pytest.mark.parametrize("name,size,entry", _params(), ids=lambda v: str(v))
def test_trace_equals_the_oracle_wherever_the_oracle_decides(hip_lib, name, size, entry):
    from voge_amd import ops
    case = tb.build(name, size)
    delta = tb.case_delta(name, size)[0]
    assert delta <= 1e-4
    fn = tb.case_oracle(name, size)
    H, W = case.rays.shape[1:3]
    got = _run(case, entry, t(case.rays))
    used, cap = ops.trace_pool_usage(DEV, 1, case.N, H, W)
    label = f"{name}/{size}/{entry}"
    compare_trace_strict(got, fn, case.K, case.thr_act, delta, tb.CAP, label, bounds=tb.bounds_fn(case), n_per_batch=case.N,
                               also={"fp32 reference formula": fn(case.K, case.thr_act, "f32")})
    log_line(f"[trace bounds] {label}: list pool used {used} of {cap}")
    assert used <= cap, "the list pool ran out: tiles fell back to streaming every Gaussian"
    if (name, size) in POOLED:
        assert used > 0, "no quad took the long path: the case does not test the pooled lists"
    for (y, x) in case.empty_pixels:
        assert (got[0][0, y, x] == -1).all() and got[4][0, y, x] == 0, f"the degenerate ray at ({y}, {x}) has hits"
    if name == "nonunit_1e-12":
        assert (got[0] == -1).all()


@pytest.mark.parametrize("name,size,entry", [("wide_2px", "binned", "scalar"), ("scrambled_supertiles", "binned", "scalar"),
                                             ("degenerate_rays", "binned", "general"), ("nonunit_random", "small", "scalar"),
                                             ("near_unit_plus", "binned", "scalar")], ids=lambda v: str(v))
def test_the_callers_cones_give_the_same_bits_as_none(hip_lib, name, size, entry):
    """voge_ray_cones' hierarchy handed in with the rays against cones = NULL (the trace derives them): the same bits."""
    lib = hip_lib
    case = tb.build(name, size)
    H, W = case.rays.shape[1:3]
    plain = _run(case, entry, t(case.rays))
    rays = t(case.rays)
    cones = torch.empty(int(lib.voge_cones_floats(1, H, W)), device=DEV)
    assert lib.voge_ray_cones(rays.data_ptr(), 1, H, W, cones.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    rays.voge_cones = (cones, rays._version)
    from voge_amd import ops
    assert ops.cones_of(rays, 1, H, W) is cones
    handed = _run(case, entry, rays)
    for a, b, what in zip(plain, handed, ("idx", "len", "act", "dsd", "cnt")):
        assert np.array_equal(a, b, equal_nan=True), what
