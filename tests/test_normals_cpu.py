"""CPU tests of the normals-from-depth extension (the reference has neither depth nor normals): Aggregation.depth_normals -- the
definition -- on planes, degenerate maps, holes and depth steps, torch.autograd.gradcheck of it, the public API's routes and
errors, the two C-ABI entries' host-side argument validation (no GPU here: anything that reached HIP would fail differently),
the kernel descriptors' scratch / spill metadata, and the CONDITIONING of the inputs tests/test_gpu_normals.py uses, which are
built here (gpu_case) so that both files see the same numbers."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from util import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- rays and inputs, shared with the GPU tests ---------------------------------------------------------------------------------
def rays_torch(R, focal, pp, H, W, rows=None, dtype=torch.float64):
    """Unit world-space pixel rays [B,h,W,3] of screen-space cameras (cameras.py's conventions: d_view = [(px - j - 0.5) / fx,
    (py - i - 0.5) / fy, 1], d_world = normalise(d_view @ R^-1)) in plain torch on the host, evaluated in `dtype`."""
    R, focal, pp = (torch.as_tensor(np.asarray(a), dtype=dtype) for a in (R, focal, pp))
    r0, r1 = (0, H) if rows is None else rows
    i = torch.arange(r0, r1, dtype=dtype)[None, :, None]
    j = torch.arange(W, dtype=dtype)[None, None, :]
    vx = ((pp[:, 0, None, None] - j - 0.5) / focal[:, 0, None, None]).expand(-1, r1 - r0, -1)
    vy = ((pp[:, 1, None, None] - i - 0.5) / focal[:, 1, None, None]).expand(-1, -1, W)
    v = torch.stack([vx, vy, torch.ones_like(vx)], -1)
    w = torch.einsum("bhwi,bij->bhwj", v, torch.linalg.inv(R))
    return w / w.norm(dim=-1, keepdim=True)


SLOPE = 0.5      # the bumps' steepest slope against the rays (tangent): about 27 degrees


def two_views():
    from voge_amd.cameras import look_at_view_transform
    R, _ = look_at_view_transform(dist=[3.0, 3.4], elev=[12.0, -25.0], azim=[20.0, 200.0])
    return R.numpy()


def gpu_case(H, W, focal, dist=3.0, holes=0.12, step=True, seed=0):
    """The GPU tests' inputs, fp32: depth [2,H,W] = dist * (1 + a sin(u i + b) cos(v j - b)) -- a = 0.08, lowered where the bumps
    would otherwise be steeper than SLOPE against the rays --, `holes` of the pixels replaced by 0 / NaN / inf / -1, the lower
    half of view 1 times 1.3; two look_at views with different focal lengths and off-centre principal points; an upstream
    gradient ~ N(0, 1).  No hole lies within two rows of the step: a one-sided difference ACROSS it (3.9 - 3 over one pixel at a
    focal length of 120) would put the normal within 0.03 of perpendicular to its ray, closer to the sign's switch than the
    conditioning test allows.  -> dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    u, v = min(9.4 / H, 0.4), min(9.4 / W, 0.4)
    a = min(0.08, SLOPE / (max(u, v) * focal))
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = np.stack([dist * (1 + a * np.sin(u * i + 0.5 * b) * np.cos(v * j - 0.3 * b)) for b in range(2)])
    if step:
        depth[1, H // 2:] *= 1.3
    if holes:
        hole = rng.random((2, H, W)) < holes
        if step:
            hole[1, max(H // 2 - 2, 0):H // 2 + 2] = False
        kind = rng.integers(0, 4, (2, H, W))
        depth[hole] = np.array([0.0, np.nan, np.inf, -1.0])[kind[hole]]
    return dict(depth=depth.astype(np.float32), R=two_views().astype(np.float32),
                focal=np.array([[focal, 1.1 * focal], [0.9 * focal, focal]], np.float32),
                pp=np.array([[W / 2 + 1.3, H / 2 - 0.7], [W / 2 - 2.1, H / 2 + 0.4]], np.float32),
                g=rng.normal(size=(2, H, W, 3)).astype(np.float32), H=H, W=W)


# (image rows, columns, focal length) of the GPU comparisons; the band is rows 5..13 of the first
GPU_SHAPES = [(19, 23, 30.0), (40, 36, 60.0), (70, 130, 120.0), (2, 2, 30.0), (1, 9, 30.0), (9, 1, 30.0)]
GPU_BAND = (5, 14)
GPU_EDGES = [None, 0.1]


def high_focal_case():
    """64 x 64 at focal length 2000 and distance 6 (the bunny's camera), no holes, no step."""
    return gpu_case(64, 64, 2000.0, dist=6.0, holes=0.0, step=False, seed=3)


def evaluate(case, edge, dtype, rows=None, view_space=False, rays=None):
    """The definition and its autograd gradient for the case's upstream gradient, on the host in `dtype`, from the case's fp32
    values -> (normals, g_depth, defined mask, rays) as numpy arrays."""
    from voge_amd.Aggregation import depth_normals
    r0, r1 = (0, case["H"]) if rows is None else rows
    d = torch.tensor(case["depth"][:, r0:r1], dtype=dtype, requires_grad=True)
    if rays is None:
        rays = rays_torch(case["R"], case["focal"], case["pp"], case["H"], case["W"], rows, torch.float64).to(dtype)
    n = depth_normals(d, rays, edge)
    defined = (n.detach() != 0).any(-1).numpy()
    out = torch.einsum("bhwi,bij->bhwj", n, torch.tensor(case["R"], dtype=dtype)) if view_space else n
    (out * torch.tensor(case["g"][:, r0:r1], dtype=dtype)).sum().backward()
    return out.detach().numpy(), d.grad.numpy(), defined, rays


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------
def plane_depth(n0, c, centre, rays):
    """Distance along unit rays from `centre` to the plane n0 . X = c."""
    return (c - (n0 * centre).sum()) / (rays * n0).sum(-1)


def test_plane_gives_its_own_normal_everywhere_borders_included():
    from voge_amd.Aggregation import depth_normals
    from voge_amd.cameras import look_at_view_transform
    R, T = look_at_view_transform(dist=4.0, elev=20.0, azim=35.0)
    R64, T64 = R.double(), T.double()
    centre = -(T64 @ torch.linalg.inv(R64[0]))[0]
    rays = rays_torch(R64, [[40.0, 44.0]], [[11.7, 8.2]], 17, 21)
    n0 = torch.tensor([0.3, -0.2, 0.933], dtype=torch.float64)
    n0 = n0 / n0.norm()
    depth = plane_depth(n0, 0.25, centre, rays)
    assert bool((depth > 0).all())
    n = depth_normals(depth, rays)
    want = torch.where(((rays * n0).sum(-1, keepdim=True) > 0), -n0, n0).expand_as(n)
    assert float((n - want).abs().max()) < 1e-12, float((n - want).abs().max())
    assert bool(((n * rays).sum(-1) < 0).all())      # towards the camera


@pytest.mark.parametrize("h,W", [(1, 9), (9, 1), (1, 1), (0, 4)])
def test_maps_without_a_second_row_or_column_have_no_normals(h, W):
    from voge_amd.Aggregation import depth_normals
    d = (3 + torch.rand(2, h, W, dtype=torch.float64)).requires_grad_(True)
    rays = torch.nn.functional.normalize(torch.rand(2, h, W, 3, dtype=torch.float64) + 0.5, dim=-1).requires_grad_(True)
    n = depth_normals(d, rays, None)
    assert n.shape == (2, h, W, 3) and bool((n == 0).all())
    (n * torch.rand_like(n)).sum().backward()
    assert bool((d.grad == 0).all()) and bool((rays.grad == 0).all())


def small_map(seed=0, h=6, W=7):
    rng = np.random.default_rng(seed)
    case = gpu_case(h, W, 12.0, holes=0.0, step=False, seed=seed)
    d = case["depth"][:1].astype(np.float64) + 0.05 * rng.random((1, h, W))
    rays = rays_torch(case["R"][:1], case["focal"][:1], case["pp"][:1], h, W)
    return d, rays


@pytest.mark.parametrize("edge", [None, 0.1])
def test_holes_give_finite_outputs_and_exactly_zero_at_the_holes(edge):
    from voge_amd.Aggregation import depth_normals
    d, rays = small_map()
    holes = {(0, 0): 0.0, (2, 3): np.nan, (4, 1): np.inf, (5, 6): -np.inf, (3, 5): -2.0, (1, 1): np.nan, (1, 2): np.inf}
    for (i, j), v in holes.items():
        d[0, i, j] = v
    for dtype in (torch.float64, torch.float32):
        dt = torch.tensor(d, dtype=dtype, requires_grad=True)
        rt = rays.to(dtype).clone().requires_grad_(True)
        n = depth_normals(dt, rt, edge)
        (n * torch.rand_like(n)).sum().backward()
        assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(dt.grad).all()) and bool(torch.isfinite(rt.grad).all())
        for (i, j) in holes:
            assert bool((n[0, i, j] == 0).all()) and float(dt.grad[0, i, j]) == 0.0
        assert float(dt.grad.abs().max()) > 0
        norms = n.detach().norm(dim=-1)
        assert bool(((norms == 0) | ((norms - 1).abs() < 1e-5)).all())
    # a pixel without a normal passes nothing on: its upstream gradient alone gives a zero gradient everywhere
    dt = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    n = depth_normals(dt, rays, edge)
    undefined = (n.detach() == 0).all(-1)
    assert int(undefined.sum()) >= len(holes)
    (n * undefined[..., None]).sum().backward()
    assert bool((dt.grad == 0).all())


@pytest.mark.parametrize("edge", [None, 0.1])
def test_gradcheck_of_the_definition_on_a_map_with_holes(edge):
    from voge_amd.Aggregation import depth_normals
    d, rays = small_map(seed=1)
    d[0, 3:] *= 1.3      # a depth step: one-sided stencils along it under edge = 0.1
    holes = [(0, 2), (2, 4), (4, 0), (5, 6), (3, 3)]
    mask = torch.ones(1, 6, 7, dtype=torch.float64)
    for k, (i, j) in enumerate(holes):
        mask[0, i, j] = 0.0
    fill = torch.zeros(1, 6, 7, dtype=torch.float64)
    for k, (i, j) in enumerate(holes):
        fill[0, i, j] = [0.0, float("nan"), float("inf"), -1.0, 0.0][k]

    def f(x, r):      # (the holes are put in behind the differentiated input: gradcheck perturbs valid depths only)
        return depth_normals(torch.where(mask > 0, x, fill), r, edge)
    x = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    r = rays.clone().requires_grad_(True)
    assert int((f(x, r).detach() != 0).any(-1).sum()) >= 25
    assert torch.autograd.gradcheck(f, (x, r), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_edge_cuts_the_stencil_at_a_depth_step():
    """A 1.3 x step between rows 4 and 5: with edge = 0.1 the rows along it use one-sided differences, so their normals are those
    of the two halves taken as maps of their own; without an edge they differ."""
    from voge_amd.Aggregation import depth_normals
    case = gpu_case(10, 9, 15.0, holes=0.0, step=False)
    d = torch.tensor(case["depth"][:1], dtype=torch.float64)
    d[0, 5:] *= 1.3
    rays = rays_torch(case["R"][:1], case["focal"][:1], case["pp"][:1], 10, 9)
    cut = depth_normals(d, rays, 0.1)
    top, bottom = depth_normals(d[:, :5], rays[:, :5], 0.1), depth_normals(d[:, 5:], rays[:, 5:], 0.1)
    assert bool((cut.norm(dim=-1) > 0.99).all())
    assert torch.equal(cut[:, :5], top) and torch.equal(cut[:, 5:], bottom)
    assert torch.equal(top, depth_normals(d[:, :5], rays[:, :5], None))      # (the halves themselves hold no jump)
    plain = depth_normals(d, rays, None)
    assert float((plain[:, 4:6] - cut[:, 4:6]).abs().max()) > 0.1
    assert torch.equal(plain[:, :4], cut[:, :4]) and torch.equal(plain[:, 6:], cut[:, 6:])


def test_bad_arguments_of_the_definition_raise():
    from voge_amd.Aggregation import depth_normals
    d, r = torch.ones(1, 3, 4), torch.ones(1, 3, 4, 3)
    for bad in ((d[0], r[0]), (d, r[:, :2]), (d, r[..., :2])):
        with pytest.raises(ValueError):
            depth_normals(*bad)
    for edge in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            depth_normals(d, r, edge)


# ---- 2. the public API -----------------------------------------------------------------------------------------------------------------
def test_get_normals_is_public_and_takes_host_tensors_through_the_definition():
    from VoGE.Renderer import get_normals
    from voge_amd import Renderer
    from voge_amd.Aggregation import depth_normals
    from voge_amd.cameras import PerspectiveCameras
    from voge_amd.distributed import Stripes
    assert get_normals is Renderer.get_normals
    doc = get_normals.__doc__
    for word in ("edge", "view_space", "UNIT ray", "not view-space z", "2^-23", "gradient", "Stripes"):
        assert word in doc, word
    case = gpu_case(8, 9, 14.0)
    rays = rays_torch(case["R"], case["focal"], case["pp"], 8, 9)
    for dtype in (torch.float64, torch.float32):
        d, r = torch.tensor(case["depth"], dtype=dtype), rays.to(dtype)
        for edge in GPU_EDGES:
            assert torch.equal(get_normals(d, r, edge=edge), depth_normals(d, r, edge))
        one = get_normals(d[0], r[0])
        assert one.shape == (8, 9, 3) and torch.equal(one, depth_normals(d[:1], r[:1])[0])
        assert torch.equal(get_normals(d[0], r[:1]), one)
    d, r = torch.tensor(case["depth"]), rays.float()
    with pytest.raises(ValueError, match="view_space"):
        get_normals(d, r, view_space=True)
    with pytest.raises(ValueError):
        get_normals(d, r[:, :7])
    with pytest.raises(ValueError):
        get_normals(d, r[:1])
    with pytest.raises(ValueError):
        get_normals(d[None], r)
    with pytest.raises(ValueError):
        get_normals(d, r, edge=-1.0)
    with pytest.raises(ValueError):
        get_normals(d, r, rows=(0, 8))
    cams = PerspectiveCameras(focal_length=torch.tensor(case["focal"]), principal_point=torch.tensor(case["pp"]),
                              R=torch.tensor(case["R"]), T=torch.zeros(2, 3), image_size=((8, 9),))
    with pytest.raises(ValueError, match="rows"):
        get_normals(d, cams, rows=(2, 9))
    with pytest.raises(ValueError, match="rows"):
        get_normals(d, cams, rows=(-1, 7))
    with pytest.raises(ValueError, match="cameras"):
        get_normals(torch.cat([d, d[:1]]), cams)
    with pytest.raises(ValueError, match="gather"):
        get_normals(d, cams, rows=Stripes(16, 0, 2, stripe_h=4))


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-NULL pointer value: nothing is dereferenced before validation is through)

    def fwd(B=2, row0=0, h=8, W=9, edge=-1.0, depth=P, R=P, focal=P, pp=P, out=P):
        return lib.voge_depth_normals_fwd(depth, R, focal, pp, B, row0, h, W, edge, 0, out, None)

    def bwd(B=2, row0=0, h=8, W=9, edge=-1.0, depth=P, R=P, focal=P, pp=P, out=P, g=P):
        return lib.voge_depth_normals_bwd(depth, R, focal, pp, g, B, row0, h, W, edge, 1, out, None)
    for f in (fwd, bwd):
        assert f(B=-1) == -1 and f(h=-1) == -1 and f(W=-1) == -1 and f(row0=-1) == -1
        assert f(edge=float("nan")) == -1
        assert f(B=65536) == -1 and f(h=262141) == -1
        assert f(B=0) == 0 and f(h=0) == 0 and f(W=0) == 0      # nothing to do: a success that launches nothing
        for name in ("depth", "R", "focal", "pp", "out"):
            assert f(**{name: None}) == -1, name
    assert bwd(g=None) == -1
    assert lib.voge_abi_version() == 7


def test_header_exports_and_ctypes_table_agree_on_the_two_entries(lib):
    import ctypes
    from voge_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voge_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("voge_depth_normals_fwd", 12), ("voge_depth_normals_bwd", 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(raw, name)
        assert not any(a.split()[-1].lstrip("*") == "T" for a in args)      # (the camera centre cancels: no T)
        # floats where the header has floats, pointers where it has pointers
        for a, c in zip(args, _lib.SIGNATURES[name][1]):
            want = ctypes.c_void_p if ("*" in a or "voge_stream_t" in a) else ctypes.c_float if a.startswith("float") else ctypes.c_int
            assert c is want, (name, a, c)
    text = open(os.path.join(ROOT, "include", "voge_hip.h")).read()
    comment = text[:text.index("int voge_depth_normals_fwd")].rsplit("/*", 1)[1]
    assert "Replaces" in comment and "depth_normals" in comment
    assert "normals.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- 4. what the compiler made of the kernels: descriptor metadata only ----------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_normals_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    out = os.path.join(str(tmp_path), "normals.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only", "-o", out,
                           os.path.join(CSRC, "normals.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (_ZN4voge\w*depth_normals_(?:fwd|bwd)_kernel\w*)\s*$", text, flags=re.M)
    assert len(names) == 2 and any("fwd" in n for n in names) and any("bwd" in n for n in names), names
    for name in names:
        d = text.index(".amdhsa_kernel " + name)
        desc = text[d:text.index(".end_amdhsa_kernel", d)]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, (name, "scratch")
        meta = [blk for blk in re.split(r"\n  - ", text[text.index("amdhsa.kernels"):]) if re.search(r"\.name:\s+" + name + r"\s", blk)]
        assert len(meta) == 1, name
        for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            assert int(re.search(r"\." + key + r":\s+(\d+)", meta[0]).group(1)) == 0, (name, key)


# ---- 5. the conditioning of the GPU tests' inputs ----------------------------------------------------------------------------------------
def _scale(a):
    return max(1.0, float(np.abs(a).max())) if a.size else 1.0


@pytest.mark.parametrize("shape", GPU_SHAPES + ["band"], ids=lambda s: s if isinstance(s, str) else f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("edge", GPU_EDGES)
def test_gpu_inputs_keep_the_fp32_reference_inside_a_quarter_of_the_tolerance(shape, edge):
    """For every case tests/test_gpu_normals.py compares at util.TOL: the fp32 evaluation of the definition (fp32 rays, fp32
    arithmetic, on the host) and of its autograd gradient lies within TOL / 4 of the fp64 one, so the reference alone cannot
    use up the tolerance; the defined-masks are the same; no defined normal is closer than 0.05 to perpendicular to its ray (the
    sign is far from its switch) and no neighbouring depths have a relative jump inside [edge / 2, 2 edge] (the edge test is far
    from its switch)."""
    rows = GPU_BAND if shape == "band" else None
    H, W, focal = GPU_SHAPES[0] if shape == "band" else shape
    case = gpu_case(H, W, focal)
    n64, g64, def64, rays = evaluate(case, edge, torch.float64, rows)
    n32, g32, def32, _ = evaluate(case, edge, torch.float32, rows)
    assert (def64 == def32).all()
    err_n = float(np.abs(n32 - n64).max()) if n64.size else 0.0
    err_g = float(np.abs(g32 - g64).max()) / _scale(g64) if g64.size else 0.0
    print(f"[conditioning] {shape} edge={edge}: fp32 definition normals {err_n:.2e}, gradient {err_g:.2e} of scale, "
          f"{int(def64.sum())} of {def64.size} pixels defined")
    assert err_n <= TOL / 4 and err_g <= TOL / 4, (err_n, err_g)
    if min(H, W) > 1:
        assert def64.mean() > 0.5 if min(H, W) > 2 else def64.any() == (edge is None)      # (2 x 2: the step cuts view 1 in two rows)
        cos = np.abs((n64 * rays.numpy()).sum(-1))[def64]
        assert cos.size == 0 or cos.min() >= 0.05, cos.min()
    else:
        assert not def64.any()
    r0, r1 = (0, H) if rows is None else rows
    d = case["depth"][:, r0:r1].astype(np.float64)
    ok = np.isfinite(d) & (d > 0)
    for a, b, va, vb in ((d[:, :, 1:], d[:, :, :-1], ok[:, :, 1:], ok[:, :, :-1]), (d[:, 1:], d[:, :-1], ok[:, 1:], ok[:, :-1])):
        both = va & vb
        with np.errstate(invalid="ignore", divide="ignore"):
            for jump in (np.abs(a - b) / a, np.abs(a - b) / b):
                jump = jump[both]
                assert not ((jump >= 0.05) & (jump <= 0.2)).any(), jump[(jump >= 0.05) & (jump <= 0.2)]
    if shape != "band" and H >= 19 and edge is not None:      # the step is there, and it cuts
        assert ok[1, H // 2 - 1:H // 2 + 1].all() and (np.abs(d[1, H // 2] - d[1, H // 2 - 1]) / d[1, H // 2]).min() > 0.2


def test_high_focal_input_is_well_conditioned_and_shows_the_fp32_floor():
    """64 x 64, focal length 2000, distance 6: the GPU test's tolerance there is 4 x the fp32 definition's own error, which this
    prints; the mask and the sign are away from their switches as above."""
    case = high_focal_case()
    n64, g64, def64, rays = evaluate(case, None, torch.float64)
    n32, g32, def32, _ = evaluate(case, None, torch.float32)
    assert def64.all() and def32.all()
    assert np.abs((n64 * rays.numpy()).sum(-1)).min() >= 0.05
    err = float(np.abs(n32 - n64).max())
    print(f"[conditioning] high focal: fp32 definition normals {err:.2e}, gradient {np.abs(g32 - g64).max() / _scale(g64):.2e} of scale")
    assert 1e-6 < err < 1e-3      # (the floor, 2^-23 * 2000 = 2.4e-4 times a small factor: neither absent nor out of hand)
