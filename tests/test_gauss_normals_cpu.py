"""CPU tests of the per-view normals of oriented Gaussians (an extension: the reference has none): Aggregation.gaussian_normals --
the definition -- against an independent fp64 numpy restatement written here and central differences, its named edge cases,
Renderer.gaussian_normals and get_rendered_normals on host tensors, the two C-ABI entries' host-side argument validation
(no GPU in this container: anything that reached HIP would fail differently), and what the compiler made of the two kernels."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the fp64 restatement: plain loops, the rules of the issue one by one ------------------------------------------------------
def rotation_np(q):
    """(w, x, y, z) -> 3x3 of q / |q|; the identity where |q|^2 is not a positive finite number."""
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        n2 = float((q * q).sum())
    if not (n2 > 0 and np.isfinite(n2)):
        return np.eye(3)
    w, x, y, z = q / np.sqrt(n2)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def axis_np(s, inverse):
    k = 0
    for j in (1, 2):
        if (s[j] < s[k]) if inverse else (s[j] > s[k]):
            k = j
    return k


def normals_np(scales, quats, verts, centres, inverse=False):
    """-> (out [B*N, 3], t [B, N]) in fp64."""
    scales, quats, verts, centres = (np.asarray(a, np.float64) for a in (scales, quats, verts, centres))
    B, N = centres.shape[0], scales.shape[-2]
    out, ts = np.zeros((B, N, 3)), np.zeros((B, N))
    for b in range(B):
        for n in range(N):
            s, q = (scales[b, n], quats[b, n]) if scales.ndim == 3 else (scales[n], quats[n])
            n0 = rotation_np(q)[:, axis_np(s, inverse)]
            delta = (verts[b, n] if verts.ndim == 3 else verts[n]) - centres[b]
            with np.errstate(all="ignore"):
                t = float(n0 @ delta)
            out[b, n], ts[b, n] = (-n0 if t > 0 else n0), t
    return out.reshape(B * N, 3), ts


def case(N=7, B=3, seed=0, per_view_orient=False, per_view_verts=False):
    rng = np.random.default_rng(seed)
    lead = (B, N) if per_view_orient else (N,)
    verts = rng.uniform(-1, 1, ((B, N, 3) if per_view_verts else (N, 3)))
    c = rng.normal(size=(B, 3))
    centres = 3 * c / np.linalg.norm(c, axis=-1, keepdims=True)
    scales = rng.uniform(0.5, 2, lead + (3,))
    quats = rng.normal(size=lead + (4,)) * rng.uniform(0.1, 10, lead + (1,))
    return scales, quats, verts, centres, rng.normal(size=(B * N, 3))


def t64(a, rg=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=rg)


def t32(a, rg=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, requires_grad=rg)


# ---- 1. the definition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("per_view_orient,per_view_verts", [(False, False), (False, True), (True, False), (True, True)])
def test_definition_values_and_gradients(inverse, per_view_orient, per_view_verts):
    """Values against the numpy restatement at 1e-13; g_quats against central differences of sum(out * g) in fp64 (step 1e-6 of
    the quaternion's norm; the case keeps every |t| above 1e-3, far from the sign's discontinuity) and orthogonal to quats;
    nothing reaches scales, verts or the camera centres."""
    from voge_amd.Aggregation import gaussian_normals
    scales, quats, verts, centres, g = case(seed=3 + 2 * per_view_orient + per_view_verts, per_view_orient=per_view_orient,
                                            per_view_verts=per_view_verts)
    want, ts = normals_np(scales, quats, verts, centres, inverse)
    assert np.abs(ts).min() > 1e-3 and (ts > 0).any() and (ts < 0).any()      # both signs occur
    s, q, v, c = t64(scales, True), t64(quats, True), t64(verts, True), t64(centres, True)
    out = gaussian_normals(s, q, v, c, inverse_sigma=inverse)
    assert out.shape == want.shape and out.dtype == torch.float64
    assert np.abs(out.detach().numpy() - want).max() <= 1e-13
    (out * t64(g)).sum().backward()
    for other in (s, v, c):
        assert other.grad is None or not other.grad.any()
    gq = q.grad.numpy()
    num = np.zeros_like(quats)
    flat = quats.reshape(-1, 4)
    for i in range(flat.shape[0]):
        h = 1e-6 * np.linalg.norm(flat[i])
        for j in range(4):
            qp, qm = flat.copy(), flat.copy()
            qp[i, j] += h
            qm[i, j] -= h
            fp = (normals_np(scales, qp.reshape(quats.shape), verts, centres, inverse)[0] * g).sum()
            fm = (normals_np(scales, qm.reshape(quats.shape), verts, centres, inverse)[0] * g).sum()
            num.reshape(-1, 4)[i, j] = (fp - fm) / (2 * h)
    scale = max(1.0, np.abs(num).max())
    assert np.abs(gq - num).max() <= 1e-7 * scale, np.abs(gq - num).max()
    assert np.abs(gq).max() > 0
    assert np.abs((gq * quats).sum(-1)).max() <= 1e-12 * scale      # orthogonal to quats


def test_shared_and_per_view_orientations_agree_and_the_shared_gradient_is_the_sum_over_the_views():
    from voge_amd.Aggregation import gaussian_normals
    scales, quats, verts, centres, g = case(N=6, B=4, seed=9)
    q1 = t64(quats, True)
    out1 = gaussian_normals(t64(scales), q1, t64(verts), t64(centres))
    qb = t64(np.broadcast_to(quats, (4,) + quats.shape).copy(), True)
    outb = gaussian_normals(t64(np.broadcast_to(scales, (4,) + scales.shape).copy()), qb,
                            t64(np.broadcast_to(verts, (4,) + verts.shape).copy()), t64(centres))
    assert torch.equal(out1, outb)
    (out1 * t64(g)).sum().backward()
    (outb * t64(g)).sum().backward()
    assert np.abs(q1.grad.numpy() - qb.grad.numpy().sum(0)).max() <= 1e-13


# ---- 2. the named edge cases (shared with the GPU file, which runs them through the kernel) --------------------------------------
def edge_cases():
    """-> list of (name, scales [3], quat [4], vert [3], centre [3], inverse, expected normal or None, zero_gradient).  fp32
    inputs: 1e20 and 1e-30 have a squared norm that overflows / underflows in fp32 only."""
    far = (0.0, 0.0, -5.0)
    ident = (1.0, 0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    cases = [
        # identity quaternion: the exact basis vector; kept where the camera is in front of it (t = -5), flipped behind it (t = 5)
        ("identity, thinnest axis 0", (3, 1, 2), ident, (0, 0, 0), (5.0, 0, 0), False, (1, 0, 0), False),
        ("identity, thinnest axis 2, flipped", (1, 2, 3), ident, (0, 0, 0), far, False, (0, 0, -1), False),
        ("identity, inverse: the smallest scale, flipped", (1, 2, 3), ident, (0, 0, 0), (-5.0, 0, 0), True, (-1, 0, 0), False),
    ]
    for name, q in (("zero", (0, 0, 0, 0)), ("NaN", (nan, 1, 0, 0)), ("inf", (1, inf, 0, 0)), ("1e20", (1e20, 1e20, 0, 0)),
                    ("1e-30", (1e-30, 0, 1e-30, 0))):
        cases.append((f"{name} quaternion: the identity column", (1, 3, 2), q, (0, 0, 0), (0.0, 5.0, 0), False, (0, 1, 0), True))
    cases += [
        ("two equal scales: the lowest index", (2, 2, 1), ident, (0, 0, 0), (5.0, 0, 0), False, (1, 0, 0), False),
        ("two equal scales (1, 2): the lowest index", (1, 2, 2), ident, (0, 0, 0), (0, 5.0, 0), False, (0, 1, 0), False),
        ("three equal scales: index 0", (2, 2, 2), ident, (0, 0, 0), (5.0, 0, 0), False, (1, 0, 0), False),
        ("three equal scales, inverse: index 0", (2, 2, 2), ident, (0, 0, 0), (5.0, 0, 0), True, (1, 0, 0), False),
        ("two equal smallest, inverse: the lowest index", (3, 1, 1), ident, (0, 0, 0), (0, 5.0, 0), True, (0, 1, 0), False),
        ("NaN scale in slot 0 stays chosen", (nan, 1, 2), ident, (0, 0, 0), (5.0, 0, 0), False, (1, 0, 0), False),
        ("NaN scale in slot 1 never wins", (1, nan, 2), ident, (0, 0, 0), (0, 0, 5.0), False, (0, 0, 1), False),
        ("NaN scale in slot 2 never wins", (1, 2, nan), ident, (0, 0, 0), (0, 5.0, 0), False, (0, 1, 0), False),
        ("NaN scale in slot 1, inverse", (2, nan, 1), ident, (0, 0, 0), (0, 0, 5.0), True, (0, 0, 1), False),
        ("n0 exactly perpendicular to delta keeps n0", (3, 1, 2), ident, (0, 1, 2), (0, 0, 0), False, (1, 0, 0), False),
        ("camera at the Gaussian keeps n0", (3, 1, 2), ident, (0.25, -0.5, 1), (0.25, -0.5, 1), False, (1, 0, 0), False),
        ("NaN vertex: a NaN t keeps n0", (3, 1, 2), ident, (nan, 0, 0), (5.0, 0, 0), False, (1, 0, 0), False),
    ]
    return cases


@pytest.mark.parametrize("case_", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_named_edge_cases(case_):
    from voge_amd.Aggregation import gaussian_normals
    name, s, q, v, c, inverse, want, zero_grad = case_
    qt = t32([q], True)
    out = gaussian_normals(t32([s]), qt, t32([v]), t32([c]), inverse_sigma=inverse)
    assert out.shape == (1, 3)
    assert out.detach().numpy().tolist() == [[float(x) for x in want]], (name, out)      # exact, signed zeros apart
    (out * t32([[0.3, -0.7, 1.1]])).sum().backward()
    g = qt.grad.numpy()
    assert np.isfinite(g).all(), (name, g)
    if zero_grad:
        assert (g == 0).all(), (name, g)
    else:
        assert np.abs(g).max() > 0 and abs(float((g * np.asarray(q, np.float32)).sum())) <= 1e-6


def test_a_tilted_quaternion_gives_the_rotated_axis():
    """A rotation by 90 degrees about z takes the x axis to y: column 0 of R is (0, 1, 0)."""
    from voge_amd.Aggregation import gaussian_normals
    h = np.sqrt(0.5)
    out = gaussian_normals(t64([[3, 1, 2]]), t64([[7 * h, 0, 0, 7 * h]]), t64([[0, 0, 0]]), t64([[0, 5.0, 0]]))
    assert np.abs(out.numpy() - [[0, 1, 0]]).max() <= 1e-15


# ---- 3. the public calls on the host -----------------------------------------------------------------------------------------------
def test_renderer_gaussian_normals_is_public_and_takes_the_definition_off_the_device():
    from VoGE.Renderer import gaussian_normals, get_rendered_normals
    from voge_amd import Renderer
    from voge_amd import Aggregation
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    assert gaussian_normals is Renderer.gaussian_normals and get_rendered_normals is Renderer.get_rendered_normals
    doc = gaussian_normals.__doc__
    assert "inverse_sigma" in doc and "get_camera_center" in doc and "once" in doc
    assert "get_normals" in get_rendered_normals.__doc__ and "get_depth" in get_rendered_normals.__doc__
    scales, quats, verts, centres, g = case(N=5, B=3, seed=1)
    for dtype in (torch.float64, torch.float32):
        for inverse in (False, True):
            s, v, c = (torch.tensor(x, dtype=dtype) for x in (scales, verts, centres))
            q = torch.tensor(quats, dtype=dtype, requires_grad=True)
            got = gaussian_normals(s, q, v, c, inverse_sigma=inverse)
            assert torch.equal(got, Aggregation.gaussian_normals(s, q, v, c, inverse_sigma=inverse))
            assert got.grad_fn is not None and type(got.grad_fn).__name__ != "_GaussNormalsBackward"      # autograd's node
            (got * torch.tensor(g, dtype=dtype)).sum().backward()
            assert q.grad.abs().max() > 0
    R, T = look_at_view_transform([3.0, 4.0, 5.0], [10.0, -20.0, 40.0], [30.0, 200.0, 300.0])
    cams = PerspectiveCameras(focal_length=100.0, principal_point=((32.0, 32.0),), image_size=((64, 64),), device="cpu")
    cams.R, cams.T = R, T
    s, q, v = t32(scales), t32(quats), t32(verts)
    assert torch.equal(gaussian_normals(s, q, v, cams), Aggregation.gaussian_normals(s, q, v, cams.get_camera_center()))


def test_bad_shapes_raise():
    from voge_amd.Aggregation import gaussian_normals as definition
    from voge_amd.Renderer import gaussian_normals
    N, B = 5, 2
    good = dict(scales=(N, 3), quats=(N, 4), verts=(N, 3), centres=(B, 3))
    bad = [dict(scales=(N, 2)), dict(scales=(N,)), dict(quats=(N, 3)), dict(quats=(N + 1, 4)), dict(quats=(B, N, 4)),
           dict(scales=(B, N, 3)), dict(scales=(B + 1, N, 3), quats=(B + 1, N, 4)), dict(verts=(N, 2)), dict(verts=(N + 1, 3)),
           dict(verts=(B + 1, N, 3)), dict(verts=(3,)), dict(centres=(3,)), dict(centres=(B, 2)), dict(centres=(1, B, 3)),
           dict(scales=(1, B, N, 3), quats=(1, B, N, 4))]
    for fn in (definition, gaussian_normals):
        assert fn(*(torch.ones(good[k]) for k in ("scales", "quats", "verts", "centres"))).shape == (B * N, 3)
        assert fn(torch.ones(B, N, 3), torch.ones(B, N, 4), torch.ones(B, N, 3), torch.ones(B, 3)).shape == (B * N, 3)
        for change in bad:
            shapes = dict(good, **change)
            with pytest.raises(ValueError):
                fn(*(torch.ones(shapes[k]) for k in ("scales", "quats", "verts", "centres")))


def host_fragments(weight, idx, valid):
    from voge_amd.Renderer import Fragments
    w = torch.tensor(weight, dtype=torch.float64, requires_grad=True)
    return Fragments(w, torch.tensor(idx, dtype=torch.int64), torch.tensor(valid, dtype=torch.int64),
                     torch.ones(w.shape, dtype=torch.float64)), w


def test_get_rendered_normals_on_host_fragments():
    """1 x 2 x 2 pixels, K = 3: an ordinary pixel, a pixel whose two normals cancel exactly (|M| = 0), a pixel with no hit, and a
    pixel whose dead slot (beyond valid_num) holds a weight that must not count.  The zero-|M| pixels return zeros and pass no
    gradient on -- to the table or to the weights."""
    from voge_amd.Renderer import get_rendered_normals
    table = torch.tensor([[0, 0, 1.0], [0, 0, -1.0], [0, 1.0, 0], [1.0, 0, 0]], dtype=torch.float64, requires_grad=True)
    weight = [[[[0.5, 0.25, 0.0], [0.5, 0.5, 0.0]], [[0.0, 0.0, 0.0], [0.5, 0.7, 0.0]]]]
    idx = [[[[0, 2, -1], [0, 1, -1]], [[-1, -1, -1], [3, 2, -1]]]]
    valid = [[[2, 2], [0, 1]]]
    frag, w = host_fragments(weight, idx, valid)
    M = get_rendered_normals(frag, table, normalize=False)
    assert M.shape == (1, 2, 2, 3)
    assert M.detach().numpy().tolist() == [[[[0, 0.25, 0.5], [0, 0, 0]], [[0, 0, 0], [0.5, 0, 0]]]]
    out = get_rendered_normals(frag, table)
    r = np.sqrt(0.25 ** 2 + 0.5 ** 2)
    assert np.abs(out.detach().numpy() - [[[[0, 0.25 / r, 0.5 / r], [0, 0, 0]], [[0, 0, 0], [1, 0, 0]]]]).max() <= 1e-15
    g = torch.arange(1.0, 13.0, dtype=torch.float64).reshape(1, 2, 2, 3)
    out.backward(g)
    assert torch.isfinite(w.grad).all() and torch.isfinite(table.grad).all()
    assert not w.grad[0, 0, 1].any() and not w.grad[0, 1, 0].any()      # the cancelling pixel and the empty one: nothing passed on
    assert not table.grad[1].any()                                      # (row 1 is read by the cancelling pixel only)
    assert w.grad[0, 0, 0, :2].abs().max() > 0 and table.grad[0].abs().max() > 0
    assert w.grad[0, 1, 1, 1] == 0                                      # the dead slot
    # a unit vector's gradient is perpendicular to it
    assert abs(float((table.grad[3] * torch.tensor([1.0, 0, 0], dtype=torch.float64)).sum())) <= 1e-15


# ---- 4. the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-NULL pointer value: nothing is dereferenced before validation is through)

    def fwd(B=2, N=10, scales=P, quats=P, verts=P, centres=P, out=P):
        return lib.voge_gauss_normals_fwd(scales, quats, verts, centres, B, N, 1, 1, 0, out, None)

    def bwd(B=2, N=10, scales=P, quats=P, verts=P, centres=P, g_out=P, out=P):
        return lib.voge_gauss_normals_bwd(scales, quats, verts, centres, g_out, B, N, 1, 1, 0, out, None)
    for f in (fwd, bwd):
        assert f(N=0) == 0 and f(B=0) == 0 and f(B=0, N=0) == 0      # nothing to do: a success that launches nothing
        assert f(N=0, scales=None, out=None) == 0
        assert f(N=-1) == -1 and f(B=-1) == -1 and f(B=-1, N=0) == -1
        for name in ("scales", "quats", "verts", "centres", "out"):
            assert f(**{name: None}) == -1, name
        assert f(B=1 << 15, N=1 << 15) == -1                          # B * N * 3 does not fit an int
    assert bwd(g_out=None) == -1
    assert lib.voge_abi_version() == 7


# ---- 5. what the compiler made of the kernels ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_no_lds_and_no_atomics(tmp_path):
    """The column of R is selected by compares on values already in registers: a run-time index into the 3x3 would put the matrix
    in scratch (or, promoted, in LDS).  The quaternion is one 16-byte load."""
    out = os.path.join(str(tmp_path), "gauss_normals.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only", "-o", out,
                           os.path.join(CSRC, "gauss_normals.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = sorted(re.findall(r"^(_ZN4voge\w*gauss_normals_(?:fwd|bwd)_kernel\w*):\s", text, flags=re.M))
    assert len(names) == 2 and "bwd" in names[0] and "fwd" in names[1], names
    for name in names:
        start = text.index(name + ":")
        body = text[start:text.index(".Lfunc_end", start)]
        d = text.index(".amdhsa_kernel " + name)
        desc = text[d:text.index(".end_amdhsa_kernel", d)]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, (name, "scratch")
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, (name, "LDS")
        assert not re.search(r"^\s+v_writelane_b32", body, flags=re.M), (name, "scalars spilled into VGPR lanes")
        assert "global_atomic" not in body, (name, "atomics")
        assert "global_load_dwordx4" in body, (name, "the quaternion's 16-byte load")
