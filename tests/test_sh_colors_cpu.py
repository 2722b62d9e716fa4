"""CPU tests of the view-dependent colours (an extension: the reference has no spherical-harmonic code): the basis that
Aggregation.sh_colors -- the definition -- uses, the definition's values and autograd gradients against an independent fp64 numpy
restatement written here and central differences, the two C-ABI entries' host-side argument validation (no GPU in this
container: anything that reached HIP would fail differently), and what the compiler made of the two kernels."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the fp64 restatement: the table of the sixteen functions, written out once more ----------------------------------------
def basis_np(d):
    """[..., 3] unit vectors -> [..., 16]."""
    x, y, z = (np.asarray(d, np.float64)[..., i] for i in range(3))
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
        1.0925484305920792 * x * y,
        -1.0925484305920792 * y * z,
        0.31539156525252005 * (2 * zz - xx - yy),
        -1.0925484305920792 * x * z,
        0.5462742152960396 * (xx - yy),
        -0.5900435899266435 * y * (3 * xx - yy),
        2.890611442640554 * x * y * z,
        -0.4570457994644658 * y * (4 * zz - xx - yy),
        0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
        -0.4570457994644658 * x * (4 * zz - xx - yy),
        1.445305721320277 * z * (xx - yy),
        -0.5900435899266435 * x * (xx - 3 * yy)], axis=-1)


def sh_colors_np(sh, verts, centres, degree=None, clamp=True):
    """-> (out [B*N, C], pre [B, N, C]) in fp64."""
    sh, verts, centres = (np.asarray(a, np.float64) for a in (sh, verts, centres))
    N, M, C = sh.shape
    B = centres.shape[0]
    active = M if degree is None else (degree + 1) ** 2
    delta = (verts if verts.ndim == 3 else verts[None]) - centres[:, None, :]
    n2 = (delta * delta).sum(-1, keepdims=True)
    ok = n2 > 1e-20
    d = np.where(ok, delta / np.sqrt(np.where(ok, n2, 1.0)), 0.0)
    pre = np.einsum("bnm,nmc->bnc", basis_np(d)[..., :active], sh[:, :active]) + 0.5
    return (np.maximum(pre, 0.0) if clamp else pre).reshape(B * N, C), pre


def case(N=5, B=2, M=16, C=3, seed=0, per_view=False, scale=0.5):
    rng = np.random.default_rng(seed)
    sh = rng.normal(0, scale, (N, M, C))
    verts = rng.uniform(-1, 1, (B, N, 3) if per_view else (N, 3))
    c = rng.normal(size=(B, 3))
    centres = 3 * c / np.linalg.norm(c, axis=-1, keepdims=True)
    return sh, verts, centres, rng.normal(size=(B * N, C))


def t64(a, rg=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=rg)


# ---- 1. the basis ------------------------------------------------------------------------------------------------------------
def test_basis_of_the_definition_is_orthonormal_and_is_the_table():
    """The sixteen Y_m the definition uses, read out by one-hot coefficients (sh[n, m, c] = [m == c], C = 16, no clamp, camera
    at the origin so d = the node itself), on a Gauss-Legendre (64, in cos theta) x uniform-azimuth (128) quadrature of the sphere:
    Gram matrix within 1e-12 of the identity, and equal to the restatement above."""
    from voge_amd.Aggregation import sh_colors
    mu, wm = np.polynomial.legendre.leggauss(64)
    phi = (np.arange(128) + 0.5) * (2 * np.pi / 128)
    st = np.sqrt(1 - mu * mu)
    d = np.stack([st[:, None] * np.cos(phi)[None], st[:, None] * np.sin(phi)[None], np.broadcast_to(mu[:, None], (64, 128))], -1).reshape(-1, 3)
    w = np.repeat(wm * (2 * np.pi / 128), 128)
    one_hot = np.broadcast_to(np.eye(16)[None], (d.shape[0], 16, 16)).copy()
    Y = sh_colors(t64(one_hot), t64(d), torch.zeros((1, 3), dtype=torch.float64), clamp=False).numpy() - 0.5
    gram = np.einsum("p,pa,pb->ab", w, Y, Y)
    assert np.abs(gram - np.eye(16)).max() < 1e-12, np.abs(gram - np.eye(16)).max()
    assert np.abs(Y - basis_np(d)).max() < 1e-14


# ---- 2. the definition against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,degree", [(1, None), (4, None), (9, None), (16, None), (16, 2), (16, 0), (9, 1)])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("per_view", [False, True])
def test_definition_values_and_gradients(M, degree, clamp, per_view):
    """Values against the numpy restatement; autograd's gradients of sum(out * g) for sh, verts and cam_center against central
    differences of the restatement (fp64, step 1e-6: error of order 1e-10).  The case is the first seed whose |pre| all stay above
    1e-3 -- no difference steps across the clamp -- and that has clamped elements at all."""
    from voge_amd.Aggregation import sh_colors
    for seed in range(100):
        sh, verts, centres, g = case(M=M, per_view=per_view, seed=seed, scale=1.5)
        want, pre = sh_colors_np(sh, verts, centres, degree, clamp)
        if np.abs(pre).min() > 1e-3 and (pre < 0).any():
            break
    else:
        raise AssertionError("no usable seed")
    a, v, c = t64(sh, True), t64(verts, True), t64(centres, True)
    out = sh_colors(a, v, c, degree=degree, clamp=clamp)
    assert out.shape == want.shape and np.abs(out.detach().numpy() - want).max() < 1e-13
    (out * t64(g)).sum().backward()

    def loss(s_, v_, c_):
        return float((sh_colors_np(s_, v_, c_, degree, clamp)[0] * g).sum())
    eps = 1e-6
    for k, (arr, grad) in enumerate(((sh, a.grad), (verts, v.grad), (centres, c.grad))):
        if grad is None:      # (degree 0 does not depend on the direction: autograd leaves no gradient at all)
            assert degree == 0 or M == 1
            grad = torch.zeros(arr.shape, dtype=torch.float64)
        fd = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            hi, lo = arr.copy(), arr.copy()
            hi[i] += eps
            lo[i] -= eps
            args_hi, args_lo = [sh, verts, centres], [sh, verts, centres]
            args_hi[k], args_lo[k] = hi, lo
            fd[i] = (loss(*args_hi) - loss(*args_lo)) / (2 * eps)
        assert np.abs(grad.numpy() - fd).max() <= 1e-7 * max(1.0, np.abs(fd).max()), (k, np.abs(grad.numpy() - fd).max())
    active = M if degree is None else (degree + 1) ** 2
    assert (a.grad[:, active:] == 0).all()      # exactly zero above the active degree
    assert a.grad[:, :active].abs().max() > 0


def test_shared_and_per_view_verts_agree():
    from voge_amd.Aggregation import sh_colors
    sh, verts, centres, g = case(B=3)
    a1, v1 = t64(sh, True), t64(verts, True)
    a2, v2 = t64(sh, True), t64(np.broadcast_to(verts[None], (3,) + verts.shape).copy(), True)
    o1, o2 = sh_colors(a1, v1, t64(centres)), sh_colors(a2, v2, t64(centres))
    assert torch.equal(o1, o2)
    (o1 * t64(g)).sum().backward()
    (o2 * t64(g)).sum().backward()
    assert torch.allclose(a1.grad, a2.grad, rtol=0, atol=1e-14) and torch.allclose(v1.grad, v2.grad.sum(0), rtol=0, atol=1e-13)


def test_bad_shapes_and_degrees_raise():
    from voge_amd.Aggregation import sh_colors
    v, c = torch.zeros(4, 3), torch.ones(2, 3)
    with pytest.raises(ValueError):
        sh_colors(torch.zeros(4, 5, 3), v, c)
    with pytest.raises(ValueError):
        sh_colors(torch.zeros(4, 9, 3), v, c, degree=3)
    with pytest.raises(ValueError):
        sh_colors(torch.zeros(4, 9, 3), v, c, degree=-1)
    with pytest.raises(ValueError):
        sh_colors(torch.zeros(5, 9, 3), v, c)


def test_a_gaussian_at_the_camera_centre_keeps_the_constant_term_only():
    from voge_amd.Aggregation import sh_colors
    sh, verts, centres, g = case(N=4, B=2)
    verts[1] = centres[0]                      # |delta| = 0 in view 0
    verts[2] = centres[1] + 1e-11              # |delta|^2 = 3e-22, below the 1e-20 floor, in view 1
    a, v, c = t64(sh, True), t64(verts, True), t64(centres, True)
    out = sh_colors(a, v, c, clamp=False)
    assert np.abs(out.detach().numpy() - sh_colors_np(sh, verts, centres, clamp=False)[0]).max() < 1e-13
    assert torch.equal(out[1], 0.28209479177387814 * a[1, 0] + 0.5) and torch.equal(out[4 + 2], 0.28209479177387814 * a[2, 0] + 0.5)
    (out * t64(g)).sum().backward()
    for grad in (a.grad, v.grad, c.grad):
        assert torch.isfinite(grad).all()
    # the vertex gradient of such a Gaussian is what its OTHER view gives: take that view away and it is exactly zero
    a1, v1 = t64(sh, True), t64(verts, True)
    (sh_colors(a1, v1, t64(centres[:1]), clamp=False) * t64(g[:4])).sum().backward()
    assert (v1.grad[1] == 0).all() and v1.grad[0].abs().max() > 0


def test_sh_to_colors_is_public_and_takes_the_definition_off_the_device():
    """Exported through VoGE.Renderer like get_depth; host tensors, fp64 and a cameras object all give the definition's values."""
    from VoGE.Renderer import sh_to_colors
    from voge_amd import Renderer
    from voge_amd.Aggregation import sh_colors
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    assert sh_to_colors is Renderer.sh_to_colors
    doc = sh_to_colors.__doc__
    assert "degree" in doc and "get_camera_center" in doc and "once" in doc
    sh, verts, centres, _ = case()
    for dtype in (torch.float64, torch.float32):
        a, v, c = (torch.tensor(x, dtype=dtype) for x in (sh, verts, centres))
        assert torch.equal(sh_to_colors(a, v, c, degree=2), sh_colors(a, v, c, degree=2, clamp=True))
    R, T = look_at_view_transform([3.0, 4.0], [10.0, -20.0], [30.0, 200.0])
    cams = PerspectiveCameras(focal_length=100.0, principal_point=((32.0, 32.0),), image_size=((64, 64),), device="cpu")
    cams.R, cams.T = R, T
    a, v = torch.tensor(sh, dtype=torch.float32), torch.tensor(verts, dtype=torch.float32)
    assert torch.equal(sh_to_colors(a, v, cams), sh_colors(a, v, cams.get_camera_center()))
    with pytest.raises(ValueError):
        sh_to_colors(torch.zeros(5, 5, 3), v, cams)


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entries_validate_before_any_hip_call(lib):
    P = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)

    def fwd(B=2, N=10, M=16, C=3, degree=3, out=P, sh=P):
        return lib.voge_sh_colors_fwd(sh, P, P, B, N, M, C, degree, 1, 1, out, None)

    def bwd(B=2, N=10, M=16, C=3, degree=3, g_sh=P, g_verts=P, g_out=P):
        return lib.voge_sh_colors_bwd(P, P, P, g_out, B, N, M, C, degree, 1, 1, g_sh, g_verts, None)
    for f in (fwd, bwd):
        assert f(M=5) == -1
        assert f(M=0) == -1
        assert f(C=0) == -1
        assert f(C=5) == -1
        assert f(degree=4) == -1
        assert f(M=9, degree=3) == -1
        assert f(degree=-1) == -1
        assert f(N=-1) == -1 and f(B=-1) == -1
        assert f(N=0) == 0 and f(B=0) == 0      # nothing to do: a success that launches nothing
    assert fwd(out=None) == -1
    assert fwd(sh=None) == -1
    assert fwd(sh=P + 4) == -1                   # 48 floats a row: 16-byte loads
    assert bwd(g_sh=None) == -1 and bwd(g_verts=None) == -1 and bwd(g_out=None) == -1
    assert bwd(g_sh=P + 8) == -1
    assert lib.voge_abi_version() == 7


# ---- 4. what the compiler made of the kernels ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sh_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """All 32 instantiations (M in 1, 4, 9, 16; C in 1..4; forward and backward): the up to 64 coefficients and 64 accumulators
    of a Gaussian live in registers -- no scratch, no scalars parked in VGPR lanes."""
    out = os.path.join(str(tmp_path), "sh_colors.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only", "-o", out,
                           os.path.join(CSRC, "sh_colors.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN4voge\w*sh_colors_(?:fwd|bwd)_kernelILi\d+ELi\d+E\w*):\s", text, flags=re.M)
    want = {f"sh_colors_{d}_kernelILi{m}ELi{c}E" for d in ("fwd", "bwd") for m in (1, 4, 9, 16) for c in (1, 2, 3, 4)}
    assert len(names) == 32 and {re.search(r"sh_colors_\w+?_kernelILi\d+ELi\d+E", n).group(0) for n in names} == want, names
    for name in names:
        start = text.index(name + ":")
        body = text[start:text.index(".Lfunc_end", start)]
        d = text.index(".amdhsa_kernel " + name)
        desc = text[d:text.index(".end_amdhsa_kernel", d)]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, (name, "scratch")
        assert not re.search(r"^\s+v_writelane_b32", body, flags=re.M), (name, "scalars spilled into VGPR lanes")
        assert "global_atomic" not in body, (name, "atomics")
