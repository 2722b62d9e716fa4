"""CPU tests of the oriented form (three scales + a quaternion per Gaussian): the torch definition (Aggregation.oriented_sigma),
the closed-form backward the finishing kernel applies, the C ABI's two new entries, the mesh classes and the converter."""
import ctypes
import os

import numpy as np
import pytest
import torch

from util import GOLDEN


def _np_rotation(q):
    """The issue's definition in numpy fp64: q / |q| (identity when |q|^2 is not a positive finite number), standard matrix."""
    q = np.asarray(q, np.float64)
    n2 = (q * q).sum(-1, keepdims=True)
    ok = (n2 > 0) & np.isfinite(n2)
    with np.errstate(all="ignore"):
        qh = np.where(ok, q / np.sqrt(np.where(ok, n2, 1.0)), np.array([1.0, 0.0, 0.0, 0.0]))
    w, x, y, z = (qh[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3)), qh, ok[..., 0]


def _np_sigma(s, q):
    R = _np_rotation(q)[0]
    return np.einsum("...ik,...k,...jk->...ij", R, np.asarray(s, np.float64), R)


def _random(n, seed, batch=()):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.3, 1.5, batch + (n, 3))
    q = rng.normal(size=batch + (n, 4)) * rng.uniform(0.5, 2.0, batch + (n, 1))
    return s, q


@pytest.mark.parametrize("batch", [(), (2,)])
def test_oriented_sigma_is_the_definition(batch):
    from voge_amd.Aggregation import oriented_sigma, quaternion_to_matrix
    s, q = _random(500, 1, batch)
    S = oriented_sigma(torch.from_numpy(s), torch.from_numpy(q))
    assert S.shape == batch + (500, 3, 3) and S.dtype == torch.float64
    assert np.abs(S.numpy() - _np_sigma(s, q)).max() < 1e-14
    assert torch.equal(S, S.transpose(-1, -2))                                   # bitwise symmetric
    assert np.abs(np.linalg.eigvalsh(S.numpy()) - np.sort(s, -1)).max() < 1e-13   # eigenvalues = scales
    R = quaternion_to_matrix(torch.from_numpy(q))
    assert np.abs(R.numpy() - _np_rotation(q)[0]).max() < 1e-14      # (a dozen fp64 roundings on entries <= 1)
    assert np.abs(R.numpy() @ R.numpy().swapaxes(-1, -2) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(R.numpy()) - 1).max() < 1e-14
    S32 = oriented_sigma(torch.from_numpy(s).float(), torch.from_numpy(q).float())
    assert S32.dtype == torch.float32 and torch.equal(S32, S32.transpose(-1, -2))
    assert np.abs(S32.numpy() - _np_sigma(s, q)).max() < 1e-5


def test_zero_non_finite_and_non_unit_quaternions():
    from voge_amd.Aggregation import oriented_sigma
    s = torch.tensor([[0.5, 1.0, 2.0]] * 5, dtype=torch.float64, requires_grad=True)
    q = torch.tensor([[1.0, 0, 0, 0], [0, 0, 0, 0], [float("nan"), 1, 0, 0], [float("inf"), 0, 0, 1], [3.0, 0, 0, 0]],
                     dtype=torch.float64, requires_grad=True)
    S = oriented_sigma(s, q)
    for i in range(5):      # identity, and the unusable norms: diag(s) exactly
        assert torch.equal(S[i], torch.diag(s[i].detach())), i
    (S * torch.arange(45.0, dtype=torch.float64).reshape(5, 3, 3)).sum().backward()
    assert torch.equal(q.grad[1:4], torch.zeros(3, 4, dtype=torch.float64))       # zero / NaN / inf norm: zero gradient, no NaN
    assert torch.isfinite(s.grad).all()
    # scaling a quaternion changes nothing
    s2, q2 = _random(50, 2)
    a = oriented_sigma(torch.from_numpy(s2), torch.from_numpy(q2))
    b = oriented_sigma(torch.from_numpy(s2), torch.from_numpy(q2 * 7.5))
    assert np.abs(a.numpy() - b.numpy()).max() < 1e-14
    with pytest.raises(AssertionError, match="scales"):
        oriented_sigma(torch.ones(4, 3), torch.ones(5, 4))


def test_oriented_sigma_gradcheck():
    from voge_amd.Aggregation import oriented_sigma
    s, q = _random(6, 3)
    st, qt = torch.from_numpy(s).requires_grad_(True), torch.from_numpy(q).requires_grad_(True)
    assert torch.autograd.gradcheck(oriented_sigma, (st, qt), eps=1e-6, atol=1e-7)


def closed_form_backward(s, q, G, inverse):
    """The chain rule voge_frame_bwd_ori's finishing pass applies (include/voge_hip.h), in numpy fp64: G = d loss / d A (raw, not
    symmetric), A = R diag(d) R^T, d = 2 s | 2 / s."""
    R, qh, ok = _np_rotation(q)
    d = 2.0 / s if inverse else 2.0 * s
    gd = np.einsum("nik,nij,njk->nk", R, G, R)
    gs = -2.0 * gd / (s * s) if inverse else 2.0 * gd
    gR = np.einsum("nij,njk->nik", G + G.swapaxes(-1, -2), R) * d[:, None, :]
    w, x, y, z = (qh[:, i] for i in range(4))
    g = lambda i, j: gR[:, i, j]      # noqa: E731
    gw = 2 * (-z * g(0, 1) + y * g(0, 2) + z * g(1, 0) - x * g(1, 2) - y * g(2, 0) + x * g(2, 1))
    gx = 2 * (y * g(0, 1) + z * g(0, 2) + y * g(1, 0) - 2 * x * g(1, 1) - w * g(1, 2) + z * g(2, 0) + w * g(2, 1) - 2 * x * g(2, 2))
    gy = 2 * (-2 * y * g(0, 0) + x * g(0, 1) + w * g(0, 2) + x * g(1, 0) + z * g(1, 2) - w * g(2, 0) + z * g(2, 1) - 2 * y * g(2, 2))
    gz = 2 * (-2 * z * g(0, 0) - w * g(0, 1) + x * g(0, 2) + w * g(1, 0) - 2 * z * g(1, 1) + y * g(1, 2) + x * g(2, 0) + y * g(2, 1))
    gqh = np.stack([gw, gx, gy, gz], -1)
    norm = np.sqrt((q * q).sum(-1, keepdims=True))
    gq = (gqh - qh * (qh * gqh).sum(-1, keepdims=True)) / norm
    return gs, np.where(ok[:, None], gq, 0.0)


@pytest.mark.parametrize("inverse", [False, True])
def test_closed_form_backward_equals_autograd(inverse):
    from voge_amd.Aggregation import oriented_sigma
    s, q = _random(300, 4)
    G = np.random.default_rng(5).normal(size=(300, 3, 3))
    st, qt = torch.from_numpy(s).requires_grad_(True), torch.from_numpy(q).requires_grad_(True)
    A = 2.0 * oriented_sigma(1.0 / st if inverse else st, qt)
    (A * torch.from_numpy(G)).sum().backward()
    gs, gq = closed_form_backward(s, q, G, inverse)
    assert np.abs(gs - st.grad.numpy()).max() < 1e-12 * max(1.0, np.abs(gs).max())
    assert np.abs(gq - qt.grad.numpy()).max() < 1e-12 * max(1.0, np.abs(gq).max())
    assert np.abs((gq * q).sum(-1)).max() < 1e-12 * max(1.0, np.abs(gq).max())       # g_q is orthogonal to q


def test_abi_has_the_oriented_entries_and_they_validate_on_the_host():
    from voge_amd import _lib
    from test_abi_cpu import header_functions
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    fns = header_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("voge_frame_trace_fwd_ori", "voge_frame_bwd_ori"):
        assert name in fns and name in _lib.SIGNATURES and hasattr(raw, name)
        assert len(_lib.SIGNATURES[name][1]) == fns[name]
    assert lib.voge_abi_version() == 7
    P = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    cam = (P, P, P, P, 0, 64, 0, 0, 1, 100, 64, 64)
    out = (P, P, P, P, P, None, None)
    ok_ws = (4.6, P, 1 << 30)
    assert lib.voge_frame_trace_fwd_ori(P, P, P, 1, 1, 1, *cam, 1000, *ok_ws, *out) == -3                 # K above VOGE_MAX_K
    assert lib.voge_frame_trace_fwd_ori(P, P, P, 1, 1, 1, *cam, 16, 4.6, P, 1000, *out) == -2             # scratch too small
    assert lib.voge_frame_trace_fwd_ori(P, P, P, 1, 1, 0, *cam, 16, *ok_ws, *out) == -1                   # sigma_mode outside {1, 2}
    assert lib.voge_frame_trace_fwd_ori(P, P, P, 1, 1, 3, *cam, 16, *ok_ws, *out) == -1
    assert lib.voge_frame_trace_fwd_ori(P, P, None, 1, 1, 1, *cam, 16, *ok_ws, *out) == -1                # no quaternions
    assert lib.voge_frame_trace_fwd_ori(P, P, P + 4, 1, 1, 1, *cam, 16, *ok_ws, *out) == -1               # quaternions not 16-byte aligned
    assert lib.voge_frame_trace_fwd_ori(P, None, P, 1, 1, 1, *cam, 16, *ok_ws, *out) == -1                # no scales
    assert lib.voge_frame_trace_fwd_ori(P, P, P, 1, 1, 1, None, P, P, P, *cam[4:], 16, *ok_ws, *out) == -1   # no R
    # the old entry still refuses kind 3 (the oriented form is an entry of its own, not a new kind)
    assert lib.voge_frame_trace_fwd_gen(P, P, 1, 1, 3, *cam, 16, *ok_ws, *out) == -1

    def bwd(form=0, scales=P, quats=P, mode=1, K=16, acc_bytes=6400, act=P, g_scales=P, g_quats=P):
        return lib.voge_frame_bwd_ori(form, P, scales, quats, 1, 1, mode, P, P, P, P, P, act, P, act, P, P, P, -1.0, P, 3, 1, None, 1.0,
                                      1, 100, 64, 64, K, 3, 100, P, acc_bytes, 1, P, g_scales, g_quats, P, None)
    assert bwd(form=7) == -1
    assert bwd(mode=0) == -1 and bwd(mode=3) == -1
    assert bwd(K=200) == -3
    assert bwd(acc_bytes=100) == -2
    assert bwd(scales=None) == -1 and bwd(quats=None) == -1
    assert bwd(g_quats=None) == -1 and bwd(g_scales=None) == -1                                           # both or neither
    assert bwd(g_quats=P + 8) == -1


def test_mesh_classes():
    import VoGE.Meshes
    from voge_amd.Meshes import GaussianMeshes, OrientedGaussianMeshes, OrientedGaussianMeshesNaive
    assert VoGE.Meshes.OrientedGaussianMeshes is OrientedGaussianMeshes
    assert VoGE.Meshes.OrientedGaussianMeshesNaive is OrientedGaussianMeshesNaive
    v, s, q = torch.zeros(2, 5, 3), torch.ones(2, 5, 3), torch.ones(2, 5, 4)
    gm = OrientedGaussianMeshes(v, s, q, gradianted_args=(True, False, True))
    assert gm.oriented and not getattr(GaussianMeshes(v[0], s[0]), "oriented", False)
    out = gm()
    assert out[0] is gm.verts and out[1] is gm.scales and out[2] is gm.quats
    assert [p is x for p, x in zip(gm.grad_parameters(), (gm.verts, gm.quats))] == [True, True] and len(gm.grad_parameters()) == 2
    assert not gm.scales.requires_grad and gm.quats.requires_grad
    assert gm.to("cpu") is gm and len(list(gm.parameters())) == 3
    one = gm[1]
    assert isinstance(one, OrientedGaussianMeshesNaive) and one.oriented and one()[2].shape == (5, 4)
    nv = OrientedGaussianMeshesNaive(v, s, q)
    assert nv.to("cpu") is nv and nv()[1] is nv.scales and nv[0]()[0].shape == (5, 3)
    with pytest.raises(ValueError, match=r"scales\[\.\.,N,3\]"):
        OrientedGaussianMeshes(v, torch.ones(2, 5, 4), q)
    with pytest.raises(ValueError, match=r"quats\[\.\.,N,4\]"):
        OrientedGaussianMeshesNaive(v, s, torch.ones(5, 4))


def test_renderer_checks_oriented_shapes():
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras

    class Bad:
        oriented = True

        def __call__(self):
            return torch.zeros(5, 3), torch.ones(5, 3), torch.ones(5, 3)
    cams = PerspectiveCameras(focal_length=60.0, principal_point=((32.0, 32.0),), image_size=((64, 64),))
    renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(64, 64), max_assign=8))
    with pytest.raises(ValueError, match=r"scales\[\.\.,3\] and quats\[\.\.,4\]"):
        renderer(Bad())


def test_matrix_to_quaternion_round_trip():
    from voge_amd.Aggregation import quaternion_to_matrix
    from voge_amd.Converter.Converters import matrix_to_quaternion
    _, q = _random(400, 6)
    q[:4] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]      # identity and the three half turns (trace = -1)
    R = _np_rotation(q)[0]
    got = matrix_to_quaternion(R)
    assert got.shape == (400, 4) and np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-14 and (got[:, 0] >= 0).all()
    assert np.abs(quaternion_to_matrix(torch.from_numpy(got)).numpy() - R).max() < 1e-13


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_normal_mesh_converter_oriented_against_the_reference_fixture(dtype):
    """(scales, quats) of normal_mesh_converter(oriented=True) compose to the reference's own dense result (the fixture
    nm_isigma) within the dense form's tolerance, every vertex included; also with the outputs stored as fp32."""
    from voge_amd.Aggregation import oriented_sigma
    from voge_amd.Converter.Converters import naive_vertices_converter, normal_mesh_converter
    g = np.load(os.path.join(GOLDEN, "converters_more.npz"))
    v2, f2 = g["mesh2_verts"], g["mesh2_faces"]
    vv, scales, quats = normal_mesh_converter(v2.astype(np.float64), f2, g["nm_normals"], percentage=0.6, shape_ratio=0.3, oriented=True)
    assert scales.shape == (len(v2), 3) and quats.shape == (len(v2), 4)
    S = oriented_sigma(torch.from_numpy(scales.astype(dtype)).double(), torch.from_numpy(quats.astype(dtype)).double()).numpy()
    scale = np.abs(g["nm_isigma"]).max()
    err = np.abs(S - g["nm_isigma"]).max()
    print(f"[oriented] normal_mesh_converter(oriented=True), outputs as {np.dtype(dtype).name}: {err / scale:.2e} of scale (tolerance 2e-6)")
    assert err < 2e-6 * scale
    # vertex 3 is the degenerate one (det(rot) = 0): auto_fix makes it (b, b, b) with the identity
    b = naive_vertices_converter(v2.astype(np.float64), f2, percentage=0.6)[1]
    assert np.array_equal(quats[3], [1.0, 0.0, 0.0, 0.0]) and np.allclose(scales[3], b[3], rtol=1e-12)
    keep = np.arange(len(v2)) != 3
    assert np.allclose(scales[keep], b[keep, None] * np.array([1.0, 1.0, 0.3]), rtol=1e-12)
    assert np.abs(np.linalg.norm(quats, axis=1) - 1).max() < 1e-12
    with pytest.raises(ValueError, match="max_sig_rate"):
        normal_mesh_converter(v2.astype(np.float64), f2, g["nm_normals"], max_sig_rate=1.5, oriented=True)
    vt, st, qt = normal_mesh_converter(torch.from_numpy(v2).float(), torch.from_numpy(f2), torch.from_numpy(g["nm_normals"]), oriented=True)
    assert st.dtype == qt.dtype == torch.float32 and st.shape == (len(v2), 3) and qt.shape == (len(v2), 4)
