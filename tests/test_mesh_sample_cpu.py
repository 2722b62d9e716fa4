"""CPU tests of mesh surface sampling: the definition (Aggregation.mesh_surface_points), Losses.SurfaceSampler and
sample_points_from_meshes on the host, and the C entries' argument validation (no GPU: nothing may reach a HIP call)."""
import os

import numpy as np
import pytest
import torch

from sample_meshes import (all_test_meshes, check_face_choice, face_cdf, grid_mesh, random_u, tetrahedron, unequal_mesh,
                           with_zero_area_faces)
from voge_amd import Aggregation, Losses, ops

BLOCK = ops.MESH_SAMPLE_BLOCK


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the ABI --------------------------------------------------------------------------------------------------------------------

def test_signatures_and_validation_before_any_hip_call(lib):
    from voge_amd import _lib
    for name in ("voge_mesh_sample_workspace_bytes", "voge_mesh_sample_fwd", "voge_mesh_sample_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert BLOCK == 256
    P = 4096      # (a non-NULL, 16-byte aligned pointer value: nothing is dereferenced before validation is through)
    n = lib.voge_mesh_sample_workspace_bytes(2562, 5120, 5000)
    assert n >= 16 + (2562 + 5120) * 24 and n >= 5120 * 8 and n % 16 == 0
    assert lib.voge_mesh_sample_workspace_bytes(0, 1, 1) == 0 and lib.voge_mesh_sample_workspace_bytes(4, 0, 1) == 0
    assert lib.voge_mesh_sample_workspace_bytes(4, 4, -1) == 0 and lib.voge_mesh_sample_workspace_bytes(4, 2 ** 28, 1) == 0
    fwd = lib.voge_mesh_sample_fwd
    assert fwd(P, 4, P, 0, P, 10, P, P, P, P, None, P, 1 << 20, None) == -1          # no faces
    assert fwd(None, 4, P, 4, P, 10, P, P, P, P, None, P, 1 << 20, None) == -1       # no verts
    assert fwd(P, 4, P, 4, P, 10, P, None, None, P, None, P, 1 << 20, None) == -1    # no face_idx
    assert fwd(P, 4, P, 4, P, 10, P, None, P, P, None, P + 8, 1 << 20, None) == -1   # workspace off the boundary
    assert fwd(P, 4, P, 4, P, 10, P, None, P, P, None, P, 8, None) == -2             # workspace too small
    assert fwd(P, 4, P, 4, None, 0, None, None, None, None, None, None, 0, None) == 0      # S == 0: nothing to do
    bwd = lib.voge_mesh_sample_bwd
    assert bwd(P, 4, P, 4, P, P, P, P, 10, P, P, None, P, 1 << 20, None) == -1       # no g_verts
    assert bwd(P, 4, P, 4, None, None, P, P, 10, P, P, P, P, 1 << 20, None) == -1    # normals' gradient without the corner table
    assert bwd(P, 4, P, 4, P, P, None, P, 10, P, P, P, P, 1 << 20, None) == -1       # no face_idx
    assert bwd(P, 4, P, 4, P, P, P, P, 10, P, P, P, P, 64, None) == -2               # workspace too small
    assert bwd(P, 0, P, 4, P, P, P, P, 10, P, P, P, P, 1 << 20, None) == -1          # no vertices


# ---- the sampler's tables -------------------------------------------------------------------------------------------------------

def test_surface_sampler_tables_and_errors():
    faces = [[0, 1, 2], [0, 2, 3], [4, 3, 2], [1, 0, 4]]
    s = Losses.SurfaceSampler(faces, num_verts=6)
    assert (s.num_verts, s.num_faces) == (6, 4)
    assert s.faces.dtype == s.corner_off.dtype == s.corner.dtype == torch.int32
    assert s.faces.tolist() == faces
    assert s.corner_off.tolist() == [0, 3, 5, 8, 10, 12, 12]      # (vertex 5: no corner)
    # entries face * 3 + role, ascending inside a vertex
    assert s.corner.tolist() == [0, 3, 10, 1, 9, 2, 4, 8, 5, 7, 6, 11]
    assert Losses.SurfaceSampler(torch.tensor(faces)).num_verts == 5
    assert s.to("cpu") is s
    for bad in ([[0, 1, 1]], [[0, 1, 6]], [[-1, 1, 2]]):
        with pytest.raises(ValueError):
            Losses.SurfaceSampler(bad, num_verts=6)
    with pytest.raises(ValueError):
        Losses.SurfaceSampler([[0.0, 1.0, 2.0]])
    with pytest.raises(ValueError):
        Losses.sample_points_from_meshes(torch.zeros(3, 3), torch.zeros((0, 3), dtype=torch.long), 4)


# ---- the distribution -----------------------------------------------------------------------------------------------------------

def test_face_counts_follow_the_areas():
    verts, faces = unequal_mesh()
    S = 200000
    u = random_u(S, 11)
    _, _, idx, _ = Aggregation.mesh_surface_points(verts, faces, u)
    A2, cdf = face_cdf(verts, faces)
    prob = A2.double() / cdf[-1]
    assert float(prob.max() / prob.min()) > 2      # unequal indeed
    count = torch.bincount(idx, minlength=len(faces)).double()
    sd = torch.sqrt(S * prob * (1 - prob))
    assert ((count - S * prob).abs() <= 5 * sd).all(), float(((count - S * prob).abs() / sd).max())


def test_points_lie_in_their_faces():
    verts, faces = unequal_mesh()
    u = random_u(5000, 12)
    p, n, idx, bary = Aggregation.mesh_surface_points(verts.double(), faces, u.double(), True)
    tri = verts.double()[faces[idx]]
    assert (bary >= 0).all() and ((bary.sum(-1) - 1).abs() <= 1e-15).all()
    assert ((bary[:, :, None] * tri).sum(1) - p).abs().max() <= 1e-15                 # the barycentric combination: inside
    assert ((p - tri[:, 0]) * n).sum(-1).abs().max() <= 1e-15                         # in the plane
    assert ((n.norm(dim=-1) - 1).abs() <= 1e-15).all()
    want = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((n - want / want.norm(dim=-1, keepdim=True)).abs() <= 1e-15).all()
    # the public function on the host is the definition
    got = Losses.sample_points_from_meshes(verts.double(), faces, u=u.double(), return_normals=True, return_faces=True)
    assert torch.equal(got[0], p) and torch.equal(got[1], n) and torch.equal(got[2], idx) and torch.equal(got[3], bary)
    assert torch.equal(Losses.sample_points_from_meshes(verts.double(), Losses.SurfaceSampler(faces), u=u.double()), p)


def test_public_shapes_and_batches():
    verts, faces = tetrahedron()
    g = torch.Generator().manual_seed(5)
    p = Losses.sample_points_from_meshes(verts, faces, 100, generator=g)
    assert p.shape == (100, 3) and p.dtype == torch.float32
    p0, n0, f0, b0 = Losses.sample_points_from_meshes(verts, faces, 0, return_normals=True, return_faces=True)
    assert p0.shape == n0.shape == b0.shape == (0, 3) and f0.shape == (0,)
    vb, ub = torch.stack((verts, verts * 2 + 1)), torch.stack((random_u(50, 1), random_u(50, 2)))
    pb, fb, bb = Losses.sample_points_from_meshes(vb, faces, u=ub, return_faces=True)
    for b in range(2):
        one = Losses.sample_points_from_meshes(vb[b], faces, u=ub[b], return_faces=True)
        assert torch.equal(pb[b], one[0]) and torch.equal(fb[b], one[1]) and torch.equal(bb[b], one[2])
    with pytest.raises(ValueError):
        Losses.sample_points_from_meshes(verts, faces, u=ub)
    with pytest.raises(ValueError):
        Losses.sample_points_from_meshes(verts[:3], Losses.SurfaceSampler(faces))


# ---- gradients ------------------------------------------------------------------------------------------------------------------

def test_gradcheck_on_the_tetrahedron_with_normals():
    verts, faces = tetrahedron()
    rng = np.random.default_rng(2)
    v = (verts.double() + torch.from_numpy(rng.normal(0, 0.05, (4, 3)))).requires_grad_(True)
    u = random_u(64, 13).double()

    def fn(x):
        p, n, _, _ = Aggregation.mesh_surface_points(x, faces, u, True)
        return p, n

    assert torch.autograd.gradcheck(fn, (v,), eps=1e-6, atol=1e-7)


# ---- the degenerate rules -------------------------------------------------------------------------------------------------------

def test_zero_area_faces_are_never_chosen_and_the_clamp():
    verts, faces = grid_mesh(4, 4)
    verts, faces = with_zero_area_faces(verts, faces, [0, 7, 8, 9, 36])
    F = len(faces)
    assert F == 37
    A2, cdf = face_cdf(verts, faces)
    assert (A2[[0, 7, 8, 9, 36]] == 0).all() and (A2 > 0).sum() == 32
    u = random_u(20000, 14)
    _, _, idx, _ = Aggregation.mesh_surface_points(verts, faces, u)
    assert (A2[idx] > 0).all() and set(idx.tolist()) == set(range(F)) - {0, 7, 8, 9, 36}
    edge = torch.tensor([[0.0, 0.3, 0.3], [1 - 2.0 ** -24, 0.3, 0.3], [-2.0, 0.3, 0.3], [5.0, 0.3, 0.3], [float("nan"), 0.3, 0.3],
                         [1.0, 0.3, 0.3]])
    _, _, idx, _ = Aggregation.mesh_surface_points(verts, faces, edge)
    assert idx.tolist() == [1, 35, 1, 35, 1, 35]
    # u1, u2 are clamped too: a NaN is 0 (the point is vertex a), 7 is 1 - 2^-24
    p, _, idx, bary = Aggregation.mesh_surface_points(verts, faces, torch.tensor([[0.5, float("nan"), 7.0]]))
    assert torch.equal(p[0], verts[faces[idx[0], 0]]) and bary[0].tolist() == [1.0, 0.0, 0.0]


def test_all_degenerate_and_nan_meshes_give_minus_one_and_zero_gradients():
    verts, faces = tetrahedron()
    flat = (verts * torch.tensor([1.0, 0.0, 0.0])).requires_grad_(True)                # every vertex on one line
    nanv = verts.clone()
    nanv[2, 1] = float("nan")
    nanv.requires_grad_(True)
    u = random_u(100, 15)
    for v in (flat, nanv):
        p, n, idx, bary = Aggregation.mesh_surface_points(v, faces, u, True)
        assert (idx == -1).all() and not p.any() and not n.any() and not bary.any()
        (p.sum() + n.sum()).backward()
        assert v.grad is not None and not v.grad.any()


# ---- the boundary rule's cap ----------------------------------------------------------------------------------------------------

def test_reversed_summation_stays_within_the_cap():
    """The definition against cumulative sums made in the REVERSED order (prefix f added from face f down to face 0: another
    order of the same terms, as a kernel's is) on every mesh the tests use: every sample passes one of the two rules -- a
    zero-area face is never chosen, nothing is substituted --, and at most 1 % pass by the boundary rule."""
    for name, (verts, faces) in all_test_meshes().items():
        A2, cdf = face_cdf(verts, faces)
        a = A2.double().numpy()
        F = len(a)
        rev = np.empty(F)
        for s0 in range(0, F, 512):      # rows s0 .. s0 + 511: row f holds A2[f], A2[f-1], .., A2[0], 0, ..; summed left to right
            rows = np.arange(s0, min(s0 + 512, F))
            k = rows[:, None] - np.arange(rows[-1] + 1)[None, :]
            rev[rows] = np.cumsum(np.where(k >= 0, a[np.maximum(k, 0)], 0.0), axis=1)[:, -1]
        # a table must not decrease; the running maximum keeps it flat over zero-area faces (a zero term leads the row's sum)
        rev = torch.from_numpy(np.maximum.accumulate(rev))
        u = random_u(20000, 16)
        t = u[:, 0].double() * cdf[-1]
        got = torch.searchsorted(rev, t, right=True).clamp(max=F - 1)
        second = check_face_choice(verts, faces, u, got)
        assert second <= 0.01 * len(u), (name, second)
