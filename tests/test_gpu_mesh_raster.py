"""GPU tests of mesh depth maps (csrc/mesh_raster.hip behind Meshing.rasterize_mesh), every case on BOTH routes:

  * the two routes return the same bits, and those are the bits of Aggregation.mesh_rasterize in fp32 on the host -- pix_to_face,
    bary and depth, compared as bit patterns (a route whose screen box is too small shows here);
  * against the definition in fp64, off the marks of step 7 (whose cap tests/test_mesh_raster_cpu.py asserts for the same cases):
    equal faces, bary and depth within the bounds tests/mesh_raster_cases.py restates from the kernel file's header;
  * the edges of the rule, list stress, the backward against fp64 autograd, dirty workspaces, graph capture, interpolate_vertex_attr.

References are computed once a module and left unchanged."""
import functools

import numpy as np
import pytest
import torch

import dirty as D
import mesh_raster_cases as rc
import meshing_cases as mc
import sample_meshes
from util import log_line
from voge_amd import Aggregation, ops
from voge_amd.Meshing import interpolate_vertex_attr, rasterize_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ("brute", "bins")
CASES = rc.main_cases()
IDS = [c.name for c in CASES]


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def device_run(verts, faces, cams, size, route, cull=False):
    return rasterize_mesh(verts.to(DEV), faces.to(DEV), mc.Cams(*(t.to(DEV) for t in cams)), size, cull_backfaces=cull, route=route)


def check_routes(verts, faces, cams, size, cull=False):
    """Both routes against the fp32 definition on the host, bit for bit -> the host's (pix_to_face, bary, depth)"""
    R, T, focal, pp = cams
    B = max(len(R), len(T))
    ref = Aggregation.mesh_rasterize(verts, faces, R.expand(B, 3, 3), T.expand(B, 3), focal.expand(B, 2), pp.expand(B, 2), size[0], size[1], cull)
    for route in ROUTES:
        got = device_run(verts, faces, cams, size, route, cull)
        assert got.pix_to_face.dtype == torch.int32 and got.pix_to_face.shape == (B,) + tuple(size)
        assert torch.equal(got.pix_to_face.cpu().long(), ref[0]), route
        assert bits(got.bary) == bits(ref[1]) and bits(got.depth) == bits(ref[2]), route
    return ref


@functools.lru_cache(maxsize=None)
def fp64_reference(name):
    c = {c.name: c for c in CASES}[name]
    return Aggregation.mesh_rasterize(c.verts.double(), c.faces, *c.args(torch.float64), mark=rc.MARK)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_routes_equal_the_fp32_definition_and_fp64_off_the_marks(case, hip_lib):
    cams = (case.R, case.T, case.focal, case.pp)
    p32, b32, d32 = check_routes(case.verts, case.faces, cams, (case.H, case.W))
    p64, b64, d64, marks = fp64_reference(case.name)
    clear = ~marks
    assert float(marks.float().mean()) <= rc.MARK_CAP and (p32[clear] == p64[clear]).all()
    e_b, e_d = rc.forward_bounds(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, p64)
    ok = clear & (p64 >= 0)
    share_d = float(((d32.double() - d64).abs() / e_d)[ok].max())
    share_b = float(((b32.double() - b64).abs().max(-1).values / e_b)[ok].max())
    log_line(f"[mesh raster] {case.name}: depth uses {share_d:.4f} of its bound, bary {share_b:.4f}; "
             f"largest depth error {float((d32.double() - d64).abs()[ok].max()):.2e} at depth {float(d64.max()):.2f}")
    assert share_d <= 1.0 and share_b <= 1.0


# ---- the edges of the rule ------------------------------------------------------------------------------------------------------

EYE = (torch.eye(3)[None], torch.zeros(1, 3))


def straight(focal=8.0, pp=8.0):
    """A camera at the origin that looks down +z: pixel (i, j) looks along ((pp - j - 0.5) / f, (pp - i - 0.5) / f, 1)"""
    return EYE + (torch.tensor([[focal, focal]]), torch.tensor([[pp, pp]]))


def test_pixel_centres_on_shared_edges_and_vertices(hip_lib):
    """An axis-aligned camera over the flat 16 x 16 grid, f = 16 and pp = 9.5: every pixel centre falls exactly on a grid line, most
    on a vertex, every z is 1 -- a tie everywhere.  No hole, and the lower index wins"""
    v, f = sample_meshes.grid_mesh(16, 16, lift=False)
    v = v + torch.tensor([-0.5, -0.5, 1.0])
    cams = straight(16.0, 9.5)
    pix, bary, depth = check_routes(v, f, cams, (18, 18))
    want, _, _ = rc.rasterize_numpy(v, f, *cams, 18, 18)      # (exact in fp64: every number is a dyadic rational)
    assert (pix.numpy() == want).all()
    inside = np.zeros((18, 18), bool)
    inside[1:18, 1:18] = True                                  # x = 0.5 + (9 - j) / 16 in [-0.5, 0.5] <=> 1 <= j <= 17
    assert ((pix[0].numpy() >= 0) == inside).all()
    d = (9 - torch.arange(18.0)) / 16
    flat = (1 + d[None, :] ** 2 + d[:, None] ** 2).sqrt()      # the plane z = 1 along the unit ray
    assert ((depth[0] - flat).abs()[torch.from_numpy(inside)] <= 4 * rc.U * flat.max()).all()


TRI = torch.tensor([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]])


def test_repeated_and_coincident_faces(hip_lib):
    pix, _, _ = check_routes(TRI, torch.tensor([[0, 1, 2], [0, 1, 2]]), straight(), (16, 16))
    assert set(pix.unique().tolist()) == {-1, 0}
    one = pix
    pix, _, _ = check_routes(TRI, torch.tensor([[0, 2, 1], [0, 1, 2]]), straight(), (16, 16))      # (their z may differ in the last bit)
    assert set(pix.unique().tolist()) <= {-1, 0, 1} and torch.equal(pix >= 0, one >= 0)
    c0, _, _ = check_routes(TRI, torch.tensor([[0, 2, 1], [0, 1, 2]]), straight(), (16, 16), cull=True)
    c1, _, _ = check_routes(TRI, torch.tensor([[0, 1, 2], [0, 2, 1]]), straight(), (16, 16), cull=True)
    assert len(c0.unique()) == 2 and torch.equal(c0 >= 0, pix >= 0) and torch.equal(c0.clamp(min=-1) >= 0, c1 >= 0)
    assert int(c0.max()) + int(c1.max()) == 1      # the same one of the two windings survives, whichever index it has


def test_faces_at_and_behind_the_camera_plane(hip_lib):
    f = torch.tensor([[0, 1, 2]])
    behind, _, _ = check_routes(TRI * torch.tensor([1.0, 1.0, -1.0]), f, straight(), (16, 16))
    assert (behind == -1).all()
    through = torch.tensor([[-1.0, -1.0, -1.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]])
    pix, _, depth = check_routes(through, f, straight(), (16, 16))
    assert 0 < int((pix >= 0).sum()) < 256 and (depth[pix >= 0] > 0).all()
    tiny, _, depth = check_routes(torch.tensor([[-1.0, -1.0, 1e-30], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]]), f, straight(), (16, 16))
    assert int((tiny >= 0).sum()) > 0 and torch.isfinite(depth).all()
    edge_on = torch.tensor([[0.0, -1.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 3.0]])      # its plane holds the camera centre
    for pp in (8.0, 8.5):      # (8.5: a column of pixel centres lies in that plane)
        check_routes(edge_on, f, straight(8.0, pp), (16, 16))


def test_degenerate_faces_and_slivers(hip_lib):
    zero = torch.cat([TRI, torch.tensor([[0.0, -1.0, 2.0]])])      # (vertex 3: the midpoint of 0 and 1)
    pix, _, _ = check_routes(zero, torch.tensor([[0, 1, 1], [0, 3, 1], [2, 2, 2]]), straight(), (16, 16))      # two corners equal; collinear; a point
    assert (pix == -1).all()
    # a sliver between two columns of pixel centres: x / z in (0.01, 0.11) while the centres sit at multiples of 1 / 8
    sliver = torch.tensor([[0.02, -1.0, 1.0], [0.2, -2.0, 2.0], [0.15, 3.0, 3.0]])
    pix, _, _ = check_routes(sliver, torch.tensor([[0, 1, 2]]), straight(8.0, 8.5), (16, 16))
    assert (pix == -1).all()
    pix, _, _ = check_routes(sliver, torch.tensor([[0, 1, 2]]), straight(8.0, 8.0), (16, 16))      # centres at odd multiples of 1 / 16: one column is hit
    assert int((pix >= 0).sum()) > 0


def test_a_face_over_the_whole_image_and_a_nan_vertex(hip_lib):
    c = CASES[0]
    cams = (c.R[:1], c.T[:1], c.focal[:1], c.pp[:1])
    plain = Aggregation.mesh_rasterize(c.verts, c.faces, *(t[:1] for t in (c.R, c.T, c.focal, c.pp)), c.H, c.W)[0]
    V = len(c.verts)
    for z in (0.5, 30.0):      # in front of the sphere and behind it, in view space
        big = torch.tensor([[-90.0, -80.0, 1.0], [90.0, -80.0, 1.0], [0.0, 95.0, 1.0]]) * z
        world = (big - c.T[0]) @ c.R[0].T
        v, f = torch.cat([c.verts, world]), torch.cat([c.faces, torch.tensor([[V, V + 1, V + 2]])])
        pix, _, _ = check_routes(v, f, cams, (c.H, c.W))
        assert (pix >= 0).all()
        if z < 1:
            assert (pix == len(c.faces)).all()
        else:
            assert torch.equal(pix[plain >= 0], plain[plain >= 0]) and (pix[plain < 0] == len(c.faces)).all()
    v = c.verts.clone()
    v[7, 1] = float("nan")
    pix, bary, depth = check_routes(v, c.faces, cams, (c.H, c.W))
    touched = (c.faces == 7).any(1)
    assert not touched[pix[pix >= 0]].any() and torch.isfinite(depth).all() and torch.isfinite(bary).all()


def test_a_mesh_far_from_the_origin(hip_lib):
    v, f = sample_meshes.tetrahedron(1.0, 1000.0)
    c = CASES[4]
    T = c.T - torch.full((3,), 1000.0) @ c.R      # the same views of the same tetrahedron, moved with it
    pix, _, _ = check_routes(v, f, (c.R, T, c.focal, c.pp), (c.H, c.W))
    assert ((pix >= 0).float().mean(dim=(1, 2)) > 0.3).all()


def test_empty_meshes_no_views_shared_cameras_and_int64_faces(hip_lib):
    c = CASES[4]
    cams = (c.R, c.T, c.focal, c.pp)
    pix, bary, depth = check_routes(c.verts, c.faces[:0], cams, (c.H, c.W))
    assert (pix == -1).all() and (bary == 0).all() and (depth == 0).all()
    for route in ROUTES:
        none = device_run(c.verts, c.faces, tuple(t[:0] for t in cams), (c.H, c.W), route)
        assert none.pix_to_face.shape == (0, c.H, c.W) and none.depth.shape == (0, c.H, c.W) and none.bary.shape == (0, c.H, c.W, 3)
        a = device_run(c.verts, c.faces, cams, (c.H, c.W), route)
        b = device_run(c.verts, c.faces.to(torch.int32), cams, (c.H, c.W), route)
        assert all(bits(x) == bits(y) for x, y in zip(a, b))
    shared = (c.R[:1], c.T[:1].expand(3, 3) + torch.tensor([[0.0, 0, 0], [0.1, 0, 0], [0, 0.1, 0.2]]), c.focal[:1], c.pp[:1])
    pix, _, _ = check_routes(c.verts, c.faces, shared, (c.H, c.W))      # B = 3 from T, one R and one set of intrinsics for all
    assert pix.shape[0] == 3 and not torch.equal(pix[0], pix[1])


# ---- list stress ----------------------------------------------------------------------------------------------------------------

def test_twenty_thousand_faces_in_one_tile(hip_lib):
    """20 000 tiny faces inside the 16 x 16 pixels of one tile of a 32 x 32 image: 79 LDS chunks on either route"""
    rng = np.random.default_rng(11)
    n = 20000
    z = rng.uniform(1.0, 3.0, n)
    ctr = np.stack([rng.uniform(-0.9, -0.1, n), rng.uniform(-0.9, -0.1, n), np.ones(n)], 1) * z[:, None]      # x / z, y / z in (-1, 0): pixels 16 .. 31
    tri = ctr[:, None, :] + rng.uniform(-0.06, 0.06, (n, 3, 3)) * np.array([1.0, 1.0, 0.3])
    v = torch.from_numpy(tri.reshape(-1, 3).astype(np.float32))
    f = torch.arange(3 * n).reshape(n, 3)
    pix, _, _ = check_routes(v, f, straight(16.0, 16.0), (32, 32))
    assert (pix[0, :15, :] == -1).all() and (pix[0, :, :15] == -1).all() and (pix[0, 17:, 17:] >= 0).float().mean() > 0.7
    assert len(pix.unique()) > 100


def test_many_short_lists(hip_lib):
    v, f = sample_meshes.grid_mesh(64, 64)
    c = CASES[2]
    pix, _, _ = check_routes(v - torch.tensor([0.5, 0.5, 0.0]), f, (c.R, c.T, torch.tensor([[95.3, 97.1]] * 2), torch.tensor([[32.4, 31.7]] * 2)), (64, 64))
    assert ((pix >= 0).float().mean(dim=(1, 2)) > 0.5).all() and len(pix.unique()) > 2000


# ---- backward -------------------------------------------------------------------------------------------------------------------

def device_grad(verts, faces, cams, size, g, route):
    vd = verts.to(DEV).requires_grad_(True)
    frags = rasterize_mesh(vd, faces.to(DEV), mc.Cams(*(t.to(DEV) for t in cams)), size, route=route)
    assert not frags.pix_to_face.requires_grad and not frags.bary.requires_grad
    (frags.depth * g.to(DEV)).sum().backward()
    return frags.pix_to_face.cpu(), vd.grad.cpu()


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]], ids=[IDS[1], IDS[3], IDS[4]])
def test_backward_against_fp64_autograd(case, hip_lib):
    """verts.grad of (depth * g).sum() against fp64 autograd of the definition at the bound of tests/mesh_raster_cases.py.  The cases
    are not free of marked pixels (only the 29 x 37 tetrahedron is); what the comparison needs is weaker and asserted here: the
    device chooses the fp64 definition's face under every pixel, marked or not, so both differentiate the same function"""
    cams = (case.R, case.T, case.focal, case.pp)
    g = torch.from_numpy(np.random.default_rng(9).standard_normal((len(case.R), case.H, case.W)).astype(np.float32))
    vd = case.verts.double().requires_grad_(True)
    p64, _, d64 = Aggregation.mesh_rasterize(vd, case.faces, *case.args(torch.float64))
    ref, = torch.autograd.grad((d64 * g.double()).sum(), vd)
    closed, bound = rc.closed_form_grad(case.verts, case.faces, *cams, case.H, case.W, p64, g)
    assert (closed - ref).abs().max() <= 1e-10 * float(ref.abs().max())
    first = None
    for route in ROUTES:
        pix, got = device_grad(case.verts, case.faces, cams, (case.H, case.W), g, route)
        assert torch.equal(pix.long(), p64)
        share = float(((got.double() - ref).abs() / bound).max())
        log_line(f"[mesh raster] backward, {case.name}, {route}: {share:.4f} of the bound, largest |grad| {float(ref.abs().max()):.3g}")
        assert share <= 1.0
        first = got if first is None else first
        assert bits(got) == bits(first)


def test_backward_bits_over_runs_and_under_a_permutation_of_the_faces(hip_lib):
    case = CASES[0]
    cams = (case.R, case.T, case.focal, case.pp)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((len(case.R), case.H, case.W)).astype(np.float32))
    pix, first = device_grad(case.verts, case.faces, cams, (case.H, case.W), g, "brute")
    for _ in range(2):
        assert bits(device_grad(case.verts, case.faces, cams, (case.H, case.W), g, "brute")[1]) == bits(first)
    perm = torch.from_numpy(np.random.default_rng(4).permutation(len(case.faces)))
    for route in ROUTES:
        ppix, pgrad = device_grad(case.verts, case.faces[perm], cams, (case.H, case.W), g, route)
        back = torch.where(ppix >= 0, perm[ppix.long().clamp(min=0)], torch.full_like(ppix, -1).long())
        assert torch.equal(back, pix.long()) and bits(pgrad) == bits(first)
    assert float(first.abs().max()) > 0


def test_backward_of_one_triangle_under_every_pixel_and_of_an_empty_image(hip_lib):
    big = torch.tensor([[-9.0, -8.0, 2.0], [9.0, -8.0, 2.5], [0.0, 9.5, 3.0]])
    f = torch.tensor([[0, 1, 2]])
    cams = straight(40.0, 32.0)
    g = torch.from_numpy(np.random.default_rng(6).standard_normal((1, 64, 64)).astype(np.float32))
    vd = big.double().requires_grad_(True)
    p64, _, d64 = Aggregation.mesh_rasterize(vd, f, *(t.double() for t in cams), 64, 64)
    assert (p64 == 0).all()
    ref, = torch.autograd.grad((d64 * g.double()).sum(), vd)
    _, bound = rc.closed_form_grad(big, f, *cams, 64, 64, p64, g)
    for route in ROUTES:
        pix, got = device_grad(big, f, cams, (64, 64), g, route)
        assert (pix == 0).all() and ((got.double() - ref).abs() <= bound).all()
    away = big * torch.tensor([1.0, 1.0, -1.0])
    for route in ROUTES:
        pix, got = device_grad(away, f, cams, (64, 64), g, route)
        assert (pix == -1).all() and (got == 0).all()


# ---- state ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", [0x00, 0x7F, 0xFF], ids=D.pattern_id)
def test_dirty_workspaces_and_outputs(pattern, hip_lib):
    case = CASES[3]
    cams = (case.R, case.T, case.focal, case.pp)
    g = torch.from_numpy(np.random.default_rng(8).standard_normal((len(case.R), case.H, case.W)).astype(np.float32))

    def run(route):
        vd = case.verts.to(DEV).requires_grad_(True)
        frags = rasterize_mesh(vd, case.faces.to(DEV), mc.Cams(*(t.to(DEV) for t in cams)), (case.H, case.W), route=route)
        (frags.depth * g.to(DEV)).sum().backward()
        return [bits(t) for t in (frags.pix_to_face, frags.bary, frags.depth, vd.grad)]

    for route in ROUTES:
        clean = run(route)
        with D.dirty(pattern) as d:
            out = run(route)
            assert d.filled > 0 and len(d.taken) == 2 and max(t[0] for t in d.taken) <= D.GROW, d.taken      # one forward, one backward
        assert out == clean, (route, D.pattern_id(pattern))


def test_the_brute_route_is_captured_into_a_graph(hip_lib):
    case = CASES[0]
    cams = mc.Cams(*(t.to(DEV) for t in (case.R, case.T, case.focal, case.pp)))
    faces = case.faces.to(DEV)
    g = torch.from_numpy(np.random.default_rng(12).standard_normal((len(case.R), case.H, case.W)).astype(np.float32)).to(DEV)

    def step(vd):
        vd.grad = None
        frags = rasterize_mesh(vd, faces, cams, (case.H, case.W), route="brute")
        (frags.depth * g).sum().backward()
        return frags.pix_to_face, frags.bary, frags.depth.detach(), vd.grad

    vd = case.verts.to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(vd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    vd.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(vd)
    for seed in (1, 2):
        moved = case.verts + 0.02 * torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(case.verts.shape)).astype(np.float32))
        with torch.no_grad():
            vd.copy_(moved)
        graph.replay()
        torch.cuda.synchronize()
        got = [bits(t) for t in out]
        eager = step(moved.to(DEV).requires_grad_(True))
        assert got == [bits(t) for t in eager]
    assert ops.mesh_raster_route(len(case.R), case.H, case.W, len(case.faces)) == "brute"


def test_a_position_attribute_reproduces_the_hit_point(hip_lib):
    """interpolate_vertex_attr of the vertices' own positions is the point centre + depth * unit ray, within the depth bound (and
    the roundings of the three products and two sums that interpolate it)"""
    from oracle import camera_np
    case = CASES[1]
    frags = device_run(case.verts, case.faces, (case.R, case.T, case.focal, case.pp), (case.H, case.W), None)
    image = interpolate_vertex_attr(frags, case.faces.to(DEV), case.verts.to(DEV), background=float("nan")).cpu()
    rays, cen = camera_np.pixel_rays(case.R.numpy(), case.T.numpy(), case.focal.numpy(), case.pp.numpy(), (case.H, case.W))
    point = torch.from_numpy(cen.astype(np.float64))[:, None, None, :] + frags.depth.cpu().double()[..., None] * torch.from_numpy(rays.astype(np.float64))
    covered = frags.pix_to_face.cpu() >= 0
    assert torch.isnan(image[~covered]).all()
    p64, _, _, marks = fp64_reference(case.name)
    _, e_d = rc.forward_bounds(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, p64)
    ok = covered & ~marks & (frags.pix_to_face.cpu().long() == p64)
    # along the ray the depth bound; across it the weights' bound e_b on a point between corners at most an edge apart; the rays of
    # camera_np are fp32 unit vectors (2^-23 of the depth), the point's own roundings 8 u of the largest coordinate
    geo = rc.pixel_geometry(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, p64)
    edge = torch.stack([(geo[x] - geo[y]).norm(dim=-1) for x, y in ("ab", "bc", "ca")], -1).max(-1).values
    e_b, _ = rc.forward_bounds(case.verts, case.faces, case.R, case.T, case.focal, case.pp, case.H, case.W, p64)
    slack = e_d + 2 * e_b * edge + 2.0 ** -22 * frags.depth.cpu().double() + 8 * rc.U * float(case.verts.abs().max() + case.T.abs().max())
    err = (image.double() - point).norm(dim=-1)
    log_line(f"[mesh raster] hit point from a position attribute: {float((err / slack)[ok].max()):.4f} of its bound")
    assert (err[ok] <= slack[ok]).all()
