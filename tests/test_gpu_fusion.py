"""GPU tests of the two fusion kernels (voge_tsdf_integrate, voge_tsdf_integrate_attr) at shapes that tell the axes apart, and of the
attribute pass of the extraction (voge_mtet_attr) at every channel count.  tests/fusion_cases.py holds the scene -- nx, ny, nz =
19, 13, 11, three lo, three voxel sizes, 40 x 56 images, fx != fy, a camera inside the grid, one that looks away and a poisoned
depth map -- and derives the bounds; tests/test_fusion_cases_cpu.py shows without a GPU that the scene populates every branch.

definition    TSDFVolume.integrate on the device against Aggregation.tsdf_integrate in fp64 off the definition's own marks: equal
              weights, tsdf within fusion_cases.tsdf_bound, from an empty volume and from a prior state under a weight cap;
rules         every skip rule and every exact edge (u = 0, u = W, v = H, the last pixel, sdf = -trunc, sdf = trunc) on single grid
              points: the bits of the definition in fp32 on the host;
channels      every instantiation C = 1 .. 8 of both attribute kernels with a different image in every channel;
host routes   one camera for all depth maps, depth in other dtypes and layouts, a strided attr_image: the bits of the plain call;
capture       one integrate captured into a graph and replayed: nothing is read back."""
import numpy as np
import pytest
import torch

import fusion_cases as fc
import meshing_attr_cases as ac
import meshing_cases as mc
from util import log_line
from voge_amd import Aggregation
from voge_amd.Meshing import extract_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def same(a, b):
    """Bit for bit, NaNs included"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_volume(a, b):
    return same(a.tsdf, b.tsdf) and same(a.weight, b.weight) and (a.attr is None or same(a.attr, b.attr))


def fuse(channels=0, with_prior=False, views=slice(None), depth=None, cameras=None, image=None, vol=None):
    """The scene (or some of its views) into a volume on the device"""
    s = fc.scene()
    vol = fc.volume(DEV, channels, fc.prior() if with_prior else None) if vol is None else vol
    depth = s.depth[views] if depth is None else depth
    cameras = fc.cams(s, DEV, views) if cameras is None else cameras
    if channels and image is None:
        image = fc.images()[views][..., :channels]
    return vol.integrate(depth.to(DEV), cameras, fc.TRUNC, max_weight=fc.MAX_WEIGHT if with_prior else None,
                         attr=None if image is None else image.to(DEV))


@pytest.fixture(scope="module")
def plain():
    """The plain kernel's volumes {with_prior: vol}, fused once and left unchanged"""
    return {p: fuse(0, p) for p in (False, True)}


# ---- against the fp64 definition ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_prior", [False, True], ids=["empty volume", "prior state, max_weight 3"])
def test_fusion_against_the_fp64_definition(plain, with_prior):
    s = fc.scene()
    ref_t, ref_w, marked, _ = fc.reference(with_prior)
    vol = plain[with_prior]
    assert vol.tsdf.is_cuda and vol.tsdf.shape == fc.SHAPE
    share = float(marked.double().mean())
    assert share <= 0.02, share
    keep = ~marked
    assert int(((ref_w > 0) & keep).sum()) > 500      # the comparison is not empty
    if with_prior:
        assert int((ref_w < fc.prior()[1].double()).sum()) > 0      # the cap lowers a prior weight above it, here and there
    got_t, got_w = vol.tsdf.cpu().double(), vol.weight.cpu().double()
    mismatches = int((got_w[keep] != ref_w[keep]).sum())
    bound = fc.tsdf_bound(s)
    worst = float((got_t - ref_t)[keep].abs().max())
    log_line(f"[parity] tsdf_integrate 19x13x11, 5 views of 40x56, {'prior state, max_weight 3' if with_prior else 'empty volume'}: marked "
             f"{share * 100:.2f} %, weight mismatches {mismatches}, max |dtsdf| {worst:.3e}, bound {bound:.3e} ({worst / bound * 100:.1f} % of it); "
             f"weights up to {int(ref_w.max())}")
    assert torch.equal(got_w[keep], ref_w[keep])
    assert worst <= bound
    # five views in one call are five calls of one view each, and a second run has the same bits
    five = fc.volume(DEV, 0, fc.prior() if with_prior else None)
    for b in range(fc.B):
        fuse(0, with_prior, slice(b, b + 1), vol=five)
    assert same_volume(five, vol)
    assert same_volume(fuse(0, with_prior), vol)


# ---- the rules, point by point ---------------------------------------------------------------------------------------------------

def one_view(value=3.0, size=8):
    """tests/test_meshing_cpu.one_view: an 8 x 8 image of constant depth, f = 8, pp at the centre"""
    return torch.full((size, size), value), (size / 2, size / 2)


def both(point, depth, pp, trunc=0.5):
    """(tsdf, weight) of the point from the plain kernel, asserted equal bit for bit to the definition in fp32 on the host -- and the
    two-channel kernel's tsdf, weight and attr to the definition's with an image whose every pixel holds its own index: an updated
    point carries its pixel's two numbers, a skipped one zeros"""
    got = fc.integrate_point(point, *fc.axis_camera(depth, pp, device=DEV), trunc, DEV)
    want = fc.integrate_point(point, *fc.axis_camera(depth, pp), trunc)
    assert same(got[0], want[0]) and same(got[1], want[1]), (point, pp, got, want)
    H, W = depth.shape
    index = torch.arange(1.0, H * W + 1).reshape(1, H, W, 1)
    image = torch.cat([index, -0.25 * index], -1)
    got_a = fc.integrate_point(point, *fc.axis_camera(depth, pp, device=DEV), trunc, DEV, image)
    want_a = fc.integrate_point(point, *fc.axis_camera(depth, pp), trunc, image=image)
    assert all(same(g, w) for g, w in zip(got_a, want_a)) and same(got_a[0], got[0]) and same(got_a[1], got[1]), (point, pp, got_a, want_a)
    assert float(got_a[2][0]) == -4 * float(got_a[2][1]) and (float(got_a[2][0]) > 0) == (float(got[1]) > 0)
    return float(got[0]), float(got[1])


def test_a_view_is_skipped_where_the_rule_says():
    """The points and depths of tests/test_meshing_cpu.py::test_a_view_is_skipped_where_the_rule_says, through the kernel"""
    depth, pp = one_view()
    t, w = both((0.1, 0.1, 0.0), depth, pp)
    assert w == 1 and abs(t - (3.0 - np.linalg.norm([0.1, 0.1, 3.0])) / 0.5) < 1e-5      # updated: sdf / trunc
    assert both((0.1, 0.1, -1.0), depth, pp) == (1.0, 1.0)                                   # far in front: clamped to 1
    for name, p in {"behind the camera": (0.1, 0.1, -4.0), "on the camera's plane": (0.1, 0.1, -3.0), "outside the image": (2.5, 0.1, 0.0),
                    "sdf < -trunc": (0.1, 0.1, 0.6)}.items():
        assert both(p, depth, pp) == (0.0, 0.0), name
    for bad in (INF, -INF, NAN, 0.0, -1.0):      # an invalid depth
        assert both((0.1, 0.1, 0.0), *one_view(bad)) == (0.0, 0.0), bad
    # at those points sdf < -trunc skips a depth <= 0 as well.  Within trunc of the camera centre nothing else does: 0.25 in front of
    # it, sdf = d - 0.25 >= -trunc for d = 0 and d = -0.125, and only step 3 of the rule (d > 0) skips the view
    for bad in (0.0, -0.0, -0.125):
        assert both((0.0, 0.0, -2.75), *one_view(bad)) == (0.0, 0.0), bad
    assert both((0.0, 0.0, -2.75), *one_view(0.125)) == (-0.25, 1.0)      # (and a small positive depth there is a surface)
    # the pixel is the one the ray convention names: pixel (i, j) looks along ((px - j - 0.5) / fx, (py - i - 0.5) / fy, 1)
    depth[1, 6] = NAN      # i = 1, j = 6
    assert both((3.0 * (4 - 6.5) / 8, 3.0 * (4 - 1.5) / 8, 0.0), depth, pp) == (0.0, 0.0)
    assert both((3.0 * (4 - 5.5) / 8, 3.0 * (4 - 1.5) / 8, 0.0), depth, pp)[1] == 1
    assert both((3.0 * (4 - 1.5) / 8, 3.0 * (4 - 6.5) / 8, 0.0), depth, pp)[1] == 1      # (i, j) = (6, 1), the transpose: finite


def only(H, W, i, j, d=3.25):
    depth = torch.full((H, W), NAN)
    depth[i, j] = d
    return depth


def test_exact_edges():
    """The optical-axis point projects to the principal point with no rounding anywhere: the same decision in every precision"""
    O = (0.0, 0.0, 0.0)
    assert both(O, only(8, 8, 0, 0), (0.0, 0.0)) == (0.5, 1.0)                       # u = v = 0: inside, and it is pixel (0, 0)
    assert both(O, torch.full((8, 8), 3.25), (8.0, 0.0)) == (0.0, 0.0)               # u = W: outside
    assert both(O, torch.full((8, 8), 3.25), (0.0, 8.0)) == (0.0, 0.0)               # v = H: outside
    assert both(O, torch.full((5, 8), 3.25), (8.0, 2.0)) == (0.0, 0.0)               # u = W of a 5 x 8 image
    assert both(O, torch.full((5, 8), 3.25), (2.0, 5.0)) == (0.0, 0.0)               # v = H of it: 5, and u = 5 < W is inside
    assert both(O, torch.full((5, 8), 3.25), (5.0, 2.0)) == (0.5, 1.0)
    assert both(O, only(5, 8, 4, 7), (7.5, 4.5)) == (0.5, 1.0)                       # pixel (H - 1, W - 1) of a 5 x 8 image
    but = torch.full((5, 8), 3.25)
    but[4, 7] = NAN
    assert both(O, but, (7.5, 4.5)) == (0.0, 0.0)                                    # (and no other pixel)
    assert both(O, only(5, 8, 3, 1), (1.5, 3.5)) == (0.5, 1.0)                       # a row index times W, not H
    assert both(O, torch.full((1, 1), 3.25), (0.5, 0.5)) == (0.5, 1.0)               # a 1 x 1 image
    assert both((0.0, 0.0, 0.5), torch.full((8, 8), 3.0), (4.0, 4.0)) == (-1.0, 1.0)      # sdf == -trunc exactly: updated, t = -1
    assert both((0.0, 0.0, 0.5 + 2.0 ** -20), torch.full((8, 8), 3.0), (4.0, 4.0)) == (0.0, 0.0)      # one step behind the band: cut
    assert both((0.0, 0.0, -0.5), torch.full((8, 8), 3.0), (4.0, 4.0)) == (1.0, 1.0)      # sdf / trunc == 1 exactly
    assert both((0.0, 0.0, -0.25), torch.full((8, 8), 3.0), (4.0, 4.0)) == (0.5, 1.0)


# ---- every channel count ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_channel():
    """attr [nz,ny,nx] of the one-channel kernel on channel c of the images and of the prior state, c = 0 .. 7"""
    out = []
    for c in range(8):
        prior = fc.prior()[:2] + (fc.prior()[2][..., c:c + 1],)
        vol = fc.volume(DEV, 1, prior)
        out.append(fuse(1, True, image=fc.images()[..., c:c + 1], vol=vol).attr[..., 0].clone())
    return out


@pytest.mark.parametrize("C", range(1, 9))
def test_every_channel_count_of_the_fusion(plain, one_channel, C):
    ref_t, ref_w, marked, ref_a = fc.reference(True)
    prior_w, prior_a = fc.prior()[1], fc.prior()[2][..., :C]
    image = fc.images()[..., :C]
    vol = fuse(C, True)
    assert vol.attr.shape == fc.SHAPE + (C,) and vol.attr.is_cuda
    keep = ~marked
    bound = fc.attr_bound(image, prior_a)
    worst = float((vol.attr.cpu().double() - ref_a[..., :C])[keep].abs().max())
    log_line(f"[parity] tsdf_integrate attr 19x13x11, 5 views of 40x56, prior state, C = {C}: max |dattr| {worst:.3e}, bound {bound:.3e} "
             f"({worst / bound * 100:.1f} % of it)")
    assert float(marked.double().mean()) <= 0.02 and worst <= bound
    # the geometry of the plain kernel, and every channel the one-channel kernel's: no channel reads another's image or prior
    assert same(vol.tsdf, plain[True].tsdf) and same(vol.weight, plain[True].weight)
    for c in range(C):
        assert same(vol.attr[..., c], one_channel[c]), c
    assert C == 1 or not same(vol.attr[..., 0], vol.attr[..., C - 1])
    # no view updates the point (the decisions do not depend on the state: weight 0 from an empty volume): the prior, bit for bit
    untouched = ((fc.reference(False)[1] == 0) & keep).to(DEV)
    assert int(untouched.sum()) > 500 and int((~untouched).sum()) > 500 and torch.equal(ref_w[untouched.cpu()], prior_w.double()[untouched.cpu()])
    assert same(vol.attr[untouched], prior_a.to(DEV)[untouched])


CASE = next(c for c in ac.extraction_cases() if c[0] == "random 17x9x33")


@pytest.fixture(scope="module")
def vertex_reference():
    """(field [33,9,17,8], the fp64 definition's (verts, faces, vert_attr [V,8]), the one-channel extractions' columns)"""
    label, values, weight, level, lo, h = CASE
    lo, h = fc.F32(lo), fc.F32(h)
    field = ac.noise_field(values.shape, 8, seed=3)
    ref = Aggregation.marching_tets(values.double(), weight, level, lo, h, attr=field.double())
    columns = [extract_mesh(values.to(DEV), None, level, lo, h, attr=field[..., c:c + 1].contiguous().to(DEV))[2][:, 0] for c in range(8)]
    return field, ref, columns


@pytest.mark.parametrize("C", range(1, 9))
def test_every_channel_count_of_the_vertex_attributes(vertex_reference, C):
    label, values, weight, level, lo, h = CASE
    lo, h = fc.F32(lo), fc.F32(h)
    assert len(set(values.shape)) == 3 and len(set(h)) == 3      # a non-cubic grid
    field, (ref_v, ref_f, ref_a), columns = vertex_reference
    attr = field[..., :C].contiguous()
    verts, faces, vert_attr = extract_mesh(values.to(DEV), None, level, lo, h, attr=attr.to(DEV))
    assert torch.equal(faces.cpu(), ref_f.to(torch.int32)) and vert_attr.shape == (len(ref_v), C) and len(ref_v) > 1000
    bound = ac.vert_attr_bound(float(attr.abs().max()))
    worst = float((vert_attr.cpu().double() - ref_a[:, :C]).abs().max())
    log_line(f"[parity] marching_tets attr {label}, C = {C}: V {len(ref_v)}, max |dattr| {worst:.3e}, bound {bound:.3e} "
             f"({worst / bound * 100:.1f} % of it)")
    assert worst <= bound
    for c in range(C):
        assert same(vert_attr[:, c], columns[c]), c


# ---- host routes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("focal", [64.0, (70.0, 55.0)], ids=["scalar focal", "focal [2]"])
def test_one_camera_for_all_depth_maps(focal):
    """R [1,3,3], T [1,3], a scalar or [2] focal length and a [2] principal point beside five depth maps: view 0's camera five times"""
    s = fc.scene()
    f2 = torch.tensor([focal, focal] if isinstance(focal, float) else focal)
    shared = mc.Cams(s.R[:1].to(DEV), s.T[:1].to(DEV), torch.tensor(focal).to(DEV), s.pp[0].to(DEV))
    copies = mc.Cams(s.R[:1].repeat(fc.B, 1, 1).to(DEV), s.T[:1].repeat(fc.B, 1).to(DEV), f2.repeat(fc.B, 1).to(DEV), s.pp[:1].repeat(fc.B, 1).to(DEV))
    for C in (0, 3):
        got, want = fuse(C, True, cameras=shared), fuse(C, True, cameras=copies)
        assert same_volume(got, want)
        assert int((want.tsdf != fc.prior()[0].to(DEV)).sum()) > 200      # (the views do something)


def test_depth_and_attributes_in_other_dtypes_and_layouts(plain):
    s = fc.scene()
    want = plain[True]
    assert same_volume(fuse(0, True, depth=s.depth.double()), want)
    half = s.depth.half()      # (the poison survives: NaN, +-inf, 0 and -1.5 are fp16 numbers)
    assert torch.isnan(half).any() and (half == -1.5).any() and not torch.equal(half.float(), s.depth)
    assert same_volume(fuse(0, True, depth=half), fuse(0, True, depth=half.float()))
    strided = s.depth.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)      # [B,H,W] over the memory of a [B,W,H] tensor
    assert strided.shape == s.depth.shape and not strided.is_contiguous()
    assert same_volume(fuse(0, True, depth=strided), want)
    image = fc.images()[..., :3]
    want = fuse(3, True)
    channel_first = image.permute(0, 3, 1, 2).contiguous().to(DEV).permute(0, 2, 3, 1)      # [B,H,W,C] over [B,C,H,W]
    assert channel_first.shape == image.shape and not channel_first.is_contiguous()
    assert same_volume(fuse(3, True, depth=strided, image=channel_first), want)
    assert same_volume(fuse(3, True, image=image.double()), want)


# ---- capture ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [0, 3], ids=["plain", "C = 3"])
def test_graph_capture_and_replay(C):
    """integrate reads nothing back: one call captured into a graph, replayed twice on the volume it was captured on, then once more
    after the depth was overwritten in place with the poisoned maps -- the bits of the eager calls each time."""
    s = fc.scene()
    cameras = fc.cams(s, DEV)
    depth = s.depth_clean.to(DEV)      # (static: the graph reads this memory)
    image = fc.images()[..., :C].to(DEV) if C else None
    vol = fc.volume(DEV, C, fc.prior())

    def reset(v):
        v.tsdf.copy_(fc.prior()[0])
        v.weight.copy_(fc.prior()[1])
        if C:
            v.attr.copy_(fc.prior()[2][..., :C])

    def step(v, d):
        v.integrate(d, cameras, fc.TRUNC, max_weight=fc.MAX_WEIGHT, attr=image)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(vol, depth)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    reset(vol)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(vol, depth)
    torch.cuda.synchronize()
    assert same(vol.tsdf, fc.prior()[0].to(DEV)) and same(vol.weight, fc.prior()[1].to(DEV))      # captured, not run
    eager = fc.volume(DEV, C, fc.prior())
    for _ in range(2):
        graph.replay()
        step(eager, depth.clone())
        torch.cuda.synchronize()
        assert same_volume(vol, eager)
    assert int((vol.tsdf != fc.prior()[0].to(DEV)).sum()) > 300
    depth.copy_(s.depth)      # view 4's poisoned map, in place
    graph.replay()
    step(eager, s.depth.to(DEV))
    torch.cuda.synchronize()
    assert same_volume(vol, eager)
    # and the poison mattered: the clean maps give another volume
    clean = fc.volume(DEV, C, fc.prior())
    for _ in range(3):
        step(clean, s.depth_clean.to(DEV))
    assert not same(clean.tsdf, vol.tsdf)
