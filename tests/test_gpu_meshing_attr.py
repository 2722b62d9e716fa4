"""GPU tests of attributes through the mesh extraction (voge_tsdf_integrate_attr, voge_mtet_attr; an extension, the reference and
the oracle have none) and of VoGE.Meshing with channels / attr= on the device.

fusion       against the definition in fp64 on the grid points it does not mark itself (test_gpu_meshing's marks): equal weights and
             attr within meshing_attr_cases.fuse_bound = 3 B eps max |attr_image|, derived in that module's header; tsdf and weight with
             the bits of the plain call; three calls are one call; C = 9 takes the definition on the device;
extraction   verts and faces with the bits of the call without attr; vert_attr within meshing_attr_cases.vert_attr_bound = 6 * 2^-23
             max |attr| of the fp64 definition; a position attribute ties the rows to the numbering of the vertices;
end to end   the property of tests/test_meshing_attr_cpu.py: with every pixel's hit point as its attribute, |vert_attr - vert| <= 1.0 h.
The grids are small on purpose."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import meshing_attr_cases as ac
import meshing_cases as mc
from util import log_line
from voge_amd import Aggregation, ops
from voge_amd.Meshing import clean_mesh, extract_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = lambda xs: tuple(float(np.float32(x)) for x in xs)
TRUNC = 2 * mc.GRID_H


def fuse(image, views=None, **kw):
    depth, R, T, focal, pp = mc.three_views() if views is None else views
    vol = ac.volume(DEV, channels=image.shape[-1])
    return vol.integrate(depth.to(DEV), ac.cams(R, T, focal, pp, DEV), TRUNC, attr=image.to(DEV), **kw)


# ---- fusion -------------------------------------------------------------------------------------------------------------------

def check_fusion(label, vol, reference, channels=slice(None)):
    image, ref_t, ref_w, marked, ref_a = reference
    share = float(marked.double().mean())
    assert share <= 0.02, share
    keep = ~marked
    got_w, got_a = vol.weight.cpu().double(), vol.attr.cpu().double()[..., channels]
    assert int((ref_w[keep] > 0).sum()) > 1000      # the comparison is not empty
    assert torch.equal(got_w[keep], ref_w[keep])
    bound = ac.fuse_bound(3, float(image.abs().max()))
    worst = float((got_a - ref_a)[keep].abs().max())
    log_line(f"[parity] tsdf_integrate attr {label}: marked {share * 100:.2f} %, max |dattr| {worst:.3e}, bound {bound:.3e} "
             f"({worst / bound * 100:.1f} % of it); weights up to {int(ref_w.max())}")
    assert worst <= bound
    assert (got_a[(ref_w == 0) & keep] == 0).all()


def test_fusion_against_the_fp64_definition():
    reference = ac.three_view_reference()
    vol = fuse(reference[0])
    assert vol.attr.is_cuda and vol.attr.dtype == torch.float32 and vol.attr.shape == (mc.GRID_N,) * 3 + (3,)
    assert int(reference[2].max()) == 3
    check_fusion("24^3 x 3 views, C = 3", vol, reference)
    # the new kernel changes no geometry: tsdf and weight with the bits of the plain call
    depth, R, T, focal, pp = mc.three_views()
    plain = ac.volume(DEV, channels=0).integrate(depth.to(DEV), ac.cams(R, T, focal, pp, DEV), TRUNC)
    assert torch.equal(vol.tsdf, plain.tsdf) and torch.equal(vol.weight, plain.weight)
    # one call with three views is three calls with one view each, bit for bit
    three = ac.volume(DEV, channels=3)
    for b in range(3):
        three.integrate(depth[b:b + 1].to(DEV), ac.cams(R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1], DEV), TRUNC,
                        attr=reference[0][b:b + 1].to(DEV))
    assert torch.equal(three.tsdf, vol.tsdf) and torch.equal(three.weight, vol.weight) and torch.equal(three.attr, vol.attr)
    # and the same bits on a second run
    assert torch.equal(fuse(reference[0]).attr, vol.attr)


def test_fusion_under_a_weight_cap():
    reference = ac.three_view_reference(max_weight=2)
    assert int(reference[2].max()) == 2
    vol = fuse(reference[0], max_weight=2)
    check_fusion("24^3 x 3 views, C = 3, max_weight 2", vol, reference)
    depth, R, T, focal, pp = mc.three_views()
    plain = ac.volume(DEV, channels=0).integrate(depth.to(DEV), ac.cams(R, T, focal, pp, DEV), TRUNC, max_weight=2)
    assert torch.equal(vol.tsdf, plain.tsdf) and torch.equal(vol.weight, plain.weight)


@pytest.mark.parametrize("C", [1, 4, 8])
def test_every_channel_count_gives_the_same_bits(C):
    """The same image in every channel: every channel of every instantiation carries the bits of the one-channel kernel"""
    one = fuse(ac.same_in_every_channel(1))
    vol = fuse(ac.same_in_every_channel(C))
    assert vol.attr.shape[-1] == C and float(one.attr.abs().max()) > 0.5
    for c in range(C):
        assert torch.equal(vol.attr[..., c], one.attr[..., 0]), c
    assert torch.equal(vol.tsdf, one.tsdf) and torch.equal(vol.weight, one.weight)


def test_nine_channels_take_the_definition_on_the_device():
    assert ops.MTET_MAX_CHANNELS == 8
    reference = ac.three_view_reference()
    image = torch.cat([reference[0]] * 3, -1)      # [3,96,96,9]
    vol = fuse(image)
    assert vol.attr.is_cuda and vol.attr.shape[-1] == 9 and vol.attr.dtype == torch.float32
    for k in range(3):
        check_fusion(f"24^3 x 3 views, C = 9 (the definition on the device), channels {3 * k} .. {3 * k + 2}", vol, reference,
                     slice(3 * k, 3 * k + 3))
    # the mesh of such a volume carries all nine: the extraction takes eight channels a launch
    verts, faces, vert_attr = extract_mesh(vol, attr=True)
    assert vert_attr.shape == (len(verts), 9) and torch.equal(vert_attr[:, :3], vert_attr[:, 6:])
    assert torch.equal(vert_attr[:, :3], extract_mesh(vol.tsdf, vol.weight, 0.0, vol.lo, vol.voxel_size, attr=vol.attr[..., :3].contiguous())[2])


# ---- extraction ---------------------------------------------------------------------------------------------------------------

CASES = ac.extraction_cases()


def extract(values, weight, level, lo, h, attr):
    return extract_mesh(values.to(DEV), None if weight is None else weight.to(DEV), level, lo, h, attr=attr.to(DEV))


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_vertex_attributes_against_the_fp64_definition(case, C):
    label, values, weight, level, lo, h = CASES[case]
    lo, h = F32(lo), F32(h)
    attr = ac.noise_field(values.shape, C, seed=case)
    ref_v, ref_f, ref_a = Aggregation.marching_tets(values.double(), weight, level, lo, h, attr=attr.double())
    verts, faces, vert_attr = extract(values, weight, level, lo, h, attr)
    plain_v, plain_f = extract_mesh(values.to(DEV), None if weight is None else weight.to(DEV), level, lo, h)
    assert torch.equal(verts, plain_v) and torch.equal(faces, plain_f) and torch.equal(faces.cpu(), ref_f.to(torch.int32))
    assert vert_attr.is_cuda and vert_attr.dtype == torch.float32 and vert_attr.shape == (len(ref_v), C) and len(ref_v) > 0
    bound = ac.vert_attr_bound(float(attr.abs().max()))
    worst = float((vert_attr.cpu().double() - ref_a).abs().max())
    log_line(f"[parity] marching_tets attr {label}, C = {C}: V {len(ref_v)}, max |dattr| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_a_position_attribute_lands_on_its_vertex(case):
    """A wrong offset or a wrong popcount puts a colour on another vertex: here that is a distance of a grid step or more"""
    label, values, weight, level, lo, h = CASES[case]
    lo, h = F32(lo), F32(h)
    pos = ac.position_field(values.shape, lo, h)
    verts, faces, vert_attr = extract(values, weight, level, lo, h, pos)
    bound = ac.vert_attr_bound(float(pos.abs().max())) + mc.vert_bound(values.shape, lo, h)
    worst = float((vert_attr.double() - verts.double()).abs().max())
    log_line(f"[parity] marching_tets attr = position, {label}: V {len(verts)}, max |vert_attr - vert| {worst:.3e}, bound {bound:.3e}")
    assert len(verts) > 0 and worst <= bound and bound < 0.01 * min(h)


def test_empty_meshes_have_empty_attributes():
    for C in (1, 3, 8):
        for fill in (-1.0, 1.0):
            out = extract_mesh(torch.full((5, 6, 7), fill, device=DEV), attr=torch.ones((5, 6, 7, C), device=DEV))
            assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0, C)
            assert out[2].is_cuda and out[2].dtype == torch.float32
        out = extract_mesh(torch.full((5, 6, 7), -1.0, device=DEV), torch.zeros((5, 6, 7), device=DEV), attr=torch.ones((5, 6, 7, C), device=DEV))
        assert out[0].shape == (0, 3) and out[2].shape == (0, C)      # nothing observed


def test_rows_beyond_the_first_scan_round():
    """The 65^3 gyroid of test_top_level_scan_runs_more_than_once with the x coordinate as the attribute: the vertices of the scan
    blocks beyond the first round of the top level carry their own x."""
    n = 65
    x, y, z = (a * (2 * np.pi / 13.7) for a in mc.grid_xyz((n, n, n)))
    g = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x) + 0.05
    values = torch.from_numpy(g.astype(np.float32)).to(DEV)
    unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    attr = ac.position_field((n, n, n))[..., :1].contiguous().to(DEV)
    verts, faces, edge_mask, face_count, vert_attr = ops.marching_tets(values, None, 0.0, *unit, return_tables=True, attr=attr)
    plain = ops.marching_tets(values, None, 0.0, *unit)
    assert torch.equal(verts, plain[0]) and torch.equal(faces, plain[1]) and vert_attr.shape == (len(verts), 1)
    last = ops.MTET_TOP * ops.MTET_BLOCK
    first_row = sum(int(((edge_mask[:last] >> k) & 1).sum()) for k in range(7))      # the vertices of the first round's blocks
    assert 0 < first_row < len(verts) - 1000
    bound = ac.vert_attr_bound(n - 1.0) + mc.vert_bound((n, n, n), *unit)
    worst = float((vert_attr[first_row:, 0].double() - verts[first_row:, 0].double()).abs().max())
    log_line(f"[parity] marching_tets attr = x, gyroid 65^3: V {len(verts)}, {len(verts) - first_row} rows beyond the first round, "
             f"max |vert_attr - x| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert float((vert_attr[:first_row, 0].double() - verts[:first_row, 0].double()).abs().max()) <= bound


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_hit_points_end_to_end_on_the_device():
    views = mc.sphere_views()
    vol = fuse(ac.hit_point_images(), views)
    verts, faces, vert_attr = extract_mesh(vol, attr=True)
    mc.assert_closed(verts, faces, chi=2)
    err = (vert_attr.double() - verts.double()).norm(dim=-1) / mc.GRID_H
    log_line(f"[parity] meshing attr end to end: V {len(verts)}, F {len(faces)}, |vert_attr - vert| max {float(err.max()):.3f} h, "
             f"mean {float(err.mean()):.3f} h")
    assert len(verts) > 2000 and float(err.max()) <= ac.HIT_CAP
    # the attribute follows clean_mesh through vert_index
    clean_v, clean_f, vert_index, face_index = clean_mesh(verts, faces, keep_largest=1, return_index=True)
    followed = vert_attr[vert_index.long()]
    assert followed.shape == clean_v.shape and len(clean_v) > 2000
    assert float((followed.double() - clean_v.double()).norm(dim=-1).max()) <= ac.HIT_CAP * mc.GRID_H


def test_demo_path_with_colour():
    """demo/ExtractMesh.py --colour at 64^3 with 8 views of 64^2: colours at the vertices, in the range of the input, and the report
    of the round trip (the mesh back as oriented Gaussians, rendered from the first camera)."""
    spec = importlib.util.spec_from_file_location("extract_mesh_demo", os.path.join(ROOT, "demo", "ExtractMesh.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    verts, faces, report = demo.run(resolution=64, views=8, image=64, out=None, colour=True)
    log_line(f"[parity] demo/ExtractMesh.py --colour 64^3, 8 views of 64^2: {report}")
    vert_attr = demo.LAST["vert_attr"]
    assert len(verts) > 100 and vert_attr.shape == (len(verts), 3) and torch.isfinite(vert_attr).all()
    lo, hi = demo.LAST["colour_range"]
    assert float(vert_attr.min()) >= lo - 1e-5 and float(vert_attr.max()) <= hi + 1e-5
    assert "round trip" in report and np.isfinite(demo.LAST["round_trip"])
    log_line(f"[parity] demo/ExtractMesh.py --colour: round-trip mean |dimage| {demo.LAST['round_trip']:.4f}")
