"""CPU tests of attributes through the mesh extraction: the attr= rules of the definitions (Aggregation.tsdf_integrate, step 6, and
Aggregation.marching_tets), VoGE.Meshing with channels / attr= on host tensors -- which takes the definitions -- and the argument
checks of voge_tsdf_integrate_attr and voge_mtet_attr.  No GPU.  meshing_attr_cases has the images, the fields and the bounds."""
import numpy as np
import pytest
import torch

import meshing_attr_cases as ac
import meshing_cases as mc
from voge_amd import Aggregation
from voge_amd.Meshing import TSDFVolume, extract_mesh

TRUNC = 2 * mc.GRID_H


def fused(depth, R, T, focal, pp, image=None, channels=0, **kw):
    vol = ac.volume(channels=channels)
    return vol.integrate(depth, ac.cams(R, T, focal, pp), TRUNC, **({} if image is None else {"attr": image}), **kw)


def test_calls_without_an_attribute_are_unchanged():
    depth, R, T, focal, pp = mc.three_views()
    plain = mc.Cams(R, T, focal, pp)
    a = TSDFVolume([mc.GRID_LO] * 3, voxel_size=mc.GRID_H, resolution=mc.GRID_N).integrate(depth, plain, TRUNC)
    b = ac.volume(channels=0).integrate(depth, plain, TRUNC, attr=None)
    assert a.attr is None and b.attr is None and a.channels == 0
    assert torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight)
    # the geometry of a volume with channels is the geometry of one without
    c = fused(depth, R, T, focal, pp, ac.noise_images(3, 3), channels=3)
    assert torch.equal(a.tsdf, c.tsdf) and torch.equal(a.weight, c.weight)
    for x, y in zip(extract_mesh(a), extract_mesh(a, attr=None)):
        assert torch.equal(x, y)
    got = extract_mesh(c, attr=True)
    assert len(got) == 3 and all(torch.equal(x, y) for x, y in zip(extract_mesh(a), got))
    values = mc.random_field()
    for x, y in zip(extract_mesh(values, None, 0.25, (1.0, 2.0, 3.0), 0.5), extract_mesh(values, None, 0.25, (1.0, 2.0, 3.0), 0.5, attr=None)):
        assert torch.equal(x, y)
    # the definitions: the keyword left out, the keyword None, and the first results with it
    centre = Aggregation.camera_centres(R.double(), T.double()).to(torch.float32)
    z = torch.zeros((mc.GRID_N,) * 3)
    args = (z, z.clone(), depth, R, T, focal, pp, [mc.GRID_LO] * 3, mc.GRID_H, TRUNC)
    old = Aggregation.tsdf_integrate(*args, centre=centre)
    new = Aggregation.tsdf_integrate(*args, centre=centre, attr=None, attr_image=None)
    with_attr = Aggregation.tsdf_integrate(*args, centre=centre, attr=torch.zeros(z.shape + (2,)), attr_image=ac.noise_images(3, 2))
    assert len(old) == 2 and len(new) == 2 and len(with_attr) == 3
    assert all(torch.equal(x, y) for x, y in zip(old, new)) and all(torch.equal(x, y) for x, y in zip(old, with_attr))
    marked = Aggregation.tsdf_integrate(*args, centre=centre, mark=ac.MARK, attr=torch.zeros(z.shape + (2,)), attr_image=ac.noise_images(3, 2))
    assert len(marked) == 4 and marked[2].dtype == torch.bool and torch.equal(marked[3], with_attr[2])
    old = Aggregation.marching_tets(values)
    new = Aggregation.marching_tets(values, attr=None)
    with_attr = Aggregation.marching_tets(values, attr=ac.noise_field(values.shape, 2))
    assert len(old) == 2 and len(new) == 2 and len(with_attr) == 3 and with_attr[2].shape == (len(old[0]), 2)
    assert all(torch.equal(x, y) for x, y in zip(old, new)) and all(torch.equal(x, y) for x, y in zip(old, with_attr))


def test_every_misuse_raises():
    depth, R, T, focal, pp = mc.three_views()
    cams = mc.Cams(R, T, focal, pp)
    image = ac.noise_images(3, 3)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            ac.volume(channels=bad)
    with pytest.raises(ValueError):      # a missing attr
        ac.volume(channels=3).integrate(depth, cams, TRUNC)
    with pytest.raises(ValueError):      # an unexpected one
        ac.volume(channels=0).integrate(depth, cams, TRUNC, attr=image)
    with pytest.raises(ValueError):      # a wrong C
        ac.volume(channels=4).integrate(depth, cams, TRUNC, attr=image)
    for wrong in (image[:2], image[:, :95], image[:, :, :95], image[..., 0], image.permute(0, 3, 1, 2)):      # a wrong B, H, W, rank, layout
        with pytest.raises(ValueError):
            ac.volume(channels=3).integrate(depth, cams, TRUNC, attr=wrong)
    for no_tensor in (image.numpy(), image.tolist(), True):
        with pytest.raises(ValueError):
            ac.volume(channels=3).integrate(depth, cams, TRUNC, attr=no_tensor)
    vol = ac.volume(channels=3)
    assert vol.integrate(depth, cams, TRUNC, attr=image) is vol and vol.attr.shape == (mc.GRID_N,) * 3 + (3,) and vol.attr.dtype == torch.float32
    with pytest.raises(ValueError):      # attr=True without channels
        extract_mesh(ac.volume(channels=0), attr=True)
    values = mc.random_field()
    with pytest.raises(ValueError):      # attr=True without a volume
        extract_mesh(values, attr=True)
    for wrong in (ac.noise_field((9, 8, 6), 3), ac.noise_field(values.shape, 3)[..., 0], ac.noise_field(values.shape, 3).numpy()):
        with pytest.raises(ValueError):
            extract_mesh(values, attr=wrong)
    z = torch.zeros((mc.GRID_N,) * 3)
    args = (z, z.clone(), depth, R, T, focal, pp, [mc.GRID_LO] * 3, mc.GRID_H, TRUNC)
    with pytest.raises(ValueError):      # one of the pair
        Aggregation.tsdf_integrate(*args, attr=torch.zeros(z.shape + (3,)))
    with pytest.raises(ValueError):
        Aggregation.tsdf_integrate(*args, attr=torch.zeros(z.shape + (2,)), attr_image=image)
    with pytest.raises(ValueError):
        Aggregation.marching_tets(values, attr=ac.noise_field((9, 8, 6), 3))
    # .to() moves the attribute with the rest
    assert vol.to("cpu").attr.device.type == "cpu" and ac.volume(channels=0).to("cpu").attr is None


def test_new_attr_entries_validate_before_any_hip_call():
    import os
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    P = 1234     # (a non-NULL pointer value: nothing is dereferenced before validation is through)
    grid = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    cams = (P, P, P, P, P)
    fuse = lambda tsdf=P, weight=P, attr=P, C=3, dims=(8, 8, 8), g=grid, depth=P, image=P, B=1, H=4, W=4, c=cams, trunc=0.1, mw=0.0: \
        lib.voge_tsdf_integrate_attr(tsdf, weight, attr, C, *dims, *g, depth, image, B, H, W, *c, trunc, mw, None)
    assert fuse(tsdf=None) == -1 and fuse(weight=None) == -1 and fuse(attr=None) == -1
    assert fuse(depth=None) == -1 and fuse(image=None) == -1 and fuse(c=(P, P, None, P, P)) == -1
    assert fuse(C=0) == -1 and fuse(C=9) == -1 and fuse(C=-3) == -1
    assert fuse(dims=(8, 1, 8)) == -1 and fuse(H=0) == -1 and fuse(B=-1) == -1
    assert fuse(trunc=0.0) == -1 and fuse(trunc=float("nan")) == -1 and fuse(mw=float("nan")) == -1
    assert fuse(g=(0.0, 0.0, 0.0, 1.0, 0.0, 1.0)) == -1 and fuse(g=(0.0, float("inf"), 0.0, 1.0, 1.0, 1.0)) == -1
    assert fuse(dims=(700, 700, 700)) == -3 and fuse(dims=(65536, 65536, 2)) == -3      # the 32-bit limit
    assert fuse(depth=None, image=None, B=0, c=(None,) * 5) == 0      # no view: nothing launched
    assert fuse(attr=None, B=0) == -1
    tabs = (P, P, P)
    carry = lambda values=P, dims=(8, 8, 8), level=0.0, attr=P, C=3, t=tabs, V=10, out=P: \
        lib.voge_mtet_attr(values, *dims, level, attr, C, *t, V, out, None)
    assert carry(values=None) == -1 and carry(attr=None) == -1 and carry(out=None) == -1
    assert carry(t=(None, P, P)) == -1 and carry(t=(P, None, P)) == -1 and carry(t=(P, P, None)) == -1
    assert carry(C=0) == -1 and carry(C=9) == -1
    assert carry(dims=(8, 8, 1)) == -1 and carry(level=float("nan")) == -1 and carry(V=-1) == -1
    assert carry(dims=(675, 675, 675)) == -3 and carry(V=1 << 31) == -3
    assert carry(V=0, out=None) == 0      # an empty mesh: nothing launched


def test_device_routes_refuse_host_attributes():
    from voge_amd import _lib, ops
    values = mc.random_field()
    with pytest.raises(_lib.VogeHipError):
        ops.marching_tets(values, None, 0.0, (0.0,) * 3, (1.0,) * 3, attr=ac.noise_field(values.shape, 3))


@pytest.mark.parametrize("max_weight", [None, 2])
def test_a_constant_image_is_fused_exactly(max_weight):
    """0.5 w + 0.5 and its quotient by w + 1 are exact, so a lost or a doubled update shows up"""
    depth, R, T, focal, pp = mc.three_views()
    vol = fused(depth, R, T, focal, pp, torch.full((3, mc.IMAGE, mc.IMAGE, 2), 0.5), channels=2, max_weight=max_weight)
    seen = vol.weight > 0
    assert int(seen.sum()) > 1000 and int(vol.weight.max()) == (3 if max_weight is None else 2)
    assert (vol.attr[seen] == 0.5).all() and (vol.attr[~seen] == 0).all()


def test_three_calls_are_one_call():
    depth, R, T, focal, pp = mc.three_views()
    image = ac.noise_images(3, 3)
    one = fused(depth, R, T, focal, pp, image, channels=3)
    three = ac.volume(channels=3)
    for b in range(3):
        three.integrate(depth[b:b + 1], ac.cams(R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1]), TRUNC, attr=image[b:b + 1])
    assert torch.equal(one.tsdf, three.tsdf) and torch.equal(one.weight, three.weight) and torch.equal(one.attr, three.attr)
    assert float(one.attr.abs().max()) > 0.5 and float(one.attr.abs().max()) <= 1.0


def test_the_rule_on_one_grid_point():
    """Step 6 by hand at every grid point all three views update: three pixels, in the views' order"""
    depth, R, T, focal, pp = mc.three_views()
    image = ac.noise_images(3, 3).double()
    tsdf, weight, attr = ac.definition_fp64(depth, R, T, focal, pp, TRUNC, image)
    per_view = [ac.definition_fp64(depth[b:b + 1], R[b:b + 1], T[b:b + 1], focal[b:b + 1], pp[b:b + 1], TRUNC, image[b:b + 1]) for b in range(3)]
    q = weight == 3
    assert int(q.sum()) > 10
    a, w = torch.zeros((int(q.sum()), 3), dtype=torch.float64), 0.0
    for b in range(3):
        assert (per_view[b][1][q] == 1).all()
        pixel = per_view[b][2][q]      # a single view from an empty volume leaves the pixel itself: (0 * 0 + p) / 1
        assert all(bool((image[b] == p).all(-1).any()) for p in pixel[:5])
        a, w = (a * w + pixel) / (w + 1), w + 1
    assert torch.equal(attr[q], a)


def test_vertex_attributes_follow_the_definition_of_t():
    """A linear attribute of the position is reproduced at the vertices, and the rows follow the vertices' order"""
    values = mc.random_field()
    lo, h = (-1.5, 0.25, 2.0), (0.5, 0.3, 0.125)
    pos = ac.position_field(values.shape, lo, h).double()
    verts, faces, vert_attr = Aggregation.marching_tets(values.double(), None, 0.25, [float(np.float32(x)) for x in lo],
                                                        [float(np.float32(x)) for x in h], attr=pos)
    assert vert_attr.shape == verts.shape and vert_attr.dtype == torch.float64
    assert float((vert_attr - verts).abs().max()) <= 2 * mc.EPS * float(pos.abs().max())      # (the field's rounding to fp32 alone)
    # through the module, on the host: fp32 out, [0,C] for an empty mesh
    v32, f32, a32 = extract_mesh(values, None, 0.25, lo, h, attr=pos.float())
    assert a32.dtype == torch.float32 and a32.shape == (len(v32), 3) and f32.dtype == torch.int32
    assert float((a32 - v32).abs().max()) <= ac.vert_attr_bound(float(pos.abs().max())) + mc.vert_bound(values.shape, lo, h)
    for fill in (-1.0, 1.0):
        out = extract_mesh(torch.full((5, 6, 7), fill), attr=torch.ones(5, 6, 7, 4))
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0, 4) and out[2].dtype == torch.float32
    out = extract_mesh(torch.full((5, 6, 7), -1.0), torch.zeros(5, 6, 7), attr=torch.ones(5, 6, 7, 4))      # nothing observed
    assert out[2].shape == (0, 4)


def test_hit_points_come_back_at_the_vertices():
    """The convention, as a property of the fp64 definition on the 14 views: with every pixel's own hit point as its attribute, both
    ends of every vertex's edge are observed and the vertex's attribute is the vertex, within meshing_attr_cases.HIT_CAP."""
    depth, R, T, focal, pp = mc.sphere_views()
    image = ac.hit_point_images()
    assert image.shape == (14, mc.IMAGE, mc.IMAGE, 3)
    on = torch.isfinite(depth)
    assert float((image[on].double().norm(dim=-1) - mc.SPHERE_R).abs().max()) < 1e-5 and (image[~on] == 0).all()
    tsdf, weight, attr = ac.definition_fp64(depth, R, T, focal, pp, TRUNC, image)
    ref_t, ref_w = mc.definition_fp64(depth, R, T, focal, pp, TRUNC)
    assert torch.equal(tsdf, ref_t) and torch.equal(weight, ref_w)
    lo, h = float(np.float32(mc.GRID_LO)), float(np.float32(mc.GRID_H))
    verts, faces, vert_attr = Aggregation.marching_tets(tsdf, weight, 0.0, [lo] * 3, h, attr=attr)
    mc.assert_closed(verts, faces, chi=2)
    ia, ib = ac.edge_ends(verts, [lo] * 3, [h] * 3)
    assert (weight[ia[:, 2], ia[:, 1], ia[:, 0]] > 0).all() and (weight[ib[:, 2], ib[:, 1], ib[:, 0]] > 0).all()
    err = (vert_attr - verts).norm(dim=-1) / h
    print(f"hit points, fp64 definition: V {len(verts)}, |vert_attr - vert| max {float(err.max()):.3f} h, mean {float(err.mean()):.3f} h")
    assert len(verts) > 2000 and float(err.max()) <= ac.HIT_CAP
