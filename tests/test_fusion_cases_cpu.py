"""tests/fusion_cases.py is fit for its purpose, checked without a GPU: the scene populates every branch of the fusion rule, the
definition marks few of its grid points, and the definition in fp32 -- the kernels' arithmetic, operation by operation -- stays
within the derived bounds of the one in fp64.  If the scene changes, these conditions decide whether the change is allowed."""
import numpy as np
import torch

import fusion_cases as fc

BRANCHES = ("behind", "front", "u<0", "u>=W", "v<0", "v>=H", "nan", "inf", "nonpositive", "cut", "clamped", "band")


def test_the_scene_is_asymmetric():
    s = fc.scene()
    assert len(set(fc.RES)) == 3 and len(set(fc.LO)) == 3 and len(set(fc.VOXEL)) == 3 and fc.IMAGE_H != fc.IMAGE_W
    assert s.depth.shape == (fc.B, fc.IMAGE_H, fc.IMAGE_W) and s.depth.dtype == torch.float32
    assert int((s.focal[:, 0] != s.focal[:, 1]).sum()) == 4
    n = fc.RES[0] * fc.RES[1] * fc.RES[2]
    assert n == 2717 and n // 256 == 10 and n % 256 == 157      # ten full workgroups and a partial one
    # the poison: 15 % of view 4, every kind present, nothing else touched
    share = float(s.poisoned.double().mean())
    assert 0.10 < share < 0.20
    bad = s.depth[4][s.poisoned]
    assert torch.isnan(bad).any() and (bad == float("inf")).any() and (bad == float("-inf")).any() and (bad == 0).any() and (bad == -1.5).any()
    keep = torch.ones_like(s.depth, dtype=torch.bool)
    keep[4] = ~s.poisoned
    assert torch.equal(s.depth[keep], s.depth_clean[keep])
    assert ((s.depth_clean > 0) & ~torch.isnan(s.depth_clean)).all()      # the clean maps: a positive number or +inf
    assert torch.isinf(s.depth_clean[3]).all()                            # view 3 looks away from the sphere as well


def test_every_branch_is_populated():
    s = fc.scene()
    counts = fc.branch_counts(s)
    n = 2717
    for b, c in enumerate(counts):
        print(f"[fusion scene] view {b}: " + ", ".join(f"{k} {c[k]}" for k in BRANCHES))
    for k in BRANCHES:
        assert any(c[k] > 0 for c in counts), k
    assert counts[3]["behind"] == n and counts[3]["front"] == 0             # whole waves skip view 3
    assert counts[2]["behind"] > 100 and counts[2]["front"] > 100           # the camera inside the grid
    assert counts[4]["nan"] > 0 and counts[4]["nonpositive"] > 0            # step 3, read by points inside the image
    for b in (0, 1, 4):
        assert counts[b]["behind"] == 0
    for b in (0, 1, 2, 4):      # a hundred points or more off the image, without a surface, behind it and in the band; some clamped
        c = counts[b]
        off = c["u<0"] + c["u>=W"] + c["v<0"] + c["v>=H"]
        assert min(off, c["nan"] + c["inf"] + c["nonpositive"], c["cut"], c["band"]) >= 100 and c["clamped"] > 0, (b, c)


def check(label, got, ref, bound, attr_bound=None):
    """fp32 definition against the fp64 one off the marks -> the largest |dtsdf|"""
    ref_t, ref_w, marked = ref[:3]
    share = float(marked.double().mean())
    keep = ~marked
    assert share <= 0.02, share
    mismatches = int((got[1].double()[keep] != ref_w[keep]).sum())
    worst = float((got[0].double() - ref_t)[keep].abs().max())
    line = f"[fusion scene] {label}: marked {share * 100:.2f} %, weight mismatches {mismatches}, max |dtsdf| {worst:.2e}, bound {bound:.2e}"
    if attr_bound is not None:
        worst_a = float((got[2].double() - ref[3])[keep].abs().max())
        line += f", max |dattr| {worst_a:.2e}, bound {attr_bound:.2e}"
    print(line)
    assert mismatches == 0 and worst <= bound
    if attr_bound is not None:
        assert worst_a <= attr_bound


def test_marked_share_and_weights():
    _, w, marked, _ = fc.reference(False)
    share = float(marked.double().mean())
    print(f"[fusion scene] marked share {share * 100:.2f} %, weights up to {int(w.max())}, {int((w > 0).sum())} points updated")
    assert 0 < share <= 0.02
    assert int(w.max()) == 3 and int(((w > 0) & ~marked).sum()) > 500
    # under the cap some prior weights FALL: min(w + 1, max_weight) below a prior 4
    prior_w = fc.prior()[1].double()
    capped = fc.reference(True)[1]
    fallen = int((capped < prior_w).sum())
    print(f"[fusion scene] prior state under max_weight {fc.MAX_WEIGHT}: {fallen} weights fall")
    assert fallen > 0 and float(capped[capped != prior_w].max()) <= fc.MAX_WEIGHT
    assert torch.equal(capped[capped < prior_w], torch.full((fallen,), float(fc.MAX_WEIGHT), dtype=torch.float64))


def test_fp32_definition_against_the_fp64_one():
    s = fc.scene()
    bound = fc.tsdf_bound(s)
    assert 1e-6 < bound < 5e-5      # a few hundred eps: the bound says something
    image, prior = fc.images(), fc.prior()
    a_bound = fc.attr_bound(image, prior[2])
    check("empty volume", fc.definition(s, torch.float32), fc.reference(False), bound)
    check("prior state, max_weight 3", fc.definition(s, torch.float32, prior, fc.MAX_WEIGHT), fc.reference(True), bound)
    check("empty volume, C = 8", fc.definition(s, torch.float32, attr_image=image), fc.reference(False), bound, fc.attr_bound(image))
    check("prior state, max_weight 3, C = 8", fc.definition(s, torch.float32, prior, fc.MAX_WEIGHT, image), fc.reference(True), bound, a_bound)
    # an attribute changes no geometry, in the definition either
    plain = fc.definition_fp64(s, prior, fc.MAX_WEIGHT)
    assert all(torch.equal(a, b) for a, b in zip(plain, fc.reference(True)[:3]))


def test_the_volume_on_the_host_is_the_fp32_definition():
    """TSDFVolume.integrate on the host: what the device results of the single grid points are compared with, bit for bit"""
    s = fc.scene()
    prior = fc.prior()
    vol = fc.volume("cpu", 2, prior).integrate(s.depth, fc.cams(s), fc.TRUNC, max_weight=fc.MAX_WEIGHT, attr=fc.images()[..., :2])
    want = fc.definition(s, torch.float32, prior, fc.MAX_WEIGHT, fc.images()[..., :2])
    assert torch.equal(vol.tsdf, want[0]) and torch.equal(vol.weight, want[1]) and torch.equal(vol.attr, want[2])


def test_the_centres_of_the_device_route():
    """Aggregation.camera_centres on a device inverts R in closed form, so that integrate reads nothing back: in fp64 that is
    torch.linalg.inv's answer to a few 2^-53 and the same fp32 centre (the scene's views, the 14 of meshing_cases, sheared ones)"""
    from voge_amd import Aggregation
    import meshing_cases as mc
    s = fc.scene()
    shear = torch.tensor([[[1.0, 0.3, 0.0], [0.0, 0.8, -0.2], [0.1, 0.0, 1.3]]], dtype=torch.float64)
    for R, T in ((s.R, s.T), mc.sphere_views()[1:3], (shear, torch.tensor([[0.3, -1.2, 2.0]]))):
        R, T = R.double(), T.double()
        want, got = Aggregation.camera_centres(R, T), Aggregation._camera_centres_closed_form(R, T)
        assert float((got - want).abs().max()) <= 16 * 2.0 ** -53 * float(want.abs().max())
        assert torch.equal(got.to(torch.float32), want.to(torch.float32))


def test_exact_edge_points_on_the_host():
    """The optical-axis point projects to the principal point exactly: the decisions at u = 0, u = W, v = H, sdf = -trunc and
    sdf = trunc as the rule states them (tests/test_gpu_fusion.py asks the kernel for the same bits)"""
    nan = float("nan")
    only = lambda H, W, i, j, d: torch.full((H, W), nan).index_put((torch.tensor(i), torch.tensor(j)), torch.tensor(d))
    get = lambda point, depth, pp, **kw: tuple(float(x) for x in fc.integrate_point(point, *fc.axis_camera(depth, pp), **kw))
    assert get((0.0, 0.0, 0.0), only(8, 8, 0, 0, 3.25), (0.0, 0.0)) == (0.5, 1.0)            # u = v = 0: inside, pixel (0, 0)
    assert get((0.0, 0.0, 0.0), torch.full((8, 8), 3.25), (8.0, 0.0)) == (0.0, 0.0)          # u = W: outside
    assert get((0.0, 0.0, 0.0), torch.full((8, 8), 3.25), (0.0, 8.0)) == (0.0, 0.0)          # v = H: outside
    assert get((0.0, 0.0, 0.0), only(5, 8, 4, 7, 3.25), (7.5, 4.5)) == (0.5, 1.0)            # the last pixel of a 5 x 8 image
    but = torch.full((5, 8), 3.25)
    but[4, 7] = nan
    assert get((0.0, 0.0, 0.0), but, (7.5, 4.5)) == (0.0, 0.0)                               # (every pixel finite BUT that one)
    assert get((0.0, 0.0, 0.0), torch.full((1, 1), 3.25), (0.5, 0.5)) == (0.5, 1.0)          # a 1 x 1 image
    assert get((0.0, 0.0, 0.5), torch.full((8, 8), 3.0), (4.0, 4.0)) == (-1.0, 1.0)          # sdf == -trunc: updated, t = -1
    assert get((0.0, 0.0, -0.5), torch.full((8, 8), 3.0), (4.0, 4.0)) == (1.0, 1.0)          # sdf / trunc == 1
    assert get((0.0, 0.0, 0.5 + 2.0 ** -20), torch.full((8, 8), 3.0), (4.0, 4.0)) == (0.0, 0.0)      # one step behind the band: cut
    assert np.isclose(get((0.0, 0.0, -0.25), torch.full((8, 8), 3.0), (4.0, 4.0))[0], 0.5)
    # within trunc of the camera centre sdf >= -trunc even for a depth <= 0: only step 3 (d > 0) skips such a view
    for bad in (0.0, -0.0, -0.125):
        assert get((0.0, 0.0, -2.75), torch.full((8, 8), bad), (4.0, 4.0)) == (0.0, 0.0), bad
    assert get((0.0, 0.0, -2.75), torch.full((8, 8), 0.125), (4.0, 4.0)) == (-0.25, 1.0)
