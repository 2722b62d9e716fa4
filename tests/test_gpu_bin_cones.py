"""The cones the frame path's bin kernels make from the camera, and the camera centre binA writes.

With the camera as input binA and binB make their bounding cones from corner rays (csrc/voge_common.h: cam_rect_cone,
cam_two_cones); voge_camera_cones evaluates the same device functions by the kernels' own calls and hands the records out:
regions (128x128 px), super-tiles (32x32), quads (16x16) and tiles (8x8).  A cone may be any valid bound of its block; what is
asserted is the bound itself: EVERY ray of a block -- the bundle the sweep writes, bit-identical to voge_rays_fwd's -- lies
inside the block's cone (cos >= its lower bound, sin <= its upper bound, measured in fp64), for whole frames, batches, bands,
interleaved stripes and ragged sizes: the sizes of test_gpu_frame.py's bundle tests.  And origin_out holds the camera centre on
the two forms of binA that take prepared records (more than 131 072 scalar-sigma Gaussians; the general entry above the
small-set size).
"""
import numpy as np
import pytest
import torch

import oracle
from oracle import camera_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ABOVE_SMALL_SET = 6000      # (binA runs from 4 097 Gaussians on)


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _scene(N, seed, lo=0.03, hi=0.08):
    from voge_amd import scenes
    return scenes.random_gaussians(N, seed=seed, r_lo=lo, r_hi=hi)


def _views(B, seed):
    rng = np.random.default_rng(seed)
    return camera_np.look_at_view_transform(list(rng.uniform(3.0, 4.0, B)), list(rng.uniform(-30, 30, B)), list(rng.uniform(-180, 180, B)))


def _cones(cam, B):
    """(hier [B, nst * 21, 8], regions [B, nst0, 8]) of voge_camera_cones for camera_tensors' tuple."""
    from voge_amd import _lib
    lib = _lib.load()
    R, T, f, pp, band, W = cam
    row0, h, stripe_h, pitch = band
    nst, nst0 = ((W + 31) // 32) * ((h + 31) // 32), ((W + 127) // 128) * ((h + 127) // 128)
    hier = torch.full((B, nst * 21, 8), float("nan"), device=DEV)
    regions = torch.full((B, nst0, 8), float("nan"), device=DEV)
    args = [x.contiguous().float() for x in (R, T, f, pp)]
    rc = lib.voge_camera_cones(*[x.data_ptr() for x in args], int(row0), int(stripe_h), int(pitch), B, int(h), int(W),
                               hier.data_ptr(), regions.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return hier, regions


def _assert_blocks_inside(rays, hier, regions, what):
    """rays [B,h,W,3]; every region, super-tile, quad and tile with a pixel in the band: ok == 1 and all of its rays inside its cone."""
    B, h, W, _ = rays.shape
    nstx, nst0x = (W + 31) // 32, (W + 127) // 128
    nst = nstx * ((h + 31) // 32)
    d = rays.double()
    d = d / d.norm(dim=-1, keepdim=True)
    checked, worst_c, worst_s = 0, np.inf, np.inf
    for level, edge in (("region", 128), ("super-tile", 32), ("quad", 16), ("tile", 8)):
        for y0 in range(0, h, edge):
            for x0 in range(0, W, edge):
                st = (y0 // 32) * nstx + x0 // 32
                if level == "region":
                    rec = regions[:, (y0 // 128) * nst0x + x0 // 128]
                elif level == "super-tile":
                    rec = hier[:, st]
                elif level == "quad":
                    rec = hier[:, nst + st * 4 + ((y0 % 32) // 16) * 2 + (x0 % 32) // 16]
                else:
                    rec = hier[:, nst * 5 + st * 16 + ((y0 % 32) // 8) * 4 + (x0 % 32) // 8]
                rec = rec.double()      # [B, 8]
                blk = d[:, y0:y0 + edge, x0:x0 + edge].reshape(B, -1, 3)
                assert bool((rec[:, 5] == 1.0).all()), (what, level, y0, x0, "ok", rec[:, 5].tolist())
                ax = rec[:, None, 0:3]
                assert bool(((ax.norm(dim=-1) - 1.0).abs() < 1e-5).all()), (what, level, y0, x0, "axis not unit")
                ax = ax / ax.norm(dim=-1, keepdim=True)
                cos = (blk * ax).sum(-1)
                sin = (blk - cos[..., None] * ax).norm(dim=-1)
                mc, ms = float((cos - rec[:, None, 3]).min()), float((rec[:, None, 4] - sin).min())
                worst_c, worst_s = min(worst_c, mc), min(worst_s, ms)
                assert mc >= 0.0 and ms >= 0.0, (what, level, y0, x0, f"cos margin {mc:.3e}, sin margin {ms:.3e}")
                checked += 1
    assert checked == sum(((h + e - 1) // e) * ((W + e - 1) // e) for e in (128, 32, 16, 8))
    print(f"[bin cones] {what}: {checked} blocks x {B} views inside their cones; smallest margins cos {worst_c:.2e} sin {worst_s:.2e}")


@pytest.mark.parametrize("B,size,rows,what", [
    (1, (64, 64), None, "a whole frame"),
    (2, (70, 53), None, "ragged sizes (partial tiles, quads and super-tiles), a batch of two"),
    (1, (256, 256), (100, 164), "a band of 64 rows"),
    (1, (96, 200), (37, 90), "a band that starts and ends inside a tile"),
    (3, (33, 31), None, "one super-tile and a bit, three views"),
])
def test_every_ray_of_a_block_lies_inside_the_blocks_cone(hip_lib, B, size, rows, what):
    from voge_amd import ops
    from voge_amd.cameras import PerspectiveCameras, camera_tensors, pixel_rays
    verts, sig, cols = _scene(N_ABOVE_SMALL_SET, seed=B * 7 + size[0])
    R, T = _views(B, seed=size[1])
    H, W = size
    cams = PerspectiveCameras(focal_length=1.3 * max(H, W), principal_point=((W / 2.0 - 0.75, H / 2.0 + 0.125),), image_size=(size,),
                              R=t(R), T=t(T), device=DEV)
    want_rays, _ = pixel_rays(cams, size, rows=rows)
    cam = camera_tensors(cams, size, rows)
    idx, ln, lz = ops.frame_trace(t(verts), t(sig), *cam[:4], cam[4], cam[5], False, oracle.thr_act_of(0.01), 12, 1, 1.0)
    hier, regions = _cones(cam, B)
    assert torch.equal(lz.rays, want_rays), what
    _assert_blocks_inside(lz.rays, hier, regions, what)


def test_every_ray_of_a_block_of_interleaved_stripes_lies_inside_its_cone(hip_lib):
    """A rank's interleaved stripes, stacked: a block's cone bounds the image rows between its first and last row (a superset)."""
    from voge_amd import ops
    from voge_amd.cameras import PerspectiveCameras, camera_tensors, pixel_rays
    from voge_amd.distributed import Stripes
    verts, sig, cols = _scene(N_ABOVE_SMALL_SET, seed=5)
    R, T = camera_np.look_at_view_transform(3.2, 20.0, -35.0)
    size = (256, 192)
    cams = PerspectiveCameras(focal_length=260.0, principal_point=((96.0, 128.0),), image_size=(size,), R=t(R), T=t(T), device=DEV)
    for stripe_h, world, rank in ((32, 4, 1), (16, 2, 1), (32, 8, 7)):
        st = Stripes(size[0], rank, world, stripe_h)
        want_rays, _ = pixel_rays(cams, size, rows=st)
        cam = camera_tensors(cams, size, st)
        idx, ln, lz = ops.frame_trace(t(verts), t(sig), *cam[:4], cam[4], cam[5], False, oracle.thr_act_of(0.01), 16, 1, 1.0)
        hier, regions = _cones(cam, 1)
        assert torch.equal(lz.rays, want_rays)
        _assert_blocks_inside(lz.rays, hier, regions, f"stripes of {stripe_h} rows, rank {rank} of {world}")


def test_origin_out_of_the_prepared_records_forms_of_binA(hip_lib):
    """binA_kernel<false> (behind iso_prep_kernel from 131 072 scalar-sigma Gaussians on, and behind prep_kernel on the general
    entry) writes the camera centre, not zeros: origin_out == voge_rays_fwd's origin, bit for bit."""
    from voge_amd import ops, scenes
    from voge_amd.cameras import PerspectiveCameras, camera_tensors, pixel_rays
    size = (64, 64)
    B = 2
    R, T = _views(B, seed=11)
    cams = PerspectiveCameras(focal_length=90.0, principal_point=((31.25, 32.5),), image_size=(size,), R=t(R), T=t(T), device=DEV)
    _, want_origin = pixel_rays(cams, size)
    assert float(want_origin.abs().max()) > 1.0      # (a camera away from the world's origin: zeros would not pass)
    cam = camera_tensors(cams, size, None)
    thr = oracle.thr_act_of(0.01)

    verts, sig, cols = _scene(140000, seed=43, lo=0.02, hi=0.04)
    origin = torch.full((B, 3), float("nan"), device=DEV)
    ops.frame_trace(t(verts), t(sig), *cam[:4], cam[4], cam[5], False, thr, 8, 1, 1.0, origin_out=origin)
    assert torch.equal(origin, want_origin), ("N = 140 000 scalar sigmas", origin.tolist(), want_origin.tolist())

    verts, sig, cols = scenes.random_gaussians(N_ABOVE_SMALL_SET, seed=44, anisotropic="diag", r_lo=0.04, r_hi=0.09)
    origin = torch.full((B, 3), float("nan"), device=DEV)
    ops.frame_trace_gen(t(verts), t(sig), *cam[:4], cam[4], cam[5], False, thr, 8, 1.0, origin_out=origin)
    assert torch.equal(origin, want_origin), ("voge_frame_trace_fwd_gen, per-axis sigmas", origin.tolist(), want_origin.tolist())
