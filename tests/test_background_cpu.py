"""CPU tests of the broadcast-background blend's entry points (voge_blend_bg_fwd / _bwd, include/voge_hip.h): argument
validation before any HIP call, the workspace query, and what the compiler made of the three kernels (no scratch, no
spills, no compare-and-swap loops, no writes or cache maintenance through the scalar unit)."""
import os
import re

import pytest

from test_isa_cpu import HIPCC, _asm, _field, _kernel

P = 4096      # a non-NULL pointer value: nothing is dereferenced before validation is through


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _fwd(lib, rgb=P, s=P, bg=P, strides=(0, 0, 0, 1), thr=-1.0, B=1, H=8, W=8, C=3, img=P):
    return lib.voge_blend_bg_fwd(rgb, s, bg, *strides, thr, B, H, W, C, img, None)


def _bwd(lib, rgb=P, s=P, bg=P, strides=(0, 0, 0, 1), thr=-1.0, g=P, gs=(3, 1), B=1, H=8, W=8, C=3, g_rgb=P, g_m=P, g_bg=P,
         gst=(192, 24, 3, 1), ws=None, nbytes=0):      # (by default a per-pixel gradient: no workspace needed)
    return lib.voge_blend_bg_bwd(rgb, s, bg, *strides, thr, g, *gs, B, H, W, C, g_rgb, g_m, g_bg, *gst, ws, nbytes, None)


def test_entries_refuse_bad_arguments_before_any_hip_call(lib):
    for kw in (dict(rgb=None), dict(s=None), dict(bg=None), dict(img=None), dict(B=0), dict(H=0), dict(W=-1), dict(C=0),
               dict(strides=(0, -1, 0, 1)), dict(H=1 << 16, W=1 << 16)):
        assert _fwd(lib, **kw) == -1, kw
    for kw in (dict(rgb=None), dict(s=None), dict(bg=None), dict(g=None), dict(B=0), dict(H=-3), dict(W=0), dict(C=0),
               dict(gs=(-3, 1)), dict(gst=(0, -1, 0, 1)),
               dict(thr=0.5),                                              # [m > thr] has no gradient: g_m must be NULL
               dict(gst=(0, 0, 0, 1), ws=None),                            # one colour overall: the slab is missing
               dict(B=2, gst=(3, 0, 0, 1), ws=P, nbytes=4),                # a colour per view: the slab is too small
               dict(gst=(0, 0, 3, 1))):                                    # [W,C]: neither per pixel nor per view
        assert _bwd(lib, **kw) == -1, kw


def test_workspace_scales_with_views_workgroups_and_channels(lib):
    ws = lib.voge_blend_bg_bwd_workspace_bytes
    one = ws(1, 16, 16, 1)                       # 256 pixels: one workgroup, one channel
    assert one == 4
    assert ws(1, 16, 16, 3) == 3 * one and ws(4, 16, 16, 3) == 12 * one
    assert ws(1, 16, 17, 1) == 2 * one           # a pixel more: a second workgroup per view
    assert ws(2, 512, 512, 3) == 2 * 1024 * 3 * 4
    assert ws(0, 16, 16, 3) == 0 and ws(1, 16, 16, 0) == 0


# writes through the scalar unit, its atomics and its cache maintenance (matched by pattern: the mnemonics themselves are
# kept out of the sources)
_SCALAR_WRITE = re.compile(r"^\s+s_\w*(?:store|atomic)\w*|^\s+s_dcache_\w+", re.M)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_background_kernels_assembly(tmp_path):
    text = _asm("merge_blend", tmp_path)
    for frag in ("blend_bg_fwd_kernel", "blend_bg_bwd_kernel", "blend_bg_slab_kernel"):
        body, desc = _kernel(text, frag)
        assert _field(desc, "amdhsa_private_segment_fixed_size") == 0, (frag, "scratch")
        assert "spill" not in body.lower(), frag
        assert not re.search(r"^\s+v_(?:writelane|readlane)_b32", body, flags=re.M), (frag, "scalars parked in VGPR lanes")
        assert "cmpswap" not in body, (frag, "compare-and-swap loop")
        assert not _SCALAR_WRITE.search(body), (frag, _SCALAR_WRITE.search(body).group(0))
