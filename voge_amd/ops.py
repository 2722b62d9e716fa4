"""torch.autograd wrappers around the C ABI (include/voge_hip.h).

torch is used here for device memory, streams and autograd bookkeeping only; every
computation on the path is a HIP kernel in libvoge_hip.so.  Ownership follows SURVEY.md §8b:
the caller (these Functions) allocates every output; the library never allocates.
"""
import math
import os
import struct

import torch

from . import _lib


# torch._C._cuda_getCurrentRawStream / _cuda_getDevice / _cuda_setDevice are private (present in torch 1.8 ..
# 2.10, the version this image ships); fall back to the public API when a build lacks them.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_set_dev = getattr(torch._C, "_cuda_setDevice", None) or torch.cuda.set_device


def _stream():
    """Raw handle of the current stream of the current device.  (torch.cuda.current_stream() builds a
    Stream object and costs ~10 us a call -- several calls per frame on a path whose small frames are
    host-bound; the raw getter is what torch's own compiled code uses.)"""
    if _raw_stream is not None:
        return _raw_stream(_get_dev())
    return torch.cuda.current_stream().cuda_stream


class _on:
    """`with _on(device)`: make `device` current for the launches inside.  Unlike torch.cuda.device it
    does nothing at all (no guard object, no driver call) when the device is already current."""
    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index if device.index is not None else _get_dev()
        self.prev = -1

    def __enter__(self):
        cur = _get_dev()
        if cur != self.idx:
            self.prev = cur
            _set_dev(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            _set_dev(self.prev)
        return False


def _dev(t, dtype, name):
    """Validate a tensor argument the way the C side cannot: device, dtype, contiguity."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.VogeHipError(
            f"{name} is on {t.device}: the VoGE hot path runs on a HIP device only (no CPU fallback)")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


_WS = {}


def _workspace(dev, nbytes):
    """Scratch for one entry point: one buffer per (device, stream), grown on demand and reused by later calls.
    Everything the library does is stream-ordered, so consecutive calls on a stream may share their scratch
    (the trace's lists are ~135 MB per 512^2 view: allocating them per call put that much churn on every frame).
    During stream capture the buffer comes from the graph's own pool (a fresh allocation, not cached)."""
    nbytes = max(int(nbytes), 16)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    key = (dev.index if dev.index is not None else _get_dev(), _stream())
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def release_workspaces(device=None):
    """Drop the cached scratch buffers (all, or those of one device): the trace's lists are 165 MB per 512^2 view and
    774 MB at 1024^2, held per (device, stream) from the first call on -- a long-lived process that is done rendering big
    frames, or that warmed a side stream for graph capture, gives the memory back here.  The next call re-allocates."""
    idx = None if device is None else (torch.device(device).index if torch.device(device).index is not None else _get_dev())
    for key in [k for k in _WS if idx is None or k[0] == idx]:
        del _WS[key]


class _GeneralPreamble(torch.autograd.Function):
    """Renderer.py:130-137 for (N,3) / (N,3,3) sigmas as one launch each way (voge_general_preamble_fwd / _bwd):
    forward(verts [N,3] | [B,N,3], sigmas [N,3] | [N,3,3] | [B,N,...], origin [B,3]) -> mus [B*N,3], isigmas [B*N,3,3]
    (= verts - origin[b], 2 * expend_sigma(sigmas)).  No gradient for origin (camera optimisation takes the torch chain)."""

    @staticmethod
    def forward(ctx, verts, sigmas, origin):
        lib = _lib.load()
        v_c, s_c, o_c = _dev(verts, torch.float32, "verts"), _dev(sigmas, torch.float32, "sigmas"), _dev(origin, torch.float32, "origin")
        B = o_c.shape[0]
        shared_v = v_c.dim() == 2
        N = v_c.shape[-2]
        kind = 2 if tuple(s_c.shape[-2:]) == (3, 3) and s_c.dim() >= 3 else 1
        shared_s = s_c.dim() == (3 if kind == 2 else 2)
        assert v_c.shape[-1] == 3 and (shared_v or v_c.shape[0] == B) and o_c.shape == (B, 3)
        assert s_c.shape[-1] == 3 and s_c.shape[-(kind + 1)] == N and (shared_s or s_c.shape[0] == B)
        mus = torch.empty((B * N, 3), dtype=torch.float32, device=v_c.device)
        isg = torch.empty((B * N, 3, 3), dtype=torch.float32, device=v_c.device)
        with _on(v_c.device):
            rc = lib.voge_general_preamble_fwd(_p(v_c), _p(s_c), _p(o_c), B, N, int(shared_v), int(shared_s), kind, _p(mus), _p(isg),
                                               _stream())
        _lib.check(rc, "voge_general_preamble_fwd")
        ctx.meta = (B, N, shared_v, shared_s, kind, tuple(v_c.shape), tuple(s_c.shape))
        ctx.set_materialize_grads(False)
        return mus, isg

    @staticmethod
    def backward(ctx, g_mus, g_isg):
        lib = _lib.load()
        B, N, shared_v, shared_s, kind, vshape, sshape = ctx.meta
        if ctx.needs_input_grad[2]:
            raise _lib.VogeHipError("the fused preamble carries no gradient for the camera centre")
        g_v = g_s = None
        gm = None if g_mus is None else _dev(g_mus, torch.float32, "grad_mus")
        ga = None if g_isg is None else _dev(g_isg, torch.float32, "grad_isigmas")
        dev = (gm if gm is not None else ga)
        if dev is None:
            return None, None, None
        dev = dev.device
        if ctx.needs_input_grad[0] and gm is not None:
            g_v = torch.empty(vshape, dtype=torch.float32, device=dev)
        if ctx.needs_input_grad[1] and ga is not None:
            g_s = torch.empty(sshape, dtype=torch.float32, device=dev)
        if g_v is not None or g_s is not None:
            with _on(dev):
                rc = lib.voge_general_preamble_bwd(_p(gm if g_v is not None else None), _p(ga if g_s is not None else None), B, N,
                                                   int(shared_v), int(shared_s), kind, _p(g_v), _p(g_s), _stream())
            _lib.check(rc, "voge_general_preamble_bwd")
        return g_v, g_s, None


def general_preamble(verts, sigmas, origin):
    """-> (mus [B*N,3], isigmas [B*N,3,3]) of the general path, one launch (see _GeneralPreamble)."""
    return _GeneralPreamble.apply(verts, sigmas, origin)


def trace_pool_usage(dev, B, N, H, W):
    """(used, capacity) of the candidate-list pool after the last forward trace of this shape on the current stream of
    `dev` (include/voge_hip.h: voge_trace_pool_usage) -- diagnostics: used > 0 means some 16x16-pixel quads held more
    candidates than the in-LDS sort takes (a small, dense object); used > capacity means the pool ran out and those
    quads fell back to streaming every Gaussian.  Synchronises."""
    import ctypes
    lib = _lib.load()
    dev = torch.device(dev)
    with _on(dev):
        nbytes = lib.voge_trace_workspace_bytes(B, N, H, W)
        ws = _workspace(dev, nbytes)
        used, cap = ctypes.c_int(0), ctypes.c_int(0)
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.voge_trace_pool_usage(_p(ws), nbytes, B, N, H, W, ctypes.byref(used), ctypes.byref(cap)), "voge_trace_pool_usage")
    return used.value, cap.value


def _tag_index(sel_idx, cnt, n_index):
    """Bookkeeping the trace leaves on the index tensor it returns:
    voge_hit_count  (cnt [B,H,W] int32, torch version of sel_idx when it was written): lets aggregation() skip its
                    pass over idx and the backwards skip empty slots.  A later in-place edit of sel_idx through
                    torch (e.g. masking Gaussians out with -1) bumps the version and invalidates the count.
    voge_index_bound  = (number of Gaussians the indices address (B*N), version): merge_final's range assert
                    (Aggregation.py:120) becomes a host-side comparison of two shapes while the tensor is unmodified."""
    if cnt is not None:
        sel_idx.voge_hit_count = (cnt, sel_idx._version)
    sel_idx.voge_index_bound = (int(n_index), sel_idx._version)


def carry_tags(src, dst):
    """A reshaped view of a fragment tensor (Fragments.unsqueeze / squeeze / [0] of a one-view batch / copy) still is
    the same memory: hand the trace's bookkeeping on, so the view keeps the fast paths (no synchronising range check,
    hit counts, the fused backward).  A true slice or a copy gets nothing."""
    if dst is src or not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.is_contiguous()
                          and dst.data_ptr() == src.data_ptr() and dst.numel() == src.numel() and dst.dtype == src.dtype):
        return dst
    tag = getattr(src, "voge_hit_count", None)
    if tag is not None:
        dst.voge_hit_count = (tag[0].view(dst.shape[:-1]), tag[1])
    for name in ("voge_index_bound", "voge_through"):
        tag = getattr(src, name, None)
        if tag is not None:
            setattr(dst, name, tag)
    return dst


def cones_of(rays, B, H, W):
    """The super-tile cones pixel_rays() left on the ray tensor it returned, if they still describe it (same
    tensor, not modified through torch since), else None -- the trace then derives them itself."""
    tag = getattr(rays, "voge_cones", None)
    if tag is None:
        return None
    cones, version = tag
    if version != rays._version or cones.device != rays.device or tuple(rays.shape) != (B, H, W, 3):
        return None
    return cones


def hit_count_of(sel_idx):
    """The trace's per-pixel hit count if it still describes `sel_idx`, else None."""
    tag = getattr(sel_idx, "voge_hit_count", None)
    if tag is None:
        return None
    cnt, version = tag
    if version != sel_idx._version or cnt.shape != sel_idx.shape[:-1] or cnt.device != sel_idx.device:
        return None
    return cnt


def check_index_range(idx, n_attr):
    """merge_final's `assert vert_attr.shape[0] > vert_assign.max()` (Aggregation.py:120).  Indices written by
    the trace carry their range (voge_index_bound = B*N) while nobody has edited them through torch: a host comparison
    (stricter than the reference's: it fails whenever the table is shorter than B*N rows, hit or not -- INTEGRATION.md
    section 4).  Any other index tensor is checked on the device as the reference does (a synchronising reduction),
    except during stream capture."""
    tag = getattr(idx, "voge_index_bound", None)
    if tag is not None and tag[1] == idx._version:
        if n_attr < tag[0]:
            raise AssertionError(
                f"vert_attr has {n_attr} rows but the fragments index {tag[0]} Gaussians (a batch of B views addresses "
                f"rows b*N+n: tile the attributes over the batch, as the reference requires -- Aggregation.py:120)")
        return
    if idx.numel() and not torch.cuda.is_current_stream_capturing():
        assert n_attr > int(idx.max()), "vert_attr.shape[0] must exceed vert_assign.max() (Aggregation.py:120)"


def _trace_inputs(mode, p0, p1, origin, rays, cam_fwd, packed=False):
    """Validate the Gaussians of a ray-bundle trace in one of its three forms against rays [B,H,W,3]:
      mode 0: p0 = mus [P,3], p1 = isigmas [P,3,3]           (general 3x3 forms)
      mode 1: p0 = mus [P,3], p1 = a [P]                     (A = a I)
      mode 2: p0 = verts [N,3] | [B,N,3], p1 = sigmas [N] | [B,N], origin [B,3]   (the renderer's preamble folded in)
    P = B*N rows unless `packed` (explicit candidate lists address any P).
    -> p0, p1, origin (mode 2, else None), rays, cam_fwd (or None) as contiguous fp32; B, N, H, W, shared."""
    p0_c, p1_c = _dev(p0, torch.float32, "means"), _dev(p1, torch.float32, "sigmas")
    rays_c = _dev(rays, torch.float32, "rays")
    assert rays_c.dim() == 4 and rays_c.shape[3] == 3 and mode in (0, 1, 2)
    B, H, W, _ = rays_c.shape
    o_c, shared = None, False
    if mode == 2:
        o_c = _dev(origin, torch.float32, "origin")
        shared = p0_c.dim() == 2
        assert p0_c.shape[-1] == 3 and (shared or p0_c.shape[0] == B) and p1_c.shape == p0_c.shape[:-1]
        assert o_c.shape == (B, 3)
        N = p0_c.shape[-2]
    else:
        P = p0_c.shape[0]
        assert p0_c.dim() == 2 and p0_c.shape[1] == 3 and p1_c.shape == ((P,) if mode == 1 else (P, 3, 3))
        assert packed or (B > 0 and P % B == 0), "mus must hold B*N rows"
        N = P // max(B, 1)
    fwd = None if cam_fwd is None else _dev(cam_fwd, torch.float32, "cam_fwd")
    return p0_c, p1_c, o_c, rays_c, fwd, B, N, H, W, shared


def _trace_bwd(mode, p0, p1, origin, shared, sigma_mode, rays, idx, cnt, g_len, g_act, g_dsd, need_rays):
    """The trace's backward alone (voge_trace_bwd / _iso / _iso_view) for the gradients of len, act and dsd of the slots idx
    [B,H,W,K] -> (g0, g1, g_rays | None): the gradients of the trace's p0 / p1 (forms as in _trace_inputs) and of the rays."""
    lib = _lib.load()
    B, H, W, K = idx.shape
    dev = rays.device
    g0, g1 = torch.empty_like(p0), torch.empty_like(p1)
    g_ray = torch.empty_like(rays) if need_rays else None
    grads = (_p(idx), _p(cnt), _p(g_len), _p(g_act), _p(g_dsd))
    with _on(dev):
        if mode == 2:
            N = p0.shape[-2]
            nbytes = lib.voge_trace_bwd_iso_workspace_bytes(B * N)
            ws = _workspace(dev, nbytes)
            rc = lib.voge_trace_bwd_iso_view(_p(p0), _p(p1), _p(origin), int(shared), int(sigma_mode), _p(rays), *grads, B, N, B * H, W,
                                             K, _p(ws), nbytes, _p(g_ray), _p(g0), _p(g1), _stream())
        elif mode == 1:
            nbytes = lib.voge_trace_bwd_iso_workspace_bytes(p0.shape[0])
            ws = _workspace(dev, nbytes)
            rc = lib.voge_trace_bwd_iso(_p(p0), _p(p1), _p(rays), *grads, p0.shape[0], B * H, W, K, _p(ws), nbytes, _p(g_ray), _p(g0),
                                        _p(g1), _stream())
        else:
            nbytes = lib.voge_trace_bwd_workspace_bytes(p0.shape[0])
            ws = _workspace(dev, nbytes)
            rc = lib.voge_trace_bwd(_p(p0), _p(p1), _p(rays), *grads, p0.shape[0], B * H, W, K, _p(ws), nbytes, _p(g_ray), _p(g0),
                                    _p(g1), _stream())
    _lib.check(rc, "voge_trace_bwd")
    return g0, g1, g_ray


def _comp_aligned(t_, K):
    """t_ itself, or a copy on the boundary of the composite kernels' accesses: 16 bytes for K % 4 == 0, 8 for other even K (a
    contiguous view into a larger buffer may start anywhere; odd K goes slot by slot).  voge_composite_fwd / _bwd refuse the rest."""
    if t_ is None or t_.data_ptr() % (16 if K % 4 == 0 else (8 if K % 2 == 0 else 4)) == 0:
        return t_
    return t_.clone()


def _composite_bwd(act, ln, dsd, weight, cnt, g_weight, occ):
    """voge_composite_bwd: the gradient of the weights -> (g_act, g_len, g_dsd)."""
    K = act.shape[-1]
    gw = _comp_aligned(_dev(g_weight, torch.float32, "grad_weight"), K)
    if weight is not None:      # (recomputed weights: the one-slot kernel, no wide access)
        act, ln, dsd, weight = (_comp_aligned(x, K) for x in (act, ln, dsd, weight))
    g_act, g_len, g_dsd = torch.empty_like(act), torch.empty_like(act), torch.empty_like(act)
    with _on(act.device):
        rc = _lib.load().voge_composite_bwd(_p(act), _p(ln), _p(dsd), _p(weight), _p(cnt), _p(gw), occ, act.numel() // max(K, 1), K,
                                            _p(g_act), _p(g_len), _p(g_dsd), _stream())
    _lib.check(rc, "voge_composite_bwd")
    return g_act, g_len, g_dsd


class _RayTrace(torch.autograd.Function):
    """Mirror of VoGE/RayTracing.py:154-206 (`_RayTraceVoGE`) for the three forms of _trace_inputs:
    forward(mode, p0, p1, origin, rays [B,H,W,3], cam_fwd, thr_act, n_assign, sigma_mode, bins, bin_size)
    -> sel_idx int32, sel_len, sel_act, sel_dsd, each [B,H,W,K].
    cam_fwd: None -> every Gaussian of the batch element is a candidate (the max_points_per_bin == -1 list of
    RayTracing.py:22-26, never materialised); [B,3] -> "all candidates in front of the camera" (view axis per batch element).
    bins (mode 0 only): explicit candidate lists [B,BH,BW,M] as in the reference (voge_trace_topk_list_fwd).
    Mode 2 sees Gaussian n in view b as (verts - origin[b], a = 2 sigma (sigma_mode 1) | 2 / sigma (2) | sigma (0)) and has no
    gradient for origin: callers that optimise the camera use the unfused form.  The scalar forms' backward returns the
    gradient of the scalar directly (four sums per Gaussian instead of twelve)."""

    @staticmethod
    def forward(ctx, mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode, bins, bin_size):
        lib = _lib.load()
        p0_c, p1_c, o_c, rays_c, fwd, B, N, H, W, shared = _trace_inputs(mode, p0, p1, origin, rays, cam_fwd, bins is not None)
        K, dev = int(n_assign), rays_c.device
        sel_idx = torch.empty((B, H, W, K), dtype=torch.int32, device=dev)
        sel_len = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
        sel_act = torch.empty_like(sel_len)
        sel_dsd = torch.empty_like(sel_len)
        # per-pixel hit count: tells the backward (and aggregation) which slots are filled, so the index tensor
        # may later be rewritten in place by merge_final (-1 -> 0, Aggregation.py:131) without a defensive copy
        cnt = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        with _on(dev):
            out = (_p(sel_idx), _p(sel_len), _p(sel_act), _p(sel_dsd), _p(cnt), _stream())
            if bins is not None:
                bins = _dev(bins, torch.int32, "bin_points")
                assert bins.dim() == 4 and bins.shape[0] == B
                rc = lib.voge_trace_topk_list_fwd(_p(p0_c), _p(p1_c), _p(rays_c), _p(bins), B, p0_c.shape[0], H, W, K, *bins.shape[1:],
                                                  int(bin_size), float(thr_act), *out)
            else:
                nbytes = lib.voge_trace_workspace_bytes(B, N, H, W)
                ws = _workspace(dev, nbytes)
                sweep = (_p(fwd), _p(cones_of(rays_c, B, H, W)), B, N, H, W, K, float(thr_act), _p(ws), nbytes, *out)
                if mode == 2:
                    rc = lib.voge_trace_topk_fwd_iso_view(_p(p0_c), _p(p1_c), _p(o_c), int(shared), int(sigma_mode), _p(rays_c), *sweep)
                elif mode == 1:
                    rc = lib.voge_trace_topk_fwd_iso(_p(p0_c), _p(p1_c), _p(rays_c), *sweep)
                else:
                    rc = lib.voge_trace_topk_fwd(_p(p0_c), _p(p1_c), _p(rays_c), *sweep)
        _lib.check(rc, "voge_trace_topk_fwd")
        ctx.save_for_backward(p0_c, p1_c, o_c, rays_c)
        ctx.sel_idx = sel_idx      # may later be rewritten in place by merge_final; cnt marks the filled slots
        ctx.cnt = cnt
        ctx.meta = (int(mode), int(sigma_mode), shared)
        _tag_index(sel_idx, cnt, B * N if mode == 2 else p0_c.shape[0])
        ctx.mark_non_differentiable(sel_idx)
        ctx.set_materialize_grads(False)
        return sel_idx, sel_len, sel_act, sel_dsd

    @staticmethod
    def backward(ctx, grad_sel_idx, grad_sel_len, grad_sel_act, grad_sel_dsd):
        p0, p1, origin, rays = ctx.saved_tensors
        mode, sigma_mode, shared = ctx.meta
        if mode == 2 and ctx.needs_input_grad[3]:
            raise _lib.VogeHipError("the fused view form has no gradient for the camera centre; "
                                    "use ray_tracing_iso on centred vertices")
        sel_idx = ctx.sel_idx
        zeros = None

        def g(t):
            nonlocal zeros
            if t is None:
                if zeros is None:
                    zeros = torch.zeros(sel_idx.shape, dtype=torch.float32, device=sel_idx.device)
                return zeros
            return _dev(t, torch.float32, "grad")
        gl, ga, gd = g(grad_sel_len), g(grad_sel_act), g(grad_sel_dsd)
        g0, g1, g_ray = _trace_bwd(mode, p0, p1, origin, shared, sigma_mode, rays, sel_idx, ctx.cnt, gl, ga, gd, ctx.needs_input_grad[4])
        return None, g0, g1, None, g_ray, None, None, None, None, None, None


class _RayTraceVoGE:
    """_RayTrace of the general 3x3 forms: apply(mus [P,3], isigmas [P,3,3], rays [B,H,W,3], bin_points, thr_act, bin_size,
    n_assign).  bin_points: None (every Gaussian of the batch element), a float [B,3] view axis per batch element (the
    candidates in front of the camera), or int explicit candidate lists [B,BH,BW,M]."""

    @staticmethod
    def apply(mus, isigmas, rays, bin_points, thr_act, bin_size, n_assign):
        if bin_points is not None and bin_points.dtype in (torch.int32, torch.int64):
            return _RayTrace.apply(0, mus, isigmas, None, rays, None, thr_act, n_assign, 0, bin_points, bin_size)
        return _RayTrace.apply(0, mus, isigmas, None, rays, bin_points, thr_act, n_assign, 0, None, bin_size)


class _RayTraceVoGEIso:
    """_RayTrace for isotropic Gaussians given as ONE scalar each (A = a I): what expend_sigma((N,)) followed by 2*sigma
    (Aggregation.py:155-157, Renderer.py:133) describes.  apply(mus [P,3], a [P], rays [B,H,W,3], cam_fwd | None, thr_act,
    n_assign)."""

    @staticmethod
    def apply(mus, a, rays, cam_fwd, thr_act, n_assign):
        return _RayTrace.apply(1, mus, a, None, rays, cam_fwd, thr_act, n_assign, 0, None, 0)


class _RayTraceVoGEIsoView:
    """_RayTraceVoGEIso with the renderer's elementwise preamble folded into the kernels (Renderer.py:130-137):
    apply(verts [N,3] | [B,N,3], sigmas [N] | [B,N], origin [B,3], rays [B,H,W,3], cam_fwd | None, thr_act, n_assign,
    sigma_mode).  No gradient for origin."""

    @staticmethod
    def apply(verts, sigmas, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode):
        return _RayTrace.apply(2, verts, sigmas, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode, None, 0)


# VOGE_THREE_KERNEL_BACKWARD=1: _Fragments.backward runs voge_composite_bwd + voge_trace_bwd* (the round-1 chain, with
# act / dsd materialised and g_len / g_act / g_dsd exchanged through memory) instead of the one-pass voge_fragment_bwd*.
THREE_KERNEL_BACKWARD = os.environ.get("VOGE_THREE_KERNEL_BACKWARD", "0") == "1"


def _grad_weight_layout(g, K):
    """How voge_fragment_bwd* should read a gradient of the weights: (tensor, stride_pix, stride_k) in elements.
    Contiguous [.., K] -> (K, 1); a per-pixel value expanded over the slots (what _Silhouette.backward returns when
    nothing else consumed the weights) -> (1, 0), read in place; anything else is made contiguous."""
    if g is None:
        return None, 0, 0
    if g.dtype == torch.float32 and g.is_cuda:
        if g.is_contiguous():
            return g, K, 1
        if g.stride(-1) == 0 and g[..., 0].is_contiguous():
            return g, 1, 0
    return _dev(g, torch.float32, "grad_weight"), K, 1


def _grad_layout(g, C):
    """How the fused backwards read the gradient of a [.., C] image: (tensor, stride_pix, stride_c) in elements.  Autograd's
    broadcast scalar (sum / mean losses) is read in place as (g, 0, 0); anything else is made contiguous, (C, 1)."""
    if g.dtype == torch.float32 and g.is_cuda and all(s == 0 for s in g.stride()):
        return g, 0, 0
    return _dev(g, torch.float32, "grad_image"), C, 1


def _fragment_bwd(mode, p0, p1, records, shared, sigma_mode, rays, idx, cnt, B, N, like, weight, act, ln, dsd, g_weight, g_len, occ):
    """Composite + trace backward in ONE pass (voge_fragment_bwd / _iso: the composite's closed form and the trace's chain rule per
    slot in registers, per-Gaussian sums in a wave-private table) for the gradients of the weights and of len, either of which may
    be None (without g_weight, `weight` is read but multiplies zero) -> (g0, g1) shaped like like[0] / like[1].  Mode 0 reads the
    means p0, the scalar forms their records; p1 is the sigmas."""
    lib = _lib.load()
    _, H, W, K = idx.shape
    gw, gs_pix, gs_k = _grad_weight_layout(g_weight, K)
    gh = None if g_len is None else _dev(g_len, torch.float32, "grad_hit_length")
    dev = rays.device
    g0 = torch.empty(like[0].shape, dtype=torch.float32, device=dev)
    g1 = torch.empty(like[1].shape, dtype=torch.float32, device=dev)
    slots = (_p(idx), _p(cnt), _p(weight), _p(act), _p(ln), _p(dsd), _p(gw), gs_pix, gs_k, _p(gh), occ)
    with _on(dev):
        nbytes = lib.voge_fragment_bwd_workspace_bytes(B * N)
        ws = _workspace(dev, nbytes)
        out = (B * H, W, K, _p(ws), nbytes, _p(g0), _p(g1), _stream())
        if mode == 0:
            rc = lib.voge_fragment_bwd(_p(p0), _p(p1), _p(rays), *slots, B * N, *out)
        else:
            rc = lib.voge_fragment_bwd_iso(_p(records), _p(p1), int(shared), sigma_mode, _p(rays), *slots, B, N, *out)
    _lib.check(rc, "voge_fragment_bwd")
    return g0, g1


def _sweep(mode, p0, p1, origin, shared, sigma_mode, rays, fwd, B, N, H, W, K, thr_act, occ, sel_idx, sel_len, act, dsd, cnt,
           weight, valid, records):
    """The fine sweep of _trace_inputs' forms with the composite in its epilogue (voge_fragments_fwd / _iso / _iso_view), or, with
    None in act, dsd, weight and valid, the trace alone (the same entries; mode 0: voge_trace_lean_fwd)."""
    lib = _lib.load()
    dev = rays.device
    with _on(dev):
        nbytes = lib.voge_trace_workspace_bytes(B, N, H, W)
        ws = _workspace(dev, nbytes)
        cones = _p(cones_of(rays, B, H, W))
        if mode == 0 and weight is None:
            rc = lib.voge_trace_lean_fwd(_p(p0), _p(p1), _p(rays), _p(fwd), cones, B, N, H, W, K, float(thr_act), _p(ws), nbytes,
                                         _p(sel_idx), _p(sel_len), _p(cnt), _p(records), _stream())
        else:
            tail = (B, N, H, W, K, float(thr_act), float(occ), _p(ws), nbytes, _p(sel_idx), _p(sel_len), _p(act), _p(dsd), _p(cnt),
                    _p(weight), _p(valid))
            if mode == 2:
                rc = lib.voge_fragments_fwd_iso_view(_p(p0), _p(p1), _p(origin), int(shared), int(sigma_mode), _p(rays), _p(fwd), cones,
                                                     *tail, _p(records), _stream())
            elif mode == 1:
                rc = lib.voge_fragments_fwd_iso(_p(p0), _p(p1), _p(rays), _p(fwd), cones, *tail, _p(records), _stream())
            else:
                rc = lib.voge_fragments_fwd(_p(p0), _p(p1), _p(rays), _p(fwd), cones, *tail, _stream())
    _lib.check(rc, "voge_fragments_fwd")


class _Fragments(torch.autograd.Function):
    """Trace + composite in one launch chain (voge_fragments_fwd*): what GaussianRenderer.forward needs from
    ray_tracing (RayTracing.py:12-30) followed by aggregation (Aggregation.py:82-107).
    forward(mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode, occ)
        -> weight, sel_idx, valid_num, sel_len | cnt, records, act, dsd  (the call's bookkeeping, non-differentiable)
    with the Gaussians in one of _trace_inputs' forms (mode 0 general 3x3, 1 A = a I, 2 the renderer's preamble folded in).
    The backward is ONE pass over the fragments (voge_fragment_bwd*: the composite's closed form and the trace's chain
    rule, nothing exchanged through memory) for whatever gradient reaches the weights and vert_hit_length -- the
    reference's training loops differentiate through interpolate_attr + get_silhouette (demo/ShapeFitting.py:217,295).
    Only a caller that needs the gradient of the RAYS takes the stand-alone composite + trace backward kernels."""

    @staticmethod
    def forward(ctx, mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode, occ):
        p0_c, p1_c, o_c, rays_c, fwd, B, N, H, W, shared = _trace_inputs(mode, p0, p1, origin, rays, cam_fwd)
        K, dev = int(n_assign), rays_c.device
        sel_idx = torch.empty((B, H, W, K), dtype=torch.int32, device=dev)
        sel_len = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
        weight = torch.empty_like(sel_len)
        # scalar sigmas: act / dsd are not materialised at all -- every consumer re-derives them from the records
        # (composite forward, fused backward) or asks for them once (_act_dsd: the three-kernel backward)
        lean = (mode != 0 and B * N < (1 << 26)      # (32-bit byte offsets of the record gathers)
                and os.environ.get("VOGE_FRAGMENTS_KEEP_ACT_DSD", "0") != "1")
        sel_act = None if lean else torch.empty_like(sel_len)
        sel_dsd = None if lean else torch.empty_like(sel_len)
        cnt = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        valid = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        # scalar forms: the per-Gaussian (centred mean, a) records outlive the call -- the fused backward reads them
        records = torch.empty((B * N, 4), dtype=torch.float32, device=dev) if mode != 0 else None
        _sweep(mode, p0_c, p1_c, o_c, shared, sigma_mode, rays_c, fwd, B, N, H, W, K, thr_act, occ, sel_idx, sel_len, sel_act, sel_dsd,
               cnt, weight, valid, records)
        ctx.save_for_backward(p0_c, p1_c, rays_c, sel_len, weight)
        # (only tensors that are NOT differentiable outputs of this node may hang on ctx as plain attributes: an output
        # with a grad_fn kept here would close the cycle ctx -> tensor -> grad_fn -> ctx and leave the frame's buffers to
        # the cyclic garbage collector)
        ctx.origin, ctx.sel_idx, ctx.cnt, ctx.records = o_c, sel_idx, cnt, records
        ctx.act_dsd = [sel_act, sel_dsd]
        ctx.meta = (int(mode), int(sigma_mode), bool(shared), float(occ), B, N)
        _tag_index(sel_idx, cnt, B * N)
        ctx.idx_version = sel_idx._version      # (an index list edited through torch afterwards may hold a Gaussian TWICE in a pixel)
        ctx.mark_non_differentiable(sel_idx, valid, cnt)
        if records is not None:
            ctx.mark_non_differentiable(records)
        if sel_act is not None:
            ctx.mark_non_differentiable(sel_act, sel_dsd)
        ctx.set_materialize_grads(False)
        return weight, sel_idx, valid, sel_len, cnt, records, sel_act, sel_dsd

    @staticmethod
    def backward(ctx, g_weight, _g_idx, _g_valid, g_hitlen, *_unused):
        p0, p1, rays, ln, weight = ctx.saved_tensors
        mode, sigma_mode, shared, occ, B, N = ctx.meta
        if g_weight is None and g_hitlen is None:      # nothing reached the fragments (e.g. _ShadeThrough took the frame)
            return (None,) * 10
        sel_idx, cnt = ctx.sel_idx, ctx.cnt
        if mode == 2 and ctx.needs_input_grad[3]:
            raise _lib.VogeHipError("the fused view form has no gradient for the camera centre; "
                                    "use ray_tracing_iso on centred vertices")
        # (the one-pass kernel adds a pixel's slots to its table without arbitration -- a pixel's Gaussians are distinct
        #  as the trace wrote them.  A list somebody edited through torch since is no longer known to be: it takes the stand-alone
        #  kernels, whose table elects one writer per key)
        edited = sel_idx._version != ctx.idx_version
        if not (ctx.needs_input_grad[4] or THREE_KERNEL_BACKWARD or B * N >= (1 << 26) or edited):
            # ONE pass (fragment_bwd.hip, SRC = 1): no act / dsd arrays, no g_len / g_act / g_dsd
            act, dsd = ctx.act_dsd
            g0, g1 = _fragment_bwd(mode, p0, p1, ctx.records, shared, sigma_mode, rays, sel_idx, cnt, B, N, (p0, p1), weight, act, ln,
                                   dsd, g_weight, g_hitlen, occ)
            return None, g0, g1, None, None, None, None, None, None, None
        act, dsd = _act_dsd(ctx.act_dsd, ctx.records, rays, sel_idx, ln, cnt, B * N)
        if g_weight is None:
            g_act, g_len, g_dsd = torch.zeros_like(act), torch.zeros_like(act), torch.zeros_like(act)
        else:
            g_act, g_len, g_dsd = _composite_bwd(act, ln, dsd, weight, cnt, g_weight, occ)
        if g_hitlen is not None:      # vert_hit_length is the trace's len itself (Aggregation.py:107)
            g_len = g_len + _dev(g_hitlen, torch.float32, "grad_hit_length")
        g0, g1, g_ray = _trace_bwd(mode, p0, p1, ctx.origin, shared, sigma_mode, rays, sel_idx, cnt, g_len, g_act, g_dsd,
                                   ctx.needs_input_grad[4])
        return None, g0, g1, None, g_ray, None, None, None, None, None


def _act_dsd(cell, records, rays, idx, ln, cnt, P):
    """act / dsd of a fragments() call: what it kept (cell = [act, dsd]), or (scalar sigmas) derived now from its records
    -- once; the arrays then stay in the cell."""
    if cell[0] is None:
        lib = _lib.load()
        act, dsd = torch.empty_like(ln), torch.empty_like(ln)
        K = idx.shape[-1]
        with _on(ln.device):
            rc = lib.voge_fragment_act_dsd_iso(_p(records), _p(rays), _p(idx), _p(ln), _p(cnt), idx.numel() // K, K, P,
                                               _p(act), _p(dsd), _stream())
        _lib.check(rc, "voge_fragment_act_dsd_iso")
        cell[0], cell[1] = act, dsd
    return cell[0], cell[1]


def fragments(mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode=0, occ=1.0):
    """-> weight, sel_idx, valid_num, sel_len.  The weight tensor carries `voge_through`: the inputs and bookkeeping
    of this call (detached: nothing in it has a grad_fn), which lets a later to_colored_background(fragments, colors)
    run shade + composite + trace backward as ONE kernel (_ShadeThrough)."""
    weight, sel_idx, valid, sel_len, cnt, records, sel_act, sel_dsd = _Fragments.apply(
        mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode, occ)
    if (p0.requires_grad or p1.requires_grad) and torch.is_grad_enabled():
        B = rays.shape[0]
        N = p0.shape[-2] if mode == 2 else p0.shape[0] // max(B, 1)
        rays_d, len_d = rays.detach(), sel_len.detach()      # (same storage and version counter, no grad_fn)
        weight.voge_through = dict(
            mode=int(mode), sigma_mode=int(sigma_mode), shared=bool(mode == 2 and p0.dim() == 2), occ=float(occ), B=B, N=N,
            records=records, rays=rays_d, act=sel_act, dsd=sel_dsd, len=len_d, cnt=cnt, idx=sel_idx,
            sigmas=p1.detach(), means=p0.detach(), p0=p0, p1=p1, rays_requires_grad=bool(rays.requires_grad),
            versions=(weight._version, len_d._version, rays_d._version, sel_idx._version))
    return weight, sel_idx, valid, sel_len


# ----------------------------------------------------------------------------------------------------------------------
# Deferred composite (scalar sigmas).  GaussianRenderer hands its Fragments back before anybody knows what they will be
# used for; the sweep's outputs (index, len, hit count, records) are all the later stages need.  With VOGE_LAZY_COMPOSITE
# (default on) the renderer therefore stops behind the sweep (_TraceLean) and the composite runs when the fragments'
# weights are first asked for:
#   * to_colored_background on untouched fragments -> _CompositeShade: weights AND image in ONE pass (the composite kernel
#     gathers the colours of the slots it holds anyway; nothing is read back);
#   * any other access (frag.vert_weight, interpolate_attr, get_silhouette, ...) -> _CompositeLean: the composite kernel alone.
# Results are the same bits as the eager chain's weights; the image's sums are associated per lane group instead of per
# DPP row (within 1e-7 of the separate kernel).  Both nodes take the Gaussians as inputs and hand them the gradient of
# everything below (composite + trace backward in one pass), like _ShadeThrough.
LAZY_COMPOSITE = os.environ.get("VOGE_LAZY_COMPOSITE", "1") != "0"


class _TraceLean(torch.autograd.Function):
    """The fine trace alone, without act / dsd (_sweep's trace-only form):
    forward(mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode) -> sel_idx, sel_len, cnt, records (mode 0: the
    packed (mu, A)).  backward: only vert_hit_length can carry a gradient here (voge_fragment_bwd* with g_weight = NULL)."""

    @staticmethod
    def forward(ctx, mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode):
        p0_c, p1_c, o_c, rays_c, fwd, B, N, H, W, shared = _trace_inputs(mode, p0, p1, origin, rays, cam_fwd)
        K, dev = int(n_assign), rays_c.device
        sel_idx = torch.empty((B, H, W, K), dtype=torch.int32, device=dev)
        sel_len = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
        cnt = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        records = torch.empty((B * N, 12 if mode == 0 else 4), dtype=torch.float32, device=dev)
        _sweep(mode, p0_c, p1_c, o_c, shared, sigma_mode, rays_c, fwd, B, N, H, W, K, thr_act, 1.0, sel_idx, sel_len, None, None, cnt,
               None, None, records)
        ctx.save_for_backward(p0_c, p1_c, rays_c, sel_len)
        ctx.sel_idx, ctx.cnt, ctx.records = sel_idx, cnt, records
        ctx.meta = (int(mode), int(sigma_mode), bool(shared), B, N)
        _tag_index(sel_idx, cnt, B * N)
        ctx.mark_non_differentiable(sel_idx, cnt, records)
        ctx.set_materialize_grads(False)
        return sel_idx, sel_len, cnt, records

    @staticmethod
    def backward(ctx, _g_idx, g_len, _g_cnt, _g_rec):
        if g_len is None:
            return (None,) * 9
        p0, p1, rays, ln = ctx.saved_tensors
        mode, sigma_mode, shared, B, N = ctx.meta
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[3]:
            raise _lib.VogeHipError("deferred-composite fragments carry no gradient for the rays / the camera centre; "
                                    "VOGE_LAZY_COMPOSITE=0 (or rays that require grad at render time) selects the eager chain")
        # (g_weight = NULL: u = 0 everywhere, the `weight` operand is read but multiplies zero -- len stands in)
        g0, g1 = _fragment_bwd(mode, p0, p1, ctx.records, shared, sigma_mode, rays, ctx.sel_idx, ctx.cnt, B, N, (p0, p1), ln, None, ln,
                               None, None, g_len, 1.0)
        return None, g0, g1, None, None, None, None, None, None


def _plain(t_, dtype, name):
    """_dev for an input the call only READS through its pointer: no torch op may see it (a `.contiguous()` on a parameter would
    put a node into the graph of a call that has none)."""
    if not t_.is_cuda:
        raise _lib.VogeHipError(f"{name} is on {t_.device}: the VoGE hot path runs on a HIP device only (no CPU fallback)")
    if t_.dtype != dtype or not t_.is_contiguous():
        t_ = t_.detach().to(dtype).contiguous()
    return t_


def _sigma_kind(sigmas):
    """(kind, shared) of a general sigma tensor: kind 1 = per-axis [.., N, 3], kind 2 = [.., N, 3, 3] (_GeneralPreamble's rule)."""
    kind = 2 if tuple(sigmas.shape[-2:]) == (3, 3) and sigmas.dim() >= 3 else 1
    return kind, sigmas.dim() == (3 if kind == 2 else 2)


def _plain16(t_, name):
    """_plain for an array the kernels read with 16-byte loads (a view into a larger buffer may start anywhere)."""
    t_ = _plain(t_, torch.float32, name)
    return t_ if t_.data_ptr() % 16 == 0 else t_.detach().clone()


def _frame_trace(verts, sigmas, R, T, focal, pp, band, W, behind, thr_act, n_assign, sigma_mode, occ, origin_out, gen, quats=None):
    """frame_trace (gen False: voge_frame_trace_fwd_iso), frame_trace_gen (gen True: voge_frame_trace_fwd_gen) and frame_trace_ori
    (quats given, sigmas = the scales: voge_frame_trace_fwd_ori)."""
    lib = _lib.load()
    v_c, s_c = _plain(verts, torch.float32, "verts"), _plain(sigmas, torch.float32, "sigmas")
    R_c, T_c = _plain(R, torch.float32, "R"), _plain(T, torch.float32, "T")
    f_c, p_c = _plain(focal, torch.float32, "focal_length"), _plain(pp, torch.float32, "principal_point")
    B = R_c.shape[0]
    row0, h, stripe_h, pitch = band
    shared = v_c.dim() == 2
    N, K, dev = v_c.shape[-2], int(n_assign), v_c.device
    assert R_c.shape == (B, 3, 3) and T_c.shape == (B, 3) and f_c.shape == (B, 2) and p_c.shape == (B, 2)
    assert v_c.shape[-1] == 3 and (shared or v_c.shape[0] == B)
    if quats is not None:
        q_c = _plain16(quats, "quats")
        shared_s = s_c.dim() == 2
        assert tuple(s_c.shape[-2:]) == (N, 3) and q_c.shape == s_c.shape[:-1] + (4,) and (shared_s or s_c.shape[0] == B)
        assert sigma_mode in (1, 2)
        nrec, form = 12, (0, int(sigma_mode), False, (3, int(shared), int(shared_s)))      # (kind 2's records; gen[0] 3: oriented)
    elif gen:
        kind, shared_s = _sigma_kind(s_c)
        assert s_c.shape[-(kind + 1)] == N and s_c.shape[-1] == 3 and (shared_s or s_c.shape[0] == B)
        nrec, form = (8 if kind == 1 else 12), (0, 0, False, (kind, int(shared), int(shared_s)))      # (kind 1: compact per-axis records)
    else:
        assert s_c.shape == v_c.shape[:-1]
        nrec, form = 4, (2, int(sigma_mode), shared, None)
    empty = torch.empty
    sel_idx = empty((B, h, W, K), dtype=torch.int32, device=dev)
    sel_len = empty((B, h, W, K), dtype=torch.float32, device=dev)
    cnt = empty((B, h, W), dtype=torch.int32, device=dev)
    records = empty((B * N, nrec), dtype=torch.float32, device=dev)
    rays = empty((B, h, W, 3), dtype=torch.float32, device=dev)
    with _on(dev):
        nbytes = lib.voge_trace_workspace_bytes(B, N, h, W)
        ws = _workspace(dev, nbytes)
        cam = (R_c.data_ptr(), T_c.data_ptr(), f_c.data_ptr(), p_c.data_ptr(), int(row0), int(stripe_h), int(pitch), int(bool(behind)), B,
               N, int(h), int(W), K, float(thr_act), ws.data_ptr(), nbytes, sel_idx.data_ptr(), sel_len.data_ptr(), cnt.data_ptr(),
               records.data_ptr(), rays.data_ptr(), _p(origin_out), _stream())
        if quats is not None:
            rc = lib.voge_frame_trace_fwd_ori(v_c.data_ptr(), s_c.data_ptr(), q_c.data_ptr(), int(shared), int(shared_s), int(sigma_mode), *cam)
        elif gen:
            rc = lib.voge_frame_trace_fwd_gen(v_c.data_ptr(), s_c.data_ptr(), int(shared), int(shared_s), kind, *cam)
        else:
            rc = lib.voge_frame_trace_fwd_iso(v_c.data_ptr(), s_c.data_ptr(), int(shared), int(sigma_mode), *cam)
    if rc:
        _lib.check(rc, "voge_frame_trace_fwd")
    _tag_index(sel_idx, cnt, B * N)
    lz = LazyComposite.__new__(LazyComposite)      # (slots assigned directly: the cheapest construction, once a frame)
    lz.mode, lz.sigma_mode, lz.shared, lz.gen = form
    (lz.occ, lz.B, lz.N, lz.K, lz.p0, lz.p1, lz.sel_idx, lz.sel_len, lz.cnt, lz.records, lz.rays, lz.rays_version, lz.grad_mode,
     lz.idx_version, lz.p0_version, lz.frame) = (float(occ), B, N, K, verts, sigmas, sel_idx, sel_len, cnt, records, rays, 0,
                                                 torch.is_grad_enabled(), sel_idx._version, verts._version, True)
    lz.p2 = quats
    lz.p12_version = None if quats is None else (sigmas._version, quats._version)
    return sel_idx, sel_len, lz


def frame_trace(verts, sigmas, R, T, focal, pp, band, W, behind, thr_act, n_assign, sigma_mode, occ, origin_out=None):
    """Round 6: the renderer's forward up to the sweep with the CAMERA as input (voge_frame_trace_fwd_iso): no ray-generation
    launch and no autograd node at all -- the trace's three kernels make rays, cones, camera centre and view axis from
    (R, T, focal, pp) themselves, with the ray kernel's own operations, and the sweep leaves the bundle behind for the composite
    and the backward.  verts [N,3] | [B,N,3], sigmas [N] | [B,N], R [B,3,3], T [B,3], focal [B,2], pp [B,2], band = (row0, h,
    stripe_h, pitch).  Fixed cameras only (callers that optimise the camera take pixel_rays + the rays-taking entries).
    origin_out: None | a contiguous fp32 [B,3] tensor that receives the camera centres.
    -> (sel_idx, sel_len, LazyComposite): sel_len carries NO grad_fn here; whoever reads Fragments.vert_hit_length gets a
    differentiable alias on demand (LazyComposite.hit_length, _HitLength) -- the weights' consumers never pay for that node."""
    return _frame_trace(verts, sigmas, R, T, focal, pp, band, W, behind, thr_act, n_assign, sigma_mode, occ, origin_out, False)


def frame_trace_gen(verts, sigmas, R, T, focal, pp, band, W, behind, thr_act, n_assign, occ, origin_out=None):
    """frame_trace for (N,3) / (N,3,3) sigmas (voge_frame_trace_fwd_gen): the camera AND the user's own arrays go in -- the record
    pass centres the vertices and expands 2 * sigma itself (Renderer.py:130-137: no ray launch, no preamble launch, no autograd
    node).  verts [N,3] | [B,N,3]; sigmas [N,3] | [N,3,3] | [B,N,3] | [B,N,3,3].  -> (sel_idx, sel_len, LazyComposite) with
    mode 0, lz.gen = (kind, shared_verts, shared_sigmas) and lz.p0 / lz.p1 the USER's tensors: every backward route of such
    fragments goes through voge_frame_bwd_gen, which hands the gradients to exactly those."""
    return _frame_trace(verts, sigmas, R, T, focal, pp, band, W, behind, thr_act, n_assign, 0, occ, origin_out, True)


def frame_trace_ori(verts, scales, quats, R, T, focal, pp, band, W, behind, thr_act, n_assign, sigma_mode, occ, origin_out=None):
    """frame_trace_gen for ORIENTED Gaussians (voge_frame_trace_fwd_ori): verts [N,3] | [B,N,3], scales [N,3] | [B,N,3], quats
    [N,4] | [B,N,4] = (w, x, y, z), not necessarily unit -- the record pass builds A = R diag(d) R^T (sigma_mode 1: d = 2 s;
    2, inverse_sigma: d = 2 / s) into kind 2's records, so the composite is the [N,3,3] frame's.  -> (sel_idx, sel_len,
    LazyComposite) with mode 0, lz.gen = (3, shared_verts, shared_sigmas) and lz.p0 / lz.p1 / lz.p2 the USER's verts / scales /
    quats: every backward route goes through voge_frame_bwd_ori, which hands the gradients to exactly those.  The kernels read a
    quaternion with one 16-byte load: a quats tensor whose storage does not start on a 16-byte boundary (a view into a larger
    buffer) is copied, once here and once in every backward (_plain16) -- any tensor torch allocated itself is read in place."""
    return _frame_trace(verts, scales, R, T, focal, pp, band, W, behind, thr_act, n_assign, sigma_mode, occ, origin_out, True, quats)


def _frame_gen_bwd(lz, form, attr, weight, ad, ln, rgb, wsum, bg, thr, g, gs0, gs1, g_hitlen, acc=None):
    """voge_frame_bwd_gen on fragments of frame_trace_gen (frame_trace_ori: voge_frame_bwd_ori): -> (g_p0, g_p1, g_p2 | None,
    g_attr | None), the gradients of the user's verts / sigmas (oriented: scales, quats) and attributes.  acc: the accumulator the
    composite zeroed on its way (good for one call), or None (scratch, filled here)."""
    lz.check()
    lib = _lib.load()
    kind, shared_v, shared_s = lz.gen
    dev = ln.device
    B, H, W = lz.cnt.shape
    K, P = lz.K, lz.B * lz.N
    g0 = torch.empty(lz.p0.shape, dtype=torch.float32, device=dev)
    g1 = torch.empty(lz.p1.shape, dtype=torch.float32, device=dev)
    g_attr = None if attr is None else torch.empty_like(attr)
    g2 = None
    C, Nattr = (0, 0) if attr is None else (attr.shape[1], attr.shape[0])
    with _on(dev):
        zeroed = acc is not None
        if acc is None:
            nbytes = lib.voge_frame_bwd_gen_acc_bytes(P)
            acc = _workspace(dev, nbytes)
        else:
            nbytes = acc.numel()
        tail = (_p(lz.rays), _p(attr), _p(lz.sel_idx), _p(lz.cnt), _p(weight), _p(ad[0]), _p(ln), _p(ad[1]), _p(rgb), _p(wsum), _p(bg),
                float(thr), _p(g), gs0, gs1, _p(g_hitlen), lz.occ, lz.B, lz.N, B * H, W, K, C, Nattr, _p(acc), nbytes, int(zeroed), _p(g0),
                _p(g1))
        if kind == 3:
            g2 = torch.empty(lz.p2.shape, dtype=torch.float32, device=dev)
            rc = lib.voge_frame_bwd_ori(form, _p(lz.records), _p(_plain(lz.p1, torch.float32, "scales")), _p(_plain16(lz.p2, "quats")),
                                        shared_v, shared_s, lz.sigma_mode, *tail, _p(g2), _p(g_attr), _stream())
        else:
            rc = lib.voge_frame_bwd_gen(form, _p(lz.records), shared_v, shared_s, kind, *tail, _p(g_attr), _stream())
    _lib.check(rc, "voge_frame_bwd_ori" if kind == 3 else "voge_frame_bwd_gen")
    return g0, g1, g2, g_attr


class _HitLength(torch.autograd.Function):
    """Fragments.vert_hit_length of the camera-input trace as a differentiable tensor (the reference's is: the trace's len itself,
    Aggregation.py:107): forward(verts, sigmas, sel_len, lz) -> an alias of sel_len with this node behind it; backward: the
    trace's chain rule for a gradient of len alone (the weights' backward with g_weight = NULL), as _TraceLean.backward."""

    @staticmethod
    def forward(ctx, p0, p1, sel_len, lz, p2=None):
        ctx.lz = lz
        ctx.save_for_backward(p1)
        ctx.set_materialize_grads(False)
        return sel_len.view_as(sel_len)

    @staticmethod
    def backward(ctx, g_len):
        if g_len is None:
            return None, None, None, None, None
        lz = ctx.lz
        (p1,) = ctx.saved_tensors
        if lz.gen is None:      # (general forms read their records: the user's sigmas are not an operand)
            p1 = _dev(p1, torch.float32, "sigmas")
        # (`weight` is read but multiplies zero -- len stands in; the trace-only form's absorptivity 1.0)
        g0, g1, g2 = _lazy_fragment_bwd(lz, p1, lz.sel_len, lz.sel_len, None, g_len=g_len, occ=1.0)
        return g0, g1, None, None, g2


# VOGE_FRAME_PATH=0 (or ops.FRAME_PATH = False): the renderer generates its ray bundle with voge_rays_fwd and traces through the
# rays-taking entries (round 5's chain); VOGE_FRAME_DIRECT_BWD=0: the frame's backward fills its accumulator itself.  Same results.
FRAME_PATH = os.environ.get("VOGE_FRAME_PATH", "1") != "0"
FRAME_DIRECT_BWD = os.environ.get("VOGE_FRAME_DIRECT_BWD", "1") != "0"


def frame_eligible(verts, sigmas, R, T, focal, pp, n_assign, numel):
    """The camera-input frame path: scalar sigmas on the device, fixed cameras, a non-empty band, 32-bit record offsets."""
    if not (LAZY_COMPOSITE and FRAME_PATH) or n_assign > _lib.MAX_K or os.environ.get("VOGE_FRAGMENTS_KEEP_ACT_DSD", "0") == "1":
        return False
    if not (verts.is_cuda and sigmas.is_cuda) or numel == 0 or verts.shape[-2] == 0:
        return False
    if sigmas.dim() != verts.dim() - 1 and not (sigmas.dim() >= 2 and sigmas.shape[-1] == 3 and sigmas.dtype == torch.float32):
        return False      # (scalar sigmas [N] | [B,N], or the general forms [.., N, 3] / [.., N, 3, 3])
    dev = verts.device
    if R.device != dev or T.device != dev or focal.device != dev or pp.device != dev:      # (fixed cameras: cameras.camera_tensors)
        return False
    return R.shape[0] * verts.shape[-2] < (1 << 26)


class LazyComposite:
    """What the deferred composite needs from a _TraceLean call (nothing in it has a grad_fn except sel_len, which the
    composite nodes take as an input)."""
    __slots__ = ("mode", "sigma_mode", "shared", "occ", "B", "N", "K", "p0", "p1", "sel_idx", "sel_len", "cnt", "records", "rays",
                 "rays_version", "grad_mode", "idx_version", "p0_version", "frame", "gen", "p2", "p12_version")

    def __init__(self, **kw):
        self.frame = False      # (made by frame_trace: the shade stage may take the frame entries of ABI 7)
        self.gen = None         # (frame_trace_gen: (kind, shared_verts, shared_sigmas) -- p0 / p1 are the USER's verts / sigmas)
        self.p2 = None          # (frame_trace_ori: gen = (3, ..), p1 the USER's scales, p2 the USER's quaternions)
        self.p12_version = None
        for k, v in kw.items():
            setattr(self, k, v)

    def hit_length(self):
        """Fragments.vert_hit_length: sel_len itself, or (frame_trace, whose sel_len has no grad_fn) its differentiable alias,
        made on first request under the render call's autograd mode."""
        if not self.frame:
            return self.sel_len
        # (NOT remembered here: the alias' grad_fn holds this object -- the Fragments that asked keeps what it gets)
        if self.grad_mode and self.wants_grad():
            with torch.enable_grad():
                return _HitLength.apply(self.p0, self.p1, self.sel_len, self, self.p2)
        return self.sel_len

    def wants_grad(self):
        return self.p0.requires_grad or self.p1.requires_grad or (self.p2 is not None and self.p2.requires_grad)

    def means(self):
        """(general forms) the centres as the trace saw them: contiguous fp32, no grad_fn."""
        assert self.gen is None, "fragments of frame_trace_gen keep the USER's vertices: their backward reads the records"
        return _dev(self.p0.detach(), torch.float32, "means")

    def usable(self):
        """The sweep's outputs must still be what it wrote (nobody edited them through torch in between)."""
        return (self.sel_len._version == 0 and self.rays._version == self.rays_version
                and hit_count_of(self.sel_idx) is not None)

    def check(self):
        """Backward-time guard: what the kernels read outside save_for_backward must be what the forward saw."""
        if self.rays._version != self.rays_version:
            raise RuntimeError("the rays were modified in place after the fragments were traced: the backward would read the "
                               "changed values (as autograd's own check for saved tensors)")
        if self.sel_idx._version != self.idx_version:
            raise RuntimeError("vert_index was modified in place after the fragments were traced: the backward would read the "
                               "changed values (as autograd's own check for saved tensors)")
        if self.mode == 0 and self.p0._version != self.p0_version:
            raise RuntimeError("the Gaussians' centres were modified in place after the fragments were traced (an optimizer "
                               "step between forward and backward?): the backward would read the changed values")
        if self.p12_version is not None and self.p12_version != (self.p1._version, self.p2._version):
            raise RuntimeError("the Gaussians' scales or quaternions were modified in place after the fragments were traced: the "
                               "backward's finishing pass would read the changed values")

    def grad(self):
        """The autograd mode the RENDER ran under, for whoever composites these fragments later: the reference computes the
        weights inside the renderer call, so reading them first under torch.no_grad() (a feature-bank update, logging) must
        neither drop the graph of a later loss nor build one for fragments rendered without."""
        return torch.set_grad_enabled(self.grad_mode)

    def through(self, weight):
        """Tag freshly composited weights the way fragments() does (a later to_colored_background takes _ShadeThrough).  The
        bookkeeping is filled in when somebody first LOOKS at it (_Through): the frame that never does pays for no detach."""
        # (fragments of frame_trace_gen carry the user's own verts / sigmas: _ShadeThrough's entry points want the centred means
        #  and the expanded forms -- such weights stay untagged and a later to_colored_background takes the ordinary nodes)
        if (self.p0.requires_grad or self.p1.requires_grad) and self.grad_mode and self.gen is None:
            weight.voge_through = _Through(self, weight)
        return weight


class _Through(dict):
    """The `voge_through` bookkeeping of deferred-composite weights (see fragments()), materialised on first lookup.  The version
    counters are read when the object is made -- that is what "untouched since" refers to."""

    def __init__(self, lz, weight):
        dict.__init__(self)
        # (this object hangs on `weight` itself: it must not hold the tensor, or every frame's buffers would wait for the cyclic
        #  collector -- and the allocator would hipMalloc new ones meanwhile: 0.3 ms of host per frame when it happened)
        self._src = (lz, getattr(weight, "voge_act_dsd", (None, None)),      # (general forms: what the composite kept)
                     (weight._version, lz.sel_len._version, lz.rays._version, lz.sel_idx._version))

    def _fill(self):
        lz, (act, dsd), versions = self._src
        self._src = None
        len_d = lz.sel_len.detach()
        self.update(mode=lz.mode, sigma_mode=lz.sigma_mode, shared=lz.shared, occ=lz.occ, B=lz.B, N=lz.N, records=lz.records,
                    rays=lz.rays, act=act, dsd=dsd, len=len_d, cnt=lz.cnt, idx=lz.sel_idx, sigmas=lz.p1.detach(), means=lz.p0.detach(),
                    p0=lz.p0, p1=lz.p1, rays_requires_grad=False, versions=versions)

    def __missing__(self, key):
        if self._src is None:
            raise KeyError(key)
        self._fill()
        return dict.__getitem__(self, key)


def _general_act_dsd(lz, sel_len, need):
    """(act, dsd) buffers the general composite fills for its backward (VOGE_GENERAL_KEEP_ACT_DSD=0: none -- the backward
    re-derives them from the packed records, 19 us slower at the cfg3 size); scalar-sigma fragments never keep them."""
    if lz.mode != 0 or os.environ.get("VOGE_GENERAL_KEEP_ACT_DSD", "1") == "0" or not need or (lz.gen is not None and lz.gen[0] == 1):
        return (None, None)      # (per-axis sigmas on the frame path: re-derived from their 32-byte records, three coefficients)
    return (torch.empty_like(sel_len), torch.empty_like(sel_len))


def _lazy_fragment_bwd(lz, p1, weight, ln, g_weight, ad=(None, None), g_len=None, occ=None):
    """_fragment_bwd on deferred-composite fragments (frame_trace_gen's: voge_frame_bwd_gen) -> (g_p0, g_p1, g_p2 | None).  occ: the
    absorptivity the kernel is handed (default lz.occ)."""
    if lz.gen is not None:
        gw, gs_pix, gs_k = _grad_weight_layout(g_weight, lz.K)
        gh = None if g_len is None else _dev(g_len, torch.float32, "grad_hit_length")
        g0, g1, g2, _ = _frame_gen_bwd(lz, 2, None, weight, ad, ln, None, None, None, -1.0, gw, gs_pix, gs_k, gh)
        return g0, g1, g2
    lz.check()
    return (*_fragment_bwd(lz.mode, lz.means() if lz.mode == 0 else None, p1, lz.records, lz.shared, lz.sigma_mode, lz.rays, lz.sel_idx,
                           lz.cnt, lz.B, lz.N, (lz.p0, lz.p1), weight, ad[0], ln, ad[1], g_weight, g_len, lz.occ if occ is None else occ), None)


def _frame_acc(lz, need, per=None):
    """(round 6) Fragments of the camera-input trace: the accumulator of the coming backward, allocated by the forward whose launch
    zeroes it on its way -- no fill launch in front of that backward (voge_frame_*_bwd_*).  None when that does not apply.
    per: bytes per Gaussian of an entry with a layout of its own (the depth form: 16, no colour term)."""
    if lz.frame and need and lz.K <= 128 and FRAME_DIRECT_BWD:
        if per is None:
            per = 32 if lz.gen is None else (48 if lz.gen[0] == 1 else 64)
        return torch.empty((lz.B * lz.N * per,), dtype=torch.uint8, device=lz.sel_idx.device)
    return None


def _composite_fwd(lz, sel_len, need, attr=None, bg=None, thr=-1.0, rgb=None, img=None, wsum=None, sil=None, acc=None):
    """The deferred composite from the sweep's records in ONE launch -> (weight, valid_num, (act, dsd)): the weights alone, or with
    attr also the merged attributes rgb, their weight sum and (bg given) the image.  The frame entries also write the silhouette sil
    and zero the accumulator acc (_frame_acc); (act, dsd) is what the general composite keeps for its backward (_general_act_dsd,
    need: whether a backward may run), left on the weights as voge_act_dsd."""
    lib = _lib.load()
    idx, K = lz.sel_idx, lz.K
    npix = idx.numel() // K
    C, Nattr = (0, 0) if attr is None else (attr.shape[1], attr.shape[0])
    nacc = 0 if acc is None else acc.numel()
    weight = torch.empty_like(sel_len)
    valid = torch.empty(idx.shape[:-1], dtype=torch.int64, device=idx.device)
    with _on(idx.device):
        ad = _general_act_dsd(lz, sel_len, need)
        src = (_p(idx), _p(lz.cnt), _p(sel_len), _p(lz.records), _p(lz.rays), lz.occ)
        args = src + (_p(attr), _p(bg), float(thr), npix, K, C, Nattr, _p(weight), _p(valid), _p(rgb), _p(img), _p(wsum))
        if lz.gen is not None:
            rc = lib.voge_frame_shade_fwd_rec(1 if lz.gen[0] == 1 else 2, *args, _p(sil), _p(ad[0]), _p(ad[1]), _p(acc), nacc, _stream())
        elif attr is None and lz.mode == 0:
            rc = lib.voge_composite_fwd_rec(*src, npix, K, _p(weight), _p(valid), _p(ad[0]), _p(ad[1]), _stream())
        elif attr is None:
            rc = lib.voge_composite_fwd_iso(*src, npix, K, _p(weight), _p(valid), _stream())
        elif lz.mode == 0:
            rc = lib.voge_composite_shade_fwd_rec(*args, _p(ad[0]), _p(ad[1]), _stream())
        elif sil is not None or acc is not None:
            rc = lib.voge_frame_shade_fwd_iso(*args, _p(sil), _p(acc), nacc, _stream())
        else:
            rc = lib.voge_composite_shade_fwd_iso(*args, _stream())
    _lib.check(rc, "voge_composite_fwd (from the records)")
    weight.voge_act_dsd = ad
    return weight, valid, ad


class _CompositeLean(torch.autograd.Function):
    """aggregation (VoGE/Aggregation.py:82-107) of a _TraceLean call, when the weights are first asked for:
    forward(p0, p1, sel_len, lz) -> weight, valid_num.  The Gaussians are inputs so that the backward (composite + trace,
    one pass: voge_fragment_bwd_iso) can hand them the gradient directly; sel_len gets none from here."""

    @staticmethod
    def forward(ctx, p0, p1, sel_len, lz, p2=None):
        weight, valid, ctx.ad = _composite_fwd(lz, sel_len, any(ctx.needs_input_grad))
        ctx.save_for_backward(_dev(p1, torch.float32, "sigmas"), sel_len, weight)
        ctx.lz = lz
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return weight, valid

    @staticmethod
    def backward(ctx, g_weight, _g_valid):
        if g_weight is None:
            return None, None, None, None, None
        p1, ln, weight = ctx.saved_tensors
        g0, g1, g2 = _lazy_fragment_bwd(ctx.lz, p1, weight, ln, g_weight, ctx.ad)
        return g0, g1, None, None, g2


def _shade_bwd(mode, means, sigmas, records, shared, sigma_mode, rays, cnt, occ, B, N, like, attr, idx, weight, act, ln, dsd, rgb,
               wsum, bg, thr, go, gs_pix, gs_c, acc=None):
    """The image's gradient go (strides gs_pix, gs_c: _grad_layout) through shade + composite + trace in ONE kernel -> (g0, g1, g_attr),
    g0 / g1 shaped like like[0] / like[1]: voge_fragment_shade_bwd (mode 0: the means), _iso (the records), or, on the accumulator
    acc that the forward zeroed (_frame_acc), voge_frame_shade_bwd_iso."""
    lib = _lib.load()
    _, H, W, K = idx.shape
    Nattr, C = attr.shape
    dev = idx.device
    g_attr = torch.empty_like(attr)
    g0 = torch.empty(like[0].shape, dtype=torch.float32, device=dev)
    g1 = torch.empty(like[1].shape, dtype=torch.float32, device=dev)
    image = (_p(rgb), _p(wsum), _p(bg), thr, _p(go), gs_pix, gs_c, occ)
    sizes = (B * H, W, K, C, Nattr)
    grads = (_p(g0), _p(g1), _p(g_attr))
    with _on(dev):
        if acc is not None:
            rc = lib.voge_frame_shade_bwd_iso(_p(records), _p(sigmas), int(shared), sigma_mode, _p(rays), _p(attr), _p(idx), _p(cnt),
                                              _p(weight), _p(ln), *image, B, N, *sizes, _p(acc), acc.numel(), *grads, _stream())
        else:
            nbytes = lib.voge_fragment_bwd_workspace_bytes(B * N)
            ws = _workspace(dev, nbytes)
            slots = (_p(attr), _p(idx), _p(cnt), _p(weight), _p(act), _p(ln), _p(dsd), *image)
            if mode == 0:
                rc = lib.voge_fragment_shade_bwd(_p(means), _p(sigmas), _p(rays), *slots, B * N, *sizes, _p(ws), nbytes, *grads, _stream())
            else:
                rc = lib.voge_fragment_shade_bwd_iso(_p(records), _p(sigmas), int(shared), sigma_mode, _p(rays), *slots, B, N, *sizes,
                                                     _p(ws), nbytes, *grads, _stream())
    _lib.check(rc, "voge_fragment_shade_bwd")
    return g0, g1, g_attr


class _CompositeShade(torch.autograd.Function):
    """aggregation + merge_final + get_silhouette + to_colored_background in ONE forward pass
    (voge_composite_shade_fwd_iso): forward(attr, p0, p1, sel_len, lz, bg, thr) -> image, weight, valid_num.
    backward: the image's gradient through voge_fragment_shade_bwd_iso (shade + composite + trace, one kernel); a gradient
    that reaches the weights from elsewhere (a silhouette loss on the same fragments) through voge_fragment_bwd_iso."""

    @staticmethod
    def forward(ctx, attr, p0, p1, sel_len, lz, bg, thr, p2=None):
        attr_c = _dev(attr, torch.float32, "colors")
        bg_c = _dev(bg, torch.float32, "background_color")
        idx = lz.sel_idx
        Nattr, C = attr_c.shape
        assert bg_c.numel() == C
        check_index_range(idx, Nattr)
        rgb = torch.empty(idx.shape[:-1] + (C,), dtype=torch.float32, device=idx.device)
        img = torch.empty_like(rgb)
        wsum = torch.empty(idx.shape[:-1], dtype=torch.float32, device=idx.device)
        ctx.gbuf = _frame_acc(lz, any(ctx.needs_input_grad[:3]) or ctx.needs_input_grad[-1])
        weight, valid, ctx.ad = _composite_fwd(lz, sel_len, any(ctx.needs_input_grad), attr_c, bg_c, thr, rgb, img, wsum, acc=ctx.gbuf)
        ctx.save_for_backward(attr_c, _dev(p1, torch.float32, "sigmas"), sel_len, weight, rgb, bg_c, wsum)
        ctx.lz, ctx.thr = lz, float(thr)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return img, weight, valid

    @staticmethod
    def backward(ctx, g_img, g_weight, _g_valid):
        attr, p1, ln, weight, rgb, bg, wsum = ctx.saved_tensors
        lz = ctx.lz
        lz.check()
        g_attr = g0 = g1 = g2 = None
        if g_img is not None:
            go, gs_pix, gs_c = _grad_layout(g_img, attr.shape[1])
            gbuf, ctx.gbuf = ctx.gbuf, None      # (zeroed by the forward, good for ONE backward: a second one takes the scratch form)
            if lz.gen is not None:      # (general forms of the frame path: the user's verts / sigmas get their gradients directly)
                g0, g1, g2, g_attr = _frame_gen_bwd(lz, 0, attr, weight, ctx.ad, ln, rgb, wsum, bg, ctx.thr, go, gs_pix, gs_c, None, acc=gbuf)
            else:
                g0, g1, g_attr = _shade_bwd(lz.mode, lz.means() if lz.mode == 0 else None, p1, lz.records, lz.shared, lz.sigma_mode,
                                            lz.rays, lz.cnt, lz.occ, lz.B, lz.N, (lz.p0, lz.p1), attr, lz.sel_idx, weight, ctx.ad[0], ln,
                                            ctx.ad[1], rgb, wsum, bg, ctx.thr, go, gs_pix, gs_c, gbuf)
        if g_weight is not None:
            h0, h1, h2 = _lazy_fragment_bwd(lz, p1, weight, ln, g_weight, ctx.ad)
            g0, g1, g2 = (h0, h1, h2) if g0 is None else (g0 + h0, g1 + h1, None if h2 is None else g2 + h2)
        need = ctx.needs_input_grad
        return ((g_attr if need[0] else None), (g0 if need[1] else None), (g1 if need[2] else None), None, None, None, None,
                (g2 if need[7] else None))


def _merge_bwd(lz, p1, attr, weight, ad, ln, go, gs_pix, gs_c, gws, wsum_fwd, acc):
    """The gradients of the merged attributes (go: _grad_layout) and of their weight sum (gws) through merge + composite + trace in
    ONE kernel -> (g0, g1, g_attr): voge_fragment_merge_bwd (mode 0), _iso, or, on the accumulator acc that the forward zeroed,
    voge_frame_merge_bwd_iso -- which also takes the silhouette's gradient as gws, with the forward's sums wsum_fwd."""
    lib = _lib.load()
    idx = lz.sel_idx
    B, H, W, K = idx.shape
    Nattr, C = attr.shape
    dev = idx.device
    g_attr = torch.empty_like(attr)
    g0 = torch.empty(lz.p0.shape, dtype=torch.float32, device=dev)
    g1 = torch.empty(lz.p1.shape, dtype=torch.float32, device=dev)
    grad = (_p(go), gs_pix, gs_c, _p(gws))
    sizes = (B * H, W, K, C, Nattr)
    grads = (_p(g0), _p(g1), _p(g_attr))
    with _on(dev):
        if acc is not None:
            rc = lib.voge_frame_merge_bwd_iso(_p(lz.records), _p(p1), int(lz.shared), lz.sigma_mode, _p(lz.rays), _p(attr), _p(idx),
                                              _p(lz.cnt), _p(weight), _p(ln), *grad, _p(wsum_fwd), lz.occ, lz.B, lz.N, *sizes, _p(acc),
                                              acc.numel(), *grads, _stream())
        else:
            nbytes = lib.voge_fragment_bwd_workspace_bytes(lz.B * lz.N)
            ws = _workspace(dev, nbytes)
            slots = (_p(attr), _p(idx), _p(lz.cnt), _p(weight), _p(ad[0]), _p(ln), _p(ad[1]), *grad, lz.occ)
            if lz.mode == 0:
                rc = lib.voge_fragment_merge_bwd(_p(lz.means()), _p(p1), _p(lz.rays), *slots, lz.B * lz.N, *sizes, _p(ws), nbytes, *grads,
                                                 _stream())
            else:
                rc = lib.voge_fragment_merge_bwd_iso(_p(lz.records), _p(p1), int(lz.shared), lz.sigma_mode, _p(lz.rays), *slots, lz.B,
                                                     lz.N, *sizes, _p(ws), nbytes, *grads, _stream())
    _lib.check(rc, "voge_fragment_merge_bwd")
    return g0, g1, g_attr


class _CompositeMerge(torch.autograd.Function):
    """aggregation + merge_final (interpolate_attr) + the per-pixel weight sum in ONE forward pass
    (voge_composite_shade_fwd_iso without a background): forward(attr, p0, p1, sel_len, lz) -> merged attributes,
    weight sum, weight, valid_num.  get_silhouette on the same fragments is min(weight sum, 1), so the reference's training
    pattern -- interpolate_attr + get_silhouette (demo/ShapeFitting.py:217-222) -- is this one kernel forward and ONE
    kernel backward (voge_fragment_merge_bwd_iso: merge backward + the sum's gradient + composite + trace)."""

    @staticmethod
    def forward(ctx, attr, p0, p1, sel_len, lz, p2=None):
        attr_c = _dev(attr, torch.float32, "vert_attr")
        idx = lz.sel_idx
        Nattr, C = attr_c.shape
        check_index_range(idx, Nattr)
        rgb = torch.empty(idx.shape[:-1] + (C,), dtype=torch.float32, device=idx.device)
        wsum = torch.empty(idx.shape[:-1], dtype=torch.float32, device=idx.device)
        # (frame path: the composite writes get_silhouette = min(weight sum, 1) next to the sum, a differentiable OUTPUT of this
        #  node -- the training pattern's silhouette costs no launch forward and none backward: see backward)
        sil = torch.empty_like(wsum) if lz.frame else None
        ctx.gbuf = _frame_acc(lz, any(ctx.needs_input_grad[:3]) or ctx.needs_input_grad[-1])
        weight, valid, ctx.ad = _composite_fwd(lz, sel_len, any(ctx.needs_input_grad), attr_c, None, -1.0, rgb, None, wsum, sil, ctx.gbuf)
        ctx.save_for_backward(attr_c, _dev(p1, torch.float32, "sigmas"), sel_len, weight, wsum)
        ctx.lz = lz
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return rgb, wsum, weight, valid, sil

    @staticmethod
    def backward(ctx, g_rgb, g_wsum, g_weight, _g_valid, g_sil=None):
        attr, p1, ln, weight, wsum = ctx.saved_tensors
        lz = ctx.lz
        lz.check()
        idx = lz.sel_idx
        C = attr.shape[1]
        g_attr = g0 = g1 = g2 = None
        # the silhouette's gradient: handed to the fused kernel as it is (with the forward's sums, which say where min(sum, 1)
        # passes it on) when that kernel runs on the forward's accumulator; any other combination turns it into the sum's own
        wsum_fwd = None
        if g_sil is not None:
            if g_wsum is None and (ctx.gbuf is not None or lz.gen is not None):
                g_wsum, wsum_fwd = g_sil, wsum
            else:
                passed = g_sil * torch.where(wsum < 1, 1.0, torch.where(wsum == 1, 0.5, 0.0))
                g_wsum = passed if g_wsum is None else g_wsum + passed
        if g_rgb is not None or g_wsum is not None:
            if g_rgb is None:
                g_rgb = torch.zeros(idx.shape[:-1] + (C,), dtype=torch.float32, device=idx.device)
            go, gs_pix, gs_c = _grad_layout(g_rgb, C)
            gws = None if g_wsum is None else _dev(g_wsum, torch.float32, "grad_weight_sum")
            gbuf, ctx.gbuf = ctx.gbuf, None      # (zeroed by the forward, good for ONE backward)
            if lz.gen is not None:
                g0, g1, g2, g_attr = _frame_gen_bwd(lz, 1, attr, weight, ctx.ad, ln, wsum_fwd, gws, None, -1.0, go, gs_pix, gs_c, None, acc=gbuf)
            else:
                g0, g1, g_attr = _merge_bwd(lz, p1, attr, weight, ctx.ad, ln, go, gs_pix, gs_c, gws, wsum_fwd, gbuf)
        if g_weight is not None:
            h0, h1, h2 = _lazy_fragment_bwd(lz, p1, weight, ln, g_weight, ctx.ad)
            g0, g1, g2 = (h0, h1, h2) if g0 is None else (g0 + h0, g1 + h1, None if h2 is None else g2 + h2)
        need = ctx.needs_input_grad
        return (g_attr if need[0] else None), (g0 if need[1] else None), (g1 if need[2] else None), None, None, (g2 if need[5] else None)


def composite_merge(lz, attr):
    """-> merged attributes, weight sum, weight, valid_num; or None when the one-pass form does not apply."""
    K = lz.K
    if K > 128 or attr.dim() != 2 or attr.shape[1] not in (3, 4) or attr.numel() >= (1 << 30) or not lz.usable():
        return None
    if os.environ.get("VOGE_SHADE_THROUGH", "1") == "0":
        return None
    with lz.grad():
        rgb, wsum, weight, valid, sil = _CompositeMerge.apply(attr, lz.p0, lz.p1, lz.sel_len, lz, lz.p2)
    return rgb, wsum, lz.through(weight), valid, sil


class _CompositeDepth(torch.autograd.Function):
    """aggregation + get_depth + the per-pixel weight sum + get_silhouette in ONE forward pass (voge_frame_depth_fwd_iso: the frame's
    composite with the depth stage instead of a colour table): forward(p0, p1, sel_len, lz, normalize, background) -> depth,
    weight sum, weight, valid_num, silhouette.  The backward is ONE fused launch (voge_frame_depth_bwd_iso: the two per-pixel
    scalars of the depth's gradient are formed inside the kernel, the silhouette's gradient folds into one of them, then composite
    + trace) on the accumulator the forward zeroed.  Scalar-sigma fragments of the frame path only (composite_depth)."""

    @staticmethod
    def forward(ctx, p0, p1, sel_len, lz, normalize, background, p2=None):
        lib = _lib.load()
        idx, K = lz.sel_idx, lz.K
        dev = idx.device
        depth = torch.empty(idx.shape[:-1], dtype=torch.float32, device=dev)
        wsum, sil = torch.empty_like(depth), torch.empty_like(depth)
        weight = torch.empty_like(sel_len)
        valid = torch.empty(idx.shape[:-1], dtype=torch.int64, device=dev)
        ctx.gbuf = acc = _frame_acc(lz, any(ctx.needs_input_grad[:2]), 16)
        with _on(dev):
            rc = lib.voge_frame_depth_fwd_iso(_p(idx), _p(lz.cnt), _p(sel_len), _p(lz.records), _p(lz.rays), lz.occ, int(normalize),
                                              float(background), idx.numel() // K, K, _p(weight), _p(valid), _p(depth), _p(wsum), _p(sil),
                                              _p(acc), 0 if acc is None else acc.numel(), _stream())
        _lib.check(rc, "voge_frame_depth_fwd_iso")
        weight.voge_act_dsd = (None, None)
        ctx.save_for_backward(_dev(p1, torch.float32, "sigmas"), sel_len, weight, depth, wsum)
        ctx.lz, ctx.normalize = lz, bool(normalize)
        ctx.mark_non_differentiable(valid, wsum)
        ctx.set_materialize_grads(False)
        return depth, wsum, weight, valid, sil

    @staticmethod
    def backward(ctx, g_depth, _g_wsum, g_weight, _g_valid, g_sil):
        p1, ln, weight, depth, wsum = ctx.saved_tensors
        lz = ctx.lz
        lz.check()
        g0 = g1 = None
        if g_depth is not None or g_sil is not None:
            lib = _lib.load()
            idx = lz.sel_idx
            B, H, W, K = idx.shape
            dev = idx.device
            gd, gs_pix = None, 0
            if g_depth is not None:
                gd, gs_pix, _ = _grad_layout(g_depth, 1)
            gs = None if g_sil is None else _dev(g_sil, torch.float32, "grad_silhouette")
            acc, ctx.gbuf = ctx.gbuf, None      # (zeroed by the forward, good for ONE backward: a second one zeroes its own)
            if acc is None:
                acc = torch.zeros((lz.B * lz.N * 16,), dtype=torch.uint8, device=dev)
            g0 = torch.empty(lz.p0.shape, dtype=torch.float32, device=dev)
            g1 = torch.empty(lz.p1.shape, dtype=torch.float32, device=dev)
            with _on(dev):
                rc = lib.voge_frame_depth_bwd_iso(_p(lz.records), _p(p1), int(lz.shared), lz.sigma_mode, _p(lz.rays), _p(idx), _p(lz.cnt),
                                                  _p(weight), _p(ln), _p(depth), _p(wsum), _p(gd), gs_pix, _p(gs), int(ctx.normalize),
                                                  lz.occ, lz.B, lz.N, B * H, W, K, _p(acc), acc.numel(), _p(g0), _p(g1), _stream())
            _lib.check(rc, "voge_frame_depth_bwd_iso")
        if g_weight is not None:
            h0, h1, _ = _lazy_fragment_bwd(lz, p1, weight, ln, g_weight)
            g0, g1 = (h0, h1) if g0 is None else (g0 + h0, g1 + h1)
        need = ctx.needs_input_grad
        return (g0 if need[0] else None), (g1 if need[1] else None), None, None, None, None, None


def composite_depth(lz, normalize, background):
    """-> depth, weight sum, weight, valid_num, silhouette of deferred-composite fragments in one pass (_CompositeDepth); or None
    when the one-pass form does not apply (anything but scalar sigmas on the frame path, K > 128, edited fragments)."""
    if not (lz.frame and lz.gen is None) or lz.K > 128 or not lz.usable():
        return None
    if os.environ.get("VOGE_SHADE_THROUGH", "1") == "0":
        return None
    with lz.grad():
        depth, wsum, weight, valid, sil = _CompositeDepth.apply(lz.p0, lz.p1, lz.sel_len, lz, normalize, background, lz.p2)
    return depth, wsum, lz.through(weight), valid, sil


def trace_lean(mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode=0, occ=1.0):
    """-> (sel_idx, sel_len, LazyComposite): the renderer's forward up to the sweep; the composite is deferred."""
    sel_idx, sel_len, cnt, records = _TraceLean.apply(mode, p0, p1, origin, rays, cam_fwd, thr_act, n_assign, sigma_mode)
    B = rays.shape[0]
    N = p0.shape[-2] if mode == 2 else p0.shape[0] // max(B, 1)
    rays_d = rays.detach()
    lz = LazyComposite(mode=int(mode), sigma_mode=int(sigma_mode), shared=bool(mode == 2 and p0.dim() == 2), occ=float(occ), B=B, N=N,
                       K=int(n_assign), p0=p0, p1=p1, sel_idx=sel_idx, sel_len=sel_len, cnt=cnt, records=records, rays=rays_d,
                       rays_version=rays_d._version, grad_mode=torch.is_grad_enabled(), idx_version=sel_idx._version,
                       p0_version=p0._version)
    return sel_idx, sel_len, lz


def lazy_eligible(mode, p0, p1, origin, rays, n_assign):
    """Deferred composite: record gathers in 32-bit offsets, nobody differentiating the rays.  (mode 0 = full 3x3 forms,
    VOGE_LAZY_GENERAL=0 keeps those on the eager chain with act / dsd.)"""
    if not LAZY_COMPOSITE or os.environ.get("VOGE_FRAGMENTS_KEEP_ACT_DSD", "0") == "1":
        return False
    if mode == 0 and os.environ.get("VOGE_LAZY_GENERAL", "1") == "0":
        return False
    B = rays.shape[0]
    P = p0.shape[-2] * B if mode == 2 else p0.shape[0]
    if P >= (1 << 26) or P == 0 or rays.numel() == 0 or rays.requires_grad or (origin is not None and origin.requires_grad):
        return False
    return p0.is_cuda and rays.is_cuda


def composite_lean(lz):
    """-> weight, valid_num of a deferred composite (the weights carry `voge_through` like fragments()' do)."""
    with lz.grad():
        weight, valid = _CompositeLean.apply(lz.p0, lz.p1, lz.sel_len, lz, lz.p2)
    return lz.through(weight), valid


def composite_shade(lz, attr, bg, thr):
    """-> image, weight, valid_num, or None when the one-pass form does not apply (K % 4, channel count, offsets)."""
    K = lz.K
    if K > 128 or attr.dim() != 2 or attr.shape[1] not in (3, 4) or attr.numel() >= (1 << 30) or not lz.usable():
        return None      # (K <= 128: the image's backward is voge_fragment_shade_bwd_iso)
    if os.environ.get("VOGE_SHADE_THROUGH", "1") == "0":
        return None
    if torch.is_grad_enabled() == lz.grad_mode:      # (the usual case: no mode switch to pay for)
        img, weight, valid = _CompositeShade.apply(attr, lz.p0, lz.p1, lz.sel_len, lz, bg, thr, lz.p2)
    else:
        with lz.grad():
            img, weight, valid = _CompositeShade.apply(attr, lz.p0, lz.p1, lz.sel_len, lz, bg, thr, lz.p2)
    return img, lz.through(weight), valid


def _shade_fwd(attr, weight, idx, valid_num, bg, thr):
    """interpolate_attr + get_silhouette + to_colored_background of composited fragments, one kernel (voge_shade_fwd)
    -> (attr, weight, valid_num, bg as the kernel read them; rgb, img, wsum)."""
    lib = _lib.load()
    attr_c = _dev(attr, torch.float32, "colors")
    w = _dev(weight, torch.float32, "weight")
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()):
        raise _lib.VogeHipError("vert_index must be a contiguous int32 tensor on the HIP device")
    vn = _dev(valid_num, torch.int64, "valid_num")
    bg_c = _dev(bg, torch.float32, "background_color")
    K = idx.shape[-1]
    Nattr, C = attr_c.shape
    assert C <= 4 and bg_c.numel() == C
    check_index_range(idx, Nattr)
    rgb = torch.empty(idx.shape[:-1] + (C,), dtype=torch.float32, device=idx.device)
    img = torch.empty_like(rgb)
    wsum = torch.empty(idx.shape[:-1], dtype=torch.float32, device=idx.device)
    with _on(idx.device):
        rc = lib.voge_shade_fwd(_p(attr_c), _p(idx), _p(w), _p(vn), _p(bg_c), float(thr), idx.numel() // max(K, 1), K, C, Nattr, 1,
                                _p(rgb), _p(img), None, _p(wsum), _stream())
    _lib.check(rc, "voge_shade_fwd")
    return attr_c, w, vn, bg_c, rgb, img, wsum


class _ShadeThrough(torch.autograd.Function):
    """to_colored_background on fragments this renderer made: the forward is _Shade's, the
    backward runs shade -> composite -> trace as ONE kernel (voge_fragment_shade_bwd_iso for scalar sigmas,
    voge_fragment_shade_bwd for full 3x3 forms) and hands the gradients
    straight to the colours AND to the Gaussians' (verts | means, sigmas | a), which are inputs of this node for that
    purpose; the weights get no gradient from here.  Every stage is linear in the gradient of the weights, so whatever
    else consumes the same weights (a silhouette loss, a second image) still flows through _Fragments.backward and the
    contributions add up in the parameters' .grad exactly as with separate nodes."""

    @staticmethod
    def forward(ctx, attr, weight, p0, p1, th, idx, valid_num, bg, thr):
        attr_c, w, _, bg_c, rgb, img, wsum = _shade_fwd(attr, weight, idx, valid_num, bg, thr)
        ctx.save_for_backward(attr_c, w, rgb, bg_c, wsum)
        ctx.th, ctx.idx, ctx.thr = th, idx, float(thr)
        return img

    @staticmethod
    def backward(ctx, g_img):
        attr, w, rgb, bg, wsum = ctx.saved_tensors
        th, idx = ctx.th, ctx.idx
        # what the kernel reads outside save_for_backward must still be what the forward saw
        if (th["len"]._version, th["rays"]._version) != th["versions"][1:3]:
            raise RuntimeError("vert_hit_length or the rays were modified in place after to_colored_background: "
                               "the fused backward would read the changed values (as autograd's own check for saved tensors)")
        go, gs_pix, gs_c = _grad_layout(g_img, attr.shape[1])
        g0, g1, g_attr = _shade_bwd(th["mode"], th["means"], th["sigmas"], th["records"], th["shared"], th["sigma_mode"], th["rays"],
                                    th["cnt"], th["occ"], th["B"], th["N"], (th["p0"], th["p1"]), attr, idx, w, th["act"], th["len"],
                                    th["dsd"], rgb, wsum, bg, ctx.thr, go, gs_pix, gs_c)
        need = ctx.needs_input_grad
        return (g_attr if need[0] else None), None, (g0 if need[2] else None), (g1 if need[3] else None), None, None, None, None, None


def through_of(fragments_weight, idx):
    """The bookkeeping fragments() left on the weights, if it still describes (fragments_weight, idx): same memory, not
    modified through torch since.  None otherwise."""
    th = getattr(fragments_weight, "voge_through", None)
    if th is None:
        return None
    tidx = th["idx"]
    if idx is not tidx and not (idx.data_ptr() == tidx.data_ptr() and idx.numel() == tidx.numel() and idx.is_contiguous()
                                and idx.dtype == tidx.dtype):
        return None
    v = th["versions"]
    if fragments_weight._version != v[0] or th["len"]._version != v[1] or th["rays"]._version != v[2] or tidx._version != v[3]:
        return None
    return th


def shade_through(attr, fragments_weight, idx, valid_num, bg, thr):
    """The fused-backward form of shade() when `fragments_weight` still is the untouched output of fragments() (K <= 128,
    <= 4 channels, nobody watching the weights' own gradient); None otherwise.  VOGE_SHADE_THROUGH=0 disables it (e.g. to
    take torch.autograd.grad with respect to the weights themselves: this node hands them no gradient)."""
    if not torch.is_grad_enabled() or os.environ.get("VOGE_SHADE_THROUGH", "1") == "0":
        return None
    th = through_of(fragments_weight, idx)
    if th is None:
        return None
    K = idx.shape[-1]
    if K > 128 or attr.dim() != 2 or attr.shape[1] > 4 or th["cnt"] is None:
        return None
    if fragments_weight.retains_grad or fragments_weight._backward_hooks or th["rays_requires_grad"]:
        return None
    if th["B"] * th["N"] >= (1 << 26) or attr.numel() >= (1 << 30):      # 32-bit byte offsets of the kernel's gathers
        return None
    img = _ShadeThrough.apply(attr, fragments_weight, th["p0"], th["p1"], th, th["idx"], valid_num, bg, thr)
    return img if idx is th["idx"] else img.view(idx.shape[:-1] + (attr.shape[1],))


class _Composite(torch.autograd.Function):
    """Fused replacement of get_cross_activation + assign2weight (VoGE/Aggregation.py:30-79)
    and of their autograd backward.  (sel_idx, sel_act, sel_len, sel_dsd, occ) -> weight, valid_num."""

    @staticmethod
    def forward(ctx, sel_idx, sel_act, sel_len, sel_dsd, occ):
        lib = _lib.load()
        idx = _dev(sel_idx, torch.int32, "sel_idx")
        # the trace forward leaves its per-pixel hit count on the index tensor it returns
        # (voge_hit_count): valid_num then needs no pass over idx
        # (ignored when sel_idx was edited through torch since: hit_count_of compares the version counter)
        cnt = hit_count_of(sel_idx) if idx is sel_idx else None
        act = _dev(sel_act, torch.float32, "sel_act")
        ln = _dev(sel_len, torch.float32, "sel_len")
        dsd = _dev(sel_dsd, torch.float32, "sel_dsd")
        K = idx.shape[-1]
        npix = idx.numel() // max(K, 1)
        act, ln, dsd = (_comp_aligned(x, K) for x in (act, ln, dsd))
        weight = torch.empty_like(act)
        valid = torch.empty(idx.shape[:-1], dtype=torch.int64, device=idx.device)
        with _on(idx.device):
            rc = lib.voge_composite_fwd(_p(idx), _p(cnt), _p(act), _p(ln), _p(dsd), float(occ), npix, K, _p(weight),
                                        _p(valid), _stream())
        _lib.check(rc, "voge_composite_fwd")
        ctx.save_for_backward(act, ln, dsd, weight)
        ctx.cnt = cnt      # the trace's hit count (or None): lets the backward skip empty slots / pixels
        ctx.occ = float(occ)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return weight, valid

    @staticmethod
    def backward(ctx, g_weight, _g_valid):
        if g_weight is None:
            return None, None, None, None, None
        act, ln, dsd, weight = ctx.saved_tensors
        g_act, g_len, g_dsd = _composite_bwd(act, ln, dsd, weight, ctx.cnt, g_weight, ctx.occ)
        return None, g_act, g_len, g_dsd, None


class _Merge(torch.autograd.Function):
    """merge_final (VoGE/Aggregation.py:111-141): (attr [N,C], weight, idx, valid_num) -> [..., C].
    Mutates idx in place (-1 -> 0) exactly like the reference (:131)."""

    @staticmethod
    def forward(ctx, attr, weight, idx, valid_num):
        lib = _lib.load()
        attr_c = _dev(attr, torch.float32, "vert_attr")
        w = _dev(weight, torch.float32, "weight")
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()):
            raise _lib.VogeHipError("vert_index must be a contiguous int32 tensor on the HIP device")
        vn = _dev(valid_num, torch.int64, "valid_num")
        K = idx.shape[-1]
        npix = idx.numel() // max(K, 1)
        Nattr, C = attr_c.shape
        check_index_range(idx, Nattr)
        out = torch.empty(idx.shape[:-1] + (C,), dtype=torch.float32, device=idx.device)
        with _on(idx.device):
            rc = lib.voge_merge_fwd(_p(attr_c), _p(idx), _p(w), _p(vn), npix, K, C, Nattr, 1, _p(out), _stream())
        _lib.check(rc, "voge_merge_fwd")
        # idx is an int tensor outside autograd; it is kept as a plain attribute because the in-place
        # fix (-1 -> 0) may be re-applied by later merges of the same fragments.  The backward masks by
        # valid_num and reads a negative index as 0, so it is insensitive to whether the fix has run.
        ctx.save_for_backward(attr_c, w, vn)
        ctx.idx = idx
        ctx.needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        attr, w, vn = ctx.saved_tensors
        idx = ctx.idx
        K = idx.shape[-1]
        npix = idx.numel() // max(K, 1)
        Nattr, C = attr.shape
        go = _dev(g_out, torch.float32, "grad_out")
        g_attr = torch.empty_like(attr) if ctx.needs[0] else None
        g_w = torch.empty_like(w) if ctx.needs[1] else None
        with _on(idx.device):
            Wd = idx.shape[-2] if idx.dim() >= 3 else npix
            rc = lib.voge_merge_bwd(_p(attr), _p(idx), _p(w), _p(vn), _p(go), npix // max(Wd, 1), Wd, K, C, Nattr,
                                    _p(g_attr), _p(g_w), _stream())
        _lib.check(rc, "voge_merge_bwd")
        return g_attr, g_w, None, None


class _Blend(torch.autograd.Function):
    """get_silhouette + to_colored_background (VoGE/Renderer.py:157-171)."""

    @staticmethod
    def forward(ctx, rgb, weight, bg, thr):
        lib = _lib.load()
        rgb_c = _dev(rgb, torch.float32, "rgb")
        w = _dev(weight, torch.float32, "weight")
        bg_c = _dev(bg, torch.float32, "background_color")
        K = w.shape[-1]
        C = rgb_c.shape[-1]
        npix = w.numel() // max(K, 1)
        assert bg_c.numel() == C and rgb_c.numel() == npix * C
        out = torch.empty_like(rgb_c)
        with _on(w.device):
            rc = lib.voge_blend_fwd(_p(rgb_c), _p(w), _p(bg_c), float(thr), npix, K, C, _p(out), None, _stream())
        _lib.check(rc, "voge_blend_fwd")
        ctx.save_for_backward(rgb_c, w, bg_c)
        ctx.thr = float(thr)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        rgb, w, bg = ctx.saved_tensors
        K = w.shape[-1]
        C = rgb.shape[-1]
        npix = w.numel() // max(K, 1)
        go = _dev(g_out, torch.float32, "grad_out")
        g_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        with _on(w.device):
            rc = lib.voge_blend_bwd(_p(rgb), _p(w), _p(bg), ctx.thr, _p(go), npix, K, C, _p(g_rgb), _p(g_w), _stream())
        _lib.check(rc, "voge_blend_bwd")
        return g_rgb, g_w, None, None


class _Shade(torch.autograd.Function):
    """interpolate_attr + get_silhouette + to_colored_background in one kernel each way
    (VoGE/Renderer.py:153-171, VoGE/Aggregation.py:111-141); attr has <= 4 channels."""

    @staticmethod
    def forward(ctx, attr, weight, idx, valid_num, bg, thr):
        attr_c, w, vn, bg_c, rgb, img, wsum = _shade_fwd(attr, weight, idx, valid_num, bg, thr)
        ctx.save_for_backward(attr_c, w, vn, rgb, bg_c, wsum)
        ctx.idx = idx      # see _Merge: kept outside the version counter on purpose
        ctx.thr = float(thr)
        return img

    @staticmethod
    def backward(ctx, g_img):
        lib = _lib.load()
        attr, w, vn, rgb, bg, wsum = ctx.saved_tensors
        idx = ctx.idx
        K = idx.shape[-1]
        npix = idx.numel() // max(K, 1)
        Nattr, C = attr.shape
        go = _dev(g_img, torch.float32, "grad_image")
        g_attr = torch.empty_like(attr) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        Wd = idx.shape[-2] if idx.dim() >= 3 else npix
        with _on(idx.device):
            rc = lib.voge_shade_bwd(_p(attr), _p(idx), _p(w), _p(vn), _p(rgb), _p(wsum), _p(bg), ctx.thr, _p(go),
                                    npix // max(Wd, 1), Wd, K, C, Nattr, _p(g_attr), _p(g_w), _stream())
        _lib.check(rc, "voge_shade_bwd")
        return g_attr, g_w, None, None, None, None


def _bg_view(bg, shape):
    """bg as the [B,H,W,C] view of bg.expand(shape): strides, never a copy (0 on the broadcast dimensions)."""
    e = bg.expand(shape)
    return e.unsqueeze(0) if e.dim() == 3 else e.reshape((-1,) + tuple(shape[-3:]))


class _BlendBackground(torch.autograd.Function):
    """to_colored_background with a background that broadcasts to the image (VoGE/Renderer.py:162-171 under torch
    broadcasting): forward(rgb [..,H,W,C], s [..,H,W], bg, thr) -> min(rgb + (1 - m) bg, 1), m = min(s, 1) ([m > thr] when
    thr > 0), one launch each way (voge_blend_bg_fwd / _bwd).  bg is read through its broadcast strides; its gradient is
    summed back to bg's own shape without atomics: plain stores when no two pixels share a cell, per-workgroup partials and a
    fixed-order second pass when a view shares one colour, a dense gradient and sum_to_size for anything else."""

    @staticmethod
    def forward(ctx, rgb, s, bg, thr):
        lib = _lib.load()
        rgb_c = _dev(rgb, torch.float32, "rgb")
        s_c = _dev(s, torch.float32, "silhouette")
        img = torch.empty_like(rgb_c)
        ctx.save_for_backward(rgb_c, s_c, bg)
        ctx.thr = float(thr)
        if img.numel() == 0:
            return img
        H, W, C = rgb_c.shape[-3:]
        e = _bg_view(bg, rgb_c.shape)
        with _on(rgb_c.device):
            rc = lib.voge_blend_bg_fwd(_p(rgb_c), _p(s_c), _p(e), *e.stride(), ctx.thr, e.shape[0], H, W, C, _p(img), _stream())
        _lib.check(rc, "voge_blend_bg_fwd")
        return img

    @staticmethod
    def backward(ctx, g_img):
        lib = _lib.load()
        rgb, s, bg = ctx.saved_tensors
        shape = rgb.shape
        need = ctx.needs_input_grad
        g_rgb = torch.empty_like(rgb) if need[0] else None
        g_s = torch.empty_like(s) if need[1] and ctx.thr <= 0 else None      # ([m > thr] passes nothing to the silhouette)
        g_bg = None
        if rgb.numel() == 0:
            return g_rgb, g_s, torch.zeros_like(bg) if need[2] else None, None
        H, W, C = shape[-3:]
        e = _bg_view(bg, shape)
        B = e.shape[0]
        go, gs_pix, gs_c = _grad_layout(g_img, C)
        out, gst, dense, ws, nbytes = None, (0, 0, 0, 0), None, None, 0
        if need[2]:
            bs = (1,) * (len(shape) - bg.dim()) + tuple(bg.shape)      # bg's shape aligned with the image's
            lead, Cg = bs[:-3], bs[-1]
            global_ = all(d == 1 for d in lead)
            if global_ or tuple(lead) == tuple(shape[:-3]):      # (one colour set for every view, or one per view)
                out = torch.empty(bs, dtype=torch.float32, device=rgb.device)
                gst = out.view(1 if global_ else B, bs[-3], bs[-2], Cg).expand(B, H, W, C).stride()
            gb, gh, gw = gst[:3]
            distinct = out is not None and (gb or B == 1) and (gh or H == 1) and (gw or W == 1)
            uniform = out is not None and (gh == 0 or H == 1) and (gw == 0 or W == 1)
            if not (distinct or uniform):
                # (e.g. a [W,C] background, or one [H,W,C] image behind several views): a dense gradient, summed down by torch
                out = dense = torch.empty((B, H, W, Cg), dtype=torch.float32, device=rgb.device)
                gst = dense.expand(B, H, W, C).stride()
            elif not distinct:
                nbytes = lib.voge_blend_bg_bwd_workspace_bytes(B, H, W, C)
                ws = _workspace(rgb.device, nbytes)
        with _on(rgb.device):
            rc = lib.voge_blend_bg_bwd(_p(rgb), _p(s), _p(e), *e.stride(), ctx.thr, _p(go), gs_pix, gs_c, B, H, W, C, _p(g_rgb),
                                       _p(g_s), _p(out), *gst, _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_blend_bg_bwd")
        if dense is not None:
            g_bg = dense.view(tuple(shape[:-1]) + (dense.shape[-1],)).sum_to_size(bs).view(bg.shape)
        elif out is not None:
            g_bg = out.view(bg.shape)
        return g_rgb, g_s, g_bg, None


def blend_background(rgb, s, bg, thr=-1.0):
    """min(rgb + (1 - m) bg, 1) with m = min(s, 1) ([m > thr] when thr > 0): rgb [.., H, W, C] (interpolate_attr), s [.., H, W]
    (get_silhouette), bg a tensor, tuple or list that broadcasts to rgb's shape WITHOUT enlarging it (a background that would
    make the image bigger raises ValueError; the reference returns the bigger image).  Arithmetic in fp32: a CPU or fp64
    background is moved and cast, autograd runs through the cast."""
    if not torch.is_tensor(bg):
        bg = torch.tensor([float(c) for c in bg], dtype=torch.float32)
    if rgb.dim() < 3 or tuple(s.shape) != tuple(rgb.shape[:-1]):
        raise ValueError(f"blend_background: rgb {tuple(rgb.shape)} must be [..., H, W, C] and s {tuple(s.shape)} its [..., H, W]")
    try:
        grown = tuple(torch.broadcast_shapes(bg.shape, rgb.shape)) != tuple(rgb.shape)
    except RuntimeError:
        grown = True
    if grown:
        raise ValueError(f"background_color of shape {tuple(bg.shape)} does not broadcast to the image's shape {tuple(rgb.shape)} "
                         "without enlarging it")
    return _BlendBackground.apply(rgb, s, bg.to(device=rgb.device, dtype=torch.float32), float(thr))


class _Silhouette(torch.autograd.Function):
    """get_silhouette (VoGE/Renderer.py:157-159): min(sum_k w_k, 1).  The backward is one value per pixel
    (g_sil * [sum w < 1]), returned as a [.., K] view with stride 0 along the slots: nothing of size [.., K] is
    written, and voge_fragment_bwd* reads the view in place when the silhouette is the weights' only consumer."""

    @staticmethod
    def forward(ctx, weight):
        lib = _lib.load()
        w = _dev(weight, torch.float32, "weight")
        K = w.shape[-1]
        npix = w.numel() // max(K, 1)
        sil = torch.empty(w.shape[:-1], dtype=torch.float32, device=w.device)
        wsum = torch.empty_like(sil)
        with _on(w.device):
            rc = lib.voge_silhouette_fwd(_p(w), npix, K, _p(sil), _p(wsum), _stream())
        _lib.check(rc, "voge_silhouette_fwd")
        ctx.save_for_backward(wsum)
        ctx.K = K
        return sil

    @staticmethod
    def backward(ctx, g_sil):
        lib = _lib.load()
        (wsum,) = ctx.saved_tensors
        go = _dev(g_sil, torch.float32, "grad_sil")
        g_pix = torch.empty_like(wsum)
        with _on(wsum.device):
            rc = lib.voge_silhouette_bwd(_p(wsum), _p(go), wsum.numel(), _p(g_pix), _stream())
        _lib.check(rc, "voge_silhouette_bwd")
        return g_pix.unsqueeze(-1).expand(*wsum.shape, ctx.K)


class _Depth(torch.autograd.Function):
    """get_depth of composited fragments (extension; voge_depth_fwd / _bwd): forward(weight [.., K], hit_length [.., K], valid_num
    [..], normalize, background) -> depth [..]: sum_{k<n} w_k len_k / sum_{k<n} w_k over the n = min(valid_num, K) live slots
    (`background` where the sum of the weights is not positive), or the un-normalised sum.  The backward hands autograd the
    gradients of the weights and of vert_hit_length, zero in the dead slots."""

    @staticmethod
    def forward(ctx, weight, hit_length, valid_num, normalize, background):
        w = _dev(weight, torch.float32, "weight")
        ln = _dev(hit_length, torch.float32, "vert_hit_length")
        vn = _dev(valid_num, torch.int64, "valid_num")
        lib = _lib.load()
        if ln.shape != w.shape or vn.shape != w.shape[:-1]:
            raise ValueError(f"get_depth: weight {tuple(w.shape)}, vert_hit_length {tuple(ln.shape)} and valid_num {tuple(vn.shape)} "
                             "do not describe the same fragments")
        K = w.shape[-1]
        depth = torch.empty(w.shape[:-1], dtype=torch.float32, device=w.device)
        wsum = torch.empty_like(depth)
        with _on(w.device):
            rc = lib.voge_depth_fwd(_p(w), _p(ln), _p(vn), w.numel() // max(K, 1), K, int(normalize), float(background), _p(depth),
                                    _p(wsum), _stream())
        _lib.check(rc, "voge_depth_fwd")
        ctx.save_for_backward(w, ln, vn, depth, wsum)
        ctx.normalize = bool(normalize)
        return depth

    @staticmethod
    def backward(ctx, g_depth):
        lib = _lib.load()
        w, ln, vn, depth, wsum = ctx.saved_tensors
        K = w.shape[-1]
        gd = _dev(g_depth, torch.float32, "grad_depth")
        g_w, g_len = torch.empty_like(w), torch.empty_like(w)
        with _on(w.device):
            rc = lib.voge_depth_bwd(_p(w), _p(ln), _p(vn), _p(depth), _p(wsum), _p(gd), w.numel() // max(K, 1), K, int(ctx.normalize),
                                    _p(g_w), _p(g_len), _stream())
        _lib.check(rc, "voge_depth_bwd")
        return g_w, g_len, None, None, None


class _Distortion(torch.autograd.Function):
    """get_distortion of composited fragments (extension; voge_distortion_fwd / _bwd): forward(weight [.., K], hit_length [.., K],
    valid_num [..], normalize) -> [..]: sum_i sum_j w_i w_j |t_i - t_j| over the n = min(max(valid_num, 0), K) live slots, or
    that over (sum_k w_k)^2 (0 where the sum is not positive) -- the values of Aggregation.distortion.  One launch each way on the
    current stream; the backward recomputes the prefix scan from the saved inputs and writes every element of both gradients,
    zero in the dead slots (no zero fill, no atomics: the same bits on every run)."""

    @staticmethod
    def forward(ctx, weight, hit_length, valid_num, normalize):
        w = _dev(weight, torch.float32, "weight")
        ln = _dev(hit_length, torch.float32, "vert_hit_length")
        vn = _dev(valid_num, torch.int64, "valid_num")
        lib = _lib.load()
        if ln.shape != w.shape or vn.shape != w.shape[:-1]:
            raise ValueError(f"get_distortion: weight {tuple(w.shape)}, vert_hit_length {tuple(ln.shape)} and valid_num "
                             f"{tuple(vn.shape)} do not describe the same fragments")
        K = w.shape[-1]
        dist = torch.empty(w.shape[:-1], dtype=torch.float32, device=w.device)
        wsum = torch.empty_like(dist)
        with _on(w.device):
            rc = lib.voge_distortion_fwd(_p(w), _p(ln), _p(vn), w.numel() // max(K, 1), K, int(normalize), _p(dist), _p(wsum), _stream())
        _lib.check(rc, "voge_distortion_fwd")
        ctx.save_for_backward(w, ln, vn, dist, wsum)
        ctx.normalize = bool(normalize)
        return dist

    @staticmethod
    def backward(ctx, g_dist):
        lib = _lib.load()
        w, ln, vn, dist, wsum = ctx.saved_tensors
        K = w.shape[-1]
        gd = _dev(g_dist, torch.float32, "grad_distortion")
        g_w, g_len = torch.empty_like(w), torch.empty_like(w)
        with _on(w.device):
            rc = lib.voge_distortion_bwd(_p(w), _p(ln), _p(vn), _p(dist), _p(wsum), _p(gd), w.numel() // max(K, 1), K,
                                         int(ctx.normalize), _p(g_w), _p(g_len), _stream())
        _lib.check(rc, "voge_distortion_bwd")
        return g_w, g_len, None, None


def _aligned16(t_):
    """t_ itself, or a copy whose first element sits on a 16-byte boundary (a slice taken in the middle of a row does not)."""
    return t_ if t_.data_ptr() % 16 == 0 else t_.clone()


class _ShColors(torch.autograd.Function):
    """View-dependent colours (extension; voge_sh_colors_fwd / _bwd): forward(sh [N,M,C], verts [N,3] | [B,N,3], centres [B,3],
    degree, clamp) -> [B*N, C], the values of Aggregation.sh_colors.  One launch each way on the current stream and no allocation
    but the outputs -- except that an `sh` off the 16-byte boundary the kernels' vector loads need is copied (_aligned16); the backward
    recomputes the directions and the clamp mask from the saved INPUTS and writes every element of g_sh and g_verts (no zero
    fill, no atomics: the same bits on every run).  The centres get no gradient here -- Renderer.sh_to_colors sends a centre that
    wants one to the torch definition."""

    @staticmethod
    def forward(ctx, sh, verts, centres, degree, clamp):
        sh = _aligned16(_dev(sh, torch.float32, "sh"))
        verts = _dev(verts, torch.float32, "verts")
        centres = _dev(centres, torch.float32, "cam_center")
        lib = _lib.load()
        N, M, C = sh.shape
        B = centres.shape[0]
        if centres.shape != (B, 3) or tuple(verts.shape) not in ((N, 3), (B, N, 3)):
            raise ValueError(f"sh_colors: sh {tuple(sh.shape)}, verts {tuple(verts.shape)} and cam_center {tuple(centres.shape)} do not "
                             "describe the same Gaussians and views")
        out = torch.empty((B * N, C), dtype=torch.float32, device=sh.device)
        with _on(sh.device):
            rc = lib.voge_sh_colors_fwd(_p(sh), _p(verts), _p(centres), B, N, M, C, degree, int(verts.dim() == 2), int(clamp), _p(out),
                                        _stream())
        _lib.check(rc, "voge_sh_colors_fwd")
        ctx.save_for_backward(sh, verts, centres)
        ctx.degree, ctx.clamp = degree, bool(clamp)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        sh, verts, centres = ctx.saved_tensors
        N, M, C = sh.shape
        B = centres.shape[0]
        go = _dev(g_out, torch.float32, "grad_colors")
        make = torch.zeros_like if B * N == 0 else torch.empty_like      # (nothing is launched for an empty batch)
        g_sh, g_verts = make(sh), make(verts)
        with _on(sh.device):
            rc = lib.voge_sh_colors_bwd(_p(sh), _p(verts), _p(centres), _p(go), B, N, M, C, ctx.degree, int(verts.dim() == 2),
                                        int(ctx.clamp), _p(g_sh), _p(g_verts), _stream())
        _lib.check(rc, "voge_sh_colors_bwd")
        return g_sh, g_verts, None, None, None


class _GaussNormals(torch.autograd.Function):
    """Per-view normals of oriented Gaussians (extension; voge_gauss_normals_fwd / _bwd): forward(scales [N,3] | [B,N,3], quats
    [N,4] | [B,N,4], verts [N,3] | [B,N,3], centres [B,3], inverse_sigma) -> [B*N, 3], the values of Aggregation.gaussian_normals.
    One launch each way on the current stream and no allocation but the outputs (a quats off the 16-byte boundary, such as a view
    at an odd offset into a flat buffer, is read element by element by the kernels: no copy); the backward recomputes the axis
    and the signs from the saved INPUTS and writes every element of g_quats (no zero fill, no atomics: the same bits on every run).
    Only quats get a gradient: the axis and the sign are constants, so scales, verts and centres have none by definition."""

    @staticmethod
    def forward(ctx, scales, quats, verts, centres, inverse_sigma):
        scales = _dev(scales, torch.float32, "scales")
        quats = _dev(quats, torch.float32, "quats")
        verts = _dev(verts, torch.float32, "verts")
        centres = _dev(centres, torch.float32, "cam_center")
        lib = _lib.load()
        B, N = centres.shape[0], scales.shape[-2] if scales.dim() >= 2 else -1
        if (centres.shape != (B, 3) or tuple(scales.shape) not in ((N, 3), (B, N, 3)) or tuple(quats.shape) != tuple(scales.shape[:-1]) + (4,)
                or tuple(verts.shape) not in ((N, 3), (B, N, 3))):
            raise ValueError(f"gauss_normals: scales {tuple(scales.shape)}, quats {tuple(quats.shape)}, verts {tuple(verts.shape)} and "
                             f"cam_center {tuple(centres.shape)} do not describe the same Gaussians and views")
        out = torch.empty((B * N, 3), dtype=torch.float32, device=quats.device)
        ctx.flags = (int(scales.dim() == 2), int(verts.dim() == 2), int(bool(inverse_sigma)))
        with _on(quats.device):
            rc = lib.voge_gauss_normals_fwd(_p(scales), _p(quats), _p(verts), _p(centres), B, N, *ctx.flags, _p(out), _stream())
        _lib.check(rc, "voge_gauss_normals_fwd")
        ctx.save_for_backward(scales, quats, verts, centres)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        lib = _lib.load()
        scales, quats, verts, centres = ctx.saved_tensors
        B, N = centres.shape[0], scales.shape[-2]
        go = _dev(g_out, torch.float32, "grad_normals")
        g_quats = (torch.zeros_like if B * N == 0 else torch.empty_like)(quats)      # (nothing is launched for an empty batch)
        with _on(quats.device):
            rc = lib.voge_gauss_normals_bwd(_p(scales), _p(quats), _p(verts), _p(centres), _p(go), B, N, *ctx.flags, _p(g_quats),
                                            _stream())
        _lib.check(rc, "voge_gauss_normals_bwd")
        return None, g_quats, None, None, None


class _MeshReg(torch.autograd.Function):
    """Mesh regularisers (extension; voge_mesh_reg_fwd / _bwd): forward(verts [V,3] | [B,V,3], topo, target_length, terms) ->
    (edge, laplacian, normal), three 0-dim views of ONE [3] buffer, the values of Aggregation.mesh_edge_term /
    mesh_laplacian_term / mesh_normal_term over the tables of a Losses.MeshTopology on the same device.  terms: bit 0 edge,
    bit 1 laplacian, bit 2 normal; a term that is off is not computed, is an exact 0 and takes no gradient.  Two launches forward
    (the items of every mesh, then one workgroup that adds the partial sums in a fixed order), one backward; the partial sums
    live in the stream's cached workspace, the forward saves L_i / (|L_i| d_i) [B,V,3] when the laplacian is on, and the backward
    reads the three upstream gradients on the device and writes every element of g_verts (no zero fill, no atomics: the same
    bits on every run).  Only verts get a gradient; no double backward."""

    @staticmethod
    def forward(ctx, verts, topo, target_length, terms):
        v = _dev(verts, torch.float32, "verts")
        lib = _lib.load()
        V, E, P = topo.num_verts, topo.num_edges, topo.num_pairs
        if tuple(v.shape[-2:]) != (V, 3) or v.dim() not in (2, 3):
            raise ValueError(f"mesh_regularisers: verts [{V},3] or [B,{V},3] expected, got {tuple(v.shape)}")
        if topo.edges.device != v.device:
            raise _lib.VogeHipError(f"mesh_regularisers: verts on {v.device}, the topology on {topo.edges.device}")
        B = v.shape[0] if v.dim() == 3 else 1
        out = (torch.zeros if B * V == 0 else torch.empty)((3,), dtype=torch.float32, device=v.device)      # (nothing is launched for an empty batch)
        lap_dir = torch.empty_like(v) if terms & 2 else None
        with _on(v.device):
            nbytes = lib.voge_mesh_reg_workspace_bytes(B, V, E, P)
            ws = _workspace(v.device, nbytes)
            rc = lib.voge_mesh_reg_fwd(_p(v), _p(topo.edges), _p(topo.nbr_off), _p(topo.nbr), _p(topo.pairs), B, V, E, P, terms,
                                       target_length, _p(lap_dir), _p(ws), nbytes, _p(out), _stream())
        _lib.check(rc, "voge_mesh_reg_fwd")
        ctx.save_for_backward(v, lap_dir)
        ctx.topo, ctx.target_length, ctx.terms = topo, target_length, terms
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_edge, g_lap, g_normal):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        lib = _lib.load()
        v, lap_dir = ctx.saved_tensors
        topo = ctx.topo
        V = topo.num_verts
        B = v.shape[0] if v.dim() == 3 else 1
        g = [None if t_ is None else _dev(t_, torch.float32, "grad_term") for t_ in (g_edge, g_lap, g_normal)]
        g_verts = (torch.zeros_like if B * V == 0 else torch.empty_like)(v)
        with _on(v.device):
            rc = lib.voge_mesh_reg_bwd(_p(v), _p(topo.nbr_off), _p(topo.nbr), _p(topo.pairs), _p(topo.inc_off), _p(topo.inc),
                                       _p(lap_dir), _p(g[0]), _p(g[1]), _p(g[2]), B, V, topo.num_edges, topo.num_pairs, ctx.terms,
                                       ctx.target_length, _p(g_verts), _stream())
        _lib.check(rc, "voge_mesh_reg_bwd")
        return g_verts, None, None, None


def _sized_workspace(dev, size_entry, *sizes):
    """(ws, nbytes): the stream's cached workspace of the bytes the library's size entry asks for these sizes"""
    nbytes = size_entry(*sizes)
    return _workspace(dev, nbytes), nbytes


def _cell_size(cell_size, what):
    """The cell edge a grid entry takes: 0.0 for None (the entry's default cell), else a positive finite fp32 number"""
    if cell_size is None:
        return 0.0
    cell = float(cell_size)
    if not (cell > 0.0 and cell < 3.0e38):
        raise ValueError(f"{what}: cell_size must be a positive finite fp32 number, got {cell_size}")
    return cell


def knn_grid(lo, hi, n, cell_size=None):
    """The uniform grid voge_knn_points searches: (cell, gx, gy, gz) for a cloud of n points whose bounding box is lo .. hi
    (three floats each).  Default: about 2 n cubic cells over the box, cell = (volume / 2n)^(1/3) -- over the axes that have an
    extent when some have none (a planar cloud: 2 n square cells), 1 when none has; cell_size asks for a cell of its own.  Either
    way g_a = floor(extent_a / cell) + 1 >= 1, and the cell is enlarged until every g_a <= 1024 and gx gy gz <= max(8 n, 2^15).
    The cell is an fp32 value: the kernels get exactly the number the counts were made from."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    if cell_size is None:
        pos = [e for e in ext if e > 0.0]
        cell = 1.0
        if pos:
            vol = 1.0
            for e in pos:
                vol *= e
            cell = (vol / (2.0 * max(n, 1))) ** (1.0 / len(pos))
    else:
        cell = _cell_size(cell_size, "knn_points")
    cap = max(8 * n, 1 << 15)
    cell = max(cell, max(ext) / 1023.0, 1e-30)
    while True:
        cell = struct.unpack("f", struct.pack("f", cell))[0]
        g = [int(e / cell) + 1 for e in ext]
        cells = g[0] * g[1] * g[2]
        if max(g) <= 1024 and cells <= cap:
            return cell, g[0], g[1], g[2]
        cell *= max(1.05, (cells / cap) ** (1.0 / 3.0))      # (every round grows the cell: at the latest a one-cell grid ends it)


def knn_points(points, k, include_self=False, cell_size=None):
    """Exact k nearest neighbours inside a cloud (extension; voge_knn_points): points [N,3] on a HIP device -> (idx [N,k] int32,
    d2 [N,k] fp32, (cell, gx, gy, gz)), the values of Converters.knn_points bit for bit, whatever the grid.  The bounding box
    comes from torch.aminmax and is read on the host (one synchronisation: a converter runs once per cloud, and not under graph
    capture); the scratch is the stream's cached workspace.  A points tensor that is not fp32, contiguous and on a 16-byte
    boundary is copied.  Non-finite coordinates raise ValueError."""
    pts = _aligned16(_dev(points, torch.float32, "points"))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"knn_points: points [N,3] expected, got {tuple(pts.shape)}")
    lib = _lib.load()
    N, k = pts.shape[0], int(k)
    idx = torch.empty((N, k), dtype=torch.int32, device=pts.device)
    d2 = torch.empty((N, k), dtype=torch.float32, device=pts.device)
    if N == 0:
        return idx, d2, (1.0, 1, 1, 1)
    box = torch.cat(torch.aminmax(pts, dim=0)).tolist()
    if not all(math.isfinite(v) for v in box):
        raise ValueError("knn_points: points hold non-finite coordinates")
    cell, gx, gy, gz = knn_grid(box[:3], box[3:], N, cell_size)
    with _on(pts.device):
        ws, nbytes = _sized_workspace(pts.device, lib.voge_knn_workspace_bytes, N, gx, gy, gz)
        rc = lib.voge_knn_points(_p(pts), N, k, int(bool(include_self)), box[0], box[1], box[2], cell, gx, gy, gz, _p(idx), _p(d2),
                                 _p(ws), nbytes, _stream())
    _lib.check(rc, "voge_knn_points")
    return idx, d2, (cell, gx, gy, gz)


def knn_frames(points, idx, toward=None):
    """Local PCA frames (extension; voge_knn_frames): points [N,3], idx [N,k] on a HIP device, toward None | [3] | [N,3] ->
    (quats [N,4], eig [N,3]) fp32, one launch on the current stream; Converters.point_cloud_frames is the definition."""
    pts = _dev(points, torch.float32, "points")
    idx = _dev(idx, torch.int32, "idx")
    N = pts.shape[0]
    if pts.dim() != 2 or pts.shape[1] != 3 or idx.dim() != 2 or idx.shape[0] != N:
        raise ValueError(f"knn_frames: points [N,3] and idx [N,k] expected, got {tuple(pts.shape)} / {tuple(idx.shape)}")
    per_point = 0
    if toward is not None:
        toward = _dev(toward, torch.float32, "toward")
        if tuple(toward.shape) not in ((3,), (N, 3)):
            raise ValueError(f"knn_frames: toward [3] or [N,3] expected, got {tuple(toward.shape)}")
        per_point = int(toward.dim() == 2)
    lib = _lib.load()
    quats = torch.empty((N, 4), dtype=torch.float32, device=pts.device)
    eig = torch.empty((N, 3), dtype=torch.float32, device=pts.device)
    with _on(pts.device):
        rc = lib.voge_knn_frames(_p(pts), _p(idx), N, idx.shape[1], _p(toward), per_point, _p(quats), _p(eig), _stream())
    _lib.check(rc, "voge_knn_frames")
    return quats, eig


CHAMFER_ROUTES = {None: 0, "brute": 1, "grid": 2}


def _chamfer_route(route):
    if route not in CHAMFER_ROUTES:
        raise ValueError(f"route must be None, 'brute' or 'grid', got {route!r}")
    return CHAMFER_ROUTES[route]


def _cloud(t, name):
    t = _dev(t, torch.float32, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} [N,3] expected, got {tuple(t.shape)}")
    return t


def nearest_points(queries, points, cell_size=None, route=None, return_grid=False):
    """The nearest point of `points` [Np,3] for every row of `queries` [Nq,3] (extension; voge_nearest_points) on a HIP device ->
    (idx [Nq] int32, d2 [Nq] fp32), the values of Converters.nearest_points bit for bit on either route.  route None chooses by
    Nq Np; "brute": one launch, "grid": a grid over both clouds chosen on the device -- nothing is read back on the host, so the
    call may be captured into a graph.  cell_size asks the grid for a cell of that edge.  return_grid=True appends a [8] int32
    device tensor, the first 32 bytes of the workspace: after a grid-route call the bits of (lo[3], cell, 1 / cell) and gx, gy, gz
    -- what the tests read to see which grid ran."""
    q, p = _cloud(queries, "queries"), _cloud(points, "points")
    r = _chamfer_route(route)
    cell = _cell_size(cell_size, "nearest_points")
    Nq, Np = q.shape[0], p.shape[0]
    if Np == 0:
        raise ValueError("nearest_points: points is empty")
    lib = _lib.load()
    idx = torch.empty((Nq,), dtype=torch.int32, device=q.device)
    d2 = torch.empty((Nq,), dtype=torch.float32, device=q.device)
    grid = None
    if Nq > 0:
        with _on(q.device):
            ws, nbytes = _sized_workspace(q.device, lib.voge_chamfer_workspace_bytes, Nq, Np)
            rc = lib.voge_nearest_points(_p(q), Nq, _p(p), Np, r, cell, _p(idx), _p(d2), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_nearest_points")
        if return_grid:
            grid = ws[:32].clone().view(torch.int32)
    return (idx, d2, grid) if return_grid else (idx, d2)


class _Chamfer(torch.autograd.Function):
    """Chamfer distance (extension; voge_chamfer_fwd / _bwd): forward(x [Nx,3], y [Ny,3], flags, route) -> (loss 0-dim, nn_x [Nx],
    nn_y [Ny] | None), the value of Aggregation.chamfer_term and the indices of Converters.nearest_points in both directions
    (int32, not differentiable).  flags: bit 0 "sum", bit 1 single_directional (nn_y is None).  The searches, the fp64 partial sums
    and the one workgroup that adds them run on the current stream from the stream's cached workspace with nothing read back on
    the host; the node saves the clouds, the indices and meta [4] int32 (the backward's scale exponent, chosen on the device).
    Backward: three launches (zero fill, integer-atomic scatter, finish), every element of g_x and g_y written: the same bits on
    every run.  No double backward."""

    @staticmethod
    def forward(ctx, x, y, flags, route):
        x, y = _cloud(x, "x"), _cloud(y, "y")
        if y.device != x.device:
            raise _lib.VogeHipError(f"chamfer_distance: x on {x.device}, y on {y.device}")
        Nx, Ny = x.shape[0], y.shape[0]
        if Nx == 0 or Ny == 0:
            raise ValueError("chamfer_distance: an empty cloud")
        lib = _lib.load()
        dev = x.device
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        nn_x = torch.empty((Nx,), dtype=torch.int32, device=dev)
        nn_y = None if flags & 2 else torch.empty((Ny,), dtype=torch.int32, device=dev)
        meta = torch.empty((4,), dtype=torch.int32, device=dev)
        with _on(dev):
            ws, nbytes = _sized_workspace(dev, lib.voge_chamfer_workspace_bytes, Nx, Ny)
            rc = lib.voge_chamfer_fwd(_p(x), Nx, _p(y), Ny, route, flags, _p(loss), _p(nn_x), _p(nn_y), _p(meta), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_chamfer_fwd")
        ctx.save_for_backward(x, y, nn_x, nn_y, meta)
        ctx.flags = flags
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*([nn_x] if nn_y is None else [nn_x, nn_y]))
        return loss[0], nn_x, nn_y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _gx, _gy):
        if g_loss is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        lib = _lib.load()
        x, y, nn_x, nn_y, meta = ctx.saved_tensors
        Nx, Ny = x.shape[0], y.shape[0]
        g = _dev(g_loss, torch.float32, "grad_loss")
        g_x, g_y = torch.empty_like(x), torch.empty_like(y)
        with _on(x.device):
            ws, nbytes = _sized_workspace(x.device, lib.voge_chamfer_workspace_bytes, Nx, Ny)
            rc = lib.voge_chamfer_bwd(_p(x), Nx, _p(y), Ny, _p(nn_x), _p(nn_y), _p(meta), _p(g), ctx.flags, _p(g_x), _p(g_y), _p(ws),
                                      nbytes, _stream())
        _lib.check(rc, "voge_chamfer_bwd")
        return (g_x if ctx.needs_input_grad[0] else None), (g_y if ctx.needs_input_grad[1] else None), None, None


def chamfer(x, y, sum_reduction=False, single_directional=False, route=None):
    """(loss, nn_x, nn_y) of ONE pair of clouds on a HIP device: _Chamfer.apply."""
    return _Chamfer.apply(x, y, int(bool(sum_reduction)) | (int(bool(single_directional)) << 1), _chamfer_route(route))


POINT_MESH_FACE_TILE = 256      # kPmFaceTile of point_mesh.hip: triangle records of an LDS tile (the tests build meshes around it)
POINT_MESH_POINT_TILE = 1024    # kPmPointTile: points of an LDS tile
POINT_MESH_MAX_PAIRS = 1 << 38  # kPmMaxPairs: the brute-force entries refuse P F above it (route None and "brute")
POINT_MESH_MAX_N = (1 << 28) - 1             # kPmMaxN: V, F and P of either route
# point_mesh_grid.h's constants, mirrored for the tests' restatement of the grid route
POINT_MESH_GRID_MIN_PAIRS = 1 << 38          # kPmGridMinPairs: route None takes the grid from this many pairs on -- the pair cap itself: the
#                                              grid wins at every size with the points near the surface and loses below the cap with
#                                              the points spread through the box (profiles/r28_point_mesh_grid.txt); shapes cannot tell
POINT_MESH_GRID_BIG = 1.0                    # kPmGridBig: a triangle is small while its half-extent <= BIG x cell
POINT_MESH_GRID_FLOOR = 1.0                  # kPmGridFloor: cell >= FLOOR x the mean largest bounding-box extent of a face
POINT_MESH_GRID_BLOCK = 128                  # kPmGridBlock: queries a workgroup of the two searches
POINT_MESH_GRID_LARGE_TILE = 256             # kPmGridLargeTile: records of an LDS tile of the large list
POINT_MESH_GRID_HALF_UP = 1.0 + 2.0 ** -22   # a half-extent is rounded up by this factor
POINT_MESH_GRID_RING_SLACK = 2.0 ** -10      # the stopping rule: X = cell (r - RING_SLACK) - h,
POINT_MESH_GRID_M = 2.0 ** -8                #   b = X (1 - M) - M_H h,
POINT_MESH_GRID_M_H = 2.0 ** -7
POINT_MESH_GRID_B_MIN = 2.0 ** -50           #   and it fires once b > B_MIN and the kept d2 <= b b
POINT_MESH_ROUTES = (None, "brute", "grid")


def _point_mesh_route(route, F, P, what):
    """The route a call of `what` takes on F faces and P points: "brute" or "grid".  None: the brute force below
    POINT_MESH_GRID_MIN_PAIRS pairs, the grid from there on -- and, like "brute", bound by POINT_MESH_MAX_PAIRS (ValueError above
    it); "grid" is bound by the sizes alone.  As measured the crossover is the cap: for points near the surface (a fit, a score)
    route="grid" is up to 110 x faster from 10^7 pairs on and worth asking for; for points far from it, it loses."""
    if route not in POINT_MESH_ROUTES:
        raise ValueError(f"{what}: route must be None, 'brute' or 'grid', got {route!r}")
    if max(F, P) > POINT_MESH_MAX_N:
        raise ValueError(f"{what}: {P} points x {F} faces: at most {POINT_MESH_MAX_N} of either")
    if route != "grid" and F * P > POINT_MESH_MAX_PAIRS:
        raise ValueError(f"{what}: {P} points x {F} faces is above the {POINT_MESH_MAX_PAIRS} pairs an exact "
                         "search takes (a brute force); for such sizes score sample_points_from_meshes against the points with "
                         "chamfer_distance.  route=\"grid\" searches a uniform grid instead and is not bound by the pair cap")
    if route is None:
        return "brute" if F * P < POINT_MESH_GRID_MIN_PAIRS else "grid"
    return route


_point_mesh_cell = _cell_size      # (the name the point-mesh tests call it by)


def _point_mesh_args(verts, faces, points, what, route=None):
    """-> (verts, faces, points, "brute" | "grid"); the route is checked with the sizes, by _point_mesh_route"""
    verts, points = _cloud(verts, "verts"), _cloud(points, "points")
    faces = _dev(faces, torch.int32, "faces")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces [F,3] expected, got {tuple(faces.shape)}")
    if points.device != verts.device or faces.device != verts.device:
        raise _lib.VogeHipError(f"{what}: verts on {verts.device}, faces on {faces.device}, points on {points.device}")
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError(f"{what}: an empty mesh")
    return verts, faces, points, _point_mesh_route(route, faces.shape[0], points.shape[0], what)


def closest_faces(points, verts, faces, route=None, cell_size=None):
    """The nearest triangle of the mesh (verts [V,3], faces [F,3] integer) for every row of points [P,3] (extension;
    voge_closest_faces / voge_closest_faces_grid) on a HIP device -> (d2 [P] fp32, face_idx [P] int32, bary [P,3] fp32): the
    squared distance of Aggregation.point_triangle_closest, the lowest face index among exact ties and the weights of the closest
    point.  route "brute": one launch over all P F pairs, at most POINT_MESH_MAX_PAIRS; "grid": a search over a uniform grid chosen
    on the device, the same bits, no pair cap (cell_size asks the grid for a cell of that edge: the tests' and the tuner's knob);
    None: by P F (_point_mesh_route).  Nothing is read back on the host on either route; no gradient."""
    verts, faces, points, route = _point_mesh_args(verts, faces, points, "closest_faces", route)
    cell = _cell_size(cell_size, "closest_faces")
    P = points.shape[0]
    d2 = torch.empty((P,), dtype=torch.float32, device=points.device)
    face_idx = torch.empty((P,), dtype=torch.int32, device=points.device)
    bary = torch.empty((P, 3), dtype=torch.float32, device=points.device)
    if P > 0:
        lib = _lib.load()
        V, F = verts.shape[0], faces.shape[0]
        with _on(points.device):
            if route == "grid":
                ws, nbytes = _sized_workspace(points.device, lib.voge_point_mesh_grid_workspace_bytes, V, F, P)
                rc = lib.voge_closest_faces_grid(_p(points), P, _p(verts), V, _p(faces), F, cell, _p(face_idx), _p(d2), _p(bary), _p(ws),
                                                 nbytes, _stream())
            else:
                rc = lib.voge_closest_faces(_p(points), P, _p(verts), V, _p(faces), F, _p(face_idx), _p(d2), _p(bary), _stream())
        _lib.check(rc, "voge_closest_faces_grid" if route == "grid" else "voge_closest_faces")
    return d2, face_idx, bary


class _PointMesh(torch.autograd.Function):
    """Point-to-mesh distance (extension; voge_point_mesh_fwd / _fwd_grid / _bwd): forward(verts [V,3], faces [F,3] int, points
    [P,3], flags, route, cell_size) -> (loss 0-dim, face_idx [P], bary_p [P,3], point_idx [F] | None, bary_f [F,3] | None), the
    value of Aggregation.point_mesh_term with the chosen pairs and the weights of their closest points (not differentiable).
    flags: bit 0 "sum", bit 1 single_directional.  route and cell_size: closest_faces's -- the two routes return the same bits.
    The two searches, the fp64 partial sums and the one workgroup that adds them run on the current stream from the stream's
    cached workspace with nothing read back on the host; the node saves the inputs, the indices, the weights and meta [4] int32
    (the backward's scale exponent, chosen on the device).  Backward, the same on both routes: three launches (zero fill,
    integer-atomic scatter, finish), every element of g_verts and g_points written: the same bits on every run.  No double
    backward."""

    @staticmethod
    def forward(ctx, verts, faces, points, flags, route=None, cell_size=None):
        verts, faces, points, route = _point_mesh_args(verts, faces, points, "point_mesh_face_distance", route)
        cell = _cell_size(cell_size, "point_mesh_face_distance")
        V, F, P = verts.shape[0], faces.shape[0], points.shape[0]
        if P == 0:
            raise ValueError("point_mesh_face_distance: an empty cloud")
        lib = _lib.load()
        dev = verts.device
        single = bool(flags & 2)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        face_idx = torch.empty((P,), dtype=torch.int32, device=dev)
        bary_p = torch.empty((P, 3), dtype=torch.float32, device=dev)
        point_idx = None if single else torch.empty((F,), dtype=torch.int32, device=dev)
        bary_f = None if single else torch.empty((F, 3), dtype=torch.float32, device=dev)
        meta = torch.empty((4,), dtype=torch.int32, device=dev)
        with _on(dev):
            if route == "grid":
                ws, nbytes = _sized_workspace(dev, lib.voge_point_mesh_grid_workspace_bytes, V, F, P)
                rc = lib.voge_point_mesh_fwd_grid(_p(verts), V, _p(faces), F, _p(points), P, flags, cell, _p(loss), _p(face_idx), _p(bary_p),
                                                  _p(point_idx), _p(bary_f), _p(meta), _p(ws), nbytes, _stream())
            else:
                ws, nbytes = _sized_workspace(dev, lib.voge_point_mesh_workspace_bytes, V, F, P)
                rc = lib.voge_point_mesh_fwd(_p(verts), V, _p(faces), F, _p(points), P, flags, _p(loss), _p(face_idx), _p(bary_p),
                                             _p(point_idx), _p(bary_f), _p(meta), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_point_mesh_fwd_grid" if route == "grid" else "voge_point_mesh_fwd")
        ctx.save_for_backward(verts, faces, points, face_idx, bary_p, point_idx, bary_f, meta)
        ctx.flags = flags | (4 if route == "grid" else 0)      # (bit 2 of the backward: pairs of the grid route, no pair cap)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[t for t in (face_idx, bary_p, point_idx, bary_f) if t is not None])
        return loss[0], face_idx, bary_p, point_idx, bary_f

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, *_unused):
        if g_loss is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
            return None, None, None, None, None, None
        lib = _lib.load()
        verts, faces, points, face_idx, bary_p, point_idx, bary_f, meta = ctx.saved_tensors
        V, F, P = verts.shape[0], faces.shape[0], points.shape[0]
        g = _dev(g_loss, torch.float32, "grad_loss")
        g_verts, g_points = torch.empty_like(verts), torch.empty_like(points)
        with _on(verts.device):
            ws, nbytes = _sized_workspace(verts.device, lib.voge_point_mesh_workspace_bytes, V, F, P)
            rc = lib.voge_point_mesh_bwd(_p(verts), V, _p(faces), F, _p(points), P, _p(face_idx), _p(bary_p), _p(point_idx), _p(bary_f),
                                         _p(meta), _p(g), ctx.flags, _p(g_verts), _p(g_points), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_point_mesh_bwd")
        return (g_verts if ctx.needs_input_grad[0] else None), None, (g_points if ctx.needs_input_grad[2] else None), None, None, None


def point_mesh(verts, faces, points, sum_reduction=False, single_directional=False, route=None, cell_size=None):
    """(loss, face_idx, bary_p, point_idx, bary_f) of ONE mesh and ONE cloud on a HIP device: _PointMesh.apply.  route and
    cell_size: closest_faces's."""
    return _PointMesh.apply(verts, faces, points, int(bool(sum_reduction)) | (int(bool(single_directional)) << 1), route, cell_size)


MESH_SAMPLE_BLOCK = 256      # kMsBlock of mesh_sample.hip: the faces of one scan block (the tests build meshes around it)
MESH_SAMPLE_LDS_BLOCKS = 2048      # kMsLdsBlocks: more scan blocks than this and the sampler searches the block table in memory


class _MeshSample(torch.autograd.Function):
    """Mesh surface sampling (extension; voge_mesh_sample_fwd / _bwd): forward(verts [V,3], sampler, u [S,3], return_normals,
    return_areas) -> (points [S,3], normals [S,3] | None, face_idx [S] int32, bary [S,3], A2 [F] | None), the values of
    Aggregation.mesh_surface_points over the tables of a Losses.SurfaceSampler on the same device; face_idx, bary and A2 are not
    differentiable.  Three launches forward and four backward on the current stream from the stream's cached workspace, nothing
    read back on the host; the node saves verts, u's outputs face_idx and bary.  The backward adds fixed-point terms with integer
    atomics and writes every element of g_verts: the same bits on every run.  Only verts get a gradient; no double backward."""

    @staticmethod
    def forward(ctx, verts, sampler, u, return_normals, return_areas):
        v = _dev(verts, torch.float32, "verts")
        u = _dev(u, torch.float32, "u")
        V, F = sampler.num_verts, sampler.num_faces
        if tuple(v.shape) != (V, 3):
            raise ValueError(f"mesh_sample: verts [{V},3] expected, got {tuple(v.shape)}")
        if u.dim() != 2 or u.shape[1] != 3:
            raise ValueError(f"mesh_sample: u [S,3] expected, got {tuple(u.shape)}")
        if F == 0:
            raise ValueError("mesh_sample: a mesh without faces")
        if sampler.faces.device != v.device or u.device != v.device:
            raise _lib.VogeHipError(f"mesh_sample: verts on {v.device}, the sampler on {sampler.faces.device}, u on {u.device}")
        lib = _lib.load()
        S, dev = u.shape[0], v.device
        points = torch.empty((S, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((S, 3), dtype=torch.float32, device=dev) if return_normals else None
        face_idx = torch.empty((S,), dtype=torch.int32, device=dev)
        bary = torch.empty((S, 3), dtype=torch.float32, device=dev)
        a2 = torch.empty((F,), dtype=torch.float32, device=dev) if return_areas else None
        with _on(dev):
            ws, nbytes = _sized_workspace(dev, lib.voge_mesh_sample_workspace_bytes, V, F, S)
            rc = lib.voge_mesh_sample_fwd(_p(v), V, _p(sampler.faces), F, _p(u), S, _p(points), _p(normals), _p(face_idx), _p(bary),
                                          _p(a2), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_mesh_sample_fwd")
        ctx.save_for_backward(v, face_idx, bary)
        ctx.sampler = sampler
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[t_ for t_ in (face_idx, bary, a2) if t_ is not None])
        return points, normals, face_idx, bary, a2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_points, g_normals, _gf, _gb, _ga):
        if not ctx.needs_input_grad[0] or (g_points is None and g_normals is None):
            return None, None, None, None, None
        lib = _lib.load()
        v, face_idx, bary = ctx.saved_tensors
        sampler = ctx.sampler
        V, F, S = sampler.num_verts, sampler.num_faces, face_idx.shape[0]
        gp = None if g_points is None else _dev(g_points, torch.float32, "grad_points")
        gn = None if g_normals is None else _dev(g_normals, torch.float32, "grad_normals")
        g_verts = torch.empty_like(v)
        with _on(v.device):
            ws, nbytes = _sized_workspace(v.device, lib.voge_mesh_sample_workspace_bytes, V, F, S)
            rc = lib.voge_mesh_sample_bwd(_p(v), V, _p(sampler.faces), F, _p(sampler.corner_off), _p(sampler.corner), _p(face_idx),
                                          _p(bary), S, _p(gp), _p(gn), _p(g_verts), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_mesh_sample_bwd")
        return g_verts, None, None, None, None


def mesh_sample(verts, sampler, u, return_normals=False, return_areas=False):
    """(points, normals | None, face_idx int32, bary) of ONE mesh on a HIP device: _MeshSample.apply.  return_areas=True appends
    A2 [F], the doubled face areas the kernel chose by (a debug output: what the tests compare with the definition's bits)."""
    out = _MeshSample.apply(verts, sampler, u, bool(return_normals), bool(return_areas))
    return out if return_areas else out[:4]


MTET_BLOCK = 256      # kMtBlock of meshing.hip: the grid points of one scan block
MTET_TOP = 1024       # kMtTop: the block totals one round of the top-level scan takes (the tests build grids around both)
MTET_MAX_CHANNELS = 8      # kMtMaxChannels: the attribute channels voge_tsdf_integrate_attr and voge_mtet_attr are compiled for


def _grid_volume(t, name):
    """An fp32 [nz,ny,nx] tensor on a HIP device that a kernel may write in place"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous():
        raise _lib.VogeHipError(f"{name}: a contiguous fp32 [nz,ny,nx] tensor on a HIP device expected (no CPU fallback)")
    return t


def tsdf_integrate(tsdf, weight, depth, R, T, centre, focal, pp, lo, voxel_size, trunc, max_weight=None, attr=None, attr_image=None):
    """Fuse depth [B,H,W] into tsdf / weight [nz,ny,nx] IN PLACE (extension; voge_tsdf_integrate): the values of
    Aggregation.tsdf_integrate in fp32.  R [B,3,3], T [B,3], centre [B,3], focal [B,2], pp [B,2] on the volume's device; lo and
    voxel_size three numbers each.  One launch on the current stream, nothing read back; not differentiable.  attr [nz,ny,nx,C]
    with attr_image [B,H,W,C], 1 <= C <= MTET_MAX_CHANNELS, both or neither: voge_tsdf_integrate_attr, still one launch, attr IN
    PLACE as well and appended to the result; tsdf and weight get the bits of the call without them."""
    tsdf, weight = _grid_volume(tsdf, "tsdf"), _grid_volume(weight, "weight")
    if weight.shape != tsdf.shape or weight.device != tsdf.device:
        raise ValueError(f"tsdf_integrate: weight {tuple(weight.shape)} on {weight.device} does not match tsdf {tuple(tsdf.shape)}")
    dev = tsdf.device
    if (attr is None) != (attr_image is None):
        raise ValueError("tsdf_integrate: attr and attr_image go together")
    if attr is not None:
        if (not isinstance(attr, torch.Tensor) or not attr.is_cuda or attr.dtype != torch.float32 or attr.dim() != 4
                or not attr.is_contiguous()):
            raise _lib.VogeHipError("attr: a contiguous fp32 [nz,ny,nx,C] tensor on a HIP device expected (no CPU fallback)")
        C = attr.shape[3]
        if attr.shape[:3] != tsdf.shape or attr.device != dev or not 1 <= C <= MTET_MAX_CHANNELS:
            raise ValueError(f"tsdf_integrate: attr {tuple(attr.shape)} on {attr.device} does not match tsdf {tuple(tsdf.shape)} with 1 .. "
                             f"{MTET_MAX_CHANNELS} channels")
        attr_image = _dev(attr_image.detach(), torch.float32, "attr_image")
        if attr_image.device != dev:
            raise _lib.VogeHipError(f"tsdf_integrate: attr_image on {attr_image.device}, the volume on {dev}")
    depth = _dev(depth, torch.float32, "depth")
    if depth.dim() != 3:
        raise ValueError(f"tsdf_integrate: depth [B,H,W] expected, got {tuple(depth.shape)}")
    B, H, W = depth.shape
    if attr is not None and tuple(attr_image.shape) != (B, H, W, C):
        raise ValueError(f"tsdf_integrate: attr_image {[B, H, W, C]} expected, got {tuple(attr_image.shape)}")
    cam = []
    for t_, shape, name in ((R, (B, 3, 3), "R"), (T, (B, 3), "T"), (centre, (B, 3), "centre"), (focal, (B, 2), "focal"), (pp, (B, 2), "pp")):
        t_ = _dev(t_.detach(), torch.float32, name)
        if tuple(t_.shape) != shape:
            raise ValueError(f"tsdf_integrate: {name} {list(shape)} expected for {B} depth maps, got {tuple(t_.shape)}")
        if t_.device != dev:
            raise _lib.VogeHipError(f"tsdf_integrate: {name} on {t_.device}, the volume on {dev}")
        cam.append(t_)
    if depth.device != dev:
        raise _lib.VogeHipError(f"tsdf_integrate: depth on {depth.device}, the volume on {dev}")
    nz, ny, nx = tsdf.shape
    lib = _lib.load()
    grid = [float(x) for x in lo] + [float(x) for x in voxel_size]
    tail = [_p(t_) for t_ in cam] + [float(trunc), 0.0 if max_weight is None else float(max_weight)]
    if attr is not None:
        with _on(dev):
            rc = lib.voge_tsdf_integrate_attr(_p(tsdf), _p(weight), _p(attr), C, nx, ny, nz, *grid, _p(depth), _p(attr_image), B, H, W, *tail,
                                              _stream())
        _lib.check(rc, "voge_tsdf_integrate_attr")
        return tsdf, weight, attr
    with _on(dev):
        rc = lib.voge_tsdf_integrate(_p(tsdf), _p(weight), nx, ny, nz, *grid, _p(depth), B, H, W, *tail, _stream())
    _lib.check(rc, "voge_tsdf_integrate")
    return tsdf, weight


def marching_tets(values, weight, level, lo, voxel_size, return_tables=False, attr=None):
    """(verts [V,3] fp32, faces [F,3] int32) of the level set of values [nz,ny,nx] fp32 on a HIP device (extension; voge_mtet_count /
    _scan / _emit): the values of Aggregation.marching_tets.  Count and scan on the current stream, then the two totals are read
    back on the host -- ONE synchronisation, what sizes the outputs -- and one launch writes the mesh.  Not differentiable, not
    capturable.  return_tables=True appends (edge_mask, face_count) for the tests.  attr [nz,ny,nx,C] fp32 on the same device
    appends vert_attr [V,C] after the faces (voge_mtet_attr: one more launch on the tables of the emit, one per MTET_MAX_CHANNELS
    channels); the mesh is the one of the call without it, bit for bit."""
    v = _dev(values.detach(), torch.float32, "values")
    if v.dim() != 3:
        raise ValueError(f"marching_tets: values [nz,ny,nx] expected, got {tuple(v.shape)}")
    if attr is not None:
        attr = _dev(attr.detach(), torch.float32, "attr")
        if attr.dim() != 4 or attr.shape[:3] != v.shape or attr.shape[3] < 1 or attr.device != v.device:
            raise ValueError(f"marching_tets: attr {tuple(attr.shape)} on {attr.device} does not match values {tuple(v.shape)} on {v.device}")
    w = None
    if weight is not None:
        w = _dev(weight.detach(), torch.float32, "weight")
        if w.shape != v.shape or w.device != v.device:
            raise ValueError(f"marching_tets: weight {tuple(w.shape)} on {w.device} does not match values {tuple(v.shape)} on {v.device}")
    nz, ny, nx = v.shape
    n = nx * ny * nz
    if min(nx, ny, nz) < 2 or n * 7 >= 2 ** 31:
        raise ValueError(f"marching_tets: every dimension >= 2 and nx ny nz 7 < 2^31 expected, got (nx, ny, nz) = ({nx}, {ny}, {nz})")
    dev = v.device
    nb = (n + MTET_BLOCK - 1) // MTET_BLOCK
    edge_mask = torch.empty((n,), dtype=torch.uint8, device=dev)
    face_count = torch.empty((n,), dtype=torch.uint8, device=dev)
    loc = torch.empty((2, n), dtype=torch.int16, device=dev)      # (16-bit prefixes: the kernels read them as unsigned)
    blocks = torch.empty((2, nb), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    grid = [float(x) for x in lo] + [float(x) for x in voxel_size]
    lib = _lib.load()
    with _on(dev):
        st = _stream()
        rc = lib.voge_mtet_count(_p(v), _p(w), nx, ny, nz, float(level), _p(edge_mask), _p(face_count), _p(loc[0]), _p(loc[1]), _p(blocks[0]),
                                 _p(blocks[1]), st)
        _lib.check(rc, "voge_mtet_count")
        _lib.check(lib.voge_mtet_scan(_p(blocks[0]), _p(blocks[1]), nb, _p(totals), st), "voge_mtet_scan")
        V, F = (int(x) for x in totals.tolist())      # the synchronisation
        if V >= 2 ** 31 or F >= 2 ** 31:
            raise ValueError(f"marching_tets: {V} vertices and {F} faces do not fit 32-bit indices")
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        rc = lib.voge_mtet_emit(_p(v), _p(w), nx, ny, nz, float(level), *grid, _p(edge_mask), _p(face_count), _p(loc[0]), _p(loc[1]),
                                _p(blocks[0]), _p(blocks[1]), V, F, _p(verts) if V else None, _p(faces) if F else None, st)
        _lib.check(rc, "voge_mtet_emit")
        if attr is not None:
            C = attr.shape[3]
            parts = []
            for c0 in range(0, C, MTET_MAX_CHANNELS):      # (more channels than one launch takes: a launch per slice of them)
                a = attr if C <= MTET_MAX_CHANNELS else attr[..., c0:c0 + MTET_MAX_CHANNELS].contiguous()
                part = torch.empty((V, a.shape[3]), dtype=torch.float32, device=dev)
                rc = lib.voge_mtet_attr(_p(v), nx, ny, nz, float(level), _p(a), a.shape[3], _p(edge_mask), _p(loc[0]), _p(blocks[0]), V,
                                        _p(part) if V else None, st)
                _lib.check(rc, "voge_mtet_attr")
                parts.append(part)
            vert_attr = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
    out = (verts, faces) + ((edge_mask, face_count) if return_tables else ())
    return out if attr is None else out + (vert_attr,)


MESH_CLEAN_BLOCK = 256      # kMcBlock of mesh_clean.hip: the flags of one scan block
MESH_CLEAN_TOP = 1024       # kMcTop: the block totals one round of the top-level scan takes (the tests build meshes around both)
MESH_MAX = 2 ** 28 - 1      # kMcMax: the vertices and the faces of one mesh


def _mesh_faces(faces, name):
    f = _dev(faces.detach(), torch.int32, "faces")
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{name}: faces [F,3] expected, got {tuple(f.shape)}")
    if f.shape[0] > MESH_MAX:
        raise ValueError(f"{name}: {f.shape[0]} faces, at most {MESH_MAX}")
    return f


def _mesh_verts(verts, name):
    v = _dev(verts.detach(), torch.float32, "verts")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{name}: verts [V,3] expected, got {tuple(v.shape)}")
    if v.shape[0] > MESH_MAX:
        raise ValueError(f"{name}: {v.shape[0]} vertices, at most {MESH_MAX}")
    return v


def mesh_components(faces, num_verts, return_count=False):
    """(vert_label [V] int32, face_label [F] int32, num_components) of faces [F,3] int32 on a HIP device (extension;
    voge_mesh_components): the values of Aggregation.mesh_components.  Three launches on the current stream, then the error word
    and the number of components are read back on the host -- ONE synchronisation.  An index outside [0, V) raises ValueError, a
    loop of the union-find that reached its trip cap VogeHipError.  Not differentiable, not capturable.  return_count=True appends
    count [V] int32: the faces of a component at its label, 0 elsewhere."""
    f = _mesh_faces(faces, "mesh_components")
    V, F, dev = int(num_verts), f.shape[0], f.device
    if V < 0 or V > MESH_MAX:
        raise ValueError(f"mesh_components: {V} vertices, 0 .. {MESH_MAX} expected")
    if V == 0 and F > 0:
        raise ValueError("mesh_components: a face names a vertex outside [0, 0)")
    parent = torch.empty((V,), dtype=torch.int32, device=dev)
    vert_label = torch.empty((V,), dtype=torch.int32, device=dev)
    face_label = torch.empty((F,), dtype=torch.int32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    meta = torch.empty((4,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with _on(dev):
        rc = lib.voge_mesh_components(_p(f) if F else None, F, V, _p(parent) if V else None, _p(vert_label) if V else None,
                                      _p(face_label) if F else None, _p(count) if V else None, _p(meta), 7, _stream())
        _lib.check(rc, "voge_mesh_components")
        err, num = meta[:2].tolist()      # the synchronisation
    if err & 2:
        raise ValueError(f"mesh_components: a face names a vertex outside [0, {V})")
    if err:
        raise _lib.VogeHipError(f"voge_mesh_components: a loop of the union-find reached its trip cap (error word {err})")
    return (vert_label, face_label, int(num), count) if return_count else (vert_label, face_label, int(num))


def mesh_clean(verts, faces, face_label, keep_root):
    """(verts' [V',3], faces' [F',3] int32, vert_index [V'] int32, face_index [F'] int32) of verts [V,3] fp32, faces [F,3] int32 on a
    HIP device (extension; voge_mesh_clean_scan / _emit): the values of Aggregation.mesh_clean for the components keep_root [V]
    (bool or bytes, at the labels) names, face_label [F] int32 from mesh_components.  Four launches, then V', F' and the error word
    are read back on the host -- ONE synchronisation, what sizes the outputs -- and one launch writes them.  Not differentiable,
    not capturable."""
    v = _mesh_verts(verts, "mesh_clean")
    f = _mesh_faces(faces, "mesh_clean")
    fl = _dev(face_label, torch.int32, "face_label")
    kr = _dev(keep_root, torch.uint8, "keep_root")
    V, F, dev = v.shape[0], f.shape[0], v.device
    if tuple(fl.shape) != (F,) or tuple(kr.shape) != (V,):
        raise ValueError(f"mesh_clean: face_label [{F}] and keep_root [{V}] expected, got {tuple(fl.shape)} / {tuple(kr.shape)}")
    if f.device != dev or fl.device != dev or kr.device != dev:
        raise _lib.VogeHipError(f"mesh_clean: verts on {dev}, faces on {f.device}, face_label on {fl.device}, keep_root on {kr.device}")
    empty = lambda n, cols, dt: torch.empty((n, 3) if cols else (n,), dtype=dt, device=dev)
    if V == 0 or F == 0:
        return empty(0, True, torch.float32), empty(0, True, torch.int32), empty(0, False, torch.int32), empty(0, False, torch.int32)
    nb = (V + MESH_CLEAN_BLOCK - 1) // MESH_CLEAN_BLOCK + (F + MESH_CLEAN_BLOCK - 1) // MESH_CLEAN_BLOCK
    vflag = torch.empty(((V + 3) // 4 * 4,), dtype=torch.uint8, device=dev)
    loc = torch.empty((V + F,), dtype=torch.int16, device=dev)      # (16-bit prefixes: the kernels read them as unsigned)
    blocks = torch.empty((nb,), dtype=torch.int32, device=dev)
    err = torch.empty((1,), dtype=torch.int32, device=dev)
    totals = torch.empty((3,), dtype=torch.int64, device=dev)
    lib = _lib.load()
    with _on(dev):
        st = _stream()
        rc = lib.voge_mesh_clean_scan(_p(f), F, V, _p(fl), _p(kr), _p(vflag), _p(loc), _p(blocks), _p(err), _p(totals), 15, st)
        _lib.check(rc, "voge_mesh_clean_scan")
        Vk, Fk, bad = (int(x) for x in totals.tolist())      # the synchronisation
        if bad:
            raise ValueError(f"mesh_clean: a face names a vertex, or carries a label, outside [0, {V})")
        out_v, out_f = empty(Vk, True, torch.float32), empty(Fk, True, torch.int32)
        vert_index, face_index = empty(Vk, False, torch.int32), empty(Fk, False, torch.int32)
        rc = lib.voge_mesh_clean_emit(_p(v), _p(f), F, V, _p(fl), _p(kr), _p(vflag), _p(loc), _p(blocks), Vk, Fk, _p(out_v) if Vk else None,
                                      _p(out_f) if Fk else None, _p(vert_index) if Vk else None, _p(face_index) if Fk else None, st)
        _lib.check(rc, "voge_mesh_clean_emit")
    return out_v, out_f, vert_index, face_index


def vertex_normals(verts, faces):
    """normals [V,3] fp32 of verts [V,3] fp32, faces [F,3] int32 on a HIP device (extension; voge_vertex_normals): the values of
    Aggregation.mesh_vertex_normals.  Four launches on the current stream from the stream's cached workspace, nothing read back:
    capturable.  Fixed-point sums with integer atomics: the same bits on every run and for every order of the faces.  Not
    differentiable."""
    v = _mesh_verts(verts, "vertex_normals")
    f = _mesh_faces(faces, "vertex_normals")
    V, F, dev = v.shape[0], f.shape[0], v.device
    if f.device != dev:
        raise _lib.VogeHipError(f"vertex_normals: verts on {dev}, faces on {f.device}")
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if V == 0:
        return out
    lib = _lib.load()
    with _on(dev):
        ws, nbytes = _sized_workspace(dev, lib.voge_vertex_normals_workspace_bytes, V)
        rc = lib.voge_vertex_normals(_p(v), V, _p(f) if F else None, F, _p(out), _p(ws), nbytes, 15, _stream())
    _lib.check(rc, "voge_vertex_normals")
    return out


MESH_SIMPLIFY_BLOCK = MESH_CLEAN_BLOCK      # the scans are mesh_clean.hip's (csrc/mesh_scan.h)
MESH_SIMPLIFY_TOP = MESH_CLEAN_TOP
MESH_SIMPLIFY_CHANNELS = 8                  # kSimpChannels of mesh_simplify.hip: the attribute channels of one launch set
MESH_SIMPLIFY_MAX_CELLS = 2 ** 21 - 1       # cells on an axis (Aggregation.MESH_SIMPLIFY_MAX_CELLS)
MESH_SIMPLIFY_LAMBDA = 1e-3                 # kSimpLambda


def mesh_simplify_capacity(V, F):
    """Entries of the table voge_mesh_simplify_scan probes: the power of two >= 2 max(V, F) (the tests step it)"""
    return 1 << max(2 * max(int(V), int(F)) - 1, 0).bit_length()


def mesh_simplify_scales(V, F):
    """(sp, sq): the fixed-point exponents of the position and the quadric sums (mesh_simplify.hip's header, SCALES)"""
    return 60 - max(int(V) - 1, 0).bit_length(), 60 - max(3 * int(F) - 1, 0).bit_length()


def mesh_simplify(verts, faces, cell_size, placement="mean", attr=None):
    """(verts' [V',3] fp32, faces' [F',3] int32, attr' [V',C] fp32 or None, vert_index [V] int32, face_index [F'] int32) of verts
    [V,3] fp32, faces [F,3] int32 (and attr [V,C] fp32) on a HIP device (extension; voge_mesh_simplify_scan / _emit / _attr): the
    values of Aggregation.mesh_simplify -- equal labels, faces and index tables; positions and attributes within the bounds
    mesh_simplify.hip's header derives.  cell_size: three fp32 numbers.  The scan's launches on the stream's cached workspace, then
    V', F' and the error word are read back on the host -- ONE synchronisation, what sizes the outputs -- and the launches that
    write them.  ValueError for an index outside [0, V), a vertex that is not finite and more than 2^21 - 1 cells on an axis.
    Fixed-point sums with integer atomics: the same bits on every run and for every order of the faces.  Not differentiable, not
    capturable."""
    v = _mesh_verts(verts, "mesh_simplify")
    f = _mesh_faces(faces, "mesh_simplify")
    V, F, dev = v.shape[0], f.shape[0], v.device
    if placement not in ("mean", "quadric"):
        raise ValueError(f"mesh_simplify: placement 'mean' or 'quadric' expected, got {placement!r}")
    quadric = int(placement == "quadric")
    h = [float(x) for x in cell_size]
    a = None
    if attr is not None:
        a = _dev(attr.detach(), torch.float32, "attr")
        if a.dim() != 2 or a.shape[0] != V or a.device != dev:
            raise ValueError(f"mesh_simplify: attr [{V},C] on {dev} expected, got {tuple(a.shape)} on {a.device}")
    if f.device != dev:
        raise _lib.VogeHipError(f"mesh_simplify: verts on {dev}, faces on {f.device}")
    C = 0 if a is None else a.shape[1]
    if V == 0 and F > 0:
        raise ValueError("mesh_simplify: a face names a vertex outside [0, 0)")
    empty = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    none = lambda: (empty((0, 3), torch.float32), empty((0, 3), torch.int32), None if a is None else empty((0, C), torch.float32),
                    torch.full((V,), -1, dtype=torch.int32, device=dev), empty((0,), torch.int32))
    if V == 0:
        return none()
    if F == 0:      # (no face, no output; the vertices are still examined -- one comparison read back)
        if not bool(torch.isfinite(v).all()):
            raise ValueError("mesh_simplify: a vertex is not finite")
        return none()
    totals = empty((3,), torch.int64)
    lib = _lib.load()
    with _on(dev):
        st = _stream()
        ws, nbytes = _sized_workspace(dev, lib.voge_mesh_simplify_workspace_bytes, V, F)
        rc = lib.voge_mesh_simplify_scan(_p(v), V, _p(f), F, h[0], h[1], h[2], _p(ws), nbytes, _p(totals), 255, st)
        _lib.check(rc, "voge_mesh_simplify_scan")
        Vk, Fk, bad = (int(x) for x in totals.tolist())      # the synchronisation
        if bad & 4:
            raise ValueError("mesh_simplify: a vertex is not finite")
        if bad & 2:
            raise ValueError(f"mesh_simplify: a face names a vertex outside [0, {V})")
        if bad & 8:
            raise ValueError(f"mesh_simplify: more than {MESH_SIMPLIFY_MAX_CELLS} cells on an axis")
        if bad:
            raise _lib.VogeHipError(f"voge_mesh_simplify_scan: a probe of the table reached its cap (error word {bad})")
        if Vk == 0 or Fk == 0:
            return none()
        out_v, out_f = empty((Vk, 3), torch.float32), empty((Fk, 3), torch.int32)
        vert_index, face_index = empty((V,), torch.int32), empty((Fk,), torch.int32)
        acc_bytes = lib.voge_mesh_simplify_acc_bytes(Vk, quadric)
        acc = empty((acc_bytes // 8,), torch.int64)
        rc = lib.voge_mesh_simplify_emit(_p(v), V, _p(f), F, h[0], h[1], h[2], quadric, _p(ws), nbytes, Vk, Fk, _p(acc), acc_bytes, _p(out_v),
                                         _p(out_f), _p(vert_index), _p(face_index), 15, st)
        _lib.check(rc, "voge_mesh_simplify_emit")
        out_a = None
        if a is not None:
            out_a = empty((Vk, C), torch.float32)
            if C:
                abytes = lib.voge_mesh_simplify_attr_workspace_bytes(Vk)
                aws = empty((abytes // 8,), torch.int64)
            for c0 in range(0, C, MESH_SIMPLIFY_CHANNELS):      # (more channels than one launch set takes: one per slice of them)
                rc = lib.voge_mesh_simplify_attr(_p(a), V, F, C, c0, min(MESH_SIMPLIFY_CHANNELS, C - c0), _p(ws), nbytes, Vk, _p(acc), quadric,
                                                 _p(aws), abytes, _p(out_a), 15, st)
                _lib.check(rc, "voge_mesh_simplify_attr")
    return out_v, out_f, out_a, vert_index, face_index


MESH_RASTER_TILE = 16      # kMrTile of mesh_raster.hip: a tile's edge in pixels, one workgroup of 256 lanes
# route=None: "brute" while B tiles F <= this many (tile, face) pairs, "bins" above.  Measured (tools/mesh_raster_time.py,
# profiles/r31_mesh_raster.txt): "brute" is the faster route at EVERY work measured up to 3.36e8 (one 512^2 view of 327 680 faces:
# 1.50 against 1.72 ms; five 128^2 views: 2.2 - 2.4 x faster at every size), the two approaching each other on the 512^2 image.  The
# constant sits just above the largest work at which "brute" was seen to win; the crossover itself lies beyond what was measured.
MESH_RASTER_BINS_MIN_WORK = 1 << 29
MESH_RASTER_ROUTES = (None, "brute", "bins")


def mesh_raster_route(B, H, W, F, route=None):
    """The route mesh_rasterize takes: `route` itself when given, else by MESH_RASTER_BINS_MIN_WORK"""
    if route not in MESH_RASTER_ROUTES:
        raise ValueError(f"mesh_rasterize: route None, 'brute' or 'bins' expected, got {route!r}")
    if route is not None:
        return route
    tiles = ((H + MESH_RASTER_TILE - 1) // MESH_RASTER_TILE) * ((W + MESH_RASTER_TILE - 1) // MESH_RASTER_TILE)
    return "brute" if B * tiles * F <= MESH_RASTER_BINS_MIN_WORK else "bins"


class _MeshRaster(torch.autograd.Function):
    """Mesh depth maps (extension; voge_mesh_raster_fwd / _bwd): forward(verts [V,3], faces [F,3] int32 | int64, R [B,3,3], T [B,3],
    focal [B,2], pp [B,2], H, W, cull_backfaces, route) -> (pix_to_face [B,H,W] int32, bary [B,H,W,3], depth [B,H,W]), the fp32 bits
    of Aggregation.mesh_rasterize, the same on both routes.  route "brute": two launches on the current stream from the stream's
    cached workspace, nothing read back (capturable).  route "bins": five launches, ONE number read back on the host (the length of
    the tiles' lists: one synchronisation), two more launches; ValueError when that length does not fit 31 bits.  int64 faces cost
    one cast.  Only depth is differentiable, and only to verts: four launches (zero fill, largest |term|, integer-atomic scatter,
    finish), every element of g_verts written, the same bits on every run, nothing read back.  No double backward."""

    @staticmethod
    def forward(ctx, verts, faces, R, T, focal, pp, H, W, cull_backfaces, route):
        v = _mesh_verts(verts, "mesh_rasterize")
        f = _mesh_faces(faces, "mesh_rasterize")
        dev = v.device
        R, T = _dev(R.detach(), torch.float32, "R"), _dev(T.detach(), torch.float32, "T")
        focal, pp = _dev(focal.detach(), torch.float32, "focal"), _dev(pp.detach(), torch.float32, "pp")
        B, V, F, H, W = R.shape[0], v.shape[0], f.shape[0], int(H), int(W)
        if tuple(R.shape) != (B, 3, 3) or tuple(T.shape) != (B, 3) or tuple(focal.shape) != (B, 2) or tuple(pp.shape) != (B, 2):
            raise ValueError(f"mesh_rasterize: R [B,3,3], T [B,3], focal [B,2], pp [B,2] expected, got {tuple(R.shape)} / {tuple(T.shape)} / "
                             f"{tuple(focal.shape)} / {tuple(pp.shape)}")
        if any(t.device != dev for t in (f, R, T, focal, pp)):
            raise _lib.VogeHipError(f"mesh_rasterize: verts on {dev}, faces on {f.device}, the cameras on {R.device}")
        if H < 1 or W < 1 or B * H * W >= 2 ** 31:
            raise ValueError(f"mesh_rasterize: B H W = {B} x {H} x {W} must lie in [1, 2^31) with H, W >= 1")
        if V == 0 and F > 0:
            raise ValueError("mesh_rasterize: a face names a vertex outside [0, 0)")
        route = mesh_raster_route(B, H, W, F, route)
        pix_to_face = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        bary = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        if B > 0:
            lib = _lib.load()
            cull = int(bool(cull_backfaces))
            with _on(dev):
                st = _stream()
                ws, nbytes = _sized_workspace(dev, lib.voge_mesh_raster_workspace_bytes, B, V, F, H, W)
                args = (_p(v) if V else None, V, _p(f) if F else None, F, _p(R), _p(T), _p(focal), _p(pp), B, H, W, cull)
                outs = (_p(pix_to_face), _p(bary), _p(depth))
                if route == "brute":
                    rc = lib.voge_mesh_raster_fwd(*args, 9, None, 0, *outs, None, _p(ws), nbytes, st)
                else:
                    total = torch.empty((1,), dtype=torch.int64, device=dev)
                    rc = lib.voge_mesh_raster_fwd(*args, 3, None, 0, *outs, _p(total), _p(ws), nbytes, st)
                    _lib.check(rc, "voge_mesh_raster_fwd")
                    n = int(total.item())      # the synchronisation
                    if n >= 2 ** 31:
                        raise ValueError(f"mesh_rasterize: the tiles' lists hold {n} entries, more than 2^31 - 1")
                    lists = torch.empty((n,), dtype=torch.int32, device=dev)
                    rc = lib.voge_mesh_raster_fwd(*args, 12, _p(lists) if n else None, n, *outs, None, _p(ws), nbytes, st)
            _lib.check(rc, "voge_mesh_raster_fwd")
        ctx.save_for_backward(v, f, R, T, focal, pp, pix_to_face)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(pix_to_face, bary)
        return pix_to_face, bary, depth

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gp, _gb, g_depth):
        if g_depth is None or not ctx.needs_input_grad[0]:
            return (None,) * 10
        v, f, R, T, focal, pp, pix_to_face = ctx.saved_tensors
        B, H, W = pix_to_face.shape
        V, F = v.shape[0], f.shape[0]
        if V == 0 or B == 0:
            return (torch.zeros_like(v),) + (None,) * 9
        lib = _lib.load()
        g = _dev(g_depth, torch.float32, "grad_depth")
        g_verts = torch.empty_like(v)
        with _on(v.device):
            ws, nbytes = _sized_workspace(v.device, lib.voge_mesh_raster_workspace_bytes, B, V, F, H, W)
            rc = lib.voge_mesh_raster_bwd(_p(v), V, _p(f) if F else None, F, _p(R), _p(T), _p(focal), _p(pp), B, H, W, _p(pix_to_face), _p(g),
                                          _p(g_verts), _p(ws), nbytes, _stream())
        _lib.check(rc, "voge_mesh_raster_bwd")
        return (g_verts,) + (None,) * 9


def mesh_rasterize(verts, faces, R, T, focal, pp, H, W, cull_backfaces=False, route=None):
    """(pix_to_face int32, bary, depth) of ONE mesh under B cameras on a HIP device: _MeshRaster.apply"""
    return _MeshRaster.apply(verts, faces, R, T, focal, pp, H, W, cull_backfaces, route)


class _DepthNormals(torch.autograd.Function):
    """Normals of a depth map (extension; voge_depth_normals_fwd / _bwd): forward(depth [B,h,W], R [B,3,3], focal [B,2], pp [B,2],
    row0, edge (None | relative depth jump), view_space) -> [B,h,W,3], the values of Aggregation.depth_normals on the rays of
    image rows row0 .. row0+h-1 (times R when view_space).  The kernels make the rays from the camera; one launch each way on the
    current stream and no allocation but the outputs.  The backward recomputes every stencil from the saved INPUTS (the forward
    saves nothing of its own) as a gather: every element of g_depth is written, no zero fill, no atomics, the same bits on every
    run.  The camera gets no gradient here -- Renderer.get_normals sends a camera that wants one to the torch definition."""

    @staticmethod
    def forward(ctx, depth, R, focal, pp, row0, edge, view_space):
        depth = _dev(depth, torch.float32, "depth")
        R, focal, pp = _dev(R, torch.float32, "R"), _dev(focal, torch.float32, "focal_length"), _dev(pp, torch.float32, "principal_point")
        lib = _lib.load()
        if depth.dim() != 3 or R.shape != (depth.shape[0], 3, 3) or focal.shape != (depth.shape[0], 2) or pp.shape != focal.shape:
            raise ValueError(f"depth_normals: depth {tuple(depth.shape)}, R {tuple(R.shape)}, focal_length {tuple(focal.shape)} and "
                             f"principal_point {tuple(pp.shape)} do not describe the same views")
        B, h, W = depth.shape
        edge = -1.0 if edge is None else float(edge)
        out = torch.empty((B, h, W, 3), dtype=torch.float32, device=depth.device)
        with _on(depth.device):
            rc = lib.voge_depth_normals_fwd(_p(depth), _p(R), _p(focal), _p(pp), B, int(row0), h, W, edge, int(bool(view_space)), _p(out),
                                            _stream())
        _lib.check(rc, "voge_depth_normals_fwd")
        ctx.save_for_backward(depth, R, focal, pp)
        ctx.args = (int(row0), edge, int(bool(view_space)))
        return out

    @staticmethod
    def backward(ctx, g_normals):
        lib = _lib.load()
        depth, R, focal, pp = ctx.saved_tensors
        B, h, W = depth.shape
        row0, edge, view_space = ctx.args
        gn = _dev(g_normals, torch.float32, "grad_normals")
        g_depth = (torch.zeros_like if depth.numel() == 0 else torch.empty_like)(depth)      # (nothing is launched for an empty map)
        with _on(depth.device):
            rc = lib.voge_depth_normals_bwd(_p(depth), _p(R), _p(focal), _p(pp), _p(gn), B, row0, h, W, edge, view_space, _p(g_depth),
                                            _stream())
        _lib.check(rc, "voge_depth_normals_bwd")
        return g_depth, None, None, None, None, None, None


class _PixelRays(torch.autograd.Function):
    """Ray bundle of VoGE/Renderer.py:124-130: (R [B,3,3], T [B,3], focal [B,2], pp [B,2]) ->
    unit world-space directions [B,h,W,3] of image rows row0..row0+h-1 and the camera centres [B,3]."""

    @staticmethod
    def forward(ctx, R, T, focal, pp, row0, h, W, stripe_h=None, pitch=0):
        lib = _lib.load()
        stripe_h = max(int(h), 1) if stripe_h is None else int(stripe_h)      # (None: one contiguous band)
        R_c, T_c = _dev(R, torch.float32, "R"), _dev(T, torch.float32, "T")
        f_c, p_c = _dev(focal, torch.float32, "focal_length"), _dev(pp, torch.float32, "principal_point")
        B = R_c.shape[0]
        assert R_c.shape == (B, 3, 3) and T_c.shape == (B, 3) and f_c.shape == (B, 2) and p_c.shape == (B, 2)
        rays = torch.empty((B, h, W, 3), dtype=torch.float32, device=R_c.device)
        origin = torch.empty((B, 3), dtype=torch.float32, device=R_c.device)
        # bounding cones of the band's 32x32-pixel super-tiles: the trace's culling aid, made here for free
        cones = torch.empty((max(int(lib.voge_cones_floats(B, int(h), int(W))), 1),), dtype=torch.float32, device=R_c.device)
        with _on(R_c.device):
            rc = lib.voge_rays_striped_fwd(_p(R_c), _p(T_c), _p(f_c), _p(p_c), B, int(row0), int(h), stripe_h, int(pitch), int(W),
                                           _p(rays), _p(origin), _p(cones), _stream())
        _lib.check(rc, "voge_rays_striped_fwd")
        ctx.save_for_backward(R_c, T_c, f_c, p_c)
        ctx.geom = (int(row0), int(h), int(W), stripe_h, int(pitch))
        ctx.mark_non_differentiable(cones)
        return rays, origin, cones

    @staticmethod
    def backward(ctx, g_rays, g_origin, _g_cones):
        lib = _lib.load()
        R, T, f, pp = ctx.saved_tensors
        row0, h, W, stripe_h, pitch = ctx.geom
        B = R.shape[0]
        gr = None if g_rays is None else _dev(g_rays, torch.float32, "grad_rays")
        go = None if g_origin is None else _dev(g_origin, torch.float32, "grad_origin")
        need = ctx.needs_input_grad
        g_R = torch.empty_like(R) if need[0] else None
        g_T = torch.empty_like(T) if need[1] else None
        g_f = torch.empty_like(f) if need[2] else None
        g_p = torch.empty_like(pp) if need[3] else None
        scratch = torch.empty((B, 16), dtype=torch.float32, device=R.device)
        with _on(R.device):
            rc = lib.voge_rays_striped_bwd(_p(R), _p(T), _p(f), _p(pp), _p(gr), _p(go), B, row0, h, stripe_h, pitch, W, _p(scratch),
                                           _p(g_R), _p(g_T), _p(g_f), _p(g_p), _stream())
        _lib.check(rc, "voge_rays_striped_bwd")
        return g_R, g_T, g_f, g_p, None, None, None, None, None


class _RayTraceVoGERay(torch.autograd.Function):
    """Dense trace, mirror of VoGE/RayTracing.py:209-220: (mus [M,3], sigmas [M,3,3], rays [N,3]) ->
    hit_len, hit_act, hit_dsd [N,M]."""

    @staticmethod
    def forward(ctx, mus, sigmas, rays):
        lib = _lib.load()
        mus_c, sig_c, rays_c = _dev(mus, torch.float32, "mus"), _dev(sigmas, torch.float32, "sigmas"), _dev(rays, torch.float32, "rays")
        M, N = mus_c.shape[0], rays_c.shape[0]
        out = [torch.empty((N, M), dtype=torch.float32, device=rays_c.device) for _ in range(3)]
        with _on(rays_c.device):
            rc = lib.voge_ray_dense_fwd(_p(mus_c), _p(sig_c), _p(rays_c), M, N, _p(out[0]), _p(out[1]), _p(out[2]), _stream())
        _lib.check(rc, "voge_ray_dense_fwd")
        ctx.save_for_backward(mus_c, sig_c, rays_c)
        return tuple(out)

    @staticmethod
    def backward(ctx, g_len, g_act, g_dsd):
        lib = _lib.load()
        mus, sig, rays = ctx.saved_tensors
        M, N = mus.shape[0], rays.shape[0]
        gs = [torch.zeros((N, M), dtype=torch.float32, device=rays.device) if g is None else _dev(g, torch.float32, "grad")
              for g in (g_len, g_act, g_dsd)]
        g_ray, g_mus, g_sig = torch.empty_like(rays), torch.empty_like(mus), torch.empty_like(sig)
        with _on(rays.device):
            rc = lib.voge_ray_dense_bwd(_p(mus), _p(sig), _p(rays), _p(gs[0]), _p(gs[1]), _p(gs[2]), M, N, _p(g_ray),
                                        _p(g_mus), _p(g_sig), _stream())
        _lib.check(rc, "voge_ray_dense_bwd")
        return g_mus, g_sig, g_ray


class _FindNearestK(torch.autograd.Function):
    """Mirror of VoGE/RayTracing.py:223-241 with the intended gradient (zero for empty slots)."""

    @staticmethod
    def forward(ctx, hit_len_in, hit_act_in, hit_dsd_in, thr_act, K):
        lib = _lib.load()
        l, a, d = (_dev(t, torch.float32, "hit") for t in (hit_len_in, hit_act_in, hit_dsd_in))
        N, M = l.shape
        idx = torch.empty((N, K), dtype=torch.int32, device=l.device)
        outs = [torch.empty((N, K), dtype=torch.float32, device=l.device) for _ in range(3)]
        with _on(l.device):
            rc = lib.voge_find_nearest_k(_p(l), _p(a), _p(d), float(thr_act), M, int(K), N, _p(idx), _p(outs[0]),
                                         _p(outs[1]), _p(outs[2]), _stream())
        _lib.check(rc, "voge_find_nearest_k")
        ctx.save_for_backward(idx)
        ctx.M = M
        ctx.mark_non_differentiable(idx)
        return idx, outs[0], outs[1], outs[2]

    @staticmethod
    def backward(ctx, _g_idx, g_len, g_act, g_dsd):
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        N, K = idx.shape
        gs = [torch.zeros((N, K), dtype=torch.float32, device=idx.device) if g is None else _dev(g, torch.float32, "grad")
              for g in (g_len, g_act, g_dsd)]
        gi = [torch.empty((N, ctx.M), dtype=torch.float32, device=idx.device) for _ in range(3)]
        with _on(idx.device):
            rc = lib.voge_find_nearest_k_bwd(_p(idx), _p(gs[0]), _p(gs[1]), _p(gs[2]), ctx.M, K, N, _p(gi[0]), _p(gi[1]),
                                             _p(gi[2]), _stream())
        _lib.check(rc, "voge_find_nearest_k_bwd")
        return gi[0], gi[1], gi[2], None, None


class _ScatterAttr(torch.autograd.Function):
    """Transpose of merge_final: out[v, c] = sum over slots (pixel, k < valid) with index v of
    weight * pix_attr[pixel, c].  This is sample_voge (VoGE/csrc/sample_voge/sample_voge.cu:35-66)
    when pix_attr = [image | 1]; it runs on the merge-backward kernel and its own backward on the
    merge forward/backward kernels."""

    @staticmethod
    def forward(ctx, pix_attr, weight, idx, valid_num, n_vert):
        lib = _lib.load()
        pa = _dev(pix_attr, torch.float32, "image")
        w = _dev(weight, torch.float32, "weight")
        ix = _dev(idx, torch.int32, "vert_index")
        vn = _dev(valid_num, torch.int64, "valid_num")
        K = ix.shape[-1]
        C = pa.shape[-1]
        npix = ix.numel() // max(K, 1)
        Wd = ix.shape[-2] if ix.dim() >= 3 else npix
        out = torch.empty((int(n_vert), C), dtype=torch.float32, device=ix.device)
        with _on(ix.device):
            rc = lib.voge_merge_bwd(None, _p(ix), _p(w), _p(vn), _p(pa), npix // max(Wd, 1), Wd, K, C, int(n_vert), _p(out),
                                    None, _stream())
        _lib.check(rc, "voge_merge_bwd")
        ctx.save_for_backward(pa, w, ix, vn)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        pa, w, ix, vn = ctx.saved_tensors
        K = ix.shape[-1]
        C = pa.shape[-1]
        npix = ix.numel() // max(K, 1)
        Wd = ix.shape[-2] if ix.dim() >= 3 else npix
        go = _dev(g_out, torch.float32, "grad_features")
        nv = go.shape[0]
        g_pa = torch.empty_like(pa) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        with _on(ix.device):
            if g_pa is not None:   # g_pix_attr = merge(g_out): sum_k w * g_out[idx_k]
                rc = lib.voge_merge_fwd(_p(go), _p(ix), _p(w), _p(vn), npix, K, C, nv, 0, _p(g_pa), _stream())
                _lib.check(rc, "voge_merge_fwd")
            if g_w is not None:    # g_w = <pix_attr, g_out[idx]>
                rc = lib.voge_merge_bwd(_p(go), _p(ix), _p(w), _p(vn), _p(pa), npix // max(Wd, 1), Wd, K, C, nv, None,
                                        _p(g_w), _stream())
                _lib.check(rc, "voge_merge_bwd")
        return g_pa, g_w, None, None, None


def rasterize_points_coarse(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius, bin_size,
                            max_points_per_bin):
    """The reference's coarse stage (VoGE._C.rasterize_points_coarse, rasterize_coarse.h:18-25) -> bin_elems
    [B,BH,BW,M] int32, -1 padded.  No gradient, like the reference (RayTracing.py:126-151)."""
    lib = _lib.load()
    pts = _dev(points.detach(), torch.float32, "points")
    rad = _dev(radius.detach(), torch.float32, "radius")
    first = _dev(cloud_to_packed_first_idx, torch.int64, "cloud_to_packed_first_idx")
    num = _dev(num_points_per_cloud, torch.int64, "num_points_per_cloud")
    assert pts.dim() == 2 and pts.shape[1] == 3 and rad.shape == (pts.shape[0], 2)
    H, W = int(image_size[0]), int(image_size[1])
    B = first.shape[0]
    out = torch.empty((B, 1 + (H - 1) // int(bin_size), 1 + (W - 1) // int(bin_size), int(max_points_per_bin)),
                      dtype=torch.int32, device=pts.device)
    with _on(pts.device):
        rc = lib.voge_bin_gaussians(_p(pts), _p(first), _p(num), B, pts.shape[0], H, W, _p(rad), int(bin_size),
                                    int(max_points_per_bin), _p(out), _stream())
    _lib.check(rc, "voge_bin_gaussians")
    return out


def scatter_attr(pix_attr, weight, idx, valid_num, n_vert):
    return _ScatterAttr.apply(pix_attr, weight, idx, valid_num, n_vert)


def scatter_max(weight, idx, n_vert):
    lib = _lib.load()
    w = _dev(weight.detach(), torch.float32, "weight")
    ix = _dev(idx, torch.int32, "vert_index")
    out = torch.empty((int(n_vert),), dtype=torch.float32, device=w.device)
    with _on(w.device):
        rc = lib.voge_scatter_max(_p(w), _p(ix), w.numel(), int(n_vert), _p(out), _stream())
    _lib.check(rc, "voge_scatter_max")
    return out


def pixel_rays(R, T, focal, pp, row0, h, W, stripe_h=None, pitch=0):
    """rays [B,h,W,3] of image rows row0 .. row0+h-1, or (stripe_h, pitch given) of every pitch-th stripe of stripe_h rows
    from row0 on, h rows in total; origin [B,3]."""
    rays, origin, cones = _PixelRays.apply(R, T, focal, pp, row0, h, W, stripe_h, pitch)
    rays.voge_cones = (cones, rays._version)      # see cones_of()
    return rays, origin


def ray_trace_fine(mus, isigmas, rays, bin_points, thr_act, bin_size, n_assign):
    return _RayTraceVoGE.apply(mus, isigmas, rays, bin_points, thr_act, bin_size, n_assign)


def composite(sel_idx, sel_act, sel_len, sel_dsd, occ=1.0):
    return _Composite.apply(sel_idx, sel_act, sel_len, sel_dsd, occ)


def merge(attr, weight, idx, valid_num):
    return _Merge.apply(attr, weight, idx, valid_num)


def blend(rgb, weight, bg, thr=-1.0):
    return _Blend.apply(rgb, weight, bg, thr)


def shade(attr, weight, idx, valid_num, bg, thr=-1.0):
    return _Shade.apply(attr, weight, idx, valid_num, bg, thr)


def silhouette(weight):
    return _Silhouette.apply(weight)


def depth(weight, hit_length, valid_num, normalize=True, background=0.0):
    return _Depth.apply(weight, hit_length, valid_num, bool(normalize), float(background))


def distortion(weight, hit_length, valid_num, normalize=False):
    return _Distortion.apply(weight, hit_length, valid_num, bool(normalize))


def sh_colors(sh, verts, centres, degree, clamp=True):
    return _ShColors.apply(sh, verts, centres, degree, clamp)


def gauss_normals(scales, quats, verts, centres, inverse_sigma=False):
    return _GaussNormals.apply(scales, quats, verts, centres, inverse_sigma)


def mesh_reg(verts, topo, target_length=0.0, terms=7):
    return _MeshReg.apply(verts, topo, float(target_length), int(terms))


def depth_normals(depth, R, focal, pp, row0=0, edge=None, view_space=False):
    return _DepthNormals.apply(depth, R, focal, pp, row0, edge, view_space)
