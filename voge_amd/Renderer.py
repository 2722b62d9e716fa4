"""Host-side mirror of VoGE/Renderer.py: GaussianRenderer (:87-150), GaussianRenderSettings
(:53-84), Fragments (:13-50), interpolate_attr (:153), get_silhouette (:157-159),
to_colored_background (:162-171), to_white_background (:174-176) -- same names, same argument
meaning; get_depth, get_distortion, get_normals, sh_to_colors, gaussian_normals and get_rendered_normals are extensions.  Every stage behind these calls is a HIP kernel (voge_amd.ops); a renderer on CPU
tensors raises instead of falling back.
"""
import math
import os
from typing import Tuple, Union

import torch
import torch.nn as nn

from . import ops
from .Aggregation import (aggregation, depth_normals, distortion, expend_sigma, gaussian_normals as _gaussian_normals_def,
                          gaussian_normals_shapes, merge_final, oriented_sigma, sh_colors, sh_degree)
from . import RayTracing
from .RayTracing import _view_axis
from .cameras import camera_tensors, pixel_rays

# Fold `verts - origin` and `2 * sigmas` into the trace kernels when the inputs allow it (see forward()).
# VOGE_FUSED_PREAMBLE=0 (or setting this flag) keeps the reference's elementwise torch ops: same results.
FUSED_PREAMBLE = os.environ.get("VOGE_FUSED_PREAMBLE", "1") != "0"


class Fragments(object):
    """vert_weight [.., K] f32, vert_index [.., K] i32, valid_num [..] i64, vert_hit_length [.., K] f32.

    Same fields and methods as VoGE/Renderer.py:13-50.  Fragments made by this renderer from scalar sigmas may arrive
    with their composite DEFERRED (`_lazy`): vert_index and vert_hit_length are there, vert_weight / valid_num are
    computed the first time anybody reads them -- or never, when to_colored_background gets the fragments first and
    produces weights and image in one pass (ops._CompositeShade).  Reading the attributes is all it takes; nothing about
    the values depends on when that happens."""

    _fields = ("vert_weight", "vert_index", "valid_num", "vert_hit_length")

    def __init__(self, vert_weight, vert_index, valid_num, vert_hit_length, _lazy=None):
        self._vert_weight = vert_weight
        self.vert_index = vert_index
        self._valid_num = valid_num
        self._hit_length = vert_hit_length
        self._lazy = _lazy if vert_weight is None else None
        # (the camera-input trace hands out vert_hit_length without a grad_fn; the differentiable alias is made when it is read)
        self._hl_src = _lazy if (_lazy is not None and _lazy.frame and _lazy.sel_len is vert_hit_length) else None
        self._wsum = None      # (per-pixel weight sum left by a one-pass composite + merge: see get_silhouette)
        # (a reshaped view -- squeeze / unsqueeze -- of fragments whose composite is still pending: (its leading dimensions, the
        #  number of leading dimensions of the trace's own tensors); what the deferred composite returns is viewed to that: _shaped)
        self._lead = None

    def _shaped(self, t_):
        """A tensor the deferred composite made in the trace's own shape, as THESE fragments' view of it (the same memory;
        ops.carry_tags hands the bookkeeping on)."""
        if self._lead is None or t_ is None:
            return t_
        lead, nlead = self._lead
        return ops.carry_tags(t_, t_.view(lead + tuple(t_.shape[nlead:])))

    @property
    def vert_hit_length(self):
        if self._hl_src is not None:
            self._hit_length, self._hl_src = self._shaped(self._hl_src.hit_length()), None
        return self._hit_length

    @vert_hit_length.setter
    def vert_hit_length(self, value):
        self._hit_length, self._hl_src = value, None

    def _composite(self):
        self._set_composite(*ops.composite_lean(self._lazy))

    def _set_composite(self, weight, valid_num):
        self._lazy = None
        self._vert_weight, self._valid_num = self._shaped(weight), self._shaped(valid_num)

    @property
    def vert_weight(self):
        if self._lazy is not None:
            self._composite()
        return self._vert_weight

    @vert_weight.setter
    def vert_weight(self, value):
        if self._lazy is not None and self._valid_num is None:      # (the reference's Fragments always has valid_num)
            self._valid_num = self._shaped(self._lazy.cnt.to(torch.int64))
        self._lazy = None
        self._wsum = None
        self._vert_weight = value

    @property
    def valid_num(self):
        if self._valid_num is None and self._lazy is not None:
            self._valid_num = self._shaped(self._lazy.cnt.to(torch.int64))      # (= the trace's hit count; the composite writes the same)
        return self._valid_num

    @valid_num.setter
    def valid_num(self, value):
        self._valid_num = value

    def _map(self, fn):
        # (views of the same memory keep the trace's bookkeeping -- ops.carry_tags -- so frag.copy(), frag.squeeze()
        #  and frag.unsqueeze() stay on the fast paths, as RenderBunny.py:45's to_white_background(frag.copy(), ...))
        if self._lazy is not None:
            # nothing composited yet: a reshaped view of the same memory (squeeze / unsqueeze / [0] of a one-view batch) stays
            # deferred -- the one-pass forms remain open to it; a true slice composites now and goes on below
            idx = self.vert_index
            v = fn(idx)
            if v.data_ptr() == idx.data_ptr() and v.numel() == idx.numel() and v.is_contiguous():
                out = Fragments(None, ops.carry_tags(idx, v), None if self._valid_num is None else fn(self._valid_num),
                                ops.carry_tags(self._hit_length, fn(self._hit_length)), _lazy=self._lazy)
                out._hl_src = self._hl_src
                out._lead = (tuple(v.shape[:-1]), self._lazy.sel_idx.dim() - 1)
                return out
        return Fragments(**{k: ops.carry_tags(getattr(self, k), fn(getattr(self, k))) for k in self._fields})

    def __getitem__(self, item):
        assert self.vert_index.dim() == 4, 'Index access is only available when batched.'
        return self._map(lambda t: t[item])

    def __len__(self):
        return self.vert_index.shape[0]

    @property
    def shape(self):
        return tuple(getattr(self, k).shape for k in self._fields)

    def squeeze(self):
        assert self.vert_index.shape[0] == 1
        return self[0]

    def unsqueeze(self):
        assert self.vert_index.dim() == 3
        return self._map(lambda t: t.unsqueeze(0))

    def to_dict(self):
        return {k: getattr(self, k) for k in self._fields}

    def copy(self):
        if self._lazy is not None:      # nothing to copy yet: the same deferred composite (tensors are shared either way,
            out = Fragments(None, self.vert_index, self._valid_num, self._hit_length, _lazy=self._lazy)   # .contiguous() is a no-op)
            out._hl_src, out._lead = self._hl_src, self._lead
            return out
        return self._map(lambda t: t.contiguous())


class GaussianRenderSettings:
    __slots__ = ['image_size', 'max_assign', 'thr_activation', 'absorptivity', 'inverse_sigma', 'principal',
                 'max_point_per_bin']

    def __init__(self, image_size: Union[int, Tuple[int, int]] = 256, max_assign: int = 20,
                 thr_activation: float = 0.01, absorptivity: float = 1, inverse_sigma: bool = False,
                 principal: Union[None, Tuple[int, int], Tuple[float, float]] = None,
                 max_point_per_bin: Union[None, int] = None, **kwargs):
        # unknown keywords (batch_size=, principal_point=, ...) are accepted and ignored, as in
        # Renderer.py:70
        self.image_size = (image_size, image_size) if isinstance(image_size, int) else image_size
        self.max_assign = max_assign
        self.thr_activation = thr_activation
        self.absorptivity = absorptivity
        self.inverse_sigma = inverse_sigma
        self.principal = principal
        self.max_point_per_bin = max_point_per_bin

    def __getitem__(self, item):
        return getattr(self, item)


class _Overridden:
    """Render settings with some entries replaced for one call (the settings object itself is the caller's)."""

    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getitem__(self, item):
        return self._over[item] if item in self._over else self._base[item]


class GaussianRenderer(nn.Module):
    to_set_args = ['R', 'T', 'focal', 'principal']

    def __init__(self, cameras, render_settings: Union[dict, GaussianRenderSettings]):
        super().__init__()
        self.cameras = cameras
        self.render_settings = render_settings
        self.device = cameras.device
        object.__setattr__(self, "_frame_memo", None)      # (see _frame_camera)

    def to(self, device):
        # cameras are not nn.Modules: move them by hand (Renderer.py:96-100)
        self.cameras = self.cameras.to(device)
        self.device = device
        return self

    def _frame_camera(self, cams, image_size, rows):
        """cameras.camera_tensors with the per-frame constants remembered: in a loop only R and T move, the intrinsics, the
        image size and the band are the same objects every frame -- their preparation (two expands, a cache look-up by
        weak reference, the band arithmetic) was 9 us of every frame's host time."""
        R, T = cams.R, cams.T
        f, p = cams.focal_length, cams.principal_point
        memo = self._frame_memo
        if (memo is not None and memo[0] is f and memo[1] is p and memo[2] is image_size and memo[3] is rows and torch.is_tensor(R)
                and torch.is_tensor(T) and R.dim() == 3 and T.dim() == 2 and R.shape[0] == memo[4] == T.shape[0] and R.is_cuda
                and R.dtype is torch.float32 is T.dtype and T.device == R.device and not (R.requires_grad or T.requires_grad)
                and (not torch.is_tensor(f) or f._version == memo[5]) and (not torch.is_tensor(p) or p._version == memo[6])
                and not torch.cuda.is_current_stream_capturing()):
            return (R, T) + memo[7]
        cam = camera_tensors(cams, image_size, rows)
        object.__setattr__(self, "_frame_memo", None)
        if (cam is not None and cam[0] is R and cam[1] is T and not torch.cuda.is_current_stream_capturing()
                and (rows is None or isinstance(rows, tuple) or hasattr(rows, "stripe_h"))):
            # (remembered by identity: the objects are held here, so an id cannot be recycled while the memo lives)
            object.__setattr__(self, "_frame_memo", (f, p, image_size, rows, R.shape[0], f._version if torch.is_tensor(f) else 0,
                                                     p._version if torch.is_tensor(p) else 0, cam[2:]))
        return cam

    def forward(self, gmeshes, **kwargs):
        """gmeshes() -> (verts [N,3] | [B,N,3], sigmas [N] | [N,3] | [N,3,3], radians), or, from a mesh with `oriented`
        (Meshes.OrientedGaussianMeshes), (verts, scales [..,N,3], quats [..,N,4]);
        R=, T= (and the inert focal=, principal=) keywords are stored on the camera object
        (Renderer.py:104-109).  `rows=(r0, r1)` (extension) renders only that pixel-row band."""
        cams = self.cameras
        assert not cams.in_ndc(), 'Got NDC camera. Cameras.in_ndc must be set to false.'
        for name in self.to_set_args:
            if name in kwargs:
                v = kwargs[name]
                setattr(cams, name, v.to(self.device) if isinstance(v, torch.Tensor) else v)
        st = self.render_settings
        image_size = st['image_size']

        verts, sigmas, _radians = gmeshes()
        if getattr(gmeshes, 'oriented', False):
            # oriented Gaussians: (verts, scales [..,N,3], quats [..,N,4]) -- the frame path takes them as they are
            # (ops.frame_trace_ori); every other route sees S = R diag(s) R^T as an (N,3,3) sigma below
            scales, quats = sigmas, _radians
            if scales.shape[-1] != 3 or quats.shape[-1] != 4 or scales.shape[:-1] != quats.shape[:-1] or scales.dim() not in (2, 3):
                raise ValueError('oriented Gaussians take scales[..,3] and quats[..,4] with the same leading dims, got '
                                 f'{tuple(scales.shape)} and {tuple(quats.shape)}')
            if (FUSED_PREAMBLE and verts.is_cuda and scales.dtype == quats.dtype == verts.dtype == torch.float32
                    and quats.is_cuda and not (st['max_point_per_bin'] != -1 and RayTracing.REFERENCE_CANDIDATES)
                    and os.environ.get("VOGE_LAZY_GENERAL", "1") != "0"):
                cam = self._frame_camera(cams, image_size, kwargs.get('rows'))
                if cam is not None and ops.frame_eligible(verts, scales, *cam[:4], st['max_assign'], cam[4][1] * cam[5]):
                    index, hit_len, lz = ops.frame_trace_ori(
                        verts, scales, quats, *cam[:4], cam[4], cam[5], st['max_point_per_bin'] != -1,
                        -math.log(st['thr_activation'] + 1 / 1e10), st['max_assign'], 2 if st['inverse_sigma'] else 1, st['absorptivity'])
                    return Fragments(None, index, None, hit_len, _lazy=lz)
            sigmas = oriented_sigma(scales, quats)
            if st['inverse_sigma']:      # (the (N,3,3) fused routes take no inverse_sigma: invert here, render as given)
                sigmas, st = torch.inverse(sigmas), _Overridden(st, inverse_sigma=False)
        shared_verts = verts.dim() == 2
        verts2d = verts                      # (the [N,3] parameter itself: indexing it back out of verts[None] would put a
        if shared_verts:                     #  select + zero-fill + copy into every backward)
            verts = verts[None]

        thr_act = -math.log(st['thr_activation'] + 1 / 1e10)                     # RayTracing.py:76,85
        K, occ = st['max_assign'], st['absorptivity']
        behind = st['max_point_per_bin'] != -1      # the coarse stage's "skip z < 0" candidate rule (rasterize_coarse.cu:35)
        if sigmas.dim() == 1 and shared_verts and FUSED_PREAMBLE and not (behind and RayTracing.REFERENCE_CANDIDATES):
            # Round 6, the frame path: one (verts [N,3], sigmas [N]) set, fixed cameras -- the trace takes the CAMERA itself
            # (ops.frame_trace: no ray-generation launch, no ray node; rays, cones, camera centre and view axis are made inside
            # binA / binB / the sweep with the ray kernel's own operations) and stops behind the sweep like trace_lean
            cam = self._frame_camera(cams, image_size, kwargs.get('rows'))
            if cam is not None and ops.frame_eligible(verts2d, sigmas, *cam[:4], K, cam[4][1] * cam[5]):
                index, hit_len, lz = ops.frame_trace(verts2d, sigmas, *cam[:4], cam[4], cam[5], behind, thr_act, K,
                                                     2 if st['inverse_sigma'] else 1, occ)
                return Fragments(None, index, None, hit_len, _lazy=lz)
        if (sigmas.dim() >= 2 and sigmas.shape[-1] == 3 and not st['inverse_sigma'] and FUSED_PREAMBLE and verts.is_cuda
                and not (behind and RayTracing.REFERENCE_CANDIDATES) and os.environ.get("VOGE_LAZY_GENERAL", "1") != "0"):
            # (N,3) / (N,3,3) sigmas on the frame path: the camera AND the user's own arrays go into the trace, whose record pass
            # does the centring and 2 * expend_sigma of Renderer.py:130-137 (no ray launch, no preamble launch, no node here)
            cam = self._frame_camera(cams, image_size, kwargs.get('rows'))
            if cam is not None and ops.frame_eligible(verts2d, sigmas, *cam[:4], K, cam[4][1] * cam[5]):
                index, hit_len, lz = ops.frame_trace_gen(verts2d, sigmas, *cam[:4], cam[4], cam[5], behind, thr_act, K, occ)
                return Fragments(None, index, None, hit_len, _lazy=lz)
        rays, origin = pixel_rays(cams, image_size, rows=kwargs.get('rows'))     # [B,h,W,3], [B,3]
        # ray_tracing (RayTracing.py:12-30) + aggregation (Aggregation.py:82-107) as ONE call: the trace's sweep
        # composites the fragments in its epilogue (voge_fragments_fwd*).  The stand-alone ray_tracing* / aggregation
        # functions remain the public API and produce the same values.
        if behind and RayTracing.REFERENCE_CANDIDATES:
            # the reference's own coarse candidate lists (lossy on purpose): explicit lists, unfused calls
            sig3 = expend_sigma(sigmas)
            if sig3.dim() == 3:
                sig3 = sig3.unsqueeze(0).expand(verts.shape[0] if not shared_verts else origin.shape[0], -1, -1, -1)
            isigma = 2 * torch.inverse(sig3) if st['inverse_sigma'] else 2 * sig3
            centred = verts - origin[:, None]
            sel_idx, sel_len, sel_act, sel_dsd = RayTracing.ray_tracing(
                cams, centred, isigma.contiguous(), rays, image_size, thr=st['thr_activation'], n_assign=K,
                max_points_per_bin=st['max_point_per_bin'])
            weight, index, valid_num, hit_len = aggregation(sel_idx, sel_act, sel_len, sel_dsd, occ)
            return Fragments(vert_weight=weight, vert_index=index, valid_num=valid_num, vert_hit_length=hit_len)

        def traced(mode, p0, p1, org, cam_fwd, smode=0):
            # stop behind the sweep when the composite can wait: it runs when the weights are first read -- or inside
            # to_colored_background's own pass (Fragments._lazy).  (Full 3x3 forms defer it too: the sweep keeps the packed
            # (mu, A) records instead of act / dsd.)  merge_final later rewrites -1 -> 0 inside the fragments' index tensor;
            # the reference clones it (Renderer.py:145) because its backward finds empty slots by idx == -1, this trace
            # backward uses the per-pixel hit count instead, so no copy is needed.
            if ops.lazy_eligible(mode, p0, p1, org, rays, K):
                index, hit_len, lz = ops.trace_lean(mode, p0, p1, org, rays, cam_fwd, thr_act, K, smode, occ)
                return Fragments(None, index, None, hit_len, _lazy=lz)
            weight, index, valid_num, hit_len = ops.fragments(mode, p0, p1, org, rays, cam_fwd, thr_act, K, smode, occ)
            return Fragments(vert_weight=weight, vert_index=index, valid_num=valid_num, vert_hit_length=hit_len)

        if sigmas.dim() == 1 and shared_verts and not origin.requires_grad and FUSED_PREAMBLE:
            # One (verts [N,3], sigmas [N]) set seen by every view, fixed cameras: the centring of
            # Renderer.py:130 and the 2*sigma / 2/sigma of :133-137 happen inside the trace's per-Gaussian
            # pass (and their chain rule inside its backward's) -- same values, no elementwise launches.
            cam_fwd = _view_axis(cams, origin[:, None]) if behind else None
            return traced(2, verts2d, sigmas, origin, cam_fwd, 2 if st['inverse_sigma'] else 1)
        if (sigmas.dim() >= 2 and not st['inverse_sigma'] and not origin.requires_grad and FUSED_PREAMBLE
                and verts.is_cuda and sigmas.shape[-1] == 3):
            # (N,3) / (N,3,3) sigmas: the centring and 2 * expend_sigma of Renderer.py:130-137 as ONE launch each way
            cam_fwd = _view_axis(cams, origin[:, None]) if behind else None
            mus0, isg0 = ops.general_preamble(verts2d if shared_verts else verts, sigmas, origin)
            return traced(0, mus0, isg0, None, cam_fwd)
        centred = verts - origin[:, None]                                         # Renderer.py:130
        cam_fwd = _view_axis(cams, centred) if behind else None
        B = centred.shape[0]
        if sigmas.dim() == 1:
            # (N,) sigmas are isotropic: expend_sigma would give sigma * I (Aggregation.py:155-157) and
            # Renderer.py:133 doubles (or inverts and doubles) it.  Keep the scalar: the trace has an
            # isotropic form whose backward produces d/d(scalar) directly.
            a = 2.0 / sigmas if st['inverse_sigma'] else 2.0 * sigmas
            a = a.unsqueeze(0).expand(B, -1)
            return traced(1, centred.reshape(-1, 3), a.reshape(-1), None, cam_fwd)
        sigmas = expend_sigma(sigmas)
        if sigmas.dim() == 3:
            sigmas = sigmas.unsqueeze(0).expand(B, -1, -1, -1)
        isigma = 2 * torch.inverse(sigmas) if st['inverse_sigma'] else 2 * sigmas
        return traced(0, centred.reshape(-1, 3), isigma.reshape(-1, 3, 3), None, cam_fwd)


def interpolate_attr(fragments: Fragments, vert_attr: torch.Tensor):
    lz = getattr(fragments, "_lazy", None)
    if lz is not None:
        # fragments whose composite is still pending: weights, merged attributes and the per-pixel weight sum in one
        # pass (ops._CompositeMerge); a get_silhouette on the same fragments then costs nothing but a clamp
        assert vert_attr.dim() == 2
        out = ops.composite_merge(lz, vert_attr)
        if out is not None:
            fragments._set_composite(out[2], out[3])
            w = fragments._vert_weight
            fragments._wsum = (fragments._shaped(out[1]), w, w._version, fragments._shaped(out[4]))
            return fragments._shaped(out[0])
    return merge_final(vert_attr=vert_attr, weight=fragments.vert_weight, valid_num=fragments.valid_num,
                       vert_assign=fragments.vert_index)


def get_silhouette(fragments: Fragments):
    ws = getattr(fragments, "_wsum", None)
    if ws is not None and ws[1] is fragments._vert_weight and ws[1]._version == ws[2]:
        if ws[3] is not None:      # (frame path: the composite wrote min(sum_k w_k, 1) itself -- an output of the same node as the merge)
            return ws[3]
        # the weight sum the one-pass composite + merge left behind: min(sum_k w_k, 1) exactly as Renderer.py:157-159
        # (torch.minimum splits the gradient at a tie like torch.min(a, b))
        return torch.minimum(ws[0], torch.ones_like(ws[0]))
    return ops.silhouette(fragments.vert_weight)


def get_depth(fragments: Fragments, normalize: bool = True, background: float = 0.0):
    """Depth map of the fragments (an extension: the reference has none) -> [..., H, W] fp32, the leading dimensions of
    vert_index[..., 0].  For a pixel with n = min(valid_num, K) live slots, A = sum_{k<n} w_k len_k and S = sum_{k<n} w_k
    (w = vert_weight, len = vert_hit_length); slots k >= n never contribute, forward or backward.

    normalize=True:  the expected hit distance A / S where S > 0; elsewhere (nothing hit, or every weight underflowed) the
                     result is `background`, a Python float, and the gradient is zero.  S is NOT bounded by 1 -- Gaussians
                     overlap along a ray -- so the un-normalised sum is not a distance; this is.
                     d/dw_k = (len_k - D) / S, d/dlen_k = w_k / S.
    normalize=False: the accumulated A (0 where nothing was hit; `background` is ignored).  d/dw_k = len_k, d/dlen_k = w_k.

    The result is not clamped.  It is a distance along the UNIT pixel ray from the camera centre, as vert_hit_length is, not
    view-space z: multiply by the ray's cosine to the view axis (rays . view_axis, e.g. from cameras.pixel_rays) to get z.
    The per-pixel sums use a fixed association: the same bits on every run.  vert_index is not rewritten (the -1 -> 0 of
    empty slots is merge_final's).

    Fragments whose composite is still pending (scalar sigmas on the frame path, K <= 128) get weights, depth, weight sum and
    silhouette from ONE launch and ONE fused launch backward (ops._CompositeDepth); a get_silhouette on the same fragments then
    costs nothing, forward or backward.  Everything else -- general and oriented Gaussians, ray-bundle traces, edited
    fragments, K > 128, weights that already exist -- takes ops._Depth on the fragments' tensors.  For an RGB-D loss call
    get_depth BEFORE to_colored_background: the colours then take the fused-backward shade on the finished weights (two
    fused backward launches a step); the other order is just as correct, with the depth's gradient going through autograd's
    [.., K] arrays (tests/test_gpu_consumers.py holds every order of nine consumers of one Fragments, this pair among them, to
    the fp64 gradients)."""
    lz = getattr(fragments, "_lazy", None)
    if lz is not None:
        out = ops.composite_depth(lz, bool(normalize), float(background))
        if out is not None:
            fragments._set_composite(out[2], out[3])
            w = fragments._vert_weight
            fragments._wsum = (fragments._shaped(out[1]), w, w._version, fragments._shaped(out[4]))
            return fragments._shaped(out[0])
    return ops.depth(fragments.vert_weight, fragments.vert_hit_length, fragments.valid_num, normalize, background)


def get_distortion(fragments: Fragments, normalize: bool = False):
    """Depth-distortion regulariser of the fragments (an extension: the reference has none) -> [..., H, W] fp32, the leading
    dimensions of vert_index[..., 0]: the term of Mip-NeRF 360 and 2D Gaussian splatting that pulls a ray's mass onto one surface.
    For a pixel with n = min(max(valid_num, 0), K) live slots, w = vert_weight and t = vert_hit_length,

        L = sum_i sum_j w_i w_j |t_i - t_j|      over the live slots; slots k >= n never contribute, forward or backward.

    normalize=False: L itself (0 where nothing is hit).  sum_k w_k is NOT bounded by 1 here (see get_depth), so L grows with the
                     square of the mass on the ray.
    normalize=True:  L / S^2 with S = sum_k w_k where S > 0 -- the distortion of the weights rescaled to sum to 1; elsewhere 0,
                     with zero gradient.

    It is evaluated as a prefix scan over the slots in the total order (t_k, k) -- ascending hit length, exact ties by slot position
    -- on u_k = t_k - t_first, the lengths recentred on the nearest live slot (Aggregation.distortion spells it out and IS the
    definition).  Tie rule: at an exact tie the gradient is the POSITIONAL subgradient, the earlier slot counting as nearer -- for
    tied i before j, d/dt_i gets -2 w_i w_j and d/dt_j gets +2 w_i w_j --, not torch's sign(0) = 0.  t is the distance along the
    UNIT pixel ray, as everywhere else here: there is no near / far mapping -- for the loss in [near, far] units multiply the
    result by 1 / (far - near).  The sums use a fixed association: the same bits on every run.

    fp32 fragments on a HIP device take one streaming launch each way (ops._Distortion), unsorted pixels (edited fragments,
    find_farest_k) included; on fragments whose composite is still pending, reading the weights runs that composite first and the
    gradient reaches the Gaussians through its backward.  Anything else -- host tensors, other dtypes -- returns
    Aggregation.distortion(...): the same values, with autograd's gradients."""
    w, ln, vn = fragments.vert_weight, fragments.vert_hit_length, fragments.valid_num
    if w.is_cuda and ln.is_cuda and vn.is_cuda and w.dtype == ln.dtype == torch.float32:
        return ops.distortion(w, ln, vn, normalize)
    return distortion(w, ln, vn, normalize)


def get_normals(depth: torch.Tensor, cameras_or_rays, rows=None, edge: Union[None, float] = None, view_space: bool = False):
    """Surface normals of a depth map (an extension: the reference has none) -> [B,h,W,3] for depth [B,h,W], [h,W,3] for [h,W].
    `depth` is what get_depth returns: the distance along each pixel's UNIT ray from the camera centre, not view-space z (a
    z-buffer has to be divided by rays . view_axis first).  The Gaussians themselves have no usable normal -- at a slot's hit point,
    the density maximum along the ray, the density gradient is perpendicular to the ray by construction -- so this is the normal of
    the RENDERED surface, from finite differences of the back-projected points P = depth * ray:

        valid: isfinite(depth) and depth > 0.  A neighbour (i, j +- 1) is usable if it is inside the image, valid and, with
        `edge` (a relative depth jump, e.g. 0.1, that cuts the stencil at occlusion boundaries), |depth_nb - depth| <= edge * depth.
        D_x = P(j+1) - P(j-1) if both are usable, the one-sided difference if one is; D_y the same along the rows of the map;
        n = +-normalise(D_x x D_y), the sign that faces the camera (n . ray <= 0); (0, 0, 0) where the pixel is not valid, a
        difference does not exist or the cross product vanishes.

    Aggregation.depth_normals spells the rules out and IS the definition.  The gradient reaches `depth` -- and through get_depth's
    backward the Gaussians -- through P, the cross product and the normalisation; the choice of stencil, the edge test and the
    sign are constants; a pixel without a normal passes no gradient on and a depth that is not valid gets exactly zero, NaN or
    inf in it reaching nothing.  view_space=True returns n_world @ R (row vectors, X_view = X_world @ R + T).

    fp32 floor: the differences cancel, so whatever rounding the depth values carry is amplified by depth / pixel footprint.  The
    plain fp32 definition is off from fp64, on the same depth values, by about 2^-23 * depth / footprint: 2e-6 to 5e-6 at focal
    lengths of 30 to 60 pixels, 3.3e-5 at 500, 1.2e-4 at 2000 and distance 6 (the bunny's camera).  The kernels difference the depth
    and the ray separately and add no such error of their own (a few 1e-7 against fp64 at any focal length), but they cannot take
    back the rounding an fp32 depth map ARRIVES with -- 2^-24 relative from get_depth, amplified the same way: at focal length 2000
    a normal from an fp32 depth map is good to about 1e-4, whoever computes it.

    cameras_or_rays is a cameras object (R, focal_length, principal_point; T is not needed) or a [B,h,W,3] tensor of unit rays:
      * cameras with fp32 tensors on the depth's HIP device, none requiring grad, and an fp32 depth: one HIP launch each way
        (ops._DepthNormals: the kernels make the rays themselves, the backward is a gather without atomics -- the same bits on
        every run -- and nothing but the outputs is allocated, so the step still captures into a HIP graph).  rows=(r0, r1) has the
        meaning of the renderer's rows=: the map holds image rows r0 .. r1-1, and r1 - r0 must be h.
      * a camera that wants a gradient, or a depth of another dtype or device: cameras.pixel_rays(...) + the torch definition --
        the same values, and autograd reaches the camera.
      * a tensor of rays: the torch definition directly, on any device; world space only (view_space=True raises).
    A distributed.Stripes band raises: stacked stripe rows are not image neighbours -- gather the depth (gather_stripes) first."""
    if hasattr(rows, "stripe_h"):
        raise ValueError("get_normals: the rows of a distributed.Stripes band are not image neighbours -- gather the depth map "
                         "(distributed.gather_stripes) and take the normals of the whole frame")
    if not torch.is_tensor(depth) or depth.dim() not in (2, 3):
        raise ValueError("get_normals: depth[B,h,W] or [h,W] expected, got " + (str(tuple(depth.shape)) if torch.is_tensor(depth) else repr(depth)))
    if edge is not None and not 0.0 <= float(edge) < math.inf:
        raise ValueError(f"get_normals: edge must be None or a finite relative depth jump >= 0, got {edge!r}")
    single = depth.dim() == 2
    d = depth[None] if single else depth
    B, h, W = d.shape
    if torch.is_tensor(cameras_or_rays):
        rays = cameras_or_rays
        if view_space:
            raise ValueError("get_normals: view_space=True needs the cameras (a tensor of rays carries no rotation)")
        if rows is not None:
            raise ValueError("get_normals: rows= goes with a cameras object; a tensor of rays already is the band's")
        if single and rays.dim() == 3:
            rays = rays[None]
        if tuple(rays.shape) != (B, h, W, 3):
            raise ValueError(f"get_normals: rays {tuple(cameras_or_rays.shape)} do not match depth {tuple(depth.shape)}")
        out = depth_normals(d, rays, edge)
        return out[0] if single else out
    cameras = cameras_or_rays
    r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if r0 < 0 or r1 - r0 != h:
        raise ValueError(f"get_normals: rows=({r0}, {r1}) do not describe the {h} rows of depth {tuple(depth.shape)}")
    views = max(cameras.R.reshape(-1, 3, 3).shape[0], 1)
    if views not in (1, B):
        raise ValueError(f"get_normals: {views} cameras for depth {tuple(depth.shape)}")
    ct = camera_tensors(cameras, (r1, W), (r0, r1))
    if ct is not None and d.is_cuda and d.dtype == torch.float32 and ct[0].device == d.device:
        R, _, focal, pp = ct[:4]
        if R.shape[0] != B:
            R, focal, pp = R.expand(B, 3, 3), focal.expand(B, 2), pp.expand(B, 2)
        out = ops.depth_normals(d, R, focal, pp, r0, edge, view_space)
        return out[0] if single else out
    rays = pixel_rays(cameras, (r1, W), rows=(r0, r1))[0]
    if rays.shape[0] != B:
        rays = rays.expand(B, h, W, 3)
    out = depth_normals(d, rays.to(device=d.device, dtype=d.dtype), edge)
    if view_space:
        R = cameras.R.reshape(-1, 3, 3).to(device=d.device, dtype=d.dtype)
        out = torch.einsum("bhwi,bij->bhwj", out, R.expand(B, 3, 3))
    return out[0] if single else out


def sh_to_colors(sh: torch.Tensor, verts: torch.Tensor, cameras_or_centres, degree: Union[None, int] = None, clamp: bool = True):
    """View-dependent colours (an extension: the reference has none) -> [B*N, C], row b*N + n: the attribute table the fragments
    of a B-view render index, to hand to to_colored_background / to_white_background / interpolate_attr like any colours.

    sh [N, M, C] holds the spherical-harmonic coefficients of each Gaussian's colour, M in {1, 4, 9, 16} (maximum degree
    sqrt(M) - 1, 0..3); verts [N,3] or [B,N,3] the centres the renderer gets; cameras_or_centres a [B,3] tensor of camera centres
    or a cameras object.  For view b and Gaussian n, with d the unit vector from the camera centre to the Gaussian,
        colour = relu(sum_{m < (degree+1)^2} Y_m(d) sh[n,m,:] + 0.5)      (clamp=False: without the relu)
    in the basis order, signs, offset and clamp trained Gaussian scenes are stored in (Aggregation.sh_colors spells Y_m out and IS
    the definition).  `degree` (default: the maximum) is the active degree: higher coefficients are not read and get a zero
    gradient, for progressive training.  The gradient is zero where the clamp is active.

    fp32 tensors on ONE HIP device with 1 <= C <= 4 and camera centres that need no gradient take one HIP launch each way
    (ops._ShColors: no atomics, the same bits on every run, nothing but the outputs allocated, so the step still captures into a
    HIP graph -- with one exception: where M * C is a multiple of 4 the kernel loads a Gaussian's coefficients 16 bytes at a time,
    and an `sh` that does not start on a 16-byte boundary, such as a view at an odd offset into a flat buffer, is copied first);
    anything else -- other dtypes, tensors on the host or on different devices, C = 0 or C > 4, a camera centre that requires
    grad -- returns
    Aggregation.sh_colors(...): the same values with autograd's gradients, the camera centres' included.

    A cameras object is asked for get_camera_center() on EVERY call -- a matrix inverse and an einsum, several launches: when the
    cameras are fixed, compute the centres once and pass the tensor."""
    centres = cameras_or_centres if torch.is_tensor(cameras_or_centres) else cameras_or_centres.get_camera_center()
    degree = sh_degree(sh, degree)
    if (sh.is_cuda and verts.device == centres.device == sh.device and sh.dtype == verts.dtype == centres.dtype == torch.float32
            and 1 <= sh.shape[2] <= 4 and not centres.requires_grad):
        return ops.sh_colors(sh, verts, centres, degree, clamp)
    return sh_colors(sh, verts, centres, degree, clamp)


def gaussian_normals(scales: torch.Tensor, quats: torch.Tensor, verts: torch.Tensor, cameras_or_centres, inverse_sigma: bool = False):
    """Per-view normals of oriented Gaussians (an extension: the reference has none) -> [B*N, 3], row b*N + n: the attribute table
    the fragments of a B-view render index, to hand to get_rendered_normals / interpolate_attr like any attributes.

    scales [N,3] or [B,N,3] and quats [N,4] or [B,N,4] (w, x, y, z; not necessarily unit) are what OrientedGaussianMeshes holds,
    verts [N,3] or [B,N,3] the centres the renderer gets; cameras_or_centres a [B,3] tensor of camera centres or a cameras object;
    inverse_sigma the renderer's setting.  An oriented, flattened Gaussian stands for a surface element whose normal is its
    THINNEST axis: the column k* of R = quaternion_to_matrix(quats) with the largest scale (inverse_sigma=False: A = 2 S, a larger
    s is a thinner extent) or the smallest (inverse_sigma=True: A = R diag(2 / s) R^T), exact ties keeping the lowest index; for
    view b the result is that column with the sign that faces the camera, n . (v - c_b) <= 0 -- the side get_normals picks
    (Aggregation.gaussian_normals spells the rules out and IS the definition).  Only quats get a gradient, through the chosen
    column, orthogonal to quats and summed over the views when the quaternions are shared; the axis and the sign are constants, so
    scales, verts and the camera centres get none, whether they require grad or not.

    fp32 tensors on ONE HIP device take one HIP launch each way (ops._GaussNormals: no atomics, the same bits on every run, nothing
    but the outputs allocated, so the step still captures into a HIP graph); anything else -- other dtypes, tensors on the host
    or on different devices -- returns Aggregation.gaussian_normals(...): the same values with autograd's gradient.

    A cameras object is asked for get_camera_center() on EVERY call -- a matrix inverse and an einsum, several launches: when the
    cameras are fixed, compute the centres once and pass the tensor."""
    centres = cameras_or_centres if torch.is_tensor(cameras_or_centres) else cameras_or_centres.get_camera_center()
    gaussian_normals_shapes(scales, quats, verts, centres)
    if (quats.is_cuda and scales.device == verts.device == centres.device == quats.device
            and scales.dtype == quats.dtype == verts.dtype == centres.dtype == torch.float32):
        return ops.gauss_normals(scales, quats, verts, centres, inverse_sigma)
    return _gaussian_normals_def(scales, quats, verts, centres, inverse_sigma)


def get_rendered_normals(fragments: Fragments, normals_table: torch.Tensor, normalize: bool = True):
    """Rendered normal map sum_k w_k n_k of the fragments (an extension: the reference has none) -> [..., H, W, 3]:
    M = interpolate_attr(fragments, normals_table) with normals_table [B*N, 3] from gaussian_normals -- on the frame path the
    merge runs inside the composite's own pass, like any attribute table.  normalize=True returns M / |M| where |M| > 0 and
    (0, 0, 0) elsewhere (nothing hit, or the weighted normals cancel); such a pixel passes no gradient on.  A thin torch
    composition: no kernel of its own.  Fragments on the host (hand-made ones) are merged by the same sum in torch.

    The normal-consistency term of 2D Gaussian splatting compares it with the normal of the rendered depth:
        n_hat = get_rendered_normals(fragments, gaussian_normals(scales, quats, verts, centres))
        n_depth = get_normals(get_depth(fragments), cameras)
        both = (n_hat != 0).any(-1) & (n_depth != 0).any(-1)
        loss = (1 - (n_hat * n_depth).sum(-1))[both].mean()
    -- 1 - (n_hat . n_depth) on the pixels where both are non-zero; both face the camera, so the term is 0 where they agree."""
    if fragments.vert_index.is_cuda:      # (vert_index: reading vert_weight would run a pending composite)
        M = interpolate_attr(fragments, normals_table)
    else:
        w, idx, K = fragments.vert_weight, fragments.vert_index, fragments.vert_weight.shape[-1]
        live = torch.arange(K, device=w.device) < fragments.valid_num[..., None]
        M = (normals_table[idx.clamp(min=0).long()] * (w * live)[..., None]).sum(-2)
    if not normalize:
        return M
    n2 = (M * M).sum(-1, keepdim=True)
    ok = n2 > 0
    return torch.where(ok, M / torch.sqrt(torch.where(ok, n2, torch.ones_like(n2))), torch.zeros_like(M))


_BG_CACHE = {}


def _background_tensor(color, device):
    """Device tensor of a constant background colour, uploaded once per (colour, device): a
    host-to-device copy per frame would also make the frame impossible to capture in a HIP graph."""
    key = (color if type(color) is tuple else tuple(color), device)      # ((1, 1, 1) and (1.0, 1.0, 1.0) hash and compare equal)
    t = _BG_CACHE.get(key)
    if t is None:
        t = _BG_CACHE[key] = torch.tensor(tuple(float(c) for c in color), dtype=torch.float32, device=device)
    return t


def _plain_color(bg, C, device):
    """A background that keeps the constant-colour routes -- a tuple, list or tensor with 1 or C elements, every leading
    dimension 1, no grad -- as a device tensor of the C values (a grey level expanded); None for anything else."""
    if not torch.is_tensor(bg):
        if len(bg) not in (1, C):
            return None
        return _background_tensor(tuple(bg) * C if len(bg) == 1 else bg, device)
    if bg.requires_grad or bg.numel() not in (1, C) or any(d != 1 for d in bg.shape[:-1]):
        return None
    if bg.numel() == C:
        return bg if bg.device == device else bg.to(device)
    if not bg.is_cuda:
        return _background_tensor((float(bg.reshape(())),) * C, device)
    return bg.to(device).reshape(1).expand(C)      # (the shade kernels' _dev copies it: no host sync)


def to_colored_background(fragments: Fragments, colors: torch.Tensor,
                          background_color: Union[torch.Tensor, tuple, list] = (1, 1, 1), thr: float = -1):
    plain = _plain_color(background_color, colors.shape[-1], colors.device)
    if plain is None:
        # an image, a colour per view, a background that requires grad (Renderer.py:162-171 under torch broadcasting):
        # interpolate_attr + get_silhouette -- one fused node each way on the frame path -- then the broadcast blend
        rgb = interpolate_attr(fragments, colors)
        return ops.blend_background(rgb, get_silhouette(fragments), background_color, thr)
    background_color = plain
    lz = getattr(fragments, "_lazy", None)
    if lz is not None:
        # fragments whose composite is still pending: weights AND image in one pass (ops._CompositeShade)
        out = ops.composite_shade(lz, colors, background_color, thr)
        if out is not None:
            fragments._set_composite(out[1], out[2])
            return fragments._shaped(out[0])
    if colors.dim() == 2 and colors.shape[1] <= 4:
        # merge + silhouette + blend fused in one kernel; on fragments of this renderer the backward of the whole
        # pipeline (this blend, the composite, the trace) is one kernel as well (ops._ShadeThrough)
        img = ops.shade_through(colors, fragments.vert_weight, fragments.vert_index, fragments.valid_num, background_color, thr)
        if img is not None:
            return img
        return ops.shade(colors, fragments.vert_weight, fragments.vert_index, fragments.valid_num, background_color, thr)
    rgb = interpolate_attr(fragments, colors)
    return ops.blend(rgb, fragments.vert_weight, background_color, thr)


def to_white_background(fragments: Fragments, colors: torch.Tensor, thr: float = -1):
    return to_colored_background(fragments=fragments, colors=colors, background_color=(1, 1, 1), thr=thr)
