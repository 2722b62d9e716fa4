"""The reference's own native extension, as oracle/build_ref.py built it (oracle/_ref/voge_ref_C.so), behind wrappers that
check what its kernels do not -- TEST INFRASTRUCTURE.

The reference kernels check nothing: an index outside its table is read (or written) as it stands.  Every wrapper therefore
asserts the conditions under which the kernel it calls stays inside its buffers, read off the kernel's source and cited per
wrapper, BEFORE the call; the tests call the wrappers only.  load() imports the file by path after torch (never through
torch.utils.cpp_extension.load, which would try to rebuild it).  Each call is timed (synchronised on both sides) into TIMES:
timing of test infrastructure, not of the product."""
import importlib.util
import os
import time

import torch      # before the extension: it links against torch's libraries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(ROOT, "oracle", "_ref", "voge_ref_C.so")
NAMES = ("rasterize_points_coarse", "ray_trace_voge_fine", "ray_trace_voge_fine_backward", "ray_trace_voge_ray",
         "ray_trace_voge_ray_backward", "find_nearest_k", "sample_voge", "sample_voge_backward", "scatter_max")
TIMES = []      # (entry point, note, milliseconds)
_mod = None


def available():
    return os.path.exists(SO_PATH)


def load():
    global _mod
    if _mod is None:
        spec = importlib.util.spec_from_file_location("voge_ref_C", SO_PATH)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _mod = mod
    return _mod


def _check(t, dtype, shape=None, name="tensor"):
    assert isinstance(t, torch.Tensor) and t.is_cuda, f"{name}: not on the device"
    assert t.dtype == dtype, f"{name}: {t.dtype}, expected {dtype}"
    assert t.is_contiguous(), f"{name}: not contiguous"
    if shape is not None:
        assert len(shape) == t.dim() and all(s is None or s == d for s, d in zip(shape, t.shape)), f"{name}: shape {tuple(t.shape)}, expected {shape}"


def _in_range(t, lo, hi, name):
    """Every entry in [lo, hi).  (One reduction and a copy of two numbers: the kernels' inputs here are small.)"""
    if t.numel():
        mn, mx = int(t.min()), int(t.max())
        assert lo <= mn and mx < hi, f"{name}: entries span [{mn}, {mx}], allowed [{lo}, {hi})"


def _timed(name, note, fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    TIMES.append((name, note, (time.perf_counter() - t0) * 1e3))
    return out


def ray_trace_voge_fine(mus, isigmas, rays, bin_points, thr_act, bin_size, K, note=""):
    """ray_trace_voge.cu:135-280.  The kernel reads bin_points[bi BH BH M + by BW M + bx M + m] (:185) for every bin of the
    ceil(H / bin_size) x ceil(W / bin_size) grid it derives from the LIST's shape, and mus / isigmas at every entry > -1."""
    f32, i32 = torch.float32, torch.int32
    _check(mus, f32, (None, 3), "mus")
    P = mus.shape[0]
    _check(isigmas, f32, (P, 3, 3), "isigmas")
    _check(rays, f32, (None, None, None, 3), "rays")
    B, H, W, _ = rays.shape
    bin_size, K = int(bin_size), int(K)
    assert bin_size >= 1 and K >= 1 and B >= 1 and H >= 1 and W >= 1
    BH, BW = (H - 1) // bin_size + 1, (W - 1) // bin_size + 1
    _check(bin_points, i32, (B, BH, BW, None), "bin_points")
    assert B == 1 or BH == BW, "the kernel strides the batch by BH * BH * M (:185): with B > 1 the bin grid must be square"
    assert P % B == 0
    _in_range(bin_points, -1, P, "bin_points")
    assert B * BH * BW * bin_size * bin_size < 2 ** 31 and B * H * W * K < 2 ** 31 and P * 9 < 2 ** 31      # int indices (:155,:176)
    return _timed("ray_trace_voge_fine", note, load().ray_trace_voge_fine, mus, isigmas, rays, bin_points, float(thr_act), bin_size, K)


def ray_trace_voge_fine_backward(mus, isigmas, rays, point_idxs, grad_len, grad_act, grad_dsd, note=""):
    """ray_trace_voge.cu:283-379.  Every slot with point_idxs != -1 (:310) reads and atomically adds at that index."""
    f32 = torch.float32
    _check(mus, f32, (None, 3), "mus")
    P = mus.shape[0]
    _check(isigmas, f32, (P, 3, 3), "isigmas")
    _check(rays, f32, (None, None, None, 3), "rays")
    B, H, W, _ = rays.shape
    _check(point_idxs, torch.int32, (B, H, W, None), "point_idxs")
    K = point_idxs.shape[3]
    for g, nm in ((grad_len, "grad_len"), (grad_act, "grad_act"), (grad_dsd, "grad_dsd")):
        _check(g, f32, (B, H, W, K), nm)
    _in_range(point_idxs, -1, P, "point_idxs")
    assert B * H * W * K < 2 ** 31
    return _timed("ray_trace_voge_fine_backward", note, load().ray_trace_voge_fine_backward, mus, isigmas, rays, point_idxs,
                  grad_len, grad_act, grad_dsd)


def ray_trace_voge_ray(mus, isigmas, rays, note=""):
    """voge_ray_tracing_ray.cu:114-143, :242-283: every (ray, Gaussian) pair, indices from the shapes alone."""
    f32 = torch.float32
    _check(mus, f32, (None, 3), "mus")
    M = mus.shape[0]
    _check(isigmas, f32, (M, 3, 3), "isigmas")
    _check(rays, f32, (None, 3), "rays")
    assert M >= 1 and rays.shape[0] >= 1 and M * rays.shape[0] < 2 ** 31
    return _timed("ray_trace_voge_ray", note, load().ray_trace_voge_ray, mus, isigmas, rays)


def ray_trace_voge_ray_backward(mus, isigmas, rays, grad_len, grad_act, grad_dsd, note=""):
    """voge_ray_tracing_ray.cu:147-188, :287-325."""
    f32 = torch.float32
    _check(mus, f32, (None, 3), "mus")
    M = mus.shape[0]
    _check(isigmas, f32, (M, 3, 3), "isigmas")
    _check(rays, f32, (None, 3), "rays")
    N = rays.shape[0]
    for g, nm in ((grad_len, "grad_len"), (grad_act, "grad_act"), (grad_dsd, "grad_dsd")):
        _check(g, f32, (N, M), nm)
    assert M >= 1 and N >= 1 and M * N < 2 ** 31
    return _timed("ray_trace_voge_ray_backward", note, load().ray_trace_voge_ray_backward, mus, isigmas, rays, grad_len, grad_act, grad_dsd)


def find_nearest_k(len_in, act_in, dsd_in, thr_act, K, note=""):
    """voge_ray_tracing_ray.cu:191-239, :328-375.  Slot `cur` is read before anything is written (:220): K >= 1."""
    f32 = torch.float32
    _check(len_in, f32, (None, None), "len")
    N, M = len_in.shape
    _check(act_in, f32, (N, M), "act")
    _check(dsd_in, f32, (N, M), "dsd")
    K = int(K)
    assert K >= 1 and N >= 1 and M >= 1 and N * max(M, K) < 2 ** 31
    return _timed("find_nearest_k", note, load().find_nearest_k, len_in, act_in, dsd_in, float(thr_act), K)


def _sampler_inputs(image, vert_weight, vert_index, num_vert):
    _check(image, torch.float32, (None, None, None, None), "image")
    B, H, W, C = image.shape
    _check(vert_weight, torch.float32, (B, H, W, None), "vert_weight")
    K = vert_weight.shape[3]
    _check(vert_index, torch.int32, (B, H, W, K), "vert_index")
    assert num_vert >= 1 and C >= 1 and K >= 1
    _in_range(vert_index, -1, int(num_vert), "vert_index")
    assert B * H * W * max(K, C) < 2 ** 31 and int(num_vert) * C < 2 ** 31


def sample_voge(image, vert_weight, vert_index, num_vert, note=""):
    """sample_voge.cu:35-66, :95-134: every slot with index != -1 adds at that vertex."""
    _sampler_inputs(image, vert_weight, vert_index, num_vert)
    return _timed("sample_voge", note, load().sample_voge, image, vert_weight, vert_index, int(num_vert))


def sample_voge_backward(image, vert_weight, vert_index, grad_feature, grad_weight_sum, note=""):
    """sample_voge.cu:173-252: reads grad_feature / grad_weight_sum at every index != -1."""
    _check(grad_feature, torch.float32, (None, image.shape[3]), "grad_feature")
    num_vert = grad_feature.shape[0]
    _check(grad_weight_sum, torch.float32, (num_vert,), "grad_weight_sum")
    _sampler_inputs(image, vert_weight, vert_index, num_vert)
    return _timed("sample_voge_backward", note, load().sample_voge_backward, image, vert_weight, vert_index, grad_feature, grad_weight_sum)


def scatter_max(vert_weight, vert_index, num_vert, note=""):
    """sample_voge.cu:69-92, :137-170.  The maximum is a compare-and-swap on the bit pattern against a table of zeros: defined
    for weights >= 0."""
    _check(vert_weight, torch.float32, (None, None, None, None), "vert_weight")
    _check(vert_index, torch.int32, tuple(vert_weight.shape), "vert_index")
    assert num_vert >= 1 and vert_weight.numel() < 2 ** 31
    _in_range(vert_index, -1, int(num_vert), "vert_index")
    assert bool((vert_weight >= 0).all()), "weights must be >= 0"
    return _timed("scatter_max", note, load().scatter_max, vert_weight, vert_index, int(num_vert))


def rasterize_points_coarse(points, first_idx, num_points, image_size, radius, bin_size, max_points_per_bin, note=""):
    """rasterize_coarse.cu:20-305.  A bin that receives more than max_points_per_bin points takes the device-side printf branch
    (:154-170); with max_points_per_bin >= the points of every cloud no bin can.  The bit mask in shared memory is
    BH BW 512 / 8 bytes (:229-230): at most 8 x 8 bins here (4 KiB)."""
    _check(points, torch.float32, (None, 3), "points")
    P = points.shape[0]
    _check(radius, torch.float32, (P, 2), "radius")
    _check(first_idx, torch.int64, (None,), "cloud_to_packed_first_idx")
    _check(num_points, torch.int64, tuple(first_idx.shape), "num_points_per_cloud")
    H, W = int(image_size[0]), int(image_size[1])
    bin_size, M = int(bin_size), int(max_points_per_bin)
    assert P >= 1 and first_idx.shape[0] >= 1 and H >= 1 and W >= 1 and bin_size >= 1
    BH, BW = (H - 1) // bin_size + 1, (W - 1) // bin_size + 1
    assert BH <= 8 and BW <= 8, "bin grid larger than 8 x 8"
    first, num = first_idx.cpu().tolist(), num_points.cpu().tolist()
    assert all(f >= 0 and c >= 0 and f + c <= P for f, c in zip(first, num)), "a cloud reaches outside the packed array"
    assert M >= max(num), "max_points_per_bin below the points of a cloud: a bin could overflow"
    return _timed("rasterize_points_coarse", note, load().rasterize_points_coarse, points, first_idx, num_points, (H, W), radius, bin_size, M)
