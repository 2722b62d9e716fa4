/*
 * voge_hip.h -- C ABI of libvoge_hip.so, the MI355X (gfx950) implementation of the VoGE
 * ray-trace + aggregation hot path.
 *
 * This is the drop-in boundary: it replaces the on-path part of the reference's pybind11
 * module `VoGE._C` (VoGE/csrc/ext.cpp:7-17) and the tensor programs of
 * VoGE/Aggregation.py that sit directly behind it.  Plain C: raw DEVICE pointers, sizes,
 * and a HIP stream handle -- no torch / ATen types.
 *
 * Conventions (all functions):
 *   - every pointer is a device pointer on the current HIP device, caller-allocated and
 *     caller-owned; the library never allocates, frees or keeps state between calls;
 *   - float = IEEE fp32, idx = int32, valid_num = int64 (Aggregation.py:104 returns int64);
 *   - tensors are contiguous, row-major, layouts as in the reference:
 *       mus [P,3], isigmas [P,3,3], rays [B,H,W,3], per-slot arrays [B,H,W,K]
 *       (ray index = b*H*W + y*W + x, ray_trace_voge.cu:176);
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream), no host synchronisation, re-entrant across streams;
 *   - return value: 0 on success, a positive hipError_t value if the HIP runtime reported an
 *     error (the reference raises via AT_CUDA_CHECK, ray_trace_voge.cu:278,:377), or a
 *     negative VOGE_ERR_* code for argument errors.  Never throws.
 */
#ifndef VOGE_HIP_H
#define VOGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOGE_ABI_VERSION 7

#define VOGE_ERR_BAD_ARG (-1)        /* null pointer / non-positive size */
#define VOGE_ERR_WORKSPACE (-2)      /* workspace smaller than one view's voge_trace_workspace_bytes(1, ...) */
#define VOGE_ERR_K_TOO_LARGE (-3)    /* K above VOGE_MAX_K (top-K lists live in LDS) */

#define VOGE_MAX_K 256

typedef void *voge_stream_t; /* hipStream_t */

/* ABI version of the loaded library (== VOGE_ABI_VERSION it was built with). */
int voge_abi_version(void);

/* Human-readable text for a return code of any function below. */
const char *voge_error_string(int code);

/*
 * Bytes of scratch the forward trace needs for B batch elements of N Gaussians and an HxW
 * image: per-Gaussian derived records (cull sphere + quadratic-form coefficients, 112 B each),
 * the binning's segments (per 32x32-px super-tile and Gaussian slice) with their extension arenas,
 * the per-tile (8x8 px) depth-ordered candidate lists, and a pool of list entries (32 per Gaussian,
 * at least 2^20) for image quads with more candidates than the in-LDS sort takes.  165 MB per view at
 * 50k Gaussians / 512^2, 774 MB at 200k / 1024^2.  Views are independent: the entry points walk a
 * batch in CHUNKS of as many views as the scratch holds (stream-ordered launches on the same
 * buffers), and this function asks for the largest chunk under 1 GiB -- never less than one
 * view, never more than the batch.  Any size >= one view's (voge_trace_workspace_bytes(1, ...))
 * is accepted and used in full; pass more to keep a big batch in one chunk.  Caller allocates,
 * 256-byte aligned (any torch allocation is); the contents need no initialisation and nothing
 * in it outlives the call except what voge_trace_pool_usage reads (every chunk's pool counter, in the scratch's last 512 bytes).
 */
size_t voge_trace_workspace_bytes(int B, int N, int H, int W);

/*
 * Diagnostic: how much of the workspace's candidate-list POOL the last forward trace that ran on `workspace` (same
 * B, N, H, W) used.  The pool holds the lists of image quads (16x16 px) with more candidates than the in-LDS sort
 * takes (a small object behind a few dozen pixels); *used > *capacity means it ran out and those quads' tiles fell
 * back to streaming every Gaussian (slow, still exact).  workspace_bytes = what the trace was given: the chunks it walked
 * follow from it, and *used is the LARGEST use of any chunk (ABI 7; ABI 6 derived the layout from the default size and saw
 * the last chunk only).  Synchronous (copies 512 bytes from the device).  No reference
 * counterpart: the reference's coarse stage drops points when a bin overflows (rasterize_coarse.cu).
 */
int voge_trace_pool_usage(const void *workspace, size_t workspace_bytes, int B, int N, int H, int W, int *used,
                          int *capacity);

/*
 * (Not part of this ABI: `voge_debug_sweep_variant(int)` exists in -DVOGE_AB builds only -- voge_amd/libvoge_hip_ab.so, a
 * test artefact that also carries round 3's sweep (csrc/sweep_r3.h: scalar-sigma and general forms) for the bit-for-bit
 * comparisons in tests/test_gpu_configs.py, test_rebuilt_sweep_equals_round_3_sweep_bit_for_bit and
 * test_general_sweep_equals_round_3_general_sweep_bit_for_bit.  The product library is stateless and has no voge_debug_* symbol;
 * -DVOGE_SWEEP_TIMES / -DVOGE_BIN_TIMES timing builds (tools/) add voge_debug_sweep_times / voge_debug_bin_*.)
 */

/*
 * Fine ray trace forward, "all Gaussians are candidates" form.
 * Replaces: VoGE._C.ray_trace_voge_fine (ray_trace_voge.h:7-15, ray_trace_voge.cu:219-280)
 * called with the bin list RayTracing.py:22-26 builds for max_points_per_bin == -1
 * (every pixel of batch b sees Gaussians b*N .. b*N+N-1).  That P-long list is never
 * materialised here.
 *
 * For each pixel ray d and Gaussian (mu, A): dsd = d^T A d, len = mu^T A d / dsd,
 * act = mu^T A mu - (mu^T A d)^2 / dsd; keep if act < thr_act (and len < 1e10, the
 * sentinel); output the K kept candidates with the smallest (len, index), ascending;
 * unused slots hold idx=-1, len=1e10, act=1e10, dsd=0 (ray_trace_voge.cu:184-214,:244-247).
 * idx holds the global index b*N+i.  Outputs need no pre-fill.  cnt: NULL, or [B,H,W] int32
 * receiving the number of hits kept per pixel (the filled prefix of the K slots).
 * A ray need not be unit: len scales with 1 / |d| as the formula says (a tile with a ray whose |d|^2 is not within 4e-5 of 1 only switches
 * the early exit off for its tile); a zero or non-finite ray, and one so short that every len is beyond 1e10, yields an empty
 * pixel (cnt 0, sentinels); a form with d^T A d == 0 (A = 0 included) is never a hit, as in the reference, whose len is 0 / 0
 * there (tests/test_gpu_trace_bounds.py).  This holds for the entry points that cull and sweep (this one, its scalar and view
 * forms, the fragments and frame entries); voge_trace_topk_list_fwd evaluates A = 0 I as a finite len with act = 0.
 *
 * cam_fwd: NULL, or [B,3] unit view axis in the rays' frame: Gaussians with mu.fwd < 0
 * are skipped, which is the candidate rule of the reference's coarse stage
 * (rasterize_coarse.cu:35, "skip z<0") used when max_points_per_bin != -1.
 * cones: NULL, or the bounding-cone hierarchy of the rays (per 32x32-pixel super-tile: its own cone, its four
 * 16x16 quads', its sixteen 8x8 tiles') that voge_rays_fwd / voge_ray_cones produced for exactly this
 * `rays` tensor (voge_cones_floats(B,H,W) floats, an opaque blob); they only steer the conservative
 * candidate culling.  NULL costs one more launch that derives them.
 */
int voge_trace_topk_fwd(const float *mus, const float *isigmas, const float *rays,
                        const float *cam_fwd, const float *cones, int B, int N, int H, int W, int K,
                        float thr_act, void *workspace, size_t workspace_bytes,
                        int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                        voge_stream_t stream);

/*
 * Fine ray trace forward with caller-supplied candidate lists.
 * Replaces: VoGE._C.ray_trace_voge_fine for an explicit bin_points tensor
 * [B,BH,BW,M] int32, -1 = empty (ray_trace_voge.cu:135-217): pixel (y,x) of batch b
 * scans bin (y/bin_size, x/bin_size).  P = total Gaussians (list entries index [0,P)).
 * Same outputs as above (cnt: NULL or [B,H,W] int32, the hits kept per pixel).  Exact ties in
 * len are ordered by index (the reference orders them by list position, which is not
 * deterministic for coarse-rasterised lists).  Measured against the reference's own kernel in
 * tests/test_gpu_reference_kernels.py: lists in ascending index order match it exactly, lists in
 * descending order differ by the swap of a tied pair and nothing else.
 */
int voge_trace_topk_list_fwd(const float *mus, const float *isigmas, const float *rays,
                             const int32_t *bin_points, int B, int P, int H, int W, int K,
                             int BH, int BW, int M, int bin_size, float thr_act,
                             int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                             voge_stream_t stream);

/*
 * Fine ray trace backward.
 * Replaces: VoGE._C.ray_trace_voge_fine_backward (ray_trace_voge.h:17-25,
 * ray_trace_voge.cu:283-379).  The pixel grid is given as nrows = B*H rows of W pixels (the
 * kernel works on 16x16 pixel tiles of that grid).  For every slot with idx >= 0 applies the
 * chain rule of ray_trace_voge.cu:324-326 and scatters into
 *   g_ray [nrows*W,3], g_mus [P,3], g_isg [P,3,3]  (raw outer products, not symmetrised).
 * g_mus / g_isg are fully written by this call (the reference allocates zeros, :354-356);
 * g_ray is fully written, or may be NULL when the ray gradient is not needed.
 * cnt: NULL, or [nrows*W] int32 = number of leading slots of each pixel that may hold a hit
 * (the forward's out_cnt): slots k >= cnt[pixel] are not even loaded.
 * workspace: >= voge_trace_bwd_workspace_bytes(P) bytes, 256-byte aligned.
 */
int voge_trace_bwd(const float *mus, const float *isigmas, const float *rays,
                   const int32_t *idx, const int32_t *cnt, const float *g_len, const float *g_act,
                   const float *g_dsd, int P, long nrows, int W, int K, void *workspace,
                   size_t workspace_bytes, float *g_ray, float *g_mus, float *g_isg,
                   voge_stream_t stream);

/* Scratch bytes voge_trace_bwd needs for P Gaussians (packed records + padded accumulator). */
size_t voge_trace_bwd_workspace_bytes(int P);

/*
 * Isotropic variants of the two calls above: every Gaussian is A = a I with ONE scalar a [P]
 * (the reference's (N,) sigma form: expend_sigma, Aggregation.py:155-157, then 2*sigma,
 * Renderer.py:133).  Same outputs as voge_trace_topk_fwd; the backward returns g_a [P], the
 * gradient of that scalar (= trace of the general call's g_isg), and g_mus [P,3].  Four sums per
 * Gaussian instead of twelve, and the caller's scalar -> 3x3 expansion (and its backward)
 * disappears.  workspace of the backward: >= voge_trace_bwd_iso_workspace_bytes(P).
 */
int voge_trace_topk_fwd_iso(const float *mus, const float *a, const float *rays,
                            const float *cam_fwd, const float *cones, int B, int N, int H, int W, int K,
                            float thr_act, void *workspace, size_t workspace_bytes,
                            int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                            voge_stream_t stream);
int voge_trace_bwd_iso(const float *mus, const float *a, const float *rays, const int32_t *idx,
                       const int32_t *cnt, const float *g_len, const float *g_act, const float *g_dsd,
                       int P, long nrows, int W, int K, void *workspace, size_t workspace_bytes,
                       float *g_ray, float *g_mus, float *g_a, voge_stream_t stream);
size_t voge_trace_bwd_iso_workspace_bytes(int P);

/*
 * The same two calls with the renderer's elementwise preamble folded in (VoGE/Renderer.py:130-137:
 * `verts - origin` per view and `2 * sigmas` / `2 / sigmas` (inverse_sigma)): the per-Gaussian pass that
 * reads the inputs anyway applies them, and the backward's per-Gaussian pass applies their chain rule,
 * so the caller launches no elementwise kernels around the trace.
 *   verts   [N,3] (shared != 0: one set seen by all B views) or [B*N,3];  sigmas [N] or [B*N]
 *   origin  [B,3] camera centres, or NULL (no centring);  sigma_mode 0: a = sigma, 1: a = 2 sigma, 2: a = 2/sigma
 * Forward outputs as voge_trace_topk_fwd (indices are b*N + n).  Backward: g_verts / g_sigmas have the
 * shapes of verts / sigmas (summed over the views when shared); no gradient is produced for origin --
 * a caller that needs it (camera pose optimisation) uses the plain calls.  Workspaces as above with P = B*N.
 */
int voge_trace_topk_fwd_iso_view(const float *verts, const float *sigmas, const float *origin, int shared,
                                 int sigma_mode, const float *rays, const float *cam_fwd, const float *cones,
                                 int B, int N, int H, int W, int K, float thr_act, void *workspace,
                                 size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                                 int32_t *cnt, voge_stream_t stream);
int voge_trace_bwd_iso_view(const float *verts, const float *sigmas, const float *origin, int shared,
                            int sigma_mode, const float *rays, const int32_t *idx, const int32_t *cnt,
                            const float *g_len, const float *g_act, const float *g_dsd, int B, int N, long nrows,
                            int W, int K, void *workspace, size_t workspace_bytes, float *g_ray,
                            float *g_verts, float *g_sigmas, voge_stream_t stream);

/*
 * The reference's coarse stage, for callers that want ITS candidate lists (the default render path does
 * not need them: see voge_trace_topk_fwd).  Replaces: VoGE._C.rasterize_points_coarse
 * (rasterize_coarse.h:18-25; rasterize_coarse.cu:20-42,44-188,254-305): points [P,3] f32 = (x_ndc, y_ndc,
 * view z), radius [P,2] f32 (half extents in NDC units), cloud_to_packed_first_idx / num_points_per_cloud
 * [B] int64 -> bin_elems [B,BH,BW,M] int32, -1 padded (BH = 1 + (H-1)/bin_size, BW likewise; both < 66).
 * A point is listed in every bin its bbox overlaps (half-pixel pad), unless z < 0; points are taken in
 * chunks of 512 and a chunk that no longer fits a bin's M slots is dropped.  Unlike the reference the
 * chunks are taken in ascending order: lists are ascending in index and deterministic.
 */
int voge_bin_gaussians(const float *points, const int64_t *cloud_to_packed_first_idx,
                       const int64_t *num_points_per_cloud, int B, int P, int H, int W, const float *radius,
                       int bin_size, int max_points_per_bin, int32_t *bin_elems, voge_stream_t stream);

/*
 * Fine trace + composite in ONE call: what GaussianRenderer.forward asks for (VoGE/Renderer.py:139-150:
 * ray_tracing, then aggregation -> Fragments).  Replaces the pair
 *   VoGE._C.ray_trace_voge_fine (ray_trace_voge.cu:135-280)  +  `aggregation` (VoGE/Aggregation.py:82-107)
 * for the all-candidates list.  Arguments as voge_trace_topk_fwd / _iso / _iso_view, plus occ (the
 * renderer's absorptivity) and the fragment outputs weight [B,H,W,K] f32 and valid_num [B,H,W] i64.
 * records (iso forms): NULL, or [B*N,4] floats receiving the per-Gaussian (centred mean, a) pairs the trace
 * derives anyway -- the fused backward (voge_fragment_shade_bwd_iso) reads them instead of packing its own.
 * idx / len / weight / valid_num are the fragments (sentinels -1 / 1e10 / 0 in empty slots); act, dsd
 * and cnt [B,H,W] (required here) are what the backward needs -- in pixels WITHOUT any hit act / dsd are
 * may be left unwritten (nothing reads them: every consumer goes by cnt).  Results are bit-identical
 * to calling the two entry points one after the other (which is what happens on the device: compositing
 * inside the sweep's epilogue was measured slower, see trace_fwd.hip); the call saves the host side one
 * autograd node and a set of allocations per frame.
 */
/* Scalar-sigma forms (_iso, _iso_view) only: act and dsd may BOTH be NULL.  The sweep then writes index and len alone
 * (no per-slot gather in its epilogue), the composite derives act / dsd from the (mean, a) records with the same
 * operations (voge_composite_fwd_iso), and so does voge_fragment_shade_bwd_iso when handed NULL for them: 168 MB per
 * frame at 50k Gaussians / 512^2 / K = 40 that are neither written nor read.  Weights are bit-identical either way.
 * voge_fragment_act_dsd_iso materialises them afterwards for consumers that want the arrays.
 * TRACE ONLY (scalar-sigma forms): weight = valid_num = act = dsd = NULL with records given -- the call stops behind the
 * sweep (idx, len, cnt, records are written) and the caller composites when it knows what it wants: voge_composite_fwd_iso
 * for the weights alone, or voge_composite_shade_fwd_iso for the weights AND the image of to_colored_background in one
 * pass (GaussianRenderer returns its Fragments before the colours are known: the Python side defers the composite
 * until the fragments' weights are first asked for, voge_amd/Renderer.py). */
/* TRACE ONLY for the general forms (mus [P,3], isigmas [P,3,3]): idx, len, cnt and `records` -- the packed (mu, A),
 * [B*N][12] floats -- are written; voge_composite_fwd_rec / voge_composite_shade_fwd_rec composite later from them, and
 * voge_fragment_shade_bwd / voge_fragment_bwd / voge_fragment_merge_bwd take act = dsd = NULL for such fragments.
 * Replaces the same reference code as voge_fragments_fwd (RayTracing.py:17-59 + ray_trace_voge.cu:219-280), deferred. */
int voge_trace_lean_fwd(const float *mus, const float *isigmas, const float *rays, const float *cam_fwd,
                        const float *cones, int B, int N, int H, int W, int K, float thr_act, void *workspace,
                        size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records,
                        voge_stream_t stream);
int voge_fragments_fwd(const float *mus, const float *isigmas, const float *rays, const float *cam_fwd,
                       const float *cones, int B, int N, int H, int W, int K, float thr_act, float occ,
                       void *workspace, size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                       int32_t *cnt, float *weight, int64_t *valid_num, voge_stream_t stream);
int voge_fragments_fwd_iso(const float *mus, const float *a, const float *rays, const float *cam_fwd,
                           const float *cones, int B, int N, int H, int W, int K, float thr_act, float occ,
                           void *workspace, size_t workspace_bytes, int32_t *idx, float *len, float *act,
                           float *dsd, int32_t *cnt, float *weight, int64_t *valid_num, float *records,
                           voge_stream_t stream);
int voge_fragments_fwd_iso_view(const float *verts, const float *sigmas, const float *origin, int shared,
                                int sigma_mode, const float *rays, const float *cam_fwd, const float *cones,
                                int B, int N, int H, int W, int K, float thr_act, float occ, void *workspace,
                                size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                                int32_t *cnt, float *weight, int64_t *valid_num, float *records, voge_stream_t stream);

/*
 * Fused backward of the fragment pipeline for isotropic Gaussians: shade (merge_final + get_silhouette +
 * to_colored_background, VoGE/Aggregation.py:111-141, VoGE/Renderer.py:157-171) -> aggregation
 * (VoGE/Aggregation.py:30-107) -> fine trace (ray_trace_voge.cu:283-332), in ONE pass over the fragments:
 * what voge_shade_bwd, voge_composite_bwd and voge_trace_bwd_iso(_view) compute one after the other, without
 * their exchanges through memory (g_weight; g_len / g_act / g_dsd) and with one accumulation table per wave.
 * records [B*N,4] = the (centred mean, a) pairs the forward kept (the `records` argument of
 * voge_fragments_fwd_iso / _iso_view); sigmas / shared / sigma_mode as in voge_trace_bwd_iso_view (pass the a
 * array, 0, 0 for plain (mus, a) inputs); rgb / wsum = voge_shade_fwd's out_rgb / out_wsum; g_img = the gradient of
 * the image, element (pixel p, channel c) at g_img[p * g_stride_pix + c * g_stride_c]: (C, 1) for a contiguous
 * [nrows*W,C] array, (0, 0) for the one broadcast scalar autograd hands back for sum() / mean() losses (no
 * materialised copy of it is needed).  Writes g_verts, g_sigmas (both or neither) and g_colors [Nattr,C].  K <= 128;
 * C <= 4; cnt required.  workspace: >= voge_fragment_bwd_workspace_bytes(B*N) bytes.
 */
size_t voge_fragment_bwd_workspace_bytes(int P);
/* act / dsd [npix,K] of scalar-sigma fragments that were traced without them (see voge_fragments_fwd_iso): records
 * [P,4] = the (centred mean, a) pairs of that call, idx / len / cnt its outputs.  Sentinels (1e10, 0) in empty slots. */
int voge_fragment_act_dsd_iso(const float *records, const float *rays, const int32_t *idx, const float *len,
                              const int32_t *cnt, long npix, int K, int P, float *act, float *dsd, voge_stream_t stream);
/* Composite forward from (idx, len) and the records instead of (act, len, dsd): what voge_fragments_fwd_iso* runs behind
 * its sweep when act / dsd are omitted.  cnt required. */
int voge_composite_fwd_iso(const int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                           const float *rays, float occ, long npix, int K, float *weight, int64_t *valid_num,
                           voge_stream_t stream);
/* Composite forward (as voge_composite_fwd_iso) with the SHADE stage in the same pass: merge_final + get_silhouette +
 * to_colored_background (VoGE/Aggregation.py:111-141, VoGE/Renderer.py:157-171) -- what voge_composite_fwd_iso followed
 * by voge_shade_fwd computes, without reading idx / weight back (8 bytes per slot) and without the second launch.
 * colors [Nattr,C], C = 3 | 4; bg [C]; thr as voge_shade_fwd.  Writes weight [npix,K], valid_num [npix], rgb / img [npix,C],
 * wsum [npix], and rewrites the empty slots of idx in place (-1 -> 0, Aggregation.py:131).  Any K <= VOGE_MAX_K; cnt required.
 * img = NULL (bg unused): merge_final and the weight sum only -- interpolate_attr / get_silhouette, no background. */
int voge_composite_shade_fwd_iso(int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                                 const float *rays, float occ, const float *colors, const float *bg, float thr,
                                 long npix, int K, int C, long Nattr, float *weight, int64_t *valid_num, float *rgb,
                                 float *img, float *wsum, voge_stream_t stream);
/* The two composite entry points above for the GENERAL path: records = the packed (mu, A) [B*N][12] of voge_trace_lean_fwd
 * (act / dsd re-derived with make_eval + pair_eval, the operations of the sweep's own epilogue: bit-identical weights).
 * act / dsd [npix,K] (both or NULL): written for the live slots when given -- the fused backward reads 8 bytes per slot
 * rather than gathering 48 and evaluating again. */
int voge_composite_fwd_rec(int32_t *idx, const int32_t *cnt, const float *len, const float *records, const float *rays,
                           float occ, long npix, int K, float *weight, int64_t *valid_num, float *act, float *dsd,
                           voge_stream_t stream);
int voge_composite_shade_fwd_rec(int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                                 const float *rays, float occ, const float *colors, const float *bg, float thr,
                                 long npix, int K, int C, long Nattr, float *weight, int64_t *valid_num, float *rgb,
                                 float *img, float *wsum, float *act, float *dsd, voge_stream_t stream);
/* The same for full 3x3 forms (mus [P,3], isigmas [P,3,3] as given to voge_fragments_fwd; P = B*N): writes g_mus
 * [P,3], g_isigmas [P,3,3] (the raw, unsymmetrised outer-product sums of ray_trace_voge.cu:324-326, as voge_trace_bwd)
 * -- both or neither -- and g_colors [Nattr,C].  Same constraints and workspace as the isotropic form. */
int voge_fragment_shade_bwd(const float *mus, const float *isigmas, const float *rays, const float *colors,
                            const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                            const float *len, const float *dsd, const float *rgb, const float *wsum, const float *bg,
                            float thr, const float *g_img, long g_stride_pix, long g_stride_c, float occ, int P,
                            long nrows, int W, int K, int C, long Nattr, void *workspace, size_t workspace_bytes,
                            float *g_mus, float *g_isigmas, float *g_colors, voge_stream_t stream);
int voge_fragment_shade_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                const float *rays, const float *colors, const int32_t *idx, const int32_t *cnt,
                                const float *weight, const float *act, const float *len, const float *dsd,
                                const float *rgb, const float *wsum, const float *bg, float thr,
                                const float *g_img, long g_stride_pix, long g_stride_c, float occ, int B, int N,
                                long nrows, int W, int K, int C, long Nattr, void *workspace, size_t workspace_bytes, float *g_verts,
                                float *g_sigmas, float *g_colors, voge_stream_t stream);

/*
 * ABI 7 -- ONE FRAME of the renderer as six launches (binA, binB, sweep | composite | fused backward, finish): the camera goes
 * in, no ray-generation launch and no fill launch run.
 *
 * voge_frame_trace_fwd_iso   GaussianRenderer.forward (VoGE/Renderer.py:102-150) up to and including ray_tracing, for scalar
 *   sigmas and one Gaussian set per view (`shared` != 0: [N,3] / [N] seen by all B views) or per batch element ([B,N,..]):
 *   the ray bundle of Renderer.py:124-128, the centring of :130, the sigma rule of :133-137 (sigma_mode 0: a = sigma,
 *   1: a = 2 sigma, 2: a = 2 / sigma), RayTracing.py:12-30 and ray_trace_voge.cu:135-217 -- as binA + binB + sweep, with
 *   NO ray-generation launch: every kernel derives the rays / bounding cones / camera centre / view axis it needs from
 *   R [B,3,3], T [B,3], focal [B,2], pp [B,2] with voge_rays_fwd's own operations (bit-identical rays; the cones are the
 *   analytic corner-ray cones of csrc/voge_common.h).  The band rendered is h stacked rows of W pixels; stacked row i is image
 *   row row0 + (i / stripe_h) * pitch + i % stripe_h (one contiguous band: stripe_h >= h, pitch = 0).  behind != 0: Gaussians
 *   behind the camera plane are no candidates (rasterize_coarse.cu:35; what cam_fwd = R[:, :, 2] selects in the other entries).
 *   Writes idx, len [B,h,W,K], cnt [B,h,W], records [B*N,4] (centred mean, a), rays [B,h,W,3] (by the sweep) and origin [B,3]
 *   (NULL: not wanted).
 *   workspace: voge_trace_workspace_bytes(B, N, h, W).  No act / dsd (the fragments' consumers re-derive them).
 * voge_frame_shade_fwd_iso   = voge_composite_shade_fwd_iso (aggregation + merge_final + get_silhouette +
 *   to_colored_background, Aggregation.py:82-141, Renderer.py:157-171; img = bg = NULL: interpolate_attr + the weight sum)
 *   that ALSO zeroes bwd_acc [bwd_acc_bytes, a multiple of 16, 16-byte aligned; NULL: nothing] on its way: the accumulator
 *   of the backward below (voge_frame_bwd_acc_bytes(B * N)), so that no fill launch stands in front of it -- and writes
 *   sil [npix] = min(sum_k w_k, 1) (get_silhouette, Renderer.py:157-159; NULL: not wanted) with the sum it has in hand: the
 *   reference's training pattern (interpolate_attr + get_silhouette, demo/ShapeFitting.py:217-222) is this ONE launch, and its
 *   backward ONE call: voge_frame_merge_bwd_iso with wsum_fwd = the forward's wsum takes g_wsum as the SILHOUETTE's gradient
 *   (passed on like torch.minimum's: all below 1, half at a tie, none above; wsum_fwd = NULL: g_wsum is the sum's own gradient).
 * voge_frame_shade_bwd_iso / voge_frame_merge_bwd_iso   = voge_fragment_shade_bwd_iso / voge_fragment_merge_bwd_iso for
 *   fragments that keep no act / dsd, taking that accumulator -- ZEROED, good for one call -- in place of a scratch they would
 *   have to fill first: the fused kernel + the finishing pass.  (Adding the per-Gaussian sums straight into the gradient
 *   arrays was built and measured: one launch less, 30 us slower -- three atomic requests per table entry instead of one.)
 */
size_t voge_frame_bwd_acc_bytes(int P);
/*
 * Diagnostic: the bounding cones the voge_frame_* entry points make from the camera inside their binning kernels, by the same
 * device functions.  hier [B][nst * 21][8] floats: per view the super-tiles' (32x32 px) records, then [nst][4] quads (16x16 px,
 * qy * 2 + qx), then [nst][16] tiles (8x8 px, ty * 4 + tx) -- voge_cones_floats' layout; regions [B][ceil(h/128) * ceil(W/128)][8]
 * floats: the 128x128-px regions.  A record is (axis xyz, lower bound of the cosine, upper bound of the sine, ok, 2 pad); ok = -1:
 * the block has no pixel in the band.  The band is h stacked rows of W pixels as in voge_frame_trace_fwd_iso.
 */
int voge_camera_cones(const float *R, const float *T, const float *focal, const float *pp, int row0, int stripe_h, int pitch,
                      int B, int h, int W, float *hier, float *regions, voge_stream_t stream);

int voge_frame_trace_fwd_iso(const float *verts, const float *sigmas, int shared, int sigma_mode, const float *R,
                             const float *T, const float *focal, const float *pp, int row0, int stripe_h, int pitch,
                             int behind, int B, int N, int h, int W, int K, float thr_act, void *workspace,
                             size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records,
                             float *rays, float *origin, voge_stream_t stream);
int voge_frame_shade_fwd_iso(int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                             const float *rays, float occ, const float *colors, const float *bg, float thr,
                             long npix, int K, int C, long Nattr, float *weight, int64_t *valid_num,
                             float *rgb, float *img, float *wsum, float *sil, void *bwd_acc, size_t bwd_acc_bytes,
                             voge_stream_t stream);
int voge_frame_shade_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                             const float *rays, const float *colors, const int32_t *idx, const int32_t *cnt,
                             const float *weight, const float *len, const float *rgb, const float *wsum,
                             const float *bg, float thr, const float *g_img, long g_stride_pix, long g_stride_c,
                             float occ, int B, int N, long nrows, int W, int K, int C, long Nattr, void *acc_zeroed,
                             size_t acc_bytes, float *g_verts, float *g_sigmas, float *g_colors, voge_stream_t stream);
int voge_frame_merge_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                             const float *rays, const float *attr, const int32_t *idx, const int32_t *cnt,
                             const float *weight, const float *len, const float *g_rgb, long g_stride_pix,
                             long g_stride_c, const float *g_wsum, const float *wsum_fwd, float occ, int B, int N, long nrows,
                             int W, int K, int C, long Nattr, void *acc_zeroed, size_t acc_bytes, float *g_verts,
                             float *g_sigmas, float *g_attr, voge_stream_t stream);

/*
 * Depth on the frame path (EXTENSION: the reference has no depth output).  With n = min(cnt, K) live slots of a pixel,
 * A = sum_{k<n} w_k len_k and S = sum_{k<n} w_k:  depth = A / S where S > 0, else `background` (normalize != 0: the expected hit
 * distance along the unit pixel ray), or A itself (normalize == 0; background ignored).  Not clamped; not view-space z.
 * voge_frame_depth_fwd_iso   = voge_frame_shade_fwd_iso without a colour table: from idx, cnt, len, records and rays it writes
 *   weight [npix][K], valid_num, depth [npix], wsum [npix] = S and sil [npix] = min(S, 1) (NULL: not wanted) in ONE launch, and
 *   zeroes bwd_acc [bwd_acc_bytes, a multiple of 16, 16-byte aligned; NULL: nothing] on its way: the accumulator of the backward
 *   below, 16 bytes per Gaussian (four sums, no colour term).  The index list is NOT rewritten (-1 stays -1).  K <= 128.
 *   Replaces the torch expression (frag.vert_weight * frag.vert_hit_length).sum(-1) / frag.vert_weight.sum(-1) -- and the
 *   composite launch in front of it.
 * voge_frame_depth_bwd_iso   = its backward, modelled on voge_frame_merge_bwd_iso: acc_zeroed [>= 16 * B * N bytes, ZEROED, good
 *   for one call], one fused launch, the finishing pass.  Per pixel it forms a = g_depth / S, b = -a depth (normalize, S > 0;
 *   zero elsewhere) or a = g_depth, b = 0, adds the pass-through of g_sil [npix] (the gradient of min(S, 1); NULL: none) to b, and
 *   feeds g_w[k] = a len_k + b and g_len[k] = a w_k to the composite + trace backward.  g_depth: element p at
 *   g_depth[p * g_stride_pix] (1: contiguous, 0: one value for every pixel) or NULL when only g_sil is given.  Replaces autograd's
 *   backward of that expression plus TWO voge_fragment_bwd_iso calls (one for g_weight, one for g_len).  K <= 128.
 */
int voge_frame_depth_fwd_iso(const int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                             const float *rays, float occ, int normalize, float background, long npix, int K,
                             float *weight, int64_t *valid_num, float *depth, float *wsum, float *sil, void *bwd_acc,
                             size_t bwd_acc_bytes, voge_stream_t stream);
int voge_frame_depth_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode, const float *rays,
                             const int32_t *idx, const int32_t *cnt, const float *weight, const float *len,
                             const float *depth, const float *wsum, const float *g_depth, long g_stride_pix,
                             const float *g_sil, int normalize, float occ, int B, int N, long nrows, int W, int K,
                             void *acc_zeroed, size_t acc_bytes, float *g_verts, float *g_sigmas, voge_stream_t stream);

/*
 * ABI 7, the frame path for (N,3) / (N,3,3) sigmas (Renderer.py:130-137 with Aggregation.py:144-175: A = 2 expend_sigma(sigmas);
 * no inverse_sigma).  voge_frame_trace_fwd_gen: voge_frame_trace_fwd_iso's contract with the USER's arrays as inputs -- verts
 * [N | B*N][3] (shared_verts: one set for all views), sigmas [N | B*N][3] (kind 1: per-axis) or [N | B*N][3][3] (kind 2) -- the record pass
 * centres and expands them (the preamble's own fp32 operations), so neither a ray launch nor a preamble launch stands in front
 * of the frame; records = kind 2: the packed (centred mu, A) [B*N][12]; kind 1: the compact (centred mu, a0, a1, a2, 0, 0) [B*N][8], which
 * the composite and the backward evaluate with the three coefficients alone (the general chain's bits on such a form).
 * voge_frame_shade_fwd_rec = voge_composite_shade_fwd_rec (C = 0: voge_composite_fwd_rec) on records of `kind` that also zeroes
 * bwd_acc (voge_frame_bwd_gen_acc_bytes); kind 1 keeps no act / dsd (pass NULL).  voge_frame_bwd_gen: EVERY backward route of such fragments -- form 0: the image's
 * gradient (voge_fragment_shade_bwd), 1: merge_final's (voge_fragment_merge_bwd; wsum = g_wsum | NULL), 2: the weights' own
 * (voge_fragment_bwd: g = g_weight with strides, g_hitlen | NULL; attr / rgb / bg unused, C = 0) -- reading the forward's records (no
 * pack launch), with acc zeroed already (acc_is_zero != 0) or filled here, and writing the gradients of verts and sigmas AS THE USER
 * HOLDS THEM (the sum over the views of a shared set, d A / d sigma = 2: no preamble-backward launch).  K <= 128 (form 2: 256).
 */
size_t voge_frame_bwd_gen_acc_bytes(int P);
int voge_frame_trace_fwd_gen(const float *verts, const float *sigmas, int shared_verts, int shared_sigmas, int kind,
                             const float *R, const float *T, const float *focal, const float *pp, int row0, int stripe_h,
                             int pitch, int behind, int B, int N, int h, int W, int K, float thr_act, void *workspace,
                             size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records, float *rays,
                             float *origin, voge_stream_t stream);
int voge_frame_shade_fwd_rec(int kind, int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                             const float *rays, float occ, const float *colors, const float *bg, float thr,
                             long npix, int K, int C, long Nattr, float *weight, int64_t *valid_num,
                             float *rgb, float *img, float *wsum, float *sil, float *act, float *dsd, void *bwd_acc,
                             size_t bwd_acc_bytes, voge_stream_t stream);
int voge_frame_bwd_gen(int form, const float *records, int shared_verts, int shared_sigmas, int kind, const float *rays,
                       const float *attr, const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                       const float *len, const float *dsd, const float *rgb, const float *wsum, const float *bg, float thr,
                       const float *g, long g_stride0, long g_stride1, const float *g_hitlen, float occ, int B, int N,
                       long nrows, int W, int K, int C, long Nattr, void *acc, size_t acc_bytes, int acc_is_zero,
                       float *g_verts, float *g_sigmas, float *g_attr, voge_stream_t stream);

/*
 * ABI 7 (additive), the frame path for ORIENTED Gaussians: three scales and a rotation per Gaussian instead of a [3][3] form.
 * Replaces: S = R(q) diag(s) R(q)^T composed in torch in front of voge_frame_trace_fwd_gen(kind 2) -- the host-side product of
 * VoGE/Converter/Converters.py:35-71 (rot @ shape @ rot^T), Aggregation.py:144-175 and Renderer.py:133-137 (A = 2 S, or A = 2 S^-1
 * under inverse_sigma) -- and autograd through it behind voge_frame_bwd_gen.
 *   scales [N | B*N][3] (> 0), quats [N | B*N][4] = (w, x, y, z), 16-byte aligned, need not be unit: qh = q / |q|; a quaternion
 *   whose squared norm, computed in fp32, is not a positive finite number (zero or underflowed, NaN, infinite or overflowed) is the
 *   identity rotation in the forward AND gets a zero gradient in the backward.  shared_sigmas covers both.
 *   R(qh) = [[1-2(y^2+z^2), 2(xy-wz), 2(xz+wy)], [2(xy+wz), 1-2(x^2+z^2), 2(yz-wx)], [2(xz-wy), 2(yz+wx), 1-2(x^2+y^2)]];
 *   A_ij = sum_k (d_k R_ik) R_jk for i <= j, mirrored (bitwise symmetric); sigma_mode 1: d = 2 s, 2: d = 2 / s (inverse_sigma).
 * voge_frame_trace_fwd_ori: voge_frame_trace_fwd_gen's contract and remaining arguments; records = kind 2's packed (centred mu, A)
 *   [B*N][12], so voge_frame_shade_fwd_rec(kind = 2, ...) composites them and nothing behind the record pass differs.
 * voge_frame_bwd_ori: voge_frame_bwd_gen(kind 2)'s forms, inputs and accumulator (voge_frame_bwd_gen_acc_bytes); the finishing pass
 *   turns the raw 3x3 sums G into g_scales [N | B*N][3] (g_d[k] = r_k^T G r_k; 2 g_d or -2 g_d / s^2) and g_quats [N | B*N][4]
 *   (through g_R = (G + G^T) R diag(d) and the normalisation: orthogonal to q), a shared set summing its views in a fixed order.
 *   g_scales and g_quats: both or neither; g_verts as voge_frame_bwd_gen.
 */
int voge_frame_trace_fwd_ori(const float *verts, const float *scales, const float *quats, int shared_verts, int shared_sigmas,
                             int sigma_mode, const float *R, const float *T, const float *focal, const float *pp, int row0,
                             int stripe_h, int pitch, int behind, int B, int N, int h, int W, int K, float thr_act, void *workspace,
                             size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records, float *rays,
                             float *origin, voge_stream_t stream);
int voge_frame_bwd_ori(int form, const float *records, const float *scales, const float *quats, int shared_verts, int shared_sigmas,
                       int sigma_mode, const float *rays, const float *attr, const int32_t *idx, const int32_t *cnt,
                       const float *weight, const float *act, const float *len, const float *dsd, const float *rgb, const float *wsum,
                       const float *bg, float thr, const float *g, long g_stride0, long g_stride1, const float *g_hitlen, float occ,
                       int B, int N, long nrows, int W, int K, int C, long Nattr, void *acc, size_t acc_bytes, int acc_is_zero,
                       float *g_verts, float *g_scales, float *g_quats, float *g_attr, voge_stream_t stream);

/* interpolate_attr (+ get_silhouette) on fragments of this renderer, backward: merge_final's own backward
 * (VoGE/Aggregation.py:111-141; g_rgb = the gradient of the merged attributes [nrows*W,C], strides as g_img above), plus
 * g_wsum [nrows*W] or NULL = the gradient of the per-pixel weight sum (get_silhouette = min(sum, 1) of the same fragments),
 * then composite and trace as above -- the reference's training pattern (demo/ShapeFitting.py:217,295) as ONE kernel.
 * attr [Nattr,C], C <= 4, K <= 128.  Writes g_verts / g_sigmas (both or neither) and g_attr [Nattr,C]. */
int voge_fragment_merge_bwd(const float *mus, const float *isigmas, const float *rays, const float *attr,
                            const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                            const float *len, const float *dsd, const float *g_rgb, long g_stride_pix,
                            long g_stride_c, const float *g_wsum, float occ, int P, long nrows, int W, int K, int C,
                            long Nattr, void *workspace, size_t workspace_bytes, float *g_mus, float *g_isigmas,
                            float *g_attr, voge_stream_t stream);      /* (the general 3x3 form of the entry point below) */
int voge_fragment_merge_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                const float *rays, const float *attr, const int32_t *idx, const int32_t *cnt,
                                const float *weight, const float *act, const float *len, const float *dsd,
                                const float *g_rgb, long g_stride_pix, long g_stride_c, const float *g_wsum,
                                float occ, int B, int N, long nrows, int W, int K, int C, long Nattr,
                                void *workspace, size_t workspace_bytes, float *g_verts, float *g_sigmas,
                                float *g_attr, voge_stream_t stream);

/*
 * The same single pass driven by the gradient of the WEIGHTS, whoever produced it: the backward of
 * `aggregation` (VoGE/Aggregation.py:30-107, autograd in the reference) followed by the fine trace's
 * (ray_trace_voge.cu:283-332) for fragments made by voge_fragments_fwd*.  This is what the reference's own training
 * loops need -- they differentiate through interpolate_attr (merge_final) and get_silhouette, not through
 * to_colored_background (demo/ShapeFitting.py:217,295; demo/ReasonOcclusion.py:106-109;
 * demo/EfficientCuboidViaOptimization.py:109-112).  Replaces voge_composite_bwd + voge_trace_bwd*(_iso, _iso_view) and
 * their exchange of g_len / g_act / g_dsd through memory; act / dsd may be NULL for scalar-sigma fragments that were
 * traced without them.
 *   g_weight: element (pixel p, slot k) at g_weight[p * gw_stride_pix + k * gw_stride_k] -- (K, 1) for a contiguous
 *             [nrows*W,K] array, (1, 0) for a per-pixel value broadcast over the slots (the gradient a silhouette
 *             loss alone hands back); NULL = zero.
 *   g_hitlen: NULL, or [nrows*W,K] contiguous: the gradient of vert_hit_length (= the trace's len, Aggregation.py:107).
 * Any K <= VOGE_MAX_K (odd K too; lists of more than 128 slots put four slots on a lane).  cnt required.
 * idx must be what the trace wrote: the first cnt[p] slots of a pixel hold DISTINCT Gaussians (the per-Gaussian
 * accumulation takes a pixel's lanes through its table together, without arbitration between them).
 * Writes g_verts / g_sigmas (iso: through the view's chain rule, as voge_trace_bwd_iso_view) or g_mus [P,3] /
 * g_isigmas [P,3,3] (raw outer-product sums, as voge_trace_bwd).  No ray gradient: callers that optimise the rays
 * themselves use voge_composite_bwd + voge_trace_bwd.  workspace: >= voge_fragment_bwd_workspace_bytes(B*N) bytes.
 */
int voge_fragment_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode, const float *rays,
                          const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                          const float *len, const float *dsd, const float *g_weight, long gw_stride_pix,
                          long gw_stride_k, const float *g_hitlen, float occ, int B, int N, long nrows, int W, int K,
                          void *workspace, size_t workspace_bytes, float *g_verts, float *g_sigmas,
                          voge_stream_t stream);
int voge_fragment_bwd(const float *mus, const float *isigmas, const float *rays, const int32_t *idx,
                      const int32_t *cnt, const float *weight, const float *act, const float *len,
                      const float *dsd, const float *g_weight, long gw_stride_pix, long gw_stride_k,
                      const float *g_hitlen, float occ, int P, long nrows, int W, int K, void *workspace,
                      size_t workspace_bytes, float *g_mus, float *g_isigmas, voge_stream_t stream);

/*
 * Composite forward.  Replaces: VoGE/Aggregation.py:82-107 `aggregation`
 * (get_cross_activation :30-51 + assign2weight :54-79), without any [npix,K,K] temporary.
 *   w_m = exp(-occ * sum_k exp(-act_k) * (erf((len_m-len_k)*sqrt(dsd_k+1e-10)) + 1)/2)
 *         * exp(-act_m) / exp(-0.5);   valid_num = #(idx >= 0)
 * cnt: NULL, or [npix] int32 = the trace forward's out_cnt for the same lists (slots k >= cnt are
 * its sentinels): valid_num = cnt, idx may be NULL and is not read, slots beyond cnt are not
 * loaded at all and workgroups whose pixels are all empty only write zeros.
 * Alignment: with K % 4 == 0 the kernel moves 16 bytes per access and act, len, dsd and weight must start on a 16-byte
 * boundary; with K % 4 == 2, 8 bytes and an 8-byte boundary; odd K goes slot by slot and takes any float pointer.  A pointer
 * off its boundary is refused with VOGE_ERR_BAD_ARG before anything is launched (row r of a [rows, K] array keeps the boundary
 * of row 0).
 */
int voge_composite_fwd(const int32_t *idx, const int32_t *cnt, const float *act, const float *len,
                       const float *dsd, float occ, long npix, int K, float *weight,
                       int64_t *valid_num, voge_stream_t stream);

/*
 * Composite backward (the reference relies on autograd through Aggregation.py:49,70,74,77).
 * g_weight [npix,K] -> g_act, g_len, g_dsd [npix,K] (fully written).  weight = the forward's
 * output for the same inputs (saves the backward recomputing it); NULL -> recomputed.
 * cnt (NULL allowed) = the trace forward's out_cnt, as in voge_composite_fwd: slots k >= cnt are
 * the trace's sentinels and are not loaded; workgroups whose pixels are all empty write zeros.
 * Alignment: with weight given and K even the kernel moves 8 bytes per access: act, len, dsd, weight, g_weight, g_act, g_len
 * and g_dsd must start on an 8-byte boundary, else VOGE_ERR_BAD_ARG and nothing is launched.  Odd K, and weight == NULL
 * (one slot per lane), take any float pointer.
 */
int voge_composite_bwd(const float *act, const float *len, const float *dsd, const float *weight,
                       const int32_t *cnt, const float *g_weight, float occ, long npix, int K, float *g_act,
                       float *g_len, float *g_dsd, voge_stream_t stream);

/*
 * Attribute merge forward.  Replaces: VoGE/Aggregation.py:111-141 `merge_final`
 * (reached through Renderer.py:153 interpolate_attr).
 *   out[pix,c] = sum_{k < valid_num[pix]} attr[max(idx_k,0)... , c] * weight[pix,k]
 * attr [Nattr,C].  If fix_negative_idx != 0, idx is updated in place the way the reference
 * does (`vert_assign += (vert_assign < 0)`, Aggregation.py:131: -1 becomes 0).
 */
int voge_merge_fwd(const float *attr, int32_t *idx, const float *weight,
                   const int64_t *valid_num, long npix, int K, int C, long Nattr,
                   int fix_negative_idx, float *out, voge_stream_t stream);

/*
 * Attribute merge backward (autograd of merge_final): g_out [nrows*W,C] ->
 * g_attr [Nattr,C] (zero-filled here, then scatter-added) and g_weight [nrows*W,K].
 * The pixel grid is nrows rows of W pixels (any factorisation of the pixel count is valid;
 * the true image width gives the best locality).
 * Either output pointer may be NULL to skip it.
 */
int voge_merge_bwd(const float *attr, const int32_t *idx, const float *weight,
                   const int64_t *valid_num, const float *g_out, long nrows, int W, int K,
                   int C, long Nattr, float *g_attr, float *g_weight, voge_stream_t stream);

/*
 * Background blend forward.  Replaces: VoGE/Renderer.py:157-171
 * (get_silhouette + to_colored_background):
 *   sil = min(sum_k w_k, 1); mask = thr > 0 ? (sil > thr) : sil;
 *   out = min(rgb + (1 - mask) * bg, 1)
 * rgb,out [npix,C], bg [C], sil_out [npix] (may be NULL).
 */
int voge_blend_fwd(const float *rgb, const float *weight, const float *bg, float thr,
                   long npix, int K, int C, float *out, float *sil_out,
                   voge_stream_t stream);

/*
 * get_silhouette alone (VoGE/Renderer.py:157-159): sil [npix] = min(sum_k weight, 1); wsum [npix] (may be NULL) = the
 * unclamped sum, which the backward needs.  Backward: g_pix [npix] = g_sil * [wsum < 1] (1/2 at wsum == 1, as
 * torch.min splits ties) -- the gradient of EVERY slot of the pixel, so the [npix,K] gradient of the weights is this
 * array viewed with stride 0 along K (voge_fragment_bwd* reads it that way: gw_stride_pix = 1, gw_stride_k = 0).
 */
int voge_silhouette_fwd(const float *weight, long npix, int K, float *sil, float *wsum, voge_stream_t stream);
int voge_silhouette_bwd(const float *wsum, const float *g_sil, long npix, float *g_pix, voge_stream_t stream);

/*
 * Depth of composited fragments (EXTENSION: the reference has no depth output).  weight, len [npix][K], valid_num [npix]
 * (int64); with n = min(max(valid_num, 0), K), A = sum_{k<n} weight_k len_k and S = sum_{k<n} weight_k:
 *   depth [npix] = A / S where S > 0, else `background` (normalize != 0), or A (normalize == 0; background ignored);
 *   wsum [npix] = S.  Slots k >= n never contribute.  The sums use a fixed association: the same bits on every run.
 * Replaces the torch expression (weight * len).sum(-1) / weight.sum(-1), which is wrong on empty slots (len = 1e10 there).
 * Backward: g_weight[k] = a len_k + b, g_len[k] = a weight_k for k < n and ZERO in the dead slots, with a = g_depth / S,
 * b = -a depth where S > 0 and a = b = 0 elsewhere (normalize), or a = g_depth, b = 0 (depth / wsum may then be NULL).
 * Replaces autograd's backward of that expression.  K <= VOGE_MAX_K.
 */
int voge_depth_fwd(const float *weight, const float *len, const int64_t *valid_num, long npix, int K, int normalize,
                   float background, float *depth, float *wsum, voge_stream_t stream);
int voge_depth_bwd(const float *weight, const float *len, const int64_t *valid_num, const float *depth,
                   const float *wsum, const float *g_depth, long npix, int K, int normalize, float *g_weight,
                   float *g_len, voge_stream_t stream);

/*
 * Depth-distortion regulariser of composited fragments (EXTENSION: the reference has none; the term of Mip-NeRF 360 and 2D
 * Gaussian splatting that pulls a ray's mass onto one surface).  weight, len [npix][K], valid_num [npix] (int64); over the
 * n = min(max(valid_num, 0), K) live slots of a pixel, with w = weight and t = len (the distance along the UNIT ray: no
 * near / far mapping),
 *   L = sum_i sum_j w_i w_j |t_i - t_j|;   dist [npix] = L (normalize == 0), or L / S^2 where S > 0 and 0 elsewhere
 *   (normalize != 0: the distortion of the weights rescaled to sum to 1);   wsum [npix] = S = sum_k w_k.
 * Slots k >= n never contribute.  Evaluated as a prefix scan: order the live slots by (t_k, k) -- ascending len, exact ties by
 * slot position --, let u_k = t_k - t_first (t_first the smallest live len: the recentring is part of the numerics, the fp32
 * closed form on t itself loses 2e-4 at t = 1000) and, over the slots before / after slot i in that order,
 * W<_i = sum w_j, X<_i = sum w_j u_j, W>_i, X>_i likewise:
 *   L = 2 sum_i w_i (u_i W<_i - X<_i),   dL/dw_i = 2 [u_i (W<_i - W>_i) - (X<_i - X>_i)],   dL/dt_i = 2 w_i (W<_i - W>_i).
 * At an exact tie this is the POSITIONAL subgradient -- the earlier slot counts as nearer: tied i before j get -2 w_i w_j and
 * +2 w_i w_j --, not torch's sign(0) = 0.  Fragments arrive in ascending (len, index) order, so the scan runs in slot order; a
 * pixel whose live len are not non-decreasing (edited fragments, find_farest_k) is walked pairwise in the same launch, with the
 * same definition.  The sums use a fixed association: the same bits on every run.
 * Replaces the torch expression (w[..., :, None] * w[..., None, :] * (t[..., :, None] - t[..., None, :]).abs()).sum((-1, -2))
 * on the live slots -- a [.., K, K] tensor -- or a sort + cumsum chain of about a dozen launches (Aggregation.distortion).
 * Backward: with a = g_dist / S^2, b = -2 g_dist dist / S where S > 0 and a = b = 0 elsewhere (normalize; dist and wsum are the
 * forward's), or a = g_dist, b = 0 (dist / wsum may then be NULL):  g_weight[k] = a dL/dw_k + b,  g_len[k] = a dL/dt_k for
 * k < n and ZERO in the dead slots: every element is written, no fill, no atomics; the scan is recomputed from weight and len.
 * Replaces autograd's backward of that expression.  K <= VOGE_MAX_K; npix == 0: success, nothing is launched.
 */
int voge_distortion_fwd(const float *weight, const float *len, const int64_t *valid_num, long npix, int K, int normalize,
                        float *dist, float *wsum, voge_stream_t stream);
int voge_distortion_bwd(const float *weight, const float *len, const int64_t *valid_num, const float *dist,
                        const float *wsum, const float *g_dist, long npix, int K, int normalize, float *g_weight,
                        float *g_len, voge_stream_t stream);

/*
 * View-dependent colours from spherical-harmonic coefficients (EXTENSION: the reference has no spherical-harmonic code).
 * sh [N][M][C] with M in {1, 4, 9, 16} (maximum degree L = sqrt(M) - 1) and C in 1..4; verts [N][3] (shared_verts != 0: one set
 * for every view) or [B][N][3]; centres [B][3], the camera centres.  For view b and Gaussian n, delta = v - c_b and
 * d = delta / |delta| (d = 0 where |delta|^2 <= 1e-20: only the constant term survives):
 *   pre = sum_{m < (degree+1)^2} Y_m(d) sh[n][m][:] + 0.5,   out [B*N][C], row b*N + n, = max(pre, 0) (clamp != 0) or pre,
 * with 0 <= degree <= L the ACTIVE degree and Y_m the orthonormal real SH in the order and with the signs of
 * voge_amd/Aggregation.py sh_colors (the convention trained Gaussian scenes store their coefficients in).  Replaces that torch
 * expression -- a normalise, up to 16 polynomials, a contraction, an offset and a clamp -- by one launch.
 * Backward: g_out [B*N][C] -> g_sh [N][M][C] (EVERY element written; zero above the active degree) and g_verts ([N][3] summed
 * over the views when shared_verts, else [B][N][3]), through d d / d v = (I - d d^T) / |delta|; zero where pre <= 0 under the clamp
 * and, for the vertices, where d = 0.  The direction and the clamp mask are recomputed from the inputs: nothing is saved by the
 * forward.  One thread owns a Gaussian and walks the views in order -- no atomics, the same bits on every run.  Replaces
 * autograd's backward of that expression.  No gradient for the centres.  B == 0 or N == 0: success, nothing is launched or
 * written.  Where M * C is a multiple of 4, sh and g_sh must be 16-byte aligned (VOGE_ERR_BAD_ARG otherwise).
 */
int voge_sh_colors_fwd(const float *sh, const float *verts, const float *centres, int B, int N, int M, int C, int degree,
                       int shared_verts, int clamp, float *out, voge_stream_t stream);
int voge_sh_colors_bwd(const float *sh, const float *verts, const float *centres, const float *g_out, int B, int N, int M, int C,
                       int degree, int shared_verts, int clamp, float *g_sh, float *g_verts, voge_stream_t stream);

/*
 * Per-view normals of oriented Gaussians (EXTENSION: the reference has neither oriented Gaussians nor normals).  scales [N][3] and
 * quats [N][4] (w, x, y, z; not necessarily unit) when shared_orient != 0 -- one set for every view -- or [B][N][3] / [B][N][4];
 * verts [N][3] (shared_verts != 0) or [B][N][3]; centres [B][3], the camera centres.  R = the rotation of q / |q|, the identity
 * for a quaternion whose squared norm as fp32 computes it is not a positive finite number (voge_frame_trace_fwd_ori's rule).
 * The oriented Gaussian S = R diag(s) R^T stands for a flat surface element; its normal is the thinnest axis, a COLUMN of R:
 *   k* = 0; for j = 1, 2 in that order: k* = j if s_j > s_k* (inverse_sigma == 0: A = 2 S, a larger s is a thinner extent) or
 *   s_j < s_k* (inverse_sigma != 0: A = R diag(2 / s) R^T) -- an exact tie keeps the lowest index, a NaN never wins, a NaN in
 *   s_0 stays chosen;   n0 = R[:][k*];
 *   for view b, delta = v - c_b and t = n0 . delta:   out [B*N][3], row b*N + n, = -n0 where t > 0 and n0 otherwise,
 * the side that faces the camera (n . delta <= 0); t == 0, delta == 0 and a NaN t keep n0.  Replaces
 * voge_amd/Aggregation.py gaussian_normals -- a normalise, the [16,9] product map, an argmax, a gather, a dot product per view
 * and a select -- by one launch.
 * Backward: g_out [B*N][3] -> g_quats ([N][4] summed over the views in a fixed order when shared_orient, else [B][N][4]), EVERY
 * element written: g_n0 = sum_b sign_b g_out[b*N + n] in fp64, through d R[:][k*] / d qh in fp64 and
 * g_q = (g_qh - qh (qh . g_qh)) / |q| -- orthogonal to q; zero for a quaternion without a usable norm.  The axis and the signs
 * are recomputed from the inputs (nothing is saved by the forward) and are constants of the gradient; scales, verts and centres
 * get none.  No atomics, the same bits on every run.  Replaces autograd's backward of that expression.  quats and g_quats are
 * read and written 16 bytes at a time where both start on a 16-byte boundary, element by element otherwise.  B == 0 or N == 0:
 * success, nothing is launched or written.  A negative size, a null pointer with work to do, or B * N * 3 beyond an int:
 * VOGE_ERR_BAD_ARG before any HIP call.
 */
int voge_gauss_normals_fwd(const float *scales, const float *quats, const float *verts, const float *centres, int B, int N,
                           int shared_orient, int shared_verts, int inverse_sigma, float *out, voge_stream_t stream);
int voge_gauss_normals_bwd(const float *scales, const float *quats, const float *verts, const float *centres, const float *g_out,
                           int B, int N, int shared_orient, int shared_verts, int inverse_sigma, float *g_quats,
                           voge_stream_t stream);

/*
 * Surface normals from a depth map (EXTENSION: the reference has neither depth nor normals).  depth [B][h][W] is the distance
 * along each pixel's unit ray (voge_depth_fwd, voge_frame_depth_fwd_iso); R [B][3][3], focal [B][2], pp [B][2] the cameras of
 * voge_rays_fwd (no T: the camera centre cancels in every difference); band row i is image row row0 + i.  The kernels make the
 * rays themselves.  With valid = isfinite(depth) && depth > 0 and P = depth * ray, a neighbour is usable if it lies inside the
 * band, is valid and (edge < 0: no test) |depth_nb - depth| <= edge * depth; D_x = P(j+1) - P(j-1), P(j+1) - P(j) or
 * P(j) - P(j-1) by which of the two are usable, D_y likewise along i; c = D_x x D_y and
 *   normals [B][h][W][3] = +-c / |c| with n . ray <= 0 (towards the camera) where the pixel is valid, both differences exist
 *   and 0 < |c|^2 < inf;  (0, 0, 0) everywhere else.   view_space != 0: n_world @ R_b (row vectors, X_view = X_world @ R + T).
 * Replaces voge_amd/Aggregation.py depth_normals on rays from voge_rays_fwd -- about 30 torch launches over [B,h,W,3]
 * temporaries -- by one launch.
 * Backward: g_normals [B][h][W][3] -> g_depth [B][h][W], EVERY element written (zero where the depth is not valid).  The
 * gradient flows through P, the cross product and the normalisation; the choice of stencil, the edge test and the sign are
 * constants.  A gather: pixel q's thread recomputes the stencils of the up to five outputs that read depth(q) and sums them in a
 * fixed order -- no atomics, the same bits on every run; nothing is saved by the forward.  Replaces autograd's backward of that
 * expression.  B, h or W == 0: success, nothing is launched or written.  row0 < 0, a NaN edge, B > 65535 or h > 262140:
 * VOGE_ERR_BAD_ARG.
 */
int voge_depth_normals_fwd(const float *depth, const float *R, const float *focal, const float *pp, int B, int row0, int h, int W,
                           float edge, int view_space, float *normals, voge_stream_t stream);
int voge_depth_normals_bwd(const float *depth, const float *R, const float *focal, const float *pp, const float *g_normals, int B,
                           int row0, int h, int W, float edge, int view_space, float *g_depth, voge_stream_t stream);

/*
 * Background blend backward: g_out [npix,C] -> g_rgb [npix,C] and the additive term
 * g_weight_add [npix,K] (d out / d weight through the silhouette; zero where thr > 0 or
 * where the silhouette is clamped).  Recomputes the clamps from rgb / weight / bg.
 */
int voge_blend_bwd(const float *rgb, const float *weight, const float *bg, float thr,
                   const float *g_out, long npix, int K, int C, float *g_rgb,
                   float *g_weight_add, voge_stream_t stream);

/*
 * Blend with a background that broadcasts to the image.  Replaces: VoGE/Renderer.py:165-171 (to_colored_background's
 * `torch.min(rgb + ones * (1 - masks) * background_color, ones)` under torch broadcasting) when background_color is an
 * image, a colour per view, a grey level or a tensor that requires grad; masks = get_silhouette (:157-159) is the input s.
 *   rgb, img [B,H,W,C] (any C >= 1), s [B,H,W]: m = min(s, 1) -- a weight sum or a silhouette; thr > 0: m = [m > thr];
 *   bg read at bg[b*sb + h*sh + w*sw + c*sc]: the element strides of bg.expand(B, H, W, C), 0 on broadcast dimensions;
 *   img = min(rgb + (1 - m) * bg, 1).
 */
int voge_blend_bg_fwd(const float *rgb, const float *s, const float *bg, long sb, long sh, long sw, long sc, float thr,
                      int B, int H, int W, int C, float *img, voge_stream_t stream);

/*
 * Its backward (autograd through Renderer.py:171).  g_img read at g_img[pix*gs_pix + c*gs_c] (0, 0: a broadcast scalar,
 * read in place).  With g = g_img * pass(x), x = rgb + (1 - m) bg, pass = 1 / 0.5 / 0 for x below / at / above 1 (torch.min):
 *   g_rgb [B,H,W,C] = g (NULL: not wanted);
 *   g_m [B,H,W] = -sum_c g * bg = d img / d m (NULL: not wanted; must be NULL when thr > 0); the caller's min(sum w, 1)
 *     applies its own pass(sum w) -- get_silhouette's backward;
 *   g_bg = g * (1 - m) summed over the broadcast dimensions (NULL: not wanted), written at g_bg[b*gb + h*gh + w*gw + c*gc]
 *     with 0 on the dimensions where the background broadcasts; gc == 0 sums the channels in the lane:
 *     - no two pixels on one cell (gb, gh, gw non-zero or their dimension 1): plain stores;
 *     - one cell per view or one overall (gh, gw zero): per-workgroup partials in `workspace`
 *       (voge_blend_bg_bwd_workspace_bytes(B, H, W, C) bytes, owned by the caller), added up by a second pass in a fixed
 *       order: bitwise the same on every run;
 *     - anything else: VOGE_ERR_BAD_ARG -- hand in a dense [B,H,W,C] (or [B,H,W,1]) gradient and sum it down.
 * No atomics; nothing to zero beforehand.
 */
int voge_blend_bg_bwd(const float *rgb, const float *s, const float *bg, long sb, long sh, long sw, long sc, float thr,
                      const float *g_img, long gs_pix, long gs_c, int B, int H, int W, int C, float *g_rgb, float *g_m,
                      float *g_bg, long gb, long gh, long gw, long gc, void *workspace, size_t workspace_bytes,
                      voge_stream_t stream);
/* Bytes of voge_blend_bg_bwd's workspace: views x workgroups per view x C floats (0 for invalid sizes). */
size_t voge_blend_bg_bwd_workspace_bytes(int B, int H, int W, int C);

/*
 * Fused merge + silhouette + blend ("shade").  Replaces, in one pass: interpolate_attr ->
 * merge_final (Aggregation.py:111-141), get_silhouette (Renderer.py:157-159) and
 * to_colored_background (Renderer.py:162-171):
 *   rgb = sum_{k < valid_num} attr[idx_k] w_k ;  sil = min(sum_k w_k, 1) ;
 *   img = min(rgb + (1 - (thr > 0 ? sil > thr : sil)) * bg, 1)
 * Outputs (each may be NULL): out_rgb [npix,C] (needed again by voge_shade_bwd), out_img
 * [npix,C] (requires bg [C]), out_sil [npix], out_wsum [npix] (sum_k w_k before the clamp; saves
 * voge_shade_bwd a pass over weight).  fix_negative_idx as in voge_merge_fwd.
 */
int voge_shade_fwd(const float *attr, int32_t *idx, const float *weight, const int64_t *valid_num,
                   const float *bg, float thr, long npix, int K, int C, long Nattr,
                   int fix_negative_idx, float *out_rgb, float *out_img, float *out_sil,
                   float *out_wsum, voge_stream_t stream);

/*
 * Backward of voge_shade_fwd for C <= 4.  g_up [nrows*W,C] is the gradient of img (bg != NULL;
 * rgb = the forward's out_rgb) or of rgb itself (bg == NULL, rgb ignored).  Writes g_weight
 * [nrows*W,K] (may be NULL) and g_attr [Nattr,C] (zero-filled here then accumulated; may be NULL).
 * wsum [nrows*W] = the forward's out_wsum (unclamped sum_k w_k); NULL -> recomputed from weight.
 */
int voge_shade_bwd(const float *attr, const int32_t *idx, const float *weight,
                   const int64_t *valid_num, const float *rgb, const float *wsum, const float *bg,
                   float thr, const float *g_up, long nrows, int W, int K, int C, long Nattr,
                   float *g_attr, float *g_weight, voge_stream_t stream);

/*
 * Pixel-ray generation.  Replaces: the PyTorch3D call in VoGE/Renderer.py:124-130
 * (NDCMultinomialRaysampler(unit_directions=True) on screen-space PerspectiveCameras):
 *   d_view(i,j) = [(px-j-0.5)/fx, (py-i-0.5)/fy, 1],  rays = normalise(d_view @ R^-1),
 *   origin = -T @ R^-1          (row vectors, X_view = X_world @ R + T).
 * R [B,3,3], T [B,3], focal [B,2], pp [B,2] (principal point, pixels).  Renders image rows
 * row0 .. row0+h-1 (a pixel-row band): rays [B,h,W,3], origin [B,3].
 * cones: NULL, or voge_cones_floats(B,h,W) floats receiving the bounding cones (axis, cos, sin of the
 * half angle, flags) of every 32x32-pixel super-tile of the band, of its quads and of its 8x8 tiles:
 * what voge_trace_topk_fwd*'s `cones` argument takes.  They come out of the same arithmetic as the
 * rays, at no extra launch.
 */
int voge_rays_fwd(const float *R, const float *T, const float *focal, const float *pp, int B,
                  int row0, int h, int W, float *rays, float *origin, float *cones, voge_stream_t stream);

/*
 * The same for a STRIPED row set: output row i is image row row0 + (i / stripe_h) * pitch + i % stripe_h -- every
 * pitch-th stripe of stripe_h rows from row0 on, h rows in total (only the last stripe may be cut short by h).  What a
 * rank renders when one frame is dealt to the ranks of a node in interleaved stripes (voge_amd/distributed.py: a
 * contiguous band per rank leaves the centre band 4x as expensive as the rim bands).  The stacked rows are an image like
 * any other to every later stage (pixels are independent; the cones bound the rays actually present).  stripe_h >= h is
 * voge_rays_fwd.  voge_rays_striped_bwd is its backward (voge_rays_bwd's arguments plus the stripe geometry).
 * No counterpart in the reference (single device).
 */
int voge_rays_striped_fwd(const float *R, const float *T, const float *focal, const float *pp, int B,
                          int row0, int h, int stripe_h, int pitch, int W, float *rays, float *origin, float *cones,
                          voge_stream_t stream);
int voge_rays_striped_bwd(const float *R, const float *T, const float *focal, const float *pp,
                          const float *g_rays, const float *g_origin, int B, int row0, int h, int stripe_h, int pitch, int W,
                          float *scratch, float *g_R, float *g_T, float *g_focal, float *g_pp,
                          voge_stream_t stream);

/* The same cones from any rays [B,H,W,3] tensor (no counterpart in the reference: culling aid). */
size_t voge_cones_floats(int B, int H, int W);
int voge_ray_cones(const float *rays, int B, int H, int W, float *cones, voge_stream_t stream);

/*
 * The renderer's elementwise preamble for (N,3) / (N,3,3) sigmas in one launch each way.
 * Replaces: VoGE/Renderer.py:130-137 with VoGE/Aggregation.py:144-175 (centred = verts - origin[b];
 * isigma = 2 * expend_sigma(sigmas)) and their autograd.  kind 1: sigmas [.., N, 3] (A = 2 diag(s)); kind 2: [.., N, 3, 3]
 * (A = 2 S).  shared_verts / shared_sigmas: one [N, ...] set for every view, or [B, N, ...].  Writes mus [B*N,3],
 * isigmas [B*N,3,3]; the backward writes g_verts / g_sigmas in the parameters' own shapes (either may be NULL), a shared
 * set summing its views in a fixed order.
 */
int voge_general_preamble_fwd(const float *verts, const float *sigmas, const float *origin, int B, int N,
                              int shared_verts, int shared_sigmas, int kind, float *mus, float *isigmas,
                              voge_stream_t stream);
int voge_general_preamble_bwd(const float *g_mus, const float *g_isigmas, int B, int N, int shared_verts,
                              int shared_sigmas, int kind, float *g_verts, float *g_sigmas, voge_stream_t stream);

/*
 * Backward of voge_rays_fwd: g_rays [B,h,W,3] (may be NULL) and g_origin [B,3] (may be NULL) ->
 * g_R [B,3,3], g_T [B,3], g_focal [B,2], g_pp [B,2] (each may be NULL).  scratch: B*16 floats.
 */
int voge_rays_bwd(const float *R, const float *T, const float *focal, const float *pp,
                  const float *g_rays, const float *g_origin, int B, int row0, int h, int W,
                  float *scratch, float *g_R, float *g_T, float *g_focal, float *g_pp,
                  voge_stream_t stream);

/* ---- rows "next" (SURVEY.md §8f): dense ray API and the sampler's helpers ------------------ */

/*
 * Dense trace: every (ray n, Gaussian m) pair.  Replaces: VoGE._C.ray_trace_voge_ray
 * (voge_ray_tracing_ray.cu:114-143, :242-283).  mus [M,3], isigmas [M,3,3], rays [N,3] ->
 * len, act, dsd [N,M] (same arithmetic as the fine trace).
 */
int voge_ray_dense_fwd(const float *mus, const float *isigmas, const float *rays, int M, long N,
                       float *len, float *act, float *dsd, voge_stream_t stream);

/*
 * Its backward.  Replaces: VoGE._C.ray_trace_voge_ray_backward (voge_ray_tracing_ray.cu:147-188).
 * g_len, g_act, g_dsd [N,M] -> g_ray [N,3], g_mus [M,3], g_isg [M,3,3] (all written).
 */
int voge_ray_dense_bwd(const float *mus, const float *isigmas, const float *rays, const float *g_len,
                       const float *g_act, const float *g_dsd, int M, long N, float *g_ray,
                       float *g_mus, float *g_isg, voge_stream_t stream);

/*
 * Top-K over dense rows.  Replaces: VoGE._C.find_nearest_k (voge_ray_tracing_ray.cu:191-239,
 * :328-375): per ray the K entries with act < thr_act and the smallest (len, m), ascending;
 * unused slots: idx -1, len 1e10, act 0, dsd 0.
 */
int voge_find_nearest_k(const float *len_in, const float *act_in, const float *dsd_in, float thr_act,
                        int M, int K, long N, int32_t *idx, float *len, float *act, float *dsd,
                        voge_stream_t stream);

/*
 * Gradient of that selection (the reference scatters in Python, RayTracing.py:230-241):
 * gi_*[n, idx[n,k]] = g_*[n,k] for idx >= 0, zero elsewhere.  gi_* [N,M] are fully written.
 */
int voge_find_nearest_k_bwd(const int32_t *idx, const float *g_len, const float *g_act, const float *g_dsd,
                            int M, int K, long N, float *gi_len, float *gi_act, float *gi_dsd,
                            voge_stream_t stream);

/*
 * Per-Gaussian maximum weight.  Replaces: VoGE._C.scatter_max (sample_voge.cu:69-92,:135-170):
 * out[idx] = max over the n slots with that index of weight (weights are >= 0); out [Nv] zero-filled.
 * (sample_voge / sample_voge_backward, sample_voge.cu:35-66,:173-252, are the transpose of
 * merge_final: use voge_merge_bwd with g_out = [image | 1] for the forward and voge_merge_fwd /
 * voge_merge_bwd for the backward -- voge_amd/Sampler.py.)
 */
int voge_scatter_max(const float *weight, const int32_t *idx, long n, long Nv, float *out,
                     voge_stream_t stream);

/*
 * Exact k nearest neighbours of every point of a cloud among the cloud's points (EXTENSION.  The reference's only neighbour
 * search is the chunked cdist + topk over all N^2 pairs of naive_point_cloud_converter, Converters.py:98-122; 3D Gaussian
 * splatting ships a second module, simple-knn, for this step).
 * points [N,3]; d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j, ..., each operation one IEEE fp32 operation.  Row i of
 * idx / d2 [N,k] holds the k lexicographically smallest (d2, j) pairs, ascending, j == i left out unless include_self; a row
 * with fewer candidates is padded with idx -1, d2 +inf.  1 <= k <= 32.  The search runs over a uniform grid of gx x gy x gz cubic
 * cells of edge `cell` whose corner is (lo_x, lo_y, lo_z): each axis in [1, 1024], gx gy gz <= max(8 N, 2^15), and the grid must
 * cover the cloud's bounding box (g_a > extent_a / cell) -- the result does not depend on which such grid it is, nor on the run.
 * workspace: voge_knn_workspace_bytes(N, gx, gy, gz) bytes on a 16-byte boundary (0: N or the grid is out of range).
 * Six small launches and the search on `stream`.
 */
size_t voge_knn_workspace_bytes(long N, int gx, int gy, int gz);
int voge_knn_points(const float *points, long N, int k, int include_self, float lo_x, float lo_y, float lo_z, float cell,
                    int gx, int gy, int gz, int32_t *idx, float *d2, void *workspace, size_t workspace_bytes,
                    voge_stream_t stream);

/*
 * Local PCA frames of a point cloud (EXTENSION; feeds the oriented Gaussians from the neighbourhoods the converter of
 * Converters.py:98-122 only takes a mean distance from).  Row i of idx [N,k] (1 <= k <= 32) lists neighbours of point i; entries
 * outside [0, N) are skipped.  Mean and covariance C of the listed points in two passes, eigenvalues eig [N,3] ascending,
 * n = eigenvector of the smallest, t1 = of the largest, quats [N,4] = the rotation [t1, n x t1, n] as (w, x, y, z), unit, w >= 0.
 * n's sign: n . (toward - p_i) >= 0 with toward [3] (toward_per_point == 0) or [N,3]; toward == NULL: n's component of largest
 * magnitude is positive (the lowest index on a tie).  Fewer than three listed points, or eig1 <= 2^-18 eig2: the identity.
 */
int voge_knn_frames(const float *points, const int32_t *idx, long N, int k, const float *toward, int toward_per_point,
                    float *quats, float *eig, voge_stream_t stream);

/*
 * Mesh regularisers (EXTENSION: the reference imports mesh_edge_loss, mesh_laplacian_smoothing and mesh_normal_consistency from
 * PyTorch3D).  verts [B][V][3]; ONE topology for the B meshes, as int32 tables in the order of voge_amd/Losses.py MeshTopology:
 * edges [E][2] (i < j), nbr_off [V+1] / nbr [2E] (CSR adjacency), pairs [P][4] = (v0, v1, a, b) -- two faces on the edge
 * (v0, v1) with the opposite vertices a and b --, inc_off [V+1] / inc [4P] (per vertex the entries pair * 4 + role it has).
 * Every index must be in range: the tables are trusted (MeshTopology validates them on the host).  terms: bit 0 edge, bit 1
 * laplacian, bit 2 normal; a term that is off costs nothing, is 0 and takes no gradient.  out [3] = (edge, laplacian, normal):
 *   edge      = (1 / BE) sum (|v_i - v_j| - target_length)^2            a zero length counts target_length^2, no gradient
 *   laplacian = (1 / BV) sum |L_i|, L_i = (1 / d_i) sum_j (v_j - v_i)   uniform weights; L_i == 0 or d_i == 0: no gradient
 *   normal    = (1 / BP) sum (1 - cos(n0, n1)), n0 = (v1 - v0) x (a - v0), n1 = -(v1 - v0) x (b - v0)
 *                                                                       a pair with a zero-area face counts 1, no gradient
 * and 0 where E, or P, is 0.  Replaces voge_amd/Aggregation.py mesh_edge_term / mesh_laplacian_term / mesh_normal_term (gathers,
 * an index_add_ with float atomics, norms, a cosine: dozens of launches) by two launches: one over the E + V + P items of every
 * mesh that leaves three partial sums a workgroup in `workspace` (>= voge_mesh_reg_workspace_bytes(B, V, E, P) bytes), and one
 * workgroup that adds them in fp64 in an order that depends on the shapes alone.  lap_dir [B][V][3] (written when the laplacian
 * is on) = L_i / (|L_i| d_i), saved for the backward.  The terms difference positions before anything else, so a translation
 * of the mesh changes nothing but the roundings of the inputs; the edge term is evaluated in fp32, the laplacian and the pairs
 * in fp64 from the fp32 positions (a sliver face or a small |L_i| would amplify the rounding of an fp32 difference).
 * Backward: g_verts [B][V][3], EVERY element written by one launch, one thread a vertex: a gather through nbr (edge terms and
 * -d_i dir_i + sum_j dir_j) and through inc (the pair's gradient recomputed for the vertex's role), sums in fp64.  g_edge, g_lap,
 * g_normal point at ONE float each on the device, the gradients of the three outputs (null: 0).  Neither way uses an atomic:
 * the same bits on every run.  B == 0 or V == 0: success, nothing is launched or written.  A negative size, a terms bit above 2,
 * a null pointer with work to do, an edges / pairs off its row's alignment (8 / 16 bytes), B * V * 3 beyond an int, E >= 2^30 or
 * P >= 2^29: VOGE_ERR_BAD_ARG; a workspace too small: VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
size_t voge_mesh_reg_workspace_bytes(int B, int V, int E, int P);
int voge_mesh_reg_fwd(const float *verts, const int32_t *edges, const int32_t *nbr_off, const int32_t *nbr, const int32_t *pairs,
                      int B, int V, int E, int P, int terms, float target_length, float *lap_dir, void *workspace,
                      size_t workspace_bytes, float *out, voge_stream_t stream);
int voge_mesh_reg_bwd(const float *verts, const int32_t *nbr_off, const int32_t *nbr, const int32_t *pairs, const int32_t *inc_off,
                      const int32_t *inc, const float *lap_dir, const float *g_edge, const float *g_lap, const float *g_normal,
                      int B, int V, int E, int P, int terms, float target_length, float *g_verts, voge_stream_t stream);

/*
 * The nearest point of a cloud for every query (EXTENSION.  Replaces the cdist + min over all Nq Np pairs that PyTorch3D's
 * chamfer_distance, which the reference's demo/ShapeFitting.py imports, stands for; voge_knn_points searches inside ONE cloud).
 * queries [Nq,3], points [Np,3]; d2(q, p) = (dx*dx + dy*dy) + dz*dz, each operation one IEEE fp32 operation.  idx [Nq] / d2 [Nq]:
 * the lexicographically smallest (d2, index) over the points -- an exact tie keeps the lower index.  route 0: chosen by Nq Np,
 * 1: brute force (the points tiled through LDS, one launch), 2: a uniform grid over the union of both clouds, chosen ON THE DEVICE
 * (bounding box, the grid rule of voge_knn_points' wrapper, both clouds binned, a ring search with knn's stopping rule at k = 1:
 * eleven small launches and the search); both return the same bits, and neither reads anything back on the host, so the call may
 * be captured into a graph.  cell_size > 0 asks the grid route for a cell of that edge (enlarged until the grid fits its caps),
 * 0: about 2 max(Nq, Np) cells.  workspace: voge_chamfer_workspace_bytes(Nq, Np) bytes on a 16-byte boundary (0: a size below 1
 * or above 2^28 - 1); its first 32 bytes hold the grid that ran (lo[3], cell, 1 / cell as floats, gx, gy, gz as ints) after a
 * grid-route call.  Non-finite coordinates: indices in range or -1, values out of contract.
 * Nq == 0: success, nothing is launched.  Np < 1, a negative or too large size, an unknown route, a cell_size that is negative or
 * not finite, a null pointer, a workspace that is null or off the 16-byte boundary: VOGE_ERR_BAD_ARG; a workspace too small:
 * VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
size_t voge_chamfer_workspace_bytes(long Nx, long Ny);
int voge_nearest_points(const float *queries, long Nq, const float *points, long Np, int route, float cell_size, int32_t *idx,
                        float *d2, void *workspace, size_t workspace_bytes, voge_stream_t stream);

/*
 * Chamfer distance between two clouds x [Nx,3] and y [Ny,3] (EXTENSION: the reference's demo/ShapeFitting.py imports
 * chamfer_distance from PyTorch3D).  Replaces voge_amd/Aggregation.py chamfer_term (rows of the Nx x Ny matrix in chunks):
 *   loss[0] = (1 / Nx) sum_i min_j d2(x_i, y_j) + (1 / Ny) sum_j min_i d2(y_j, x_i)
 * flags bit 0: the sums without their divisors ("sum"); bit 1: the first sum alone (single_directional; nn_y is not touched).
 * nn_x [Nx] / nn_y [Ny] int32: the nearest indices, the values of voge_nearest_points (route as there), saved for the backward;
 * meta [4] int32: meta[0] = s, the scale exponent of the backward's fixed-point sums, chosen on the device from the largest d2 and
 * max(Nx, Ny).  Every d2 is fp32; the sums are fp64 -- one partial per 1024 queries, added by ONE workgroup in an order that depends
 * on the shapes alone -- and the loss is rounded to fp32 once.  The same bits on every run; no host read-back: capturable.
 * Backward: g_x [Nx,3], g_y [Ny,3], EVERY element written, from g_loss (ONE float on the device):
 *   g_x[i] = g (2 / Nx) (x_i - y_nn(i)) + g (2 / Ny) sum_{j: nn(j) = i} (x_i - y_j), g_y likewise;
 * three launches: a zero fill of the [Nx + Ny][3] int64 accumulators in the workspace, a scatter that adds every fp32 difference,
 * scaled by 2^s and rounded to an integer, with 64-bit INTEGER atomics (exact: the sum does not depend on the order; a list of m
 * points is off by at most m 2^-s / 2 per component), and a finish that adds the gather term in fp64 and rounds once.  An index
 * outside its cloud is skipped.  No float atomics.  workspace: voge_chamfer_workspace_bytes(Nx, Ny) serves both calls.
 * Nx < 1 or Ny < 1, a size above 2^28 - 1, an unknown route or flag, a null pointer (nn_y may be null with flags bit 1), a workspace
 * that is null or off the 16-byte boundary: VOGE_ERR_BAD_ARG; a workspace too small: VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
int voge_chamfer_fwd(const float *x, long Nx, const float *y, long Ny, int route, int flags, float *loss, int32_t *nn_x,
                     int32_t *nn_y, int32_t *meta, void *workspace, size_t workspace_bytes, voge_stream_t stream);
int voge_chamfer_bwd(const float *x, long Nx, const float *y, long Ny, const int32_t *nn_x, const int32_t *nn_y,
                     const int32_t *meta, const float *g_loss, int flags, float *g_x, float *g_y, void *workspace,
                     size_t workspace_bytes, voge_stream_t stream);

/*
 * Points on the surface of a triangle mesh, chosen by area (EXTENSION: PyTorch3D's sample_points_from_meshes, what its shape
 * fitting tutorial -- the one the reference's demo/ShapeFitting.py was written from -- puts the chamfer term on).  Replaces
 * voge_amd/Aggregation.py mesh_surface_points (cross, norm, cumsum, searchsorted, gathers, lerps; a backward of three index_adds
 * with float atomics).  verts [V,3] fp32, faces [F,3] int32, u [S,3] fp32 (clamped to [0, 1 - 2^-24], a NaN taken as 0), one mesh:
 *   A2_f = |(b - a) x (c - a)| in fp32, operation by operation the definition's; cdf = the inclusive sum of A2 in fp64;
 *   face_idx[s] = the smallest f with cdf[f] > double(u_s0) cdf[F-1], strictly: a face of area 0 is never chosen;
 *   r = sqrt(u_s1), bary[s] = (1 - r, r (1 - u_s2), r u_s2), points[s] = a + (w1 (b - a) + w2 (c - a)), normals[s] = cr / A2.
 * Three launches: areas with a scan per 256 faces, one workgroup that scans the block totals, one sample per lane with a
 * two-level binary search whose trip counts are bounded by the table sizes.  The sums are made in an order fixed by the shapes
 * (the same bits on every run) and differ from the definition's by at most F 2^-52 of the total.  A total that is 0 or not finite
 * (a NaN vertex): every face_idx is -1 and points, normals, bary are 0; so is a sample whose face names a vertex outside [0, V).
 * normals may be null (not written); a2_out [F] (may be null) receives A2, for the tests.  Nothing is read back on the host.
 * Backward: g_verts [V,3], EVERY element written, from g_points [S,3] and g_normals [S,3] (either may be null: 0).  Four
 * launches: a zero fill of the int64 accumulators in the workspace, the largest |g| by an integer atomic max, a scatter that
 * adds round(w_r g 2^s) to the face's three vertices (w = (1 - w1 - w2, w1, w2) from bary) and round(g_n 2^s) to the face with
 * 64-bit INTEGER atomics -- s = 62 - ceil(log2 S) - e with 2^e > max |g|, chosen on the device; exact, so the order does not
 * matter and a list of m samples is off by at most m 2^-s / 2 per component --, and a finish, one thread a vertex, that adds in
 * fp64 the face-normal Jacobian of every corner of the vertex (corner_off [V+1] / corner [3F]: entries face * 3 + role, ascending;
 * needed with g_normals only) and rounds once.  A sample with face_idx outside [0, F) is skipped.  No float atomics.
 * workspace: voge_mesh_sample_workspace_bytes(V, F, S) bytes on a 16-byte boundary serves both calls (0: V or F below 1, S below
 * 0, a size above 2^28 - 1).  Such sizes, a null pointer with work to do, a workspace that is null or off the 16-byte boundary:
 * VOGE_ERR_BAD_ARG; a workspace too small: VOGE_ERR_WORKSPACE -- all before any HIP call.  S == 0: the forward launches nothing
 * (unless a2_out is given), the backward writes zeros.
 */
size_t voge_mesh_sample_workspace_bytes(long V, long F, long S);
int voge_mesh_sample_fwd(const float *verts, long V, const int32_t *faces, long F, const float *u, long S, float *points,
                         float *normals, int32_t *face_idx, float *bary, float *a2_out, void *workspace, size_t workspace_bytes,
                         voge_stream_t stream);
int voge_mesh_sample_bwd(const float *verts, long V, const int32_t *faces, long F, const int32_t *corner_off, const int32_t *corner,
                         const int32_t *face_idx, const float *bary, long S, const float *g_points, const float *g_normals,
                         float *g_verts, void *workspace, size_t workspace_bytes, voge_stream_t stream);

/*
 * The nearest triangle of a mesh for every point (EXTENSION: the search inside PyTorch3D's point_mesh_face_distance; what an
 * extracted mesh is scored with against ground-truth points).  Replaces the rows of the P x F matrix of voge_amd/Aggregation.py
 * point_triangle_closest.  points [P,3], verts [V,3] fp32, faces [F,3] int32, one mesh.  d2(p, T), every operation one IEEE fp32
 * operation: e0 = b - a, e1 = c - a, v = p - a first; the interior candidate (n = e0 x e1, w2 = ((e0 x v).n) / nn, w1 = ((v x e1).n) / nn,
 * w0 = (1 - w1) - w2, only if nn > 0 and all three >= 0) and the segments ab, bc, ca (t = clamp((p - s).e / e.e, 0, 1), t = 0 when
 * e.e = 0); the smallest |p - q|^2 wins, a tie keeps the earlier candidate.  A triangle without area is its three segments, an edge
 * without length a point; no area threshold.  The reciprocals are taken once per triangle: no division per pair.
 * face_idx [P] / d2 [P]: the lexicographically smallest (d2, face) -- an exact tie keeps the lower index; bary [P,3]: the weights of
 * the closest point on (a, b, c), from one more evaluation of the winner's pair.  One launch: a point per lane, 64 a workgroup, the
 * triangles' records (16 floats, built by the workgroup while staging) tiled through LDS 256 at a time, the four waves take a quarter
 * of a tile each and meet in LDS.  A face that names a vertex outside [0, V) never wins.  Nothing is read back: capturable.
 * P == 0: success, nothing is launched.  V or F below 1, a size above 2^28 - 1, a null pointer: VOGE_ERR_BAD_ARG; P F above the pair
 * cap 2^38 (this search is a brute force; larger pairs go through voge_closest_faces_grid below): VOGE_ERR_K_TOO_LARGE --
 * all before any HIP call.
 */
int voge_closest_faces(const float *points, long P, const float *verts, long V, const int32_t *faces, long F, int32_t *face_idx,
                       float *d2, float *bary, voge_stream_t stream);

/*
 * Point-to-mesh distance (EXTENSION: PyTorch3D's point_mesh_face_distance).  Replaces voge_amd/Aggregation.py point_mesh_term
 * (the P x F matrix in chunks of points):
 *   loss[0] = (1 / P) sum_i min_f d2(p_i, T_f) + (1 / F) sum_f min_i d2(p_i, T_f),      d2 of voge_closest_faces
 * flags bit 0: the sums without their divisors ("sum"); bit 1: the first sum alone (single_directional; point_idx and bary_f are
 * not touched).  face_idx [P], bary_p [P,3]: the values of voge_closest_faces; point_idx [F], bary_f [F,3]: the nearest point of
 * every face (a triangle per lane with its record in registers, the points tiled through LDS 1024 at a time; a tie keeps the lower
 * index) and the weights of the closest point on it; meta [4] int32: meta[0] = s, the scale exponent of the backward's fixed-point
 * sums, chosen on the device from the largest d2 and ceil(log2(P + F)).  Every d2 is fp32; the sums are fp64 -- one partial per
 * 1024 items, added by ONE workgroup in an order that depends on the shapes alone -- and the loss is rounded to fp32 once.  Four
 * launches (two with bit 1 less one), the same bits on every run, no host read-back: capturable.
 * Backward: g_verts [V,3], g_points [P,3], EVERY element written, from g_loss (ONE float on the device); with r = p - q of a chosen
 * pair and w the weights of q (q minimises over the triangle: the weights' own derivative drops out),
 *   g_points[i] = g (2 / P) r_i + g (2 / F) sum_{f: nn(f) = i} r_f
 *   g_verts[v]  = - g (2 / P) sum_{i, k: faces[f_i][k] = v} w_ik r_i - g (2 / F) sum_{f, k: faces[f][k] = v} w_fk r_f;
 * three launches: a zero fill of the [V + P][3] int64 accumulators in the workspace, one scatter over the P + F items that adds
 * every term, scaled by 2^s and rounded to an integer, with 64-bit INTEGER atomics (exact: the sum does not depend on the order; a
 * list of m terms is off by at most m 2^-s / 2 per component; linear cost however the items crowd), and a finish that adds a point's
 * own term in fp64 and rounds once.  An index outside its range is skipped.  No float atomics.
 * workspace: voge_point_mesh_workspace_bytes(V, F, P) bytes on a 16-byte boundary serves both calls (0: a size below 1 or above
 * 2^28 - 1).  Such a size, an unknown flag, a null pointer (point_idx and bary_f may be null with flags bit 1), a workspace that is
 * null or off the 16-byte boundary: VOGE_ERR_BAD_ARG; P F above the pair cap 2^38: VOGE_ERR_K_TOO_LARGE (the backward with flags
 * bit 2 -- pairs of voge_point_mesh_fwd_grid -- has no pair cap); a workspace too small: VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
size_t voge_point_mesh_workspace_bytes(long V, long F, long P);
int voge_point_mesh_fwd(const float *verts, long V, const int32_t *faces, long F, const float *points, long P, int flags,
                        float *loss, int32_t *face_idx, float *bary_p, int32_t *point_idx, float *bary_f, int32_t *meta,
                        void *workspace, size_t workspace_bytes, voge_stream_t stream);
int voge_point_mesh_bwd(const float *verts, long V, const int32_t *faces, long F, const float *points, long P,
                        const int32_t *face_idx, const float *bary_p, const int32_t *point_idx, const float *bary_f,
                        const int32_t *meta, const float *g_loss, int flags, float *g_verts, float *g_points, void *workspace,
                        size_t workspace_bytes, voge_stream_t stream);

/*
 * The grid route of the two searches above (EXTENSION): the same outputs, element for element the BITS of voge_closest_faces /
 * voge_point_mesh_fwd on the same input -- the winner is the smallest key (d2 bits << 32 | index) over the candidates, and the
 * search only proves that it never skips an item that could hold it --, without the pair cap: P F may exceed 2^38.  A uniform
 * grid over the box of verts and points is chosen ON THE DEVICE (the rule of voge_nearest_points with n = max(F, P), and a cell
 * of at least the mean largest bounding-box extent of a face; cell_size > 0 asks for a cell of that size, 0 for the default);
 * every triangle is binned by the centre of its bounding box, the ones whose half-extent exceeds the cell go to a list every
 * point tests by brute force; a point walks rings of cells over the cell-ordered records, a triangle rings over the cell-ordered
 * points, and each stops by a proven bound (voge_amd/csrc/point_mesh_grid.h).  Nothing is read back, the workspace and every
 * launch are sized by (V, F, P) alone: capturable.  voge_point_mesh_fwd_grid's flags, outputs, loss and meta are
 * voge_point_mesh_fwd's; the backward is voge_point_mesh_bwd, whose flags bit 2 (4) says that the pairs came from this route and
 * lifts its pair cap.  A mesh of mostly large triangles is a brute force with extra steps, and one huge triangle idles its
 * wave's other lanes: correct and bounded, slow.
 * workspace: voge_point_mesh_grid_workspace_bytes(V, F, P) bytes on a 16-byte boundary (0: a size below 1 or above 2^28 - 1); it
 * also serves the backward.  voge_closest_faces_grid with P == 0: success, nothing is launched.  A size out of range, an unknown
 * flag, a cell_size that is negative or not finite, a null pointer, a workspace that is null or off the 16-byte boundary:
 * VOGE_ERR_BAD_ARG; a workspace too small: VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
size_t voge_point_mesh_grid_workspace_bytes(long V, long F, long P);
int voge_closest_faces_grid(const float *points, long P, const float *verts, long V, const int32_t *faces, long F, float cell_size,
                            int32_t *face_idx, float *d2, float *bary, void *workspace, size_t workspace_bytes,
                            voge_stream_t stream);
int voge_point_mesh_fwd_grid(const float *verts, long V, const int32_t *faces, long F, const float *points, long P, int flags,
                             float cell_size, float *loss, int32_t *face_idx, float *bary_p, int32_t *point_idx, float *bary_f,
                             int32_t *meta, void *workspace, size_t workspace_bytes, voge_stream_t stream);

/*
 * Depth maps fused into a truncated signed distance volume (EXTENSION: the reference has no mesh extraction; this and
 * voge_mtet_* are the last step of the 2D Gaussian splatting pipeline).  Replaces voge_amd/Aggregation.py tsdf_integrate, the
 * definition, operation by operation in fp32.  tsdf, weight [nz,ny,nx] fp32, updated IN PLACE; grid point (ix,iy,iz) sits at
 * lo + (ix hx, iy hy, iz hz).  depth [B,H,W]: the distance along the UNIT pixel ray from the camera centre (voge_depth_fwd's), not
 * view z; R [B,3,3], T [B,3], focal [B,2], pp [B,2]: the cameras of voge_rays_fwd (X_view = X_world @ R + T, pixel (i,j) looks along
 * ((px - j - 0.5)/fx, (py - i - 0.5)/fy, 1)); centre [B,3] = -T @ R^-1.  For a grid point x and the views b = 0 .. B-1 in that order:
 *   p = x @ R_b + T_b, skipped unless p_z > 0; j = floor(px - fx p_x / p_z), i = floor(py - fy p_y / p_z), skipped unless inside the
 *   image; d = depth[b,i,j], skipped unless finite and > 0; sdf = d - |x - centre_b|, skipped if sdf < -trunc;
 *   tsdf <- (tsdf w + min(1, sdf / trunc)) / (w + 1); w <- w + 1, or min(w + 1, max_weight) when max_weight > 0.
 * One launch, one grid point per thread with the loop over the views inside: 16 bytes a grid point per call, no atomics, the
 * same bits on every run, and one call with B views gives the bits of B calls with one view each.  Nothing is read back.
 * A dimension below 2, B < 0, H or W < 1, trunc or a voxel size that is not positive and finite, a lo that is not finite, a NaN
 * max_weight, a null pointer: VOGE_ERR_BAD_ARG; nx ny nz 7 >= 2^31 (the extraction's 32-bit indices): VOGE_ERR_K_TOO_LARGE -- all
 * before any HIP call.  B == 0: success, nothing is launched.
 */
int voge_tsdf_integrate(float *tsdf, float *weight, int nx, int ny, int nz, float lox, float loy, float loz, float hx, float hy,
                        float hz, const float *depth, int B, int H, int W, const float *R, const float *T, const float *centre,
                        const float *focal, const float *pp, float trunc, float max_weight, voge_stream_t stream);

/*
 * The level set of a scalar field on a regular grid as a triangle mesh: marching tetrahedra on Kuhn's six-tetrahedron split of
 * every cell (EXTENSION).  Replaces voge_amd/Aggregation.py marching_tets, the definition (its docstring has the tetrahedra,
 * the 16 cases and the winding: normals from inside to outside).  values [nz,ny,nx] fp32, weight the same or null; a grid point is
 * observed when its value is finite (and its weight > 0) and inside when value < level, strictly; linear index q = (iz ny + iy) nx + ix.
 * Three entries and one read-back between the second and the third:
 *   voge_mtet_count   a grid point per thread, 256 a workgroup: edge_mask [n] (bit d - 1: the edge of direction d = 1 .. 7 -- bit 0 = +x,
 *                     bit 1 = +y, bit 2 = +z -- from the point carries a vertex), face_count [n] (0 .. 12, the triangles of the cell the
 *                     point is the low corner of), vloc / floc [n] (the exclusive prefixes of both counts inside the workgroup) and
 *                     block_v / block_f [ceil(n / 256)] (the workgroups' totals): 6 bytes a grid point;
 *   voge_mtet_scan    ONE workgroup: block_v / block_f become their exclusive scans in place, 1024 entries a round, and
 *                     totals[0] = V, totals[1] = F.  The caller reads totals back to allocate verts [V,3] and faces [F,3]: the
 *                     one synchronisation of an extraction, which is a one-off step and not a step of an iteration;
 *   voge_mtet_emit    a grid point per thread: the vertex of edge (q, d) has the id block_v[q / 256] + vloc[q] +
 *                     popcount(edge_mask[q] & ((1 << (d - 1)) - 1)) and sits at p_a + t (p_b - p_a), t = (level - v_a) / (v_b - v_a),
 *                     p = lo + i h, a = q: vertices ascend by (q, d), faces by (cell, tetrahedron, triangle); int32 vertex ids.
 *                     values, weight, level and the grid must be those of the count.  Writes are guarded by V and F.
 * Integer sums only, no atomics: the same bits on every run.  A dimension below 2, a null pointer (weight may be null; verts
 * with V == 0 and faces with F == 0 too), a NaN level, a negative V or F, nblocks < 1, a voxel size that is not positive and finite:
 * VOGE_ERR_BAD_ARG; nx ny nz 7 >= 2^31, V or F above 2^31 - 1, nblocks above what such a grid has: VOGE_ERR_K_TOO_LARGE -- all before
 * any HIP call.  V == 0 and F == 0: emit launches nothing.
 */
int voge_mtet_count(const float *values, const float *weight, int nx, int ny, int nz, float level, uint8_t *edge_mask,
                    uint8_t *face_count, uint16_t *vloc, uint16_t *floc, uint32_t *block_v, uint32_t *block_f, voge_stream_t stream);
int voge_mtet_scan(uint32_t *block_v, uint32_t *block_f, long nblocks, long long *totals, voge_stream_t stream);
int voge_mtet_emit(const float *values, const float *weight, int nx, int ny, int nz, float level, float lox, float loy, float loz,
                   float hx, float hy, float hz, const uint8_t *edge_mask, const uint8_t *face_count, const uint16_t *vloc,
                   const uint16_t *floc, const uint32_t *block_v, const uint32_t *block_f, long V, long F, float *verts,
                   int32_t *faces, voge_stream_t stream);

/*
 * Attributes through the mesh extraction (EXTENSION): C floats a pixel -- a colour, a rendered normal, any row a renderer
 * interpolates -- fused beside the distance and carried to the vertices.  1 <= C <= 8, a compile-time number of the kernels; the
 * volume attr [nz,ny,nx,C] and the images attr_image [B,H,W,C] are fp32, channel last.  Both replace the attr= rules of
 * voge_amd/Aggregation.py tsdf_integrate and marching_tets, the definitions, operation by operation in fp32.
 *   voge_tsdf_integrate_attr   voge_tsdf_integrate with its arguments, tsdf and weight updated IN PLACE with that entry's bits, and
 *                     attr beside them: where a view updates a grid point (no other condition), for every channel and with w the
 *                     weight BEFORE its own update, attr <- (attr w + attr_image[b,i,j]) / (w + 1), (i,j) the depth's own nearest
 *                     pixel.  The pixel's values are not examined: a NaN poisons the grid points that read it.  One launch, the
 *                     loop over the views inside and the C running averages in registers: 16 + 8 C bytes a grid point per call.
 *   voge_mtet_attr    one launch after voge_mtet_emit, on the tables of that extraction (edge_mask, vloc, block_v after the scan) and
 *                     its values, level and grid: vert_attr [V,C] row block_v[q / 256] + vloc[q] + popcount(edge_mask[q] &
 *                     ((1 << (d - 1)) - 1)) = attr_a + t (attr_b - attr_a), t = (level - v_a) / (v_b - v_a), a = q.  Writes are guarded by V.
 * Gathers only, no atomics: the same bits on every run.  The errors of voge_tsdf_integrate and voge_mtet_emit, and C outside 1 .. 8 or
 * a null attr / attr_image / vert_attr (vert_attr with V == 0 may be null): VOGE_ERR_BAD_ARG -- all before any HIP call.  B == 0 and
 * V == 0: success, nothing is launched.
 */
int voge_tsdf_integrate_attr(float *tsdf, float *weight, float *attr, int C, int nx, int ny, int nz, float lox, float loy, float loz,
                             float hx, float hy, float hz, const float *depth, const float *attr_image, int B, int H, int W,
                             const float *R, const float *T, const float *centre, const float *focal, const float *pp, float trunc,
                             float max_weight, voge_stream_t stream);
int voge_mtet_attr(const float *values, int nx, int ny, int nz, float level, const float *attr, int C, const uint8_t *edge_mask,
                   const uint16_t *vloc, const uint32_t *block_v, long V, float *vert_attr, voge_stream_t stream);

/*
 * Connected components of a triangle mesh (EXTENSION: the clean-up the 2D Gaussian splatting pipeline runs between extracting a
 * mesh and scoring it).  Replaces voge_amd/Aggregation.py mesh_components, the definition: two vertices are connected when a chain
 * of faces links them (each face joins its three vertices), and a component's label is its smallest vertex index.  faces [F,3]
 * int32, V vertices.  A lock-free union-find over parent [V] (csrc/mesh_clean.hip's header has the invariant and the argument);
 * `stages` is a bit mask of the launches to make, 7 for a call:
 *   1  init     parent[x] = x, count[x] = 0, meta[0 .. 3] = 0;
 *   2  link     one face per thread;
 *   4  labels   vert_label [V] (a vertex no face names: its own index), face_label [F] = the label of the face's first vertex,
 *               count [V] = the faces of the component at its label and 0 elsewhere, meta[1] = the number of components.
 * meta [4] int32: meta[0] is an error word the caller reads back with meta[1] -- bit 0: a loop reached its trip cap or met a
 * pointer that does not lead downwards (never in a correct run), bit 1: a face names a vertex outside [0, V) (it joins nothing and
 * gets the label -1).  Integer atomics only: the same numbers on every run.  V or F negative or above 2^28 - 1, a null pointer
 * that a size above 0 needs, stages outside 1 .. 7: VOGE_ERR_BAD_ARG before any HIP call.
 */
int voge_mesh_components(const int32_t *faces, long F, long V, int32_t *parent, int32_t *vert_label, int32_t *face_label,
                         int32_t *count, int32_t *meta, int stages, voge_stream_t stream);

/*
 * The component filter (EXTENSION).  Replaces voge_amd/Aggregation.py mesh_clean, the definition, given its choice of components:
 * keep_root [V] bytes, non-zero at the labels that stay; face_label [F] from voge_mesh_components.  A face stays when its label
 * does, a vertex when a face that stays names it; both keep their order, and the faces are renumbered.
 *   voge_mesh_clean_scan   `stages` is a bit mask of its launches, 15 for a call: 1 the zero fill of vflag [V rounded up to 4]
 *                          and err [1]; 2 the kept faces mark vflag; 4 the exclusive prefixes of the flags inside blocks of 256 --
 *                          loc [V + F], the vertices' first -- and the blocks' totals -- blocks [ceil(V / 256) + ceil(F / 256)]; 8 ONE
 *                          workgroup turns the totals into their exclusive scans in place, 1024 entries a round, and writes
 *                          totals [3] = (V', F', error word: bit 1 when a label or an index lies outside [0, V)).  The caller
 *                          reads totals back to allocate the outputs: the one synchronisation of the filter;
 *   voge_mesh_clean_emit   one launch: verts_out [V',3] (the kept vertices' bits), faces_out [F',3], vert_index [V'] and face_index [F']
 *                          (the old indices).  Writes are guarded by V' and F'.
 * Integer sums only: the same bits on every run.  V or F below 1 or above 2^28 - 1, a null pointer (the outputs of a size 0 may
 * be null), V' or F' negative or above V or F, stages outside 1 .. 15: VOGE_ERR_BAD_ARG before any HIP call.
 */
int voge_mesh_clean_scan(const int32_t *faces, long F, long V, const int32_t *face_label, const uint8_t *keep_root, uint8_t *vflag,
                         uint16_t *loc, uint32_t *blocks, int32_t *err, long long *totals, int stages, voge_stream_t stream);
int voge_mesh_clean_emit(const float *verts, const int32_t *faces, long F, long V, const int32_t *face_label,
                         const uint8_t *keep_root, const uint8_t *vflag, const uint16_t *loc, const uint32_t *blocks, long Vk, long Fk,
                         float *verts_out, int32_t *faces_out, int32_t *vert_index, int32_t *face_index, voge_stream_t stream);

/*
 * Area-weighted vertex normals (EXTENSION: PyTorch3D's verts_normals_packed).  Replaces voge_amd/Aggregation.py
 * mesh_vertex_normals, the definition: normals [V,3] = the normalised sum of (b - a) x (c - a) over the corners that name the
 * vertex; (0, 0, 0) where the sum is zero, where a term is not finite and for a vertex no face names.  The cross product has the
 * bits of voge_mesh_sample_fwd's; the sum is made in fixed point with 64-bit integer atomics (csrc/mesh_clean.hip's header), so the
 * bits do not depend on the order of the faces.  `stages` is a bit mask of the launches, 15 for a call: 1 the zero fill of the
 * workspace, 2 the largest |component|, 4 the scatter, 8 the finish.  Nothing is read back.  A face that names a vertex outside
 * [0, V) is skipped.  V below 1, V or F above 2^28 - 1, a null pointer, a workspace that is null or off the 16-byte boundary, stages
 * outside 1 .. 15: VOGE_ERR_BAD_ARG; a workspace below voge_vertex_normals_workspace_bytes(V): VOGE_ERR_WORKSPACE -- all before any
 * HIP call.
 */
size_t voge_vertex_normals_workspace_bytes(long V);
int voge_vertex_normals(const float *verts, long V, const int32_t *faces, long F, float *normals, void *workspace,
                        size_t workspace_bytes, int stages, voge_stream_t stream);

/*
 * Mesh simplification (EXTENSION): vertex clustering on a uniform grid with mean or quadric placement.  Replaces
 * voge_amd/Aggregation.py mesh_simplify, the definition, whose docstring states the rule in five steps; csrc/mesh_simplify.hip's
 * header has the launches, the table's argument and the derived bounds.  verts [V,3] fp32, faces [F,3] int32, cells of
 * (hx, hy, hz).  Integer atomics only: the same bits on every run and under any permutation of the faces.
 *   voge_mesh_simplify_scan   steps 1 to 4 on a workspace of voge_mesh_simplify_workspace_bytes(V, F), which the other two entries
 *                             read.  `stages` is a bit mask, 255 for a call: 1 the fills and the bounding box, 2 the cells into
 *                             the table, 4 the labels, 8 the rotated triples, 16 the refill and the triples into the table, 32 the
 *                             face and label flags, 64 and 128 the two scan levels.  totals [3] = (V', F', error word), what the
 *                             caller reads back to allocate the outputs -- the one synchronisation.  Error word: bit 0 a probe
 *                             reached its cap (never in a correct run), bit 1 a face index outside [0, V), bit 2 a vertex that is
 *                             not finite, bit 3 more than 2^21 - 1 cells on an axis.
 *   voge_mesh_simplify_emit   step 5 and the outputs: verts_out [V',3], faces_out [F',3], vert_index [V] (the output row of every
 *                             input vertex, -1: dropped), face_index [F'] (the input faces that stay); acc: scratch of
 *                             voge_mesh_simplify_acc_bytes(V', quadric), 8-byte aligned, read again by voge_mesh_simplify_attr.
 *                             `stages`, 15 for a call: 1 the zero fill of acc, 2 indices and position sums, 4 the quadrics
 *                             (quadric != 0 only), 8 the finish.  V' and F' as read back, both >= 1 (an empty result needs no call).
 *   voge_mesh_simplify_attr   attr_out [V',C] channels c0 .. c0 + nc - 1 (nc <= 8) of attr [V,C]: the clusters' means, after emit,
 *                             on a scratch of voge_mesh_simplify_attr_workspace_bytes(V'), 16-byte aligned.  `stages`, 15 for a
 *                             call: 1 its zero fill, 2 the largest |value|, 4 the scatter, 8 the finish.
 * V or F below 1 or above 2^28 - 1, a cell size that is not positive and finite, a null pointer, a misaligned workspace, V' or F'
 * outside 1 .. V or F, stages outside their mask: VOGE_ERR_BAD_ARG; a workspace too small: VOGE_ERR_WORKSPACE -- all before any
 * HIP call.
 */
size_t voge_mesh_simplify_workspace_bytes(long V, long F);
size_t voge_mesh_simplify_acc_bytes(long Vk, int quadric);
size_t voge_mesh_simplify_attr_workspace_bytes(long Vk);
int voge_mesh_simplify_scan(const float *verts, long V, const int32_t *faces, long F, float hx, float hy, float hz, void *workspace,
                            size_t workspace_bytes, long long *totals, int stages, voge_stream_t stream);
int voge_mesh_simplify_emit(const float *verts, long V, const int32_t *faces, long F, float hx, float hy, float hz, int quadric,
                            void *workspace, size_t workspace_bytes, long Vk, long Fk, void *acc, size_t acc_bytes, float *verts_out,
                            int32_t *faces_out, int32_t *vert_index, int32_t *face_index, int stages, voge_stream_t stream);
int voge_mesh_simplify_attr(const float *attr, long V, long F, int C, int c0, int nc, const void *workspace, size_t workspace_bytes,
                            long Vk, const void *acc, int quadric, void *attr_workspace, size_t attr_workspace_bytes, float *attr_out,
                            int stages, voge_stream_t stream);

/*
 * Mesh depth maps (EXTENSION: PyTorch3D's rasterize_meshes, one face a pixel).  Replaces voge_amd/Aggregation.py mesh_rasterize,
 * the definition, whose docstring states the rule in seven steps; csrc/mesh_raster.hip's header has the launches, the box's pad
 * and the derived bounds.  verts [V,3] fp32, faces [F,3] int32, one mesh under B cameras R [B,3,3], T [B,3], focal [B,2], pp [B,2]
 * (those of voge_tsdf_integrate), images of H x W in tiles of 16 x 16.  Outputs pix_to_face [B,H,W] int32 (-1: nothing hit), bary
 * [B,H,W,3] and depth [B,H,W] fp32 (zeros there; depth is voge_depth_fwd's: along the unit pixel ray): the definition's fp32 bits,
 * the same on both routes.  The workspace of voge_mesh_raster_workspace_bytes(B, V, F, H, W) holds the records and the bins
 * route's tables (forward) or the fixed-point accumulators (backward); the backward reads nothing the forward left there.
 *   voge_mesh_raster_fwd   `stages` is a bit mask of launches: 1 the records [B F], 2 the bins route's tables (zero fill, count,
 *                          two scan levels; total [1] = the length of all the tiles' lists, what the caller reads back to
 *                          allocate list -- the one synchronisation of that route), 4 the fill of list [list_len] int32 (the
 *                          total as read back, at most 2^31 - 1), 8 the raster -- over the tiles' lists when stage 4 is in the
 *                          same call, over all F records otherwise.  Route "brute": one call with stages 9, two launches, nothing
 *                          read back.  Route "bins": stages 3, the read-back, stages 12 on the same workspace.
 *   voge_mesh_raster_bwd   g_verts [V,3] of g_depth [B,H,W] at the faces pix_to_face names: zero fill, the largest |term|, the
 *                          scatter with 64-bit integer atomics, the finish per vertex in fp64 (the rotation back through R^T,
 *                          rounded once).  No float atomics, nothing read back, the same bits on every run.
 * A face that names a vertex outside [0, V) hits nothing.  B below 1, V below 1 in voge_mesh_raster_bwd (there is no gradient to write: the
 * caller returns an empty one), V or F above 2^28 - 1, B H W above 2^31 - 1, B F or B V above
 * 2^36, a null pointer, a workspace that is null or off the 16-byte boundary, stages outside 1 .. 15: VOGE_ERR_BAD_ARG; a workspace
 * too small: VOGE_ERR_WORKSPACE -- all before any HIP call.
 */
size_t voge_mesh_raster_workspace_bytes(long B, long V, long F, long H, long W);
int voge_mesh_raster_fwd(const float *verts, long V, const int32_t *faces, long F, const float *R, const float *T, const float *focal,
                         const float *pp, long B, long H, long W, int cull_backfaces, int stages, int32_t *list, long list_len,
                         int32_t *pix_to_face, float *bary, float *depth, long long *total, void *workspace, size_t workspace_bytes,
                         voge_stream_t stream);
int voge_mesh_raster_bwd(const float *verts, long V, const int32_t *faces, long F, const float *R, const float *T, const float *focal,
                         const float *pp, long B, long H, long W, const int32_t *pix_to_face, const float *g_depth, float *g_verts,
                         void *workspace, size_t workspace_bytes, voge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VOGE_HIP_H */
