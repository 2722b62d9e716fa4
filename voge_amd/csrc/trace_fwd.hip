// Fine ray trace forward for gfx950: per-Gaussian prep, cone-culled LDS-tiled sweep with a
// per-lane top-K in LDS, and the explicit-candidate-list variant.
//
// Reference behaviour being reproduced: RayTraceFineVogeKernel
// (VoGE/csrc/ray_trace_voge/ray_trace_voge.cu:135-217) + the host wrapper (:219-280) and the
// "-1" candidate list of VoGE/RayTracing.py:22-26.  Design notes are in DESIGN.md §Kernels.
#include "voge_common.h"

namespace voge {

// ------------------------------------------------------------------------------------------
// prep: one thread per Gaussian.  Reads mu (12 B) + A (36 B), writes cull (16 B) + eval (48 B).
// The reach uses the smallest eigenvalue of sym(A) (closed form, fp64 -- P-sized work).
// ------------------------------------------------------------------------------------------
__device__ inline double lambda_min_sym3(double a00, double a11, double a22, double a01,
                                         double a02, double a12) {
  const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
  if (p1 == 0.0) return fmin(a00, fmin(a11, a22));
  const double q = (a00 + a11 + a22) / 3.0;
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
  const double p = sqrt(p2 / 6.0);
  const double ip = 1.0 / p;
  const double c00 = b00 * ip, c11 = b11 * ip, c22 = b22 * ip;
  const double c01 = a01 * ip, c02 = a02 * ip, c12 = a12 * ip;
  double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) +
                    c02 * (c01 * c12 - c11 * c02));
  r = fmin(1.0, fmax(-1.0, r));
  const double phi = acos(r) / 3.0;
  return q + 2.0 * p * cos(phi + 2.0943951023931953);
}

__device__ __forceinline__ void prep_one(const int g, const float *__restrict__ mus, const float *__restrict__ isg,
                                         const float *__restrict__ cam_fwd, const int N, const float thr_act,
                                         const int iso_in, float4 *__restrict__ cull, float4 *__restrict__ evr,
                                         float4 *__restrict__ ms, float4 *__restrict__ ell, const IsoView view,
                                         float4 *__restrict__ pk = nullptr /* [P][3] packed (mu, A): kept by the caller */,
                                         const CamView cam = no_camera()) {
  float mx, my, mz;
  const int src = view.shared ? g % N : g;
  float fwd[3] = {0.f, 0.f, 0.f};
  bool has_fwd = false;
  if (cam.R != nullptr) {      // (round 6) centre and view axis from the camera, as rays_fwd_kernel / _view_axis make them
    const int b = g / N;
    const CamK ck = cam_load(cam, b);
    float ox, oy, oz;
    cam_origin(ck, cam.T + 3 * b, ox, oy, oz);
    mx = mus[3 * (size_t)src + 0] - ox; my = mus[3 * (size_t)src + 1] - oy; mz = mus[3 * (size_t)src + 2] - oz;
    if (cam.origin_out != nullptr && g == b * N) { cam.origin_out[3 * b] = ox; cam.origin_out[3 * b + 1] = oy; cam.origin_out[3 * b + 2] = oz; }
    if (cam.behind) { const float *r = cam.R + 9 * b; fwd[0] = r[2]; fwd[1] = r[5]; fwd[2] = r[8]; has_fwd = true; }
  } else if (view.origin != nullptr) {   // centring of Renderer.py:130 done here: the same single fp32 subtraction
    const float *o = view.origin + 3 * (g / N);
    mx = mus[3 * (size_t)src + 0] - o[0]; my = mus[3 * (size_t)src + 1] - o[1]; mz = mus[3 * (size_t)src + 2] - o[2];
  } else {
    mx = mus[3 * (size_t)src + 0]; my = mus[3 * (size_t)src + 1]; mz = mus[3 * (size_t)src + 2];
  }
  float A[9];
  if (iso_in) {   // isg holds one scalar per Gaussian: A = a I
    const float a = iso_view_a(isg[src], view.mode);
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = (i % 4 == 0) ? a : 0.0f;
  } else if (view.gen_kind == 1) {      // the user's per-axis sigmas: A = 2 diag(s) (general_preamble_fwd_kernel's operations)
    const float *sg = isg + 3 * (size_t)(view.sigma_shared ? g % N : g);
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = (i % 4 == 0) ? 2.0f * sg[i / 4] : 0.0f;
  } else if (view.gen_kind == 2) {      // the user's [3][3] sigmas: A = 2 S
    const float *sg = isg + 9 * (size_t)(view.sigma_shared ? g % N : g);
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = 2.0f * sg[i];
  } else if (view.gen_kind == 3) {      // the user's (scales, quaternion): A = R diag(d) R^T, six entries computed, mirrored
    const size_t so = view.sigma_shared ? g % N : g;
    const float *sg = isg + 3 * so;
    const float4 q = reinterpret_cast<const float4 *>(view.quats)[so];      // (w, x, y, z): one 16-byte load
    float Rm[9], qh[4], inv;
    quat_rotation<float>(quat_usable(q.x, q.y, q.z, q.w), q.x, q.y, q.z, q.w, Rm, qh, inv);
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = view.ori_mode == 2 ? 2.0f / sg[k] : 2.0f * sg[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = i; j < 3; ++j) {
        const float a = ((d[0] * Rm[3 * i]) * Rm[3 * j] + (d[1] * Rm[3 * i + 1]) * Rm[3 * j + 1]) + (d[2] * Rm[3 * i + 2]) * Rm[3 * j + 2];
        A[3 * i + j] = a; A[3 * j + i] = a;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = isg[9 * (size_t)g + i];
  }
  const EvalRec e = make_eval(mx, my, mz, A);
  if (pk != nullptr && view.gen_kind == 1) {      // per-axis sigmas: the compact (centred mu, a0, a1, a2) record, 32 bytes
    pk[2 * (size_t)g + 0] = make_float4(mx, my, mz, A[0]);
    pk[2 * (size_t)g + 1] = make_float4(A[4], A[8], 0.0f, 0.0f);
  } else if (pk != nullptr) {      // what the deferred composite and the fused backward gather (fragment_bwd.hip's record layout)
    pk[3 * (size_t)g + 0] = make_float4(mx, my, mz, A[0]);
    pk[3 * (size_t)g + 1] = make_float4(A[1], A[2], A[3], A[4]);
    pk[3 * (size_t)g + 2] = make_float4(A[5], A[6], A[7], A[8]);
  }

  const double lmin = lambda_min_sym3(A[0], A[4], A[8], 0.5 * ((double)A[1] + A[3]),
                                      0.5 * ((double)A[2] + A[6]), 0.5 * ((double)A[5] + A[7]));
  const double lmax_bound = fabs((double)A[0]) + fabs((double)A[4]) + fabs((double)A[8]) +
                            fabs((double)A[1] + A[3]) + fabs((double)A[2] + A[6]) + fabs((double)A[5] + A[7]);
  const double lsafe = lmin * (1.0 - 1e-6) - 1e-12 * lmax_bound;
  float reach = INFINITY;
  if (lsafe > 0.0 && lsafe < 1e300) {
    const double nb = sqrt((double)e.bx * e.bx + (double)e.by * e.by + (double)e.bz * e.bz);
    const double nk = sqrt((double)e.kx * e.kx + (double)e.ky * e.ky + (double)e.kz * e.kz);
    const double nm = sqrt((double)mx * mx + (double)my * my + (double)mz * mz);
    // act >= lmin*dist^2 - |len|*|k|, |len| <= |b|/lmin  ->  dist^2 <= (thr + |k||b|/lmin)/lmin
    const double thr2 = (double)thr_act + 1.000001 * nk * nb / lsafe;
    const double r = sqrt(fmax(thr2, 0.0) / lsafe) * (1.0 + 1e-5) + 1e-5 * nm + 1e-30;
    reach = (float)(r * (1.0 + 1e-6));
    if (!(reach >= 0.0f)) reach = INFINITY;  // NaN guard
    // Anisotropic Gaussians also get the ELLIPSOID every hit must touch: a ray with act < thr_act has
    // its peak point x = len d inside E = {x : (x-mu)^T S (x-mu) <= thr2}, S = sym(A) (same bound as
    // above, before lambda_min replaces S).  Record M = thr2 S^-1, so that the support function of E
    // is h(n) = sqrt(n^T M n); the bin kernels look for a plane that separates E from a ray cone.
    // The lowest mantissa bit of `reach` says whether the record exists (rounding reach UP is safe).
    uint32_t rb = __float_as_uint(reach);
    bool has_ell = false;
    if (!is_iso(e) && reach < 3e38f) {
      const double s00 = A[0], s11 = A[4], s22 = A[8], s01 = 0.5 * ((double)A[1] + A[3]),
                   s02 = 0.5 * ((double)A[2] + A[6]), s12 = 0.5 * ((double)A[5] + A[7]);
      const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
      const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
      const double det = s00 * c00 + s01 * c01 + s02 * c02;
      const double f = fmax(thr2, 0.0) * (1.0 + 1e-4) / det;
      const double m00 = c00 * f, m11 = c11 * f, m22 = c22 * f, m01 = c01 * f, m02 = c02 * f, m12 = c12 * f;
      const double msum = fabs(m00) + fabs(m11) + fabs(m22) + 2.0 * (fabs(m01) + fabs(m02) + fabs(m12));
      // a positive definite S has det > 0 and positive diagonal cofactors; anything else keeps the sphere only
      if (det > 0.0 && f > 0.0 && m00 > 0.0 && m11 > 0.0 && m22 > 0.0 && msum < 1e30) {
        ell[2 * (size_t)g + 0] = make_float4((float)m00, (float)m11, (float)m22, (float)m01);
        // .z: absolute slack for n^T M n evaluated in fp32 (|n| <= 1.001); .w: additive slack of h
        ell[2 * (size_t)g + 1] = make_float4((float)m02, (float)m12, (float)(8e-6 * msum) + 1e-30f,
                                             (float)(1e-5 * nm + 1e-5 * r) + 1e-30f);
        has_ell = true;
      }
    }
    rb = has_ell ? (rb | 1u) : ((rb + 1u) & ~1u);
    reach = __uint_as_float(rb);
  }
  if (cam_fwd != nullptr) {
    const float *f = cam_fwd + 3 * (g / N);
    if (fmaf(mz, f[2], fmaf(my, f[1], mx * f[0])) < 0.0f) reach = -1.0f;
  }
  if (has_fwd && fmaf(mz, fwd[2], fmaf(my, fwd[1], mx * fwd[0])) < 0.0f) reach = -1.0f;
  cull[g] = make_float4(mx, my, mz, reach);
  evr[3 * (size_t)g + 0] = make_float4(e.s00, e.s11, e.s22, e.s01);
  evr[3 * (size_t)g + 1] = make_float4(e.s02, e.s12, e.bx, e.by);
  evr[3 * (size_t)g + 2] = make_float4(e.bz, e.kx, e.ky, e.kz);
  // epilogue record: everything an isotropic Gaussian needs in one 16-byte gather; w = NaN sends
  // the reader to the full records
  ms[g] = make_float4(mx, my, mz, is_iso(e) ? e.s00 : __uint_as_float(0x7fc00000u));
}

__device__ __forceinline__ EvalRec unpack_eval(const float4 a, const float4 b, const float4 c) {
  EvalRec e;
  e.s00 = a.x; e.s11 = a.y; e.s22 = a.z; e.s01 = a.w;
  e.s02 = b.x; e.s12 = b.y; e.bx = b.z; e.by = b.w;
  e.bz = c.x; e.kx = c.y; e.ky = c.z; e.kz = c.w;
  return e;
}

// One thread per Gaussian: the general (3x3) entry point's records.  (The scalar-sigma entry points derive
// theirs inside binA.)
// Small sets (VOGE_SMALL_N Gaussians per batch element or fewer): no binA at all.  The prep pass marks every (super-tile,
// slice) segment as overflowed (count -1) and resets binB's pool counter, which is what binA does for a slice it could not
// hold -- binB then takes a quad's candidates straight from the per-Gaussian records (its tested fallback: N / 256 cone tests per
// thread and pass).  For a few thousand Gaussians that is cheaper than a launch whose workgroups are pure latency (binA: 8.4 us
// at cfg5's 2 562 Gaussians; profiles/r5_kernel_trace_cfg5_loop.txt).
__device__ __forceinline__ void small_set_marks(int *__restrict__ seg_count, const long n_seg, unsigned long long *__restrict__ pool_top) {
  if (seg_count == nullptr) return;
  const long t = ((long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
  const long nt = (long)gridDim.x * gridDim.y * blockDim.x;
  for (long i = t; i < n_seg; i += nt) seg_count[i] = -1;
  if (t == 0) *pool_top = 0ull;
}

__global__ void __launch_bounds__(256)
prep_kernel(const float *__restrict__ mus, const float *__restrict__ isg, const float *__restrict__ cam_fwd, const int N,
            const int P, const float thr_act, float4 *__restrict__ cull, float4 *__restrict__ evr,
            float4 *__restrict__ ms, float4 *__restrict__ ell, float4 *__restrict__ pk, const IsoView view, const CamView cam,
            int *__restrict__ seg_count = nullptr, const long n_seg = 0, unsigned long long *__restrict__ pool_top = nullptr) {
  small_set_marks(seg_count, n_seg, pool_top);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < P) prep_one(g, mus, isg, cam_fwd, N, thr_act, 0, cull, evr, ms, ell, view, pk, cam);
}

}  // namespace voge

#include "trace_bin.h"
#include "composite_core.h"

#ifndef VOGE_SMALL_N
#define VOGE_SMALL_N 4096      // Gaussians per batch element up to which binA is skipped (small_set_marks)
#endif
#ifndef VOGE_ISO_PREP_SPLIT
#define VOGE_ISO_PREP_SPLIT 131072      // Gaussians per batch element from which on the scalar-sigma records get their own pass
#endif

namespace voge {

// The scalar-sigma records as a pass of their own: binA_kernel<true> derives them inside every (region, slice) workgroup -- one
// launch less, and free while a slice is one round (cfg3: 3 Gaussians per thread).  At 200k Gaussians every thread derives 12
// records -- as the same slice's workgroup of every other region does -- and the kernel is VALU-bound on it (5 of a workgroup's
// 15.8 us, VOGE_HIP_LIB=bt.so tools/bin_times.py cfg4_200k_1024): from VOGE_ISO_PREP_SPLIT Gaussians on this pass runs first and
// binA reads the records (cfg4: entry 297 -> 287 us, renderer form 272 -> 257).  Same functions, same bits.
__global__ void __launch_bounds__(256)
iso_prep_kernel(const float *__restrict__ mus, const float *__restrict__ isg, const float *__restrict__ cam_fwd, const int N,
                const float thr_act, const IsoView view, float4 *__restrict__ cull, float4 *__restrict__ ms, const CamView cam,
                int *__restrict__ seg_count = nullptr, const long n_seg = 0, unsigned long long *__restrict__ pool_top = nullptr) {
  small_set_marks(seg_count, n_seg, pool_top);
  const int g = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (g >= N) return;
  CamK ck;
  if (cam.R != nullptr) ck = cam_load(cam, b);      // (uniform)
  const BinAView V = binA_view<true>(b, cam_fwd, view, cam, &ck);
  if (cam.R != nullptr && cam.origin_out != nullptr && g == 0) {
    cam.origin_out[3 * b] = V.ox; cam.origin_out[3 * b + 1] = V.oy; cam.origin_out[3 * b + 2] = V.oz;
  }
  const BinARaw raw = binA_fetch<true>(g, b, N, nullptr, mus, isg, view);
  float a;
  const float4 c = binA_derive<true>(raw, true, V, thr_act, view, a);
  cull[(size_t)b * N + g] = c;
  ms[(size_t)b * N + g] = make_float4(c.x, c.y, c.z, a);
}

#ifdef VOGE_SWEEP_TIMES      // timing builds only (tools/sweep_stats.py): sweep_iso_kernel's per-tile stamps, read by voge_debug_sweep_times
__device__ unsigned long long g_sweep_times[8192 * 8];   // per WG: start, after cones, fill sum, consume sum, loop end, end, evals, smid
#endif

}  // namespace voge
#include "sweep_iso.h"      // round 4's scalar-sigma sweep (sweep_iso_kernel)
namespace voge {

// ------------------------------------------------------------------------------------------
// explicit candidate lists (the reference's bin_points tensor): one ray per lane, each lane
// walks the list of the bin its pixel falls in.  Compatibility path, no culling.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
trace_list_fwd_kernel(const float *__restrict__ mus, const float *__restrict__ isg,
                      const float *__restrict__ rays, const int32_t *__restrict__ bins,
                      const int P, const int H, const int W, const int K, const int BH,
                      const int BW, const int M, const int bin_size, const float thr_act,
                      int32_t *__restrict__ out_idx, float *__restrict__ out_len,
                      float *__restrict__ out_act, float *__restrict__ out_dsd, int32_t *__restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint64_t *keys = reinterpret_cast<uint64_t *>(smem_raw);
  const int lane = threadIdx.x;
  const int tiles_x = (W + 7) / 8;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, b = blockIdx.y;
  const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
  if (px >= W || py >= H) return;  // no barriers below
  const size_t pix = ((size_t)b * H + py) * W + px;
  const float dx = rays[3 * pix + 0], dy = rays[3 * pix + 1], dz = rays[3 * pix + 2];
  const float qxx = dx * dx, qyy = dy * dy, qzz = dz * dz, qxy = dx * dy, qxz = dx * dz, qyz = dy * dz;
  const int by = min(py / bin_size, BH - 1), bx = min(px / bin_size, BW - 1);
  const int32_t *lst = bins + (((size_t)b * BH + by) * BW + bx) * M;
  uint64_t *mykeys = keys + lane;
  int cnt = 0;
  uint64_t worst = ~0ull, tail = 0ull;
  for (int m = 0; m < M; ++m) {
    const int p = lst[m];
    if (p < 0 || p >= P) continue;
    float A[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = isg[9 * (size_t)p + i];
    const float mx = mus[3 * (size_t)p], my = mus[3 * (size_t)p + 1], mz = mus[3 * (size_t)p + 2];
    const EvalRec e = make_eval(mx, my, mz, A);
    const PairOut o = pair_eval(mx, my, mz, e, dx, dy, dz, qxx, qyy, qzz, qxy, qxz, qyz);
    if (o.act < thr_act && o.len < VOGE_SENT_LEN) {
      const uint64_t key = ((uint64_t)f2ord(o.len) << 32) | (uint32_t)p;
      if (key < worst) topk_insert(mykeys, 64, K, cnt, worst, tail, key);
    }
  }
  for (int s = 0; s < K; ++s) {
    int32_t oi = -1;
    float ol = VOGE_SENT_LEN, oa = VOGE_SENT_ACT, od = 0.0f;
    if (s < cnt) {
      const uint64_t key = mykeys[(size_t)s * 64];
      oi = (int32_t)(uint32_t)key;
      float A[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) A[i] = isg[9 * (size_t)oi + i];
      const float mx = mus[3 * (size_t)oi], my = mus[3 * (size_t)oi + 1], mz = mus[3 * (size_t)oi + 2];
      const EvalRec e = make_eval(mx, my, mz, A);
      const PairOut o = pair_eval(mx, my, mz, e, dx, dy, dz, qxx, qyy, qzz, qxy, qxz, qyz);
      ol = ord2f((uint32_t)(key >> 32));
      oa = o.act;
      od = o.dsd;
    }
    out_idx[pix * K + s] = oi;
    out_len[pix * K + s] = ol;
    out_act[pix * K + s] = oa;
    out_dsd[pix * K + s] = od;
  }
  if (out_cnt != nullptr) out_cnt[pix] = cnt;
}

struct TraceWs {
  float4 *cull, *evr, *ms, *ell;     // per-Gaussian records
  ConeRec *cones;                     // per super-tile
  int *seg_count;                     // binA -> binB: per (super-tile, slice) segment
  int32_t *seg_id;
  int *q_count;                       // quad lists in memory: only the fallback of an overflowed tile list
  int32_t *q_id;
  float *q_lb;
  int *tl_count;                      // per sweep tile
  int32_t *tl_id;
  float *tl_lb;
  float4 *seg_rec;
  int2 *order;                        // launch order of the sweep: (tile, list length) by super-tile rank and slot
  unsigned long long *pool_top;       // binB's long path: lists of quads with more than kQCap candidates
  int32_t *pool_id;
  float *pool_lb;
  int *tl_off;                        // per sweep tile: start of its pooled list
  int pool_cap;
  int *seg_ext;                       // binA -> binB: extensions of segments with more than kSegCap entries
  int32_t *ext_id;
  int ext_arena;                      // ids per (region, slice) workgroup of binA
  int nstx, nsty, nst0x, nst0y, nbin;
};

// Entries of the list pool: a Gaussian sits in the list of every tile its (conservative) footprint touches -- a handful
// for the small footprints that make a quad overflow in the first place.
static size_t trace_pool_entries(const size_t P) {
  const size_t want = 32 * P;
  return want < ((size_t)1 << 20) ? ((size_t)1 << 20) : (want > ((size_t)1 << 30) ? ((size_t)1 << 30) : want);
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// The list pool's counters: one per chunk of the batch an entry point walks (chunk c uses slot min(c, kPoolSlots - 1)), in the
// LAST kPoolTail bytes of the scratch the caller handed over -- the same addresses whatever a chunk's view count, so that
// voge_trace_pool_usage finds every chunk's counter behind the call, and out of the way of a caller who lets later, smaller
// entry points reuse the buffer's head (voge_amd.ops._workspace does: at the head of the scratch the fused backward's
// records overwrote them).
constexpr int kPoolSlots = 64;
constexpr size_t kPoolTail = 512;
static unsigned long long *trace_pool_slots(void *workspace, const size_t workspace_bytes) {
  return reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(workspace) + ((workspace_bytes - kPoolTail) & ~(size_t)255));
}

static size_t trace_ws_layout(int B, int N, int H, int W, void *base, TraceWs *ws) {
  const size_t P = (size_t)B * N;
  const int nstx = (W + kST - 1) / kST, nsty = (H + kST - 1) / kST;
  const size_t nbin = (size_t)B * nstx * nsty;
  const size_t ntile = (size_t)B * ((W + 7) / 8) * ((H + 7) / 8);
  size_t off = 0;
  char *p = reinterpret_cast<char *>(base);
  auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += align256(bytes); return q; };
  char *c = take(P * 16), *e = take(P * 48), *m4 = take(P * 16), *el = take(P * 32), *cn = take(cone_records(1, nbin) * sizeof(ConeRec)),
       *sc = take(nbin * kParts * 4), *si = take(nbin * kParts * (size_t)kSegCap * 4), *bc = take(nbin * 4 * 4),
       *bi = take(nbin * 4 * kQCap * 4), *bl = take(nbin * 4 * kQCap * 4), *tc = take(ntile * 4),
       *ti = take(ntile * kTileCap * 4), *tl = take(ntile * kTileCap * 4), *sr = take(nbin * kParts * (size_t)kSegCap * 16),
       *cq = take(nbin * kTilesPerBin * 8 * 2);      // (second half: unused since the exact order sort went -- HISTORY.md, "Removed switches")
  const size_t npool = trace_pool_entries(P);
  char *pi = take(npool * 4), *pl = take(npool * 4), *to = take(ntile * 4);
  const int nst0x = (W + kST0 - 1) / kST0, nst0y = (H + kST0 - 1) / kST0;
  size_t arena = (size_t)kExtMul * slice_cap(N);
  // (seg_ext holds 32-bit offsets into ext_id: a batch so large that the extensions would pass 2^31 ids goes without them
  // -- such segments then count as overflowed and binB re-tests their slice, as before round 3)
  if ((size_t)B * nst0x * nst0y * kParts * arena > (size_t)0x7fffffff) arena = 0;
  char *se = take(nbin * kParts * kExtChunks * 4), *ei = take((size_t)B * nst0x * nst0y * kParts * arena * 4);
  if (ws) {
    ws->seg_ext = reinterpret_cast<int *>(se); ws->ext_id = reinterpret_cast<int32_t *>(ei); ws->ext_arena = (int)arena;
    ws->pool_top = nullptr /* (trace_pool_slots: the scratch's tail) */; ws->pool_id = reinterpret_cast<int32_t *>(pi);
    ws->pool_lb = reinterpret_cast<float *>(pl); ws->tl_off = reinterpret_cast<int *>(to);
    ws->pool_cap = (int)npool;
    ws->cull = reinterpret_cast<float4 *>(c); ws->evr = reinterpret_cast<float4 *>(e);
    ws->ms = reinterpret_cast<float4 *>(m4); ws->ell = reinterpret_cast<float4 *>(el);
    ws->cones = reinterpret_cast<ConeRec *>(cn);
    ws->seg_count = reinterpret_cast<int *>(sc); ws->seg_id = reinterpret_cast<int32_t *>(si);
    ws->q_count = reinterpret_cast<int *>(bc); ws->q_id = reinterpret_cast<int32_t *>(bi);
    ws->q_lb = reinterpret_cast<float *>(bl);
    ws->tl_count = reinterpret_cast<int *>(tc); ws->tl_id = reinterpret_cast<int32_t *>(ti);
    ws->tl_lb = reinterpret_cast<float *>(tl);
    ws->seg_rec = reinterpret_cast<float4 *>(sr); ws->order = reinterpret_cast<int2 *>(cq);
    ws->nstx = nstx; ws->nsty = nsty;
    ws->nst0x = (W + kST0 - 1) / kST0; ws->nst0y = (H + kST0 - 1) / kST0;
    ws->nbin = (int)nbin;
  }
  return off;
}

}  // namespace voge
#ifdef VOGE_AB
#include "sweep_r3.h"      // round 3's sweep and the switch to it: the A/B library's bit-for-bit oracle, never in the product
#else
namespace voge { constexpr bool ab_round3_selected() { return false; } }
#endif
namespace voge {

// binB + the sweep (one wave = one 8x8-pixel tile per workgroup)
template <bool ISO>
static int launch_trace(const TraceWs &ws, const ConeRec *cones, const float *rays, int B, int N, int H, int W, int K,
                        float thr_act, int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt, hipStream_t st,
                        const CamView &cam, const bool diag = false) {
  constexpr int T = 64;
  // (diag: every general form of the launch is a per-axis one -- the frame path's gen_kind 1 -- sweep_iso_kernel<2>)
  const int gen = ISO ? 0 : (diag ? 2 : 1);
  const auto sweep = ISO ? sweep_iso_kernel<0> : (diag ? sweep_iso_kernel<2> : sweep_iso_kernel<1>);
  // sweep_iso_kernel (sweep_iso.h: float-compare commits, 6-byte list entries) -- <0> for scalar sigmas (round 4), <1> / <2>
  // for the general forms (round 5)
  const bool v2 = !ab_round3_selected();      // (always true in the product library: sweep_r3.h)
  const size_t lds2 = sweep2_lds_bytes(K, gen);
  {
    static DynLdsCache cache2[2];      // (one per kernel of this instantiation)
    if (v2) {
      const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(sweep), lds2, cache2[diag ? 1 : 0]);
      if (rc) return rc;
    }
  }
  hipLaunchKernelGGL(binB_kernel<!ISO>, dim3(ws.nstx * ws.nsty * 4, B), dim3(kQT), 0, st, ws.cull, ws.ell, ws.seg_count, ws.seg_id, ws.seg_rec,
                     cones, N, H, W, ws.nstx, ws.nsty, ws.nbin, ws.q_count, ws.q_id, ws.q_lb, ws.tl_count, ws.tl_id, ws.tl_lb,
                     ws.order, ws.pool_top, ws.pool_cap, ws.pool_id, ws.pool_lb, ws.tl_off, ws.seg_ext, ws.ext_id, K,
                     (v2 && act == nullptr) ? nullptr : idx /* (sweep_iso_kernel writes the empty tiles itself) */, len, act, dsd, cnt,
                     nullptr, nullptr, cam);
  {
    int rc = launch_status();
    if (rc) return rc;
  }
  dim3 grid(ws.nbin * kTilesPerBin);     // one workgroup per tile slot of every super-tile (slots outside the image exit)
#ifdef VOGE_AB
  if (!v2) return launch_sweep_r3<ISO>(ws, rays, grid, N, H, W, K, thr_act, idx, len, act, dsd, cnt, st, cam);
#endif
  hipLaunchKernelGGL(sweep, grid, dim3(T), lds2, st, ws.cull, ws.ms, ws.evr, rays, ws.q_count, ws.q_id, ws.q_lb, ws.tl_id,
                     ws.tl_lb, ws.pool_id, ws.pool_lb, ws.tl_off, ws.order, ((W + 7) / 8) * ((H + 7) / 8), ws.nstx, ws.nstx * ws.nsty, N, H, W, K,
                     thr_act, idx, len, act, dsd, cnt, cam);
  return launch_status();
}

}  // namespace voge

using namespace voge;

#ifdef VOGE_SWEEP_TIMES
extern "C" int voge_debug_sweep_times(unsigned long long *out, int n_wg) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(voge::g_sweep_times), sizeof(unsigned long long) * 8 * (size_t)n_wg);
}
#endif

#ifdef VOGE_BIN_TIMES
extern "C" int voge_debug_bin_wave(unsigned long long *out, int n_wg) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(voge::g_bin_wave), sizeof(unsigned long long) * 64 * (size_t)n_wg);
}
extern "C" int voge_debug_bin_times(unsigned long long *out, int which, int n_wg) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(voge::g_bin_times), sizeof(unsigned long long) * 8 * (size_t)n_wg,
                                  sizeof(unsigned long long) * 8 * 1024 * (size_t)which);
}
#endif


// Round 5: the scratch is sized for a CHUNK of the batch, not for all of it (it used to be B x 165 MB at 512^2, B x 774 MB at
// 1024^2: 6.2 GB for eight 1024^2 views).  Views are independent in every stage, so the entry points walk a batch in
// chunks of as many views as the scratch they were given holds -- stream-ordered launches on the same buffers -- and the
// size asked for here is what the largest chunk under kTraceWsCap needs (never less than one view).  A caller that wants a
// big batch in ONE chunk passes more: any size >= this is accepted and used.
constexpr size_t kTraceWsCap = (size_t)1 << 30;
static size_t trace_ws_bytes(const int nb, const int N, const int H, const int W) {      // a chunk's arrays + the counters' tail
  return trace_ws_layout(nb, N, H, W, nullptr, nullptr) + 256 + kPoolTail;
}
static int trace_views_that_fit(const int B, const int N, const int H, const int W, const size_t bytes) {
  int nb = 1;      // (layout is monotone in the view count: the largest nb whose layout fits)
  for (int step = B; step >= 1; step >>= 1)
    while (nb + step <= B && trace_ws_bytes(nb + step, N, H, W) <= bytes) nb += step;
  return nb;
}
extern "C" size_t voge_trace_workspace_bytes(int B, int N, int H, int W) {
  if (B <= 0 || N < 0 || H <= 0 || W <= 0) return 0;
  return trace_ws_bytes(trace_views_that_fit(B, N, H, W, kTraceWsCap), N, H, W);
}

extern "C" int voge_trace_pool_usage(const void *workspace, size_t workspace_bytes, int B, int N, int H, int W, int *used,
                                     int *capacity) {
  if (!workspace || !used || !capacity || B <= 0 || N < 0 || H <= 0 || W <= 0) return VOGE_ERR_BAD_ARG;
  if (workspace_bytes < trace_ws_bytes(1, N, H, W)) return VOGE_ERR_WORKSPACE;
  // the chunks the entry point walked with THIS scratch (the same rule: trace_topk_fwd_impl), each with a counter of its own in
  // the scratch's tail; reported: the largest use of any chunk, against the smallest capacity
  const int per = trace_views_that_fit(B, N, H, W, workspace_bytes);
  const int nchunks = (B + per - 1) / per;
  unsigned long long tops[kPoolSlots];
  const hipError_t e = hipMemcpy(tops, trace_pool_slots(const_cast<void *>(workspace), workspace_bytes), sizeof(tops), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  unsigned long long top = 0ull;
  for (int c = 0; c < nchunks && c < kPoolSlots; ++c) top = tops[c] > top ? tops[c] : top;
  TraceWs ws;
  trace_ws_layout(per, N, H, W, const_cast<void *>(workspace), &ws);
  *capacity = ws.pool_cap;
  if (nchunks > 1 && B % per != 0) {      // (the last, shorter chunk: its pool is sized for its own Gaussians)
    trace_ws_layout(B % per, N, H, W, const_cast<void *>(workspace), &ws);
    *capacity = ws.pool_cap < *capacity ? ws.pool_cap : *capacity;
  }
  *used = top > 0x7fffffffull ? 0x7fffffff : (int)top;
  return 0;
}

extern "C" int voge_ray_cones(const float *rays, int B, int H, int W, float *cones, voge_stream_t stream);   // rays.hip
extern "C" int voge_composite_fwd_iso(const int32_t *idx, const int32_t *cnt, const float *len, const float *records,
                                      const float *rays, float occ, long npix, int K, float *weight, int64_t *valid_num,
                                      voge_stream_t stream);                                                     // composite.hip

// idx[i] += off where idx[i] >= 0 (a chunk's indices are local to its first view: see trace_topk_fwd_impl)
__global__ void __launch_bounds__(256) idx_rebase_kernel(int32_t *__restrict__ idx, const size_t n4, const int off) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    int4 v = reinterpret_cast<int4 *>(idx)[i];
    v.x = v.x >= 0 ? v.x + off : v.x; v.y = v.y >= 0 ? v.y + off : v.y; v.z = v.z >= 0 ? v.z + off : v.z; v.w = v.w >= 0 ? v.w + off : v.w;
    reinterpret_cast<int4 *>(idx)[i] = v;
  }
}
__global__ void __launch_bounds__(256) idx_rebase1_kernel(int32_t *__restrict__ idx, const size_t n, const int off) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int v = idx[i];
    if (v >= 0) idx[i] = v + off;
  }
}

static int trace_chunk_fwd(const int iso_in, const IsoView view, const float *mus, const float *isigmas, const float *rays,
                           const float *cam_fwd, const float *cones_in, int B, int N, int H, int W, int K,
                           float thr_act, void *workspace, int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                           voge_stream_t stream, float occ, float *weight, int64_t *valid_num, float *records, const CamView &cam,
                           unsigned long long *pool_top);

static int trace_topk_fwd_impl(const int iso_in, const IsoView view, const float *mus, const float *isigmas, const float *rays,
                               const float *cam_fwd, const float *cones_in, int B, int N, int H, int W, int K,
                               float thr_act, void *workspace, size_t workspace_bytes,
                               int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                               voge_stream_t stream, float occ = 1.0f, float *weight = nullptr, int64_t *valid_num = nullptr,
                               float *records = nullptr, const CamView cam = no_camera()) {
  if (B < 0 || N < 0 || H < 0 || W < 0 || K <= 0) return VOGE_ERR_BAD_ARG;
  if (K > VOGE_MAX_K) return VOGE_ERR_K_TOO_LARGE;
  if ((size_t)B * H * W == 0) return 0;  // numel == 0 early return (ray_trace_voge.cu:248-251)
  // (with a camera the kernels make the rays themselves; the bundle they leave in cam.rays_out is what a composite behind the
  //  sweep reads.  That form keeps no act / dsd: the sweep's epilogue would have to read the bundle back.)
  if (cam.R != nullptr) {
    if (rays || cones_in || cam_fwd || act || dsd || !cam.T || !cam.focal || !cam.pp || cam.stripe_h <= 0 || cam.pitch < 0 ||
        cam.h != H || cam.W != W || (weight != nullptr && !cam.rays_out))
      return VOGE_ERR_BAD_ARG;
  } else if (!rays) {
    return VOGE_ERR_BAD_ARG;
  }
  if (!idx || !len || !workspace || (act == nullptr) != (dsd == nullptr)) return VOGE_ERR_BAD_ARG;
  // act / dsd may be omitted by the scalar-sigma fragment entry points only (they are re-derived where needed)
  // (with weights: composited behind the sweep; without: records kept, the caller composites later)
  // (general forms: trace only, with the packed (mu, A) records kept for the deferred composite -- voge_trace_lean_fwd)
  if (act == nullptr && !((iso_in ? (weight != nullptr || records != nullptr) : (weight == nullptr && records != nullptr)) &&
                          cnt != nullptr && (long)B * N < (1l << 26)))
    return VOGE_ERR_BAD_ARG;
  if (N > 0 && (!mus || !isigmas)) return VOGE_ERR_BAD_ARG;
  // (one view's scratch is the least that works; voge_trace_workspace_bytes(B, ...) is what to allocate)
  if (workspace_bytes < trace_ws_bytes(1, N, H, W)) return VOGE_ERR_WORKSPACE;
  // the top-K lists of one 8x8 tile fit the CU's LDS at every K the check above lets through
  static_assert(sweep2_lds_bytes(VOGE_MAX_K, 0) <= 160 * 1024 && sweep2_lds_bytes(VOGE_MAX_K, 1) <= 160 * 1024 &&
                sweep2_lds_bytes(VOGE_MAX_K, 2) <= 160 * 1024, "sweep_iso_kernel's LDS at VOGE_MAX_K");
  // ---- the batch in chunks of as many views as the scratch holds (all of them, when it was sized for that): every array the
  // caller sees is offset to the chunk's first view, the chunk runs as a batch of its own, and the indices it wrote -- local
  // to that first view -- are moved up by b0 N afterwards (one pass over idx, chunks behind the first only)
  const int per = trace_views_that_fit(B, N, H, W, workspace_bytes);
  const size_t npv = (size_t)H * W;      // pixels per view
  const size_t nst = (size_t)((W + kST - 1) / kST) * ((H + kST - 1) / kST);
  const size_t stride_mu = view.shared ? 0 : (size_t)N * 3;
  const size_t stride_sg = iso_in ? (view.shared ? 0 : (size_t)N)
                                  : (view.gen_kind ? (view.sigma_shared ? 0 : (size_t)N * (view.gen_kind == 2 ? 9 : 3)) : (size_t)N * 9);
  for (int b0 = 0; b0 < B; b0 += per) {
    const int nb = (B - b0 < per) ? B - b0 : per;
    IsoView v = view;
    if (v.origin != nullptr) v.origin += 3 * (size_t)b0;
    if (v.quats != nullptr && !v.sigma_shared) v.quats += 4 * (size_t)b0 * N;
    auto at = [&](auto *p, const size_t per_view) { return p ? p + (size_t)b0 * per_view : p; };
    if (cam.R != nullptr) v.cam_origin = 1;
    CamView cv = cam;
    cv.R = at(cam.R, 9); cv.T = at(cam.T, 3); cv.focal = at(cam.focal, 2); cv.pp = at(cam.pp, 2);
    cv.origin_out = at(cam.origin_out, 3); cv.rays_out = at(cam.rays_out, npv * 3);
    const int rc = trace_chunk_fwd(iso_in, v, at(mus, stride_mu), at(isigmas, stride_sg), at(rays, npv * 3), at(cam_fwd, 3),
                                   at(cones_in, nst * kConeRecsPerST * (sizeof(ConeRec) / sizeof(float))), nb, N, H, W, K, thr_act, workspace,
                                   at(idx, npv * K), at(len, npv * K), at(act, npv * K), at(dsd, npv * K), at(cnt, npv), stream, occ,
                                   at(weight, npv * K), at(valid_num, npv), at(records, (size_t)N * (iso_in ? 4 : (view.gen_kind == 1 ? 8 : 12))), cv,
                                   trace_pool_slots(workspace, workspace_bytes) + ((b0 / per) < kPoolSlots ? (b0 / per) : kPoolSlots - 1));
    if (rc) return rc;
    if (b0 > 0 && N > 0) {
      const size_t n = (size_t)nb * npv * K;
      int32_t *ic = idx + (size_t)b0 * npv * K;
      if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(ic) & 15) == 0) {
        const size_t n4 = n >> 2;
        hipLaunchKernelGGL(idx_rebase_kernel, dim3((unsigned)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096)), dim3(256), 0,
                           (hipStream_t)stream, ic, n4, b0 * N);
      } else {
        hipLaunchKernelGGL(idx_rebase1_kernel, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0,
                           (hipStream_t)stream, ic, n, b0 * N);
      }
      const int rc2 = launch_status();
      if (rc2) return rc2;
    }
  }
  return 0;
}

static int trace_chunk_fwd(const int iso_in, const IsoView view, const float *mus, const float *isigmas, const float *rays,
                           const float *cam_fwd, const float *cones_in, int B, int N, int H, int W, int K,
                           float thr_act, void *workspace, int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                           voge_stream_t stream, float occ, float *weight, int64_t *valid_num, float *records, const CamView &cam,
                           unsigned long long *pool_top) {
  hipStream_t st = (hipStream_t)stream;
  const int P = B * N;
  TraceWs ws;
  trace_ws_layout(B, N, H, W, workspace, &ws);
  ws.pool_top = pool_top;      // (this chunk's own counter, in the scratch's tail: voge_trace_pool_usage)
  if (records != nullptr && iso_in) ws.ms = reinterpret_cast<float4 *>(records);      // the caller keeps the (centre, a) records (backward)
  // super-tile cones: the caller's (voge_rays_fwd makes them while it makes the rays), or one more launch here
  const ConeRec *cones = reinterpret_cast<const ConeRec *>(cones_in);
  if (cones == nullptr && cam.R == nullptr) {
    const int rc = voge_ray_cones(rays, B, H, W, reinterpret_cast<float *>(ws.cones), stream);
    if (rc) return rc;
    cones = ws.cones;
  }
  const dim3 gridA(ws.nst0x * ws.nst0y * kParts, B);
  // (the scan of tools/small_set_scan.py, profiles/r5_small_set_scan.txt: at 128^2 / 256^2 skipping binA pays up to ~4 096 Gaussians,
  //  at 512^2 -- four times the quads, each reading every record -- up to ~2 000)
  const bool small_set = N > 0 && N <= ((long)H * W <= 131072 ? VOGE_SMALL_N : VOGE_SMALL_N / 2);
  const long n_seg = (long)B * ws.nstx * ws.nsty * kParts;
  if (small_set && iso_in) {
    // a few thousand Gaussians: records + "every segment overflowed" marks, no binA (small_set_marks)
    hipLaunchKernelGGL(iso_prep_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, mus, isigmas, cam_fwd, N, thr_act, view, ws.cull, ws.ms,
                       cam, ws.seg_count, n_seg, ws.pool_top);
  } else if (small_set) {
    hipLaunchKernelGGL(prep_kernel, dim3((P + 255) / 256), dim3(256), 0, st, mus, isigmas, cam_fwd, N, P, thr_act, ws.cull,
                       ws.evr, ws.ms, ws.ell, reinterpret_cast<float4 *>(records), view, cam, ws.seg_count, n_seg, ws.pool_top);
  } else if (iso_in && N >= VOGE_ISO_PREP_SPLIT) {
    // scalar sigmas, slices of more than two rounds: the records in a pass of their own (iso_prep_kernel)
    hipLaunchKernelGGL(iso_prep_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, mus, isigmas, cam_fwd, N, thr_act, view, ws.cull, ws.ms, cam);
    hipLaunchKernelGGL(binA_kernel<false>, gridA, dim3(kBinThreads), 0, st, cones, ws.nstx, ws.nsty, ws.nst0x, mus, isigmas,
                       cam_fwd, N, thr_act, view, ws.cull, ws.ms, ws.seg_count, ws.seg_id, ws.seg_rec, ws.pool_top, ws.seg_ext, ws.ext_id, ws.ext_arena, cam);
  } else if (iso_in) {
    // scalar sigmas: binA derives the per-Gaussian records itself -- two launches in front of the sweep
    hipLaunchKernelGGL(binA_kernel<true>, gridA, dim3(kBinThreads), 0, st, cones, ws.nstx, ws.nsty, ws.nst0x, mus, isigmas,
                       cam_fwd, N, thr_act, view, ws.cull, ws.ms, ws.seg_count, ws.seg_id, ws.seg_rec, ws.pool_top, ws.seg_ext, ws.ext_id, ws.ext_arena, cam);
  } else {
    if (P > 0)
      hipLaunchKernelGGL(prep_kernel, dim3((P + 255) / 256), dim3(256), 0, st, mus, isigmas, cam_fwd, N, P, thr_act, ws.cull,
                         ws.evr, ws.ms, ws.ell, reinterpret_cast<float4 *>(records), view, cam);
    hipLaunchKernelGGL(binA_kernel<false>, gridA, dim3(kBinThreads), 0, st, cones, ws.nstx, ws.nsty, ws.nst0x, mus, isigmas,
                       cam_fwd, N, thr_act, view, ws.cull, ws.ms, ws.seg_count, ws.seg_id, ws.seg_rec, ws.pool_top, ws.seg_ext, ws.ext_id, ws.ext_arena, cam);
  }
  {
    int rc = launch_status();
    if (rc) return rc;
  }
  // One wave (an 8x8 pixel tile) per sweep workgroup.  Residency is set by the LDS top-K lists (~7 waves per CU at
  // K = 40), and independent single-wave workgroups measured 4-10 % faster than 16x8 / 16x16 tiles in round 1.
  // Fragments wanted as well (weight != NULL): the stand-alone composite kernel runs behind the sweep.  Compositing
  // inside the sweep's epilogue was built and measured (same bits; HISTORY.md §5, in round 3's sweep): the sweep holds ~1.5 waves per
  // SIMD (its top-K lists fill the LDS), so the composite's row walks run latency-bound there -- sweep 64 -> 142 us at
  // cfg3 against 52 us for the kernel it would replace, which does the same instructions at eight waves per SIMD and
  // reads its 126 MB mostly from the Infinity Cache.
  int rc;
  if (iso_in) rc = launch_trace<true>(ws, cones, rays, B, N, H, W, K, thr_act, idx, len, act, dsd, cnt, st, cam);
  else rc = launch_trace<false>(ws, cones, rays, B, N, H, W, K, thr_act, idx, len, act, dsd, cnt, st, cam, view.gen_kind == 1);
  if (rc || weight == nullptr) return rc;
  if (act == nullptr)
    return voge_composite_fwd_iso(idx, cnt, len, reinterpret_cast<const float *>(ws.ms), cam.R != nullptr ? cam.rays_out : rays, occ,
                                  (long)B * H * W, K, weight, valid_num, stream);
  return voge_composite_fwd(idx, cnt, act, len, dsd, occ, (long)B * H * W, K, weight, valid_num, stream);
}

extern "C" int voge_trace_topk_fwd(const float *mus, const float *isigmas, const float *rays,
                                   const float *cam_fwd, const float *cones, int B, int N, int H, int W, int K,
                                   float thr_act, void *workspace, size_t workspace_bytes,
                                   int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                                   voge_stream_t stream) {
  return trace_topk_fwd_impl(0, IsoView{nullptr, 0, 0}, mus, isigmas, rays, cam_fwd, cones, B, N, H, W, K, thr_act, workspace,
                             workspace_bytes, idx, len, act, dsd, cnt, stream);
}

extern "C" int voge_trace_topk_fwd_iso(const float *mus, const float *a, const float *rays,
                                       const float *cam_fwd, const float *cones, int B, int N, int H, int W, int K,
                                       float thr_act, void *workspace, size_t workspace_bytes,
                                       int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                                       voge_stream_t stream) {
  return trace_topk_fwd_impl(1, IsoView{nullptr, 0, 0}, mus, a, rays, cam_fwd, cones, B, N, H, W, K, thr_act, workspace,
                             workspace_bytes, idx, len, act, dsd, cnt, stream);
}

extern "C" int voge_trace_topk_list_fwd(const float *mus, const float *isigmas, const float *rays,
                                        const int32_t *bin_points, int B, int P, int H, int W, int K,
                                        int BH, int BW, int M, int bin_size, float thr_act,
                                        int32_t *idx, float *len, float *act, float *dsd, int32_t *cnt,
                                        voge_stream_t stream) {
  if (B < 0 || P < 0 || H < 0 || W < 0 || K <= 0 || BH <= 0 || BW <= 0 || M < 0 || bin_size <= 0)
    return VOGE_ERR_BAD_ARG;
  if (K > VOGE_MAX_K) return VOGE_ERR_K_TOO_LARGE;
  if ((size_t)B * H * W == 0) return 0;
  if (!rays || !idx || !len || !act || !dsd || (M > 0 && !bin_points)) return VOGE_ERR_BAD_ARG;
  if (P > 0 && (!mus || !isigmas)) return VOGE_ERR_BAD_ARG;
  const size_t lds = sizeof(uint64_t) * (size_t)K * 64;
  {
    static DynLdsCache cache;
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(trace_list_fwd_kernel), lds, cache);
    if (rc) return rc;
  }
  dim3 grid(((W + 7) / 8) * ((H + 7) / 8), B);
  hipLaunchKernelGGL(trace_list_fwd_kernel, grid, dim3(64), lds, (hipStream_t)stream, mus, isigmas, rays,
                     bin_points, P, H, W, K, BH, BW, M, bin_size, thr_act, idx, len, act, dsd, cnt);
  return launch_status();
}

extern "C" int voge_trace_topk_fwd_iso_view(const float *verts, const float *sigmas, const float *origin, int shared,
                                            int sigma_mode, const float *rays, const float *cam_fwd, const float *cones,
                                            int B, int N, int H, int W, int K, float thr_act, void *workspace,
                                            size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                                            int32_t *cnt, voge_stream_t stream) {
  if (sigma_mode < 0 || sigma_mode > 2) return VOGE_ERR_BAD_ARG;
  return trace_topk_fwd_impl(1, IsoView{origin, shared ? 1 : 0, sigma_mode}, verts, sigmas, rays, cam_fwd, cones, B, N, H, W, K,
                             thr_act, workspace, workspace_bytes, idx, len, act, dsd, cnt, stream);
}

// ---- the general trace alone (no act / dsd, no composite): index, len, hit counts, and the packed (mu, A) records
// [B*N][12] the deferred composite (voge_composite_fwd_rec / voge_composite_shade_fwd_rec) and the fused backward read ----
extern "C" int voge_trace_lean_fwd(const float *mus, const float *isigmas, const float *rays, const float *cam_fwd,
                                   const float *cones, int B, int N, int H, int W, int K, float thr_act, void *workspace,
                                   size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records,
                                   voge_stream_t stream) {
  if (!cnt || !records) return VOGE_ERR_BAD_ARG;
  return trace_topk_fwd_impl(0, IsoView{nullptr, 0, 0}, mus, isigmas, rays, cam_fwd, cones, B, N, H, W, K, thr_act, workspace,
                             workspace_bytes, idx, len, nullptr, nullptr, cnt, stream, 1.0f, nullptr, nullptr, records);
}

// ---- trace + composite in one call: fragments (weight, idx, valid_num, len) plus act / dsd / cnt for the backward ----
extern "C" int voge_fragments_fwd(const float *mus, const float *isigmas, const float *rays, const float *cam_fwd,
                                  const float *cones, int B, int N, int H, int W, int K, float thr_act, float occ,
                                  void *workspace, size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                                  int32_t *cnt, float *weight, int64_t *valid_num, voge_stream_t stream) {
  if (!weight || !valid_num || !cnt) return VOGE_ERR_BAD_ARG;
  return trace_topk_fwd_impl(0, IsoView{nullptr, 0, 0}, mus, isigmas, rays, cam_fwd, cones, B, N, H, W, K, thr_act, workspace,
                             workspace_bytes, idx, len, act, dsd, cnt, stream, occ, weight, valid_num);
}

extern "C" int voge_fragments_fwd_iso(const float *mus, const float *a, const float *rays, const float *cam_fwd,
                                      const float *cones, int B, int N, int H, int W, int K, float thr_act, float occ,
                                      void *workspace, size_t workspace_bytes, int32_t *idx, float *len, float *act,
                                      float *dsd, int32_t *cnt, float *weight, int64_t *valid_num, float *records,
                                      voge_stream_t stream) {
  if (!cnt || (weight == nullptr) != (valid_num == nullptr) || (!weight && (!records || act || dsd))) return VOGE_ERR_BAD_ARG;
  return trace_topk_fwd_impl(1, IsoView{nullptr, 0, 0}, mus, a, rays, cam_fwd, cones, B, N, H, W, K, thr_act, workspace,
                             workspace_bytes, idx, len, act, dsd, cnt, stream, occ, weight, valid_num, records);
}

extern "C" int voge_fragments_fwd_iso_view(const float *verts, const float *sigmas, const float *origin, int shared,
                                           int sigma_mode, const float *rays, const float *cam_fwd, const float *cones,
                                           int B, int N, int H, int W, int K, float thr_act, float occ, void *workspace,
                                           size_t workspace_bytes, int32_t *idx, float *len, float *act, float *dsd,
                                           int32_t *cnt, float *weight, int64_t *valid_num, float *records,
                                           voge_stream_t stream) {
  if (sigma_mode < 0 || sigma_mode > 2 || !cnt || (weight == nullptr) != (valid_num == nullptr) ||
      (!weight && (!records || act || dsd)))
    return VOGE_ERR_BAD_ARG;
  return trace_topk_fwd_impl(1, IsoView{origin, shared ? 1 : 0, sigma_mode}, verts, sigmas, rays, cam_fwd, cones, B, N, H, W, K,
                             thr_act, workspace, workspace_bytes, idx, len, act, dsd, cnt, stream, occ, weight, valid_num, records);
}

// ---- Round 6: the renderer's trace with the CAMERA as its input (GaussianRenderer.forward, Renderer.py:102-150, up to and
// including ray_tracing: the ray bundle of :124-128, the centring of :130, the sigma rule of :133-137, RayTracing.py:12-30 and
// ray_trace_voge.cu:135-217) as three launches -- binA, binB, sweep -- with no ray-generation launch in front: every kernel
// makes the rays, cones, camera centre and view axis it needs from (R, T, focal, principal point) with rays_fwd_kernel's own
// operations (voge_common.h: CamView).  Outputs: idx, len, cnt, records as voge_fragments_fwd_iso_view's trace-only form, plus
// the ray bundle `rays` [B,h,W,3] (written by the sweep: the composite and the backward read it) and `origin` [B,3].
// rows: the band is h stacked rows; stacked row i is image row row0 + (i / stripe_h) * pitch + i % stripe_h (a contiguous
// band: stripe_h >= h, pitch 0; a rank's interleaved stripes: voge_rays_striped_fwd's meaning).  behind != 0: the reference's
// "skip z < 0" candidate rule (rasterize_coarse.cu:35), the view axis being column 2 of R.
// Diagnostic (tests/test_gpu_bin_cones.py): the cones the frame path's bin kernels make from the camera, by the calls they make --
// binA's region (cam_rect_cone over kST0 pixels) and child cones (over kST), binB's quad and tile cones (cam_two_cones, one
// workgroup per quad and one wave per tile, as in binB_kernel).
namespace voge {
__global__ void __launch_bounds__(kQT)
camera_cones_kernel(const CamView cam, const int nstx, const int nsty, const int nst0x, const int nst0y,
                    ConeRec *__restrict__ hier /* [B][nst * kConeRecsPerST] */, ConeRec *__restrict__ regions /* [B][nst0] */) {
  const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.y;
  const int binl = blockIdx.x >> 2, qq = blockIdx.x & 3;
  const int stx = binl % nstx, sty = binl / nstx;
  const size_t nst = (size_t)nstx * nsty;
  const CamK ck = cam_load(cam, b);
  const int tx = stx * (kST / 8) + (qq & 1) * 2 + (wave & 1), ty = sty * (kST / 8) + (qq >> 1) * 2 + (wave >> 1);
  ConeRec tcr, qcr;
  cam_two_cones(ck, cam, tx * 8, ty * 8, 8, stx * kST + (qq & 1) * kQuad, sty * kST + (qq >> 1) * kQuad, kQuad, tcr, qcr);
  if ((tid & 63) == 0) hier[cone_tile_at(b, nst, binl, ((qq >> 1) * 2 + (wave >> 1)) * 4 + (qq & 1) * 2 + (wave & 1))] = tcr;
  if (tid == 0) hier[cone_quad_at(b, nst, binl, qq)] = qcr;
  if (tid == 0 && qq == 0) hier[cone_super_at(b, nst, binl)] = cam_rect_cone(ck, cam, stx * kST, stx * kST + kST - 1, sty * kST, sty * kST + kST - 1);
  if (tid == 0 && qq == 1 && binl < nst0x * nst0y) {
    const int rx = binl % nst0x, ry = binl / nst0x;
    regions[(size_t)b * nst0x * nst0y + binl] = cam_rect_cone(ck, cam, rx * kST0, rx * kST0 + kST0 - 1, ry * kST0, ry * kST0 + kST0 - 1);
  }
}
}  // namespace voge

extern "C" int voge_camera_cones(const float *R, const float *T, const float *focal, const float *pp, int row0, int stripe_h, int pitch,
                                 int B, int h, int W, float *hier, float *regions, voge_stream_t stream) {
  if (!R || !T || !focal || !pp || !hier || !regions || stripe_h <= 0 || pitch < 0 || B <= 0 || h <= 0 || W <= 0) return VOGE_ERR_BAD_ARG;
  const CamView cam{R, T, focal, pp, row0, stripe_h, pitch, h, W, 0, nullptr, nullptr};
  const int nstx = (W + kST - 1) / kST, nsty = (h + kST - 1) / kST, nst0x = (W + kST0 - 1) / kST0, nst0y = (h + kST0 - 1) / kST0;
  hipLaunchKernelGGL(camera_cones_kernel, dim3(nstx * nsty * 4, B), dim3(kQT), 0, (hipStream_t)stream, cam, nstx, nsty, nst0x, nst0y,
                     reinterpret_cast<ConeRec *>(hier), reinterpret_cast<ConeRec *>(regions));
  return launch_status();
}

extern "C" int voge_frame_trace_fwd_iso(const float *verts, const float *sigmas, int shared, int sigma_mode, const float *R,
                                        const float *T, const float *focal, const float *pp, int row0, int stripe_h, int pitch,
                                        int behind, int B, int N, int h, int W, int K, float thr_act, void *workspace,
                                        size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records,
                                        float *rays, float *origin, voge_stream_t stream) {
  if (sigma_mode < 0 || sigma_mode > 2 || !cnt || !records || !R || !T || !focal || !pp || stripe_h <= 0 || pitch < 0)
    return VOGE_ERR_BAD_ARG;      // (origin may be NULL: nobody on the frame's path reads it)
  if ((size_t)B * h * W > 0 && !rays) return VOGE_ERR_BAD_ARG;
  const CamView cam{R, T, focal, pp, row0, stripe_h, pitch, h, W, behind ? 1 : 0, origin, rays};
  return trace_topk_fwd_impl(1, IsoView{nullptr, shared ? 1 : 0, sigma_mode}, verts, sigmas, nullptr, nullptr, nullptr, B, N, h, W, K,
                             thr_act, workspace, workspace_bytes, idx, len, nullptr, nullptr, cnt, stream, 1.0f, nullptr, nullptr, records,
                             cam);
}

// ... and for (N,3) / (N,3,3) sigmas (Renderer.py:130-137 with Aggregation.py:144-175: centred = verts - origin[b], A = 2 *
// expend_sigma(sigmas); no inverse_sigma here): the general trace with the camera AND the user's own arrays as inputs -- the
// record pass does the centring and the expansion (general_preamble_fwd_kernel's operations: the same bits), so neither the ray
// launch nor the preamble launch stands in front of the frame.  kind 1: sigmas [N | B*N][3], kind 2: [N | B*N][3][3];
// shared_verts / shared_sigmas: one set seen by every view.  records: what the deferred composite and voge_frame_bwd_gen read --
// kind 2: the packed (centred mu, A) [B*N][12]; kind 1: the compact (centred mu, a0, a1, a2, 0, 0) [B*N][8].
extern "C" int voge_frame_trace_fwd_gen(const float *verts, const float *sigmas, int shared_verts, int shared_sigmas, int kind,
                                        const float *R, const float *T, const float *focal, const float *pp, int row0, int stripe_h,
                                        int pitch, int behind, int B, int N, int h, int W, int K, float thr_act, void *workspace,
                                        size_t workspace_bytes, int32_t *idx, float *len, int32_t *cnt, float *records, float *rays,
                                        float *origin, voge_stream_t stream) {
  if ((kind != 1 && kind != 2) || !cnt || !records || !R || !T || !focal || !pp || stripe_h <= 0 || pitch < 0) return VOGE_ERR_BAD_ARG;
  if ((size_t)B * h * W > 0 && !rays) return VOGE_ERR_BAD_ARG;
  const CamView cam{R, T, focal, pp, row0, stripe_h, pitch, h, W, behind ? 1 : 0, origin, rays};
  IsoView view{nullptr, shared_verts ? 1 : 0, 0};
  view.gen_kind = kind; view.sigma_shared = shared_sigmas ? 1 : 0;
  return trace_topk_fwd_impl(0, view, verts, sigmas, nullptr, nullptr, nullptr, B, N, h, W, K, thr_act, workspace, workspace_bytes, idx, len,
                             nullptr, nullptr, cnt, stream, 1.0f, nullptr, nullptr, records, cam);
}

// ... and for ORIENTED Gaussians: scales [N | B*N][3] and unit-or-not quaternions [N | B*N][4] (w, x, y, z; 16-byte aligned) in
// place of a [3][3] form -- what a caller of voge_frame_trace_fwd_gen(kind 2) composes in torch in front of it, S = R diag(s) R^T
// (Renderer.py:133-137 then doubles it, or inverts and doubles it: sigma_mode 1: d = 2 s, 2: d = 2 / s).  The record pass builds
// A = R diag(d) R^T itself (voge_common.h: quat_rotation), bitwise symmetric; records = kind 2's packed (centred mu, A) [B*N][12],
// so everything behind the record pass is kind 2's, unchanged.
extern "C" int voge_frame_trace_fwd_ori(const float *verts, const float *scales, const float *quats, int shared_verts,
                                        int shared_sigmas, int sigma_mode, const float *R, const float *T, const float *focal,
                                        const float *pp, int row0, int stripe_h, int pitch, int behind, int B, int N, int h, int W,
                                        int K, float thr_act, void *workspace, size_t workspace_bytes, int32_t *idx, float *len,
                                        int32_t *cnt, float *records, float *rays, float *origin, voge_stream_t stream) {
  if ((sigma_mode != 1 && sigma_mode != 2) || !cnt || !records || !R || !T || !focal || !pp || stripe_h <= 0 || pitch < 0) return VOGE_ERR_BAD_ARG;
  if ((size_t)B * h * W > 0 && !rays) return VOGE_ERR_BAD_ARG;
  if (N > 0 && (!quats || (reinterpret_cast<uintptr_t>(quats) & 15) != 0)) return VOGE_ERR_BAD_ARG;
  const CamView cam{R, T, focal, pp, row0, stripe_h, pitch, h, W, behind ? 1 : 0, origin, rays};
  IsoView view{nullptr, shared_verts ? 1 : 0, 0};
  view.gen_kind = 3; view.sigma_shared = shared_sigmas ? 1 : 0; view.quats = quats; view.ori_mode = sigma_mode;
  return trace_topk_fwd_impl(0, view, verts, scales, nullptr, nullptr, nullptr, B, N, h, W, K, thr_act, workspace, workspace_bytes, idx, len,
                             nullptr, nullptr, cnt, stream, 1.0f, nullptr, nullptr, records, cam);
}
