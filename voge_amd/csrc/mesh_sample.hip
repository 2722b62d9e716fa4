// Mesh surface sampling (EXTENSION: PyTorch3D's sample_points_from_meshes, what feeds a chamfer loss between two SURFACES; the
// torch form is a cross, a norm, a cumsum, a searchsorted, three gathers and lerps, and a backward of three index_adds with float
// atomics).  One mesh per call: verts [V,3] fp32, faces [F,3] int32, u [S,3] fp32 in [0,1).  Aggregation.mesh_surface_points is
// the definition.
//
// voge_mesh_sample_fwd, three launches.
//   (1) ms_area_scan_kernel, one face per thread, kMsBlock faces a workgroup: e1 = b - a, e2 = c - a, cr = e1 x e2 (every component
//       (p q) - (r s)), A2 = sqrt((crx^2 + cry^2) + crz^2), every operation one IEEE fp32 operation (-ffp-contract=off): the bits of
//       the definition.  The workgroup writes the fp64 inclusive scan of its own A2 (cdf_local [F]) and its total.
//   (2) ms_block_scan_kernel, ONE workgroup: the fp64 inclusive scan of the block totals (bincl [nb]; the last entry is the total).
//   (3) ms_sample_kernel, one sample per lane: t = double(u0) total; the smallest block b with bincl[b] > t, then the smallest face
//       of that block with cdf_local[f] > t - bincl[b - 1] -- two binary searches, no pass that adds the offsets to the faces --,
//       then r = sqrt(u1), w = (1 - r, r (1 - u2), r u2), p = a + (w1 e1 + w2 e2), n = cr / A2.
// Every scan is SEQUENTIAL inside a segment and composed as value = fl(offset_of_the_segment + prefix_inside_the_segment), the
// offsets being the same composition one level up (16 x 16 faces in (1); thread segments x 32 x 32 in (2)).  fl(x + a) >= x for
// a >= 0 and = x for a = 0, and the last value of a segment IS the next segment's offset, so every table is non-decreasing and a
// face of area 0 repeats its predecessor's value, whatever the roundings (a shuffle-tree scan has neither property).  A search for
// "the smallest index whose value is > t" therefore ends on a face with cdf[f] > t >= cdf[f - 1]: never a zero-area face.  The
// order of every addition is fixed by the shapes: the same bits on every run.  Against the definition's cumulative sum a value
// differs by at most F 2^-52 total (any order of F non-negative terms), so a sample may land on the neighbouring face only when
// t is that close to a boundary.  The rounding of t - bincl[b - 1] can push it to the block's total or beyond; it is then set to
// the double just below the total, which selects the block's last face of positive area.
// The searches are bounded by the table sizes (32 and 9 trips), not by the data: NaN vertices give NaN tables, every comparison
// is false, the search runs to the end and the sample is written as face -1 with zero outputs.  So is every sample when the total
// is 0 or not finite, when a face names a vertex outside [0, V), and u is clamped to [0, 1 - 2^-24] with a NaN taken as 0.
//
// voge_mesh_sample_bwd, four launches, no float atomics.  p = (1 - w1 - w2) a + w1 b + w2 c, so a sample adds w_r g_s to the three
// vertices of its face, and its normal's gradient to its face.  Lists can be as long as S (one face), so the sums are made in
// FIXED POINT (fixed_point.h: the head, the exponent rule and its bound) as chamfer.hip's are: the zero fill of the accumulators, ms_absmax_kernel (D = max |g| over g_points and g_normals
// by an integer atomic max on the bits of |g|: a maximum has no order), ms_scatter_kernel (s = 62 - L - e with 2^L >= S and
// 2^e > D chosen by every thread from D, clamped to +-1000; round(w_r g 2^s) added with 64-bit INTEGER atomics into acc_v [V][3],
// round(g_n 2^s) into acc_f [F][3]; |w_r| <= 1, so |sum| < 2^62 + S cannot overflow), and ms_finish_kernel, one thread a vertex:
// the accumulator as fp64, and -- with normals -- a walk over the vertex's corners (corner_off / corner, entries face * 3 + role,
// ascending) that adds the face-normal Jacobian of the face's summed G_f: n = cr / |cr|, dL/dcr = (G - n (n . G)) / A2,
// dL/de1 = e2 x dL/dcr, dL/de2 = dL/dcr x e1, a gets minus both; e1, e2 are exact fp64 differences of the fp32 positions and the
// whole term is fp64; A2 == 0 passes nothing.  One rounding to fp32, EVERY element of g_verts written.  Integer addition is exact,
// so the bits do not depend on the order of the atomics.  Error: with q = 2^-s <= 2^(L - 61) D a vertex that m samples touch is
// off by at most m q / 2 per component before the final rounding, a face's G_f by m_f q / 2; D non-finite gives s = 0 and values
// out of contract.  Cost: linear in S + V + F.
#include <math.h>

#include "voge_common.h"
#include "fixed_point.h"

namespace voge {

constexpr int kMsBlock = 256;           // faces of a scan block (= threads of launch 1); ops.MESH_SAMPLE_BLOCK
constexpr int kMsSeg = 16;              // kMsBlock = kMsSeg segments of kMsSeg faces
constexpr int kMsLdsBlocks = 2048;      // block offsets staged in LDS up to this many (16 KiB)
constexpr long kMsMax = 268435455l;     // V, F, S <= 2^28 - 1
static_assert(kMsSeg * kMsSeg == kMsBlock, "two levels of kMsSeg");

struct MsFace {
  float ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z, crx, cry, crz, A2;
};

// (the indices were checked by the caller)
__device__ __forceinline__ MsFace ms_face(const float *__restrict__ verts, const int ia, const int ib, const int ic) {
  MsFace f;
  const float *a = verts + 3 * (size_t)ia, *b = verts + 3 * (size_t)ib, *c = verts + 3 * (size_t)ic;
  f.ax = a[0]; f.ay = a[1]; f.az = a[2];
  f.e1x = b[0] - f.ax; f.e1y = b[1] - f.ay; f.e1z = b[2] - f.az;
  f.e2x = c[0] - f.ax; f.e2y = c[1] - f.ay; f.e2z = c[2] - f.az;
  f.crx = (f.e1y * f.e2z) - (f.e1z * f.e2y);
  f.cry = (f.e1z * f.e2x) - (f.e1x * f.e2z);
  f.crz = (f.e1x * f.e2y) - (f.e1y * f.e2x);
  f.A2 = sqrtf((f.crx * f.crx + f.cry * f.cry) + f.crz * f.crz);
  return f;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kMsBlock)
ms_area_scan_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                    double *__restrict__ cdf_local, double *__restrict__ btotal, float *__restrict__ a2_out) {
  __shared__ double val[kMsBlock];
  __shared__ double segoff[kMsSeg + 1];
  const int tid = threadIdx.x;
  const size_t f = (size_t)blockIdx.x * kMsBlock + tid;
  float A2 = 0.0f;
  if (f < (size_t)F) {
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (face_in_range(ia, ib, ic, V)) A2 = ms_face(verts, ia, ib, ic).A2;      // (a face off the table: area 0, never chosen)
    if (a2_out) a2_out[f] = A2;
  }
  val[tid] = (double)A2;
  __syncthreads();
  if (tid < kMsSeg) {      // the inclusive prefix inside segment tid, sequentially
    double run = 0.0;
    for (int k = 0; k < kMsSeg; ++k) {
      run += val[tid * kMsSeg + k];
      val[tid * kMsSeg + k] = run;
    }
  }
  __syncthreads();
  if (tid == 0) {          // the segments' offsets, sequentially
    double run = 0.0;
    for (int j = 0; j < kMsSeg; ++j) {
      segoff[j] = run;
      run += val[j * kMsSeg + kMsSeg - 1];
    }
    segoff[kMsSeg] = run;
    btotal[blockIdx.x] = run;      // == the value the last thread writes below
  }
  __syncthreads();
  if (f < (size_t)F) cdf_local[f] = segoff[tid / kMsSeg] + val[tid];
}

// ONE workgroup of 1024: thread j owns the entries [j len, j len + len) of btotal; threads are grouped by 32, groups by 32.
// bincl[i] = fl(goff[g] + fl(lpx[j] + lp_i)): lp_i the prefix inside the thread's segment, lpx[j] the prefix of the segment totals
// before j inside its group, goff[g] the prefix of the group totals -- each of them sequential (header).
__global__ void __launch_bounds__(1024)
ms_block_scan_kernel(const double *__restrict__ btotal, const int nb, double *__restrict__ bincl) {
  __shared__ double tot[1024];
  __shared__ double goff[33];
  const int j = threadIdx.x;
  const int len = (nb + 1023) / 1024;
  const long i0 = (long)j * len, i1 = i0 + len < (long)nb ? i0 + len : (long)nb;
  double run = 0.0;
  for (long i = i0; i < i1; ++i) run += btotal[i];
  tot[j] = run;
  __syncthreads();
  if (j < 32) {
    double r = 0.0;
    for (int k = 0; k < 32; ++k) {
      r += tot[j * 32 + k];
      tot[j * 32 + k] = r;
    }
  }
  __syncthreads();
  if (j == 0) {
    double r = 0.0;
    for (int g = 0; g < 32; ++g) {
      goff[g] = r;
      r += tot[g * 32 + 31];
    }
    goff[32] = r;
  }
  __syncthreads();
  const double lpx = (j & 31) ? tot[j - 1] : 0.0, go = goff[j >> 5];
  run = 0.0;
  for (long i = i0; i < i1; ++i) {
    run += btotal[i];
    bincl[i] = go + (lpx + run);
  }
}

// the smallest i in [0, n) with tab[i] > t, n when there is none (or when the table is not ordered: NaN); at most `trips` rounds
template <typename T>
__device__ __forceinline__ int ms_upper(const T *tab, const int n, const double t, const int trips) {
  int lo = 0, hi = n;
  for (int k = 0; k < trips && lo < hi; ++k) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tab[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo < hi ? n : lo;      // (the trip count covers every n the callers pass: lo == hi here)
}

__device__ __forceinline__ float ms_clamp_u(const float v) {
  return v != v ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f - 0x1p-24f);
}

__global__ void __launch_bounds__(256)
ms_sample_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                 const float *__restrict__ u, const int S, const double *__restrict__ cdf_local, const double *__restrict__ bincl,
                 const int nb, float *__restrict__ points, float *__restrict__ normals, int32_t *__restrict__ face_idx,
                 float *__restrict__ bary) {
  __shared__ double stage[kMsLdsBlocks];
  const bool staged = nb <= kMsLdsBlocks;
  if (staged) {
    for (int i = threadIdx.x; i < nb; i += 256) stage[i] = bincl[i];
    __syncthreads();
  }
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (size_t)S) return;      // (no barrier below)
  const float u0 = ms_clamp_u(u[3 * s]), u1 = ms_clamp_u(u[3 * s + 1]), u2 = ms_clamp_u(u[3 * s + 2]);
  const double total = staged ? stage[nb - 1] : bincl[nb - 1];
  int f = -1;
  if (total > 0.0 && total < (double)INFINITY) {
    const double t = (double)u0 * total;
    const int b = staged ? ms_upper(stage, nb, t, 32) : ms_upper(bincl, nb, t, 32);
    if (b >= 0 && b < nb) {
      const double excl = b ? (staged ? stage[b - 1] : bincl[b - 1]) : 0.0;
      const size_t base = (size_t)b * kMsBlock;
      const int n = (int)((size_t)F - base < (size_t)kMsBlock ? (size_t)F - base : (size_t)kMsBlock);
      const double bt = cdf_local[base + n - 1];
      double tl = t - excl;
      if (!(tl >= 0.0)) tl = 0.0;
      if (!(tl < bt) && bt > 0.0) tl = __longlong_as_double(__double_as_longlong(bt) - 1);      // the double just below bt
      const int k = ms_upper(cdf_local + base, n, tl, 9);
      if (k >= 0 && k < n) f = (int)(base + k);
    }
  }
  float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
  if (f >= 0 && f < F) {
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if (face_in_range(ia, ib, ic, V)) {
      const MsFace g = ms_face(verts, ia, ib, ic);
      const float r = sqrtf(u1);
      w0 = 1.0f - r;
      w1 = r * (1.0f - u2);
      w2 = r * u2;
      px = g.ax + (w1 * g.e1x + w2 * g.e2x);
      py = g.ay + (w1 * g.e1y + w2 * g.e2y);
      pz = g.az + (w1 * g.e1z + w2 * g.e2z);
      if (g.A2 > 0.0f) { nx = g.crx / g.A2; ny = g.cry / g.A2; nz = g.crz / g.A2; }
    } else {
      f = -1;
    }
  } else {
    f = -1;
  }
  face_idx[s] = f;
  points[3 * s] = px; points[3 * s + 1] = py; points[3 * s + 2] = pz;
  bary[3 * s] = w0; bary[3 * s + 1] = w1; bary[3 * s + 2] = w2;
  if (normals) { normals[3 * s] = nx; normals[3 * s + 1] = ny; normals[3 * s + 2] = nz; }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------

// the largest |g| (as bits: |g| >= 0 orders as its bits do, and a NaN lies above the infinity) over g_points and g_normals
__global__ void __launch_bounds__(256)
ms_absmax_kernel(const float *__restrict__ g_points, const float *__restrict__ g_normals, const size_t n, FixedHead *__restrict__ head) {
  uint32_t m = 0u;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (g_points) m = max(m, __float_as_uint(g_points[i]) & 0x7fffffffu);
    if (g_normals) m = max(m, __float_as_uint(g_normals[i]) & 0x7fffffffu);
  }
  fixed_commit_max(head, m);
}

__global__ void __launch_bounds__(256)
ms_scatter_kernel(const int32_t *__restrict__ faces, const int V, const int F, const int32_t *__restrict__ face_idx,
                  const float *__restrict__ bary, const int S, const float *__restrict__ g_points, const float *__restrict__ g_normals,
                  const FixedHead *__restrict__ head, const int list_bits, long long *__restrict__ acc_v, long long *__restrict__ acc_f) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (size_t)S) return;
  const int f = face_idx[s];
  if (f < 0 || f >= F) return;
  const double scale = ldexp(1.0, fixed_scale_exponent(head, list_bits));
  if (g_points) {
    const int iv[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
    if (face_in_range(iv[0], iv[1], iv[2], V)) {
      const double w1 = (double)bary[3 * s + 1], w2 = (double)bary[3 * s + 2];
      const double w[3] = {(1.0 - w1) - w2, w1, w2};
      const double gx = (double)g_points[3 * s] * scale, gy = (double)g_points[3 * s + 1] * scale, gz = (double)g_points[3 * s + 2] * scale;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        long long *acc = acc_v + 3 * (size_t)iv[r];
        atomic_add_i64(acc, llrint(w[r] * gx));
        atomic_add_i64(acc + 1, llrint(w[r] * gy));
        atomic_add_i64(acc + 2, llrint(w[r] * gz));
      }
    }
  }
  if (g_normals) {
    long long *acc = acc_f + 3 * (size_t)f;
    atomic_add_i64(acc, llrint((double)g_normals[3 * s] * scale));
    atomic_add_i64(acc + 1, llrint((double)g_normals[3 * s + 1] * scale));
    atomic_add_i64(acc + 2, llrint((double)g_normals[3 * s + 2] * scale));
  }
}

__global__ void __launch_bounds__(256)
ms_finish_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                 const int32_t *__restrict__ corner_off, const int32_t *__restrict__ corner, const FixedHead *__restrict__ head,
                 const int list_bits, const long long *__restrict__ acc_v, const long long *__restrict__ acc_f,
                 float *__restrict__ g_verts) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  const double unscale = ldexp(1.0, -fixed_scale_exponent(head, list_bits));
  double gx = (double)acc_v[3 * v] * unscale, gy = (double)acc_v[3 * v + 1] * unscale, gz = (double)acc_v[3 * v + 2] * unscale;
  if (acc_f) {
    const long c0 = corner_off[v], c1 = corner_off[v + 1];
    const long n3 = 3l * (long)F;
    for (long c = c0 > 0 ? c0 : 0; c < c1 && c < n3; ++c) {      // (corner_off is a CSR over the 3 F corners: a guard, not a route)
      const int entry = corner[c];
      if (entry < 0 || (long)entry >= n3) continue;
      const int f = entry / 3, role = entry - 3 * f;
      const long long *af = acc_f + 3 * (size_t)f;
      if ((af[0] | af[1] | af[2]) == 0) continue;      // (no sample on the face asked for its normal, or the requests cancel: + 0)
      const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
      if (!face_in_range(ia, ib, ic, V)) continue;
      const float *a = verts + 3 * (size_t)ia, *b = verts + 3 * (size_t)ib, *cc = verts + 3 * (size_t)ic;
      const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
      const double e2x = (double)cc[0] - (double)a[0], e2y = (double)cc[1] - (double)a[1], e2z = (double)cc[2] - (double)a[2];
      const double crx = e1y * e2z - e1z * e2y, cry = e1z * e2x - e1x * e2z, crz = e1x * e2y - e1y * e2x;
      const double A2 = sqrt((crx * crx + cry * cry) + crz * crz);
      if (!(A2 > 0.0) || !(ms_face(verts, ia, ib, ic).A2 > 0.0f)) continue;      // (the forward's own A2: what decided whether a normal was written)
      const double nx = crx / A2, ny = cry / A2, nz = crz / A2;
      const double Gx = (double)af[0] * unscale, Gy = (double)af[1] * unscale, Gz = (double)af[2] * unscale;
      const double nG = (nx * Gx + ny * Gy) + nz * Gz;
      const double dx = (Gx - nx * nG) / A2, dy = (Gy - ny * nG) / A2, dz = (Gz - nz * nG) / A2;      // dL / dcr
      // dL/de1 = e2 x d, dL/de2 = d x e1
      const double p1x = e2y * dz - e2z * dy, p1y = e2z * dx - e2x * dz, p1z = e2x * dy - e2y * dx;
      const double p2x = dy * e1z - dz * e1y, p2y = dz * e1x - dx * e1z, p2z = dx * e1y - dy * e1x;
      if (role == 0) { gx -= p1x + p2x; gy -= p1y + p2y; gz -= p1z + p2z; }
      else if (role == 1) { gx += p1x; gy += p1y; gz += p1z; }
      else { gx += p2x; gy += p2y; gz += p2z; }
    }
  }
  g_verts[3 * v] = (float)gx; g_verts[3 * v + 1] = (float)gy; g_verts[3 * v + 2] = (float)gz;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct MsLayout {
  size_t cdf, btotal, bincl, fwd, head, acc_v, acc_f, bwd;
  int nb;
};
static MsLayout ms_layout(const long V, const long F, const long S) {
  (void)S;
  MsLayout l;
  l.nb = (int)((F + kMsBlock - 1) / kMsBlock);
  Carve fwd, bwd;      // (two calls on one workspace: each starts at its front)
  l.cdf = fwd.take((size_t)F * sizeof(double));
  l.btotal = fwd.take((size_t)l.nb * sizeof(double));
  l.bincl = fwd.take((size_t)l.nb * sizeof(double));
  l.fwd = fwd.at;
  l.head = bwd.take_exact(sizeof(FixedHead));
  l.acc_v = bwd.take_exact((size_t)V * 3 * sizeof(long long));
  l.acc_f = bwd.take_exact((size_t)F * 3 * sizeof(long long));
  l.bwd = up16(bwd.at);
  return l;
}

static bool ms_sizes_ok(const long V, const long F, const long S) {
  return V >= 1 && F >= 1 && S >= 0 && V <= kMsMax && F <= kMsMax && S <= kMsMax;
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_mesh_sample_workspace_bytes(long V, long F, long S) {
  if (!ms_sizes_ok(V, F, S)) return 0;
  const MsLayout l = ms_layout(V, F, S);
  return l.fwd > l.bwd ? l.fwd : l.bwd;
}

extern "C" int voge_mesh_sample_fwd(const float *verts, long V, const int32_t *faces, long F, const float *u, long S, float *points,
                                    float *normals, int32_t *face_idx, float *bary, float *a2_out, void *workspace,
                                    size_t workspace_bytes, voge_stream_t stream) {
  if (!ms_sizes_ok(V, F, S)) return VOGE_ERR_BAD_ARG;
  if (S == 0 && !a2_out) return 0;
  if (!verts || !faces || bad_workspace(workspace) || (S > 0 && (!u || !points || !face_idx || !bary))) return VOGE_ERR_BAD_ARG;
  const MsLayout l = ms_layout(V, F, S);
  if (workspace_bytes < l.fwd) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  double *cdf = reinterpret_cast<double *>(ws + l.cdf), *btotal = reinterpret_cast<double *>(ws + l.btotal),
         *bincl = reinterpret_cast<double *>(ws + l.bincl);
  hipLaunchKernelGGL(ms_area_scan_kernel, dim3((unsigned)l.nb), dim3(kMsBlock), 0, st, verts, (int)V, faces, (int)F, cdf, btotal, a2_out);
  if (S > 0) {
    hipLaunchKernelGGL(ms_block_scan_kernel, dim3(1), dim3(1024), 0, st, btotal, l.nb, bincl);
    hipLaunchKernelGGL(ms_sample_kernel, dim3(blocks256(S)), dim3(256), 0, st, verts, (int)V, faces, (int)F, u, (int)S, cdf,
                       bincl, l.nb, points, normals, face_idx, bary);
  }
  return launch_status();
}

extern "C" int voge_mesh_sample_bwd(const float *verts, long V, const int32_t *faces, long F, const int32_t *corner_off,
                                    const int32_t *corner, const int32_t *face_idx, const float *bary, long S, const float *g_points,
                                    const float *g_normals, float *g_verts, void *workspace, size_t workspace_bytes,
                                    voge_stream_t stream) {
  if (!ms_sizes_ok(V, F, S)) return VOGE_ERR_BAD_ARG;
  if (!verts || !faces || !g_verts || bad_workspace(workspace) || (S > 0 && (!face_idx || !bary))) return VOGE_ERR_BAD_ARG;
  if (g_normals && (!corner_off || !corner)) return VOGE_ERR_BAD_ARG;
  const MsLayout l = ms_layout(V, F, S);
  const size_t bytes = g_normals ? l.bwd : l.acc_f;      // (without normals the faces' accumulators are not used)
  if (workspace_bytes < bytes) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  FixedHead *head = reinterpret_cast<FixedHead *>(ws + l.head);
  long long *acc_v = reinterpret_cast<long long *>(ws + l.acc_v);
  long long *acc_f = g_normals ? reinterpret_cast<long long *>(ws + l.acc_f) : nullptr;
  const hipError_t fe = voge_fill_async(workspace, 0, g_normals ? l.acc_f + (size_t)F * 3 * sizeof(long long) : l.acc_f, st);
  if (fe != hipSuccess) return (int)fe;
  const int bits = ceil_log2(S);      // S <= 2^bits: every list of the scatter
  if (S > 0 && (g_points || g_normals)) {
    const size_t n = (size_t)S * 3;
    hipLaunchKernelGGL(ms_absmax_kernel, dim3(blocks256_capped(n)), dim3(256), 0, st, g_points, g_normals, n, head);
    hipLaunchKernelGGL(ms_scatter_kernel, dim3(blocks256(S)), dim3(256), 0, st, faces, (int)V, (int)F, face_idx, bary, (int)S,
                       g_points, g_normals, head, bits, acc_v, acc_f);
  }
  hipLaunchKernelGGL(ms_finish_kernel, dim3(blocks256(V)), dim3(256), 0, st, verts, (int)V, faces, (int)F, corner_off, corner,
                     head, bits, acc_v, acc_f, g_verts);
  return launch_status();
}
