// Point clouds (EXTENSION: the reference's only neighbour search is the chunked cdist + topk of Converters.py:98-122, on all
// N^2 pairs): exact k nearest neighbours over a uniform grid, and a local-PCA frame per point on top of them.
//
// voge_knn_points.  d2(q, p) = (dx*dx + dy*dy) + dz*dz with dx = xq - xp, ..., every operation one IEEE fp32 operation (the
// library is built with -ffp-contract=off); row i of the output holds the k lexicographically smallest (d2, index) pairs,
// ascending, padded with (-1, +inf).  That is a property of the SET of candidates, so any search that provably visits every
// point that can be among the k smallest returns the same bits, whatever the grid and whatever the visiting order:
//   (a) knn_count_kernel: cell of every point, c_a = clamp(floorf((x_a - lo_a) * inv_cell), 0, G_a - 1) in fp32, kept per
//       point, and integer atomic counts per cell;
//   (b) an exclusive scan of the counts in three launches (2048 cells a workgroup, the workgroups' sums by one workgroup);
//   (c) knn_fill_kernel: (x, y, z, index bits) as a float4 in cell order (the order INSIDE a cell depends on the atomics'
//       arrival -- it decides which lane serves which query, never a result);
//   (d) knn_search_kernel: one query per lane, in cell order (a wave's lanes share their candidate cells), rings of cells
//       r = 0, 1, 2, ... around the query's cell, the k best as sorted 64-bit keys (d2 bits << 32 | index; d2 >= 0, so its
//       bits order as the value does) in one LDS column per lane (topk_insert of voge_common.h).
// The stopping rule.  After ring r every cell within Chebyshev distance r of the query's has been visited, so an unvisited point
// p differs from the query q by >= r + 1 in the cell index of some axis.  Let t(x) = (x - lo) / cell and u(x) = fl(fl(x - lo) *
// fl(1 / cell)) = t(x) (1 + e), |e| < 3 * 2^-24 < 2^-22.  floorf and the clamp are monotone and the clamp never widens a
// difference, so floor(u_p) - floor(u_q) >= r + 1, hence u_p - u_q > r, hence t_p - t_q > r - 2^-22 (t_p + t_q) > r - 2^-11
// (t < 1024: the host makes G_a = floor(extent_a / cell) + 1 <= 1024 from the same box, which is why the grid must cover the
// cloud): p is farther than cell (r - 2^-11) from q ON THAT AXIS.
// The search stops after ring r once the list is full and its k-th d2 <= b * b, b = cell (r - 2^-10) (1 - 2^-20) > 0: the
// factor (1 - 2^-20) covers the three roundings of b, the one of b * b and the four of an fp32 d2 >= dx^2 (each <= 2^-24
// relative), so every unvisited point has an fp32 d2 strictly above the k-th -- no tie can be missed either.  It also stops when
// the cube covers the grid.  Every loop is bounded by the grid or by k; no wait on another workgroup, no float atomics.
//
// voge_knn_frames.  One point per lane: mean and covariance (two passes, on differences to the query point, fp32) of the valid
// neighbours of a row of idx, scaled by its trace, 8 cyclic Jacobi sweeps, n = eigenvector of the smallest eigenvalue, t1 = of
// the largest, R = [t1, n x t1, n] as a quaternion (w, x, y, z) with w >= 0.  Entries of idx outside [0, N) are skipped.
#include <math.h>

#include "knn_grid.h"      // the grid, its binning steps and the scan, shared with chamfer.hip and point_mesh_grid.h

namespace voge {

constexpr int kKnnMaxK = 32;
constexpr int kKnnSearchBlock = 128;      // lanes (queries) a workgroup: k * 128 * 8 bytes of LDS, 32 KB at k = 32

__global__ void __launch_bounds__(256)
knn_count_kernel(const float *__restrict__ pts, const int N, const KnnGrid g, int *__restrict__ cellid, int *__restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N) return;
  grid_count_point(g, pts, i, cellid, counts);
}

__global__ void __launch_bounds__(256)
knn_fill_kernel(const float *__restrict__ pts, const int N, const int *__restrict__ cellid, int *__restrict__ counts,
                const int *__restrict__ start, float4 *__restrict__ sorted) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N) return;
  grid_fill_point(pts, i, cellid[i], counts, start, N, sorted);
}

template <bool SELF>
__global__ void __launch_bounds__(kKnnSearchBlock)
knn_search_kernel(const float4 *__restrict__ sorted, const int *__restrict__ start, const int N, const int k, const KnnGrid g,
                  int32_t *__restrict__ idx, float *__restrict__ d2out) {
  extern __shared__ uint64_t knn_keys[];      // [k][kKnnSearchBlock]
  const size_t t = (size_t)blockIdx.x * kKnnSearchBlock + threadIdx.x;
  if (t >= (size_t)N) return;      // (no barrier below)
  const float4 q = sorted[t];
  const int qi = __float_as_int(q.w);
  if (qi < 0 || qi >= N) return;      // (every slot of `sorted` was filled with an index below N: a guard on the output row, not a route)
  const int cx = knn_axis_cell(q.x, g.lox, g.inv, g.gx), cy = knn_axis_cell(q.y, g.loy, g.inv, g.gy),
            cz = knn_axis_cell(q.z, g.loz, g.inv, g.gz);
  uint64_t *col = knn_keys + threadIdx.x;
  int cnt = 0;
  uint64_t worst = ~0ull, tail = 0ull;
  // the ring at which the cube covers the grid
  const int rmax = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
  for (int r = 0; r <= rmax; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.gx - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, g.gy - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.gz - 1);
    for (int zz = z0; zz <= z1; ++zz) {
      for (int yy = y0; yy <= y1; ++yy) {
        const int row = (zz * g.gy + yy) * g.gx;
        // a row of the shell's faces in y or z: cells x0 .. x1 are consecutive in cell order, one range; an inner row:
        // the two cells at x = cx -+ r (r >= 1 there), where the grid has them
        const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
#pragma unroll
        for (int part = 0; part < 2; ++part) {
          int ca, cb;      // cells [ca, cb] of the row
          if (face) {
            if (part == 1) break;
            ca = x0; cb = x1;
          } else {
            ca = cb = part == 0 ? cx - r : cx + r;
            if (ca < 0 || ca >= g.gx) continue;
          }
          const int j0 = start[row + ca], j1 = start[row + cb + 1];
          for (int j = j0; j < j1; ++j) {
            const float4 p = sorted[j];
            const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const int pi = __float_as_int(p.w);
            const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)pi;
            if ((SELF || pi != qi) && key < worst) topk_insert(col, kKnnSearchBlock, k, cnt, worst, tail, key);
          }
        }
      }
    }
    if (cnt == k) {
      const float b = g.cell * ((float)r - 0x1p-10f) * (1.0f - 0x1p-20f);
      if (b > 0.0f && __uint_as_float((uint32_t)(worst >> 32)) <= b * b) break;
    }
  }
  int32_t *oi = idx + (size_t)qi * k;
  float *od = d2out + (size_t)qi * k;
  for (int s = 0; s < k; ++s) {
    const uint64_t key = s < cnt ? col[s * kKnnSearchBlock] : 0ull;
    oi[s] = s < cnt ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
    od[s] = s < cnt ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
  }
}

// ---- local PCA frames ------------------------------------------------------------------------------------------------------

// one Jacobi rotation in the (p, q) plane of a symmetric 3x3 (r the third index): app, aqq, apq and the two off-diagonal
// entries towards r; the eigenvector matrix V's columns p and q (vp*, vq*).  theta = (aqq - app) / (2 apq), t = sgn(theta) /
// (|theta| + sqrt(theta^2 + 1)): the smaller root, |t| <= 1.
__device__ __forceinline__ void knn_jacobi(float &app, float &aqq, float &apq, float &arp, float &arq, float &vp0, float &vp1,
                                           float &vp2, float &vq0, float &vq1, float &vq2) {
  if (!(fabsf(apq) > 0.0f)) return;
  const float theta = (aqq - app) / (2.0f * apq);
  const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const float p0 = vp0, p1 = vp1, p2 = vp2;
  vp0 = c * p0 - s * vq0; vp1 = c * p1 - s * vq1; vp2 = c * p2 - s * vq2;
  vq0 = s * p0 + c * vq0; vq1 = s * p1 + c * vq1; vq2 = s * p2 + c * vq2;
}

// (l, v) pairs into ascending order of l
__device__ __forceinline__ void knn_order(float &la, float &a0, float &a1, float &a2, float &lb, float &b0, float &b1, float &b2) {
  if (lb < la) {
    float s;
    s = la; la = lb; lb = s;
    s = a0; a0 = b0; b0 = s;
    s = a1; a1 = b1; b1 = s;
    s = a2; a2 = b2; b2 = s;
  }
}

__global__ void __launch_bounds__(256)
knn_frames_kernel(const float *__restrict__ pts, const int32_t *__restrict__ idx, const int N, const int k,
                  const float *__restrict__ toward, const int toward_per_point, float *__restrict__ quats, float *__restrict__ eig) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N) return;
  const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const int32_t *row = idx + i * (size_t)k;
  int n = 0;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int s = 0; s < k; ++s) {
    const int j = row[s];
    if (j < 0 || j >= N) continue;
    sx += pts[3 * (size_t)j] - px; sy += pts[3 * (size_t)j + 1] - py; sz += pts[3 * (size_t)j + 2] - pz;
    ++n;
  }
  const float rn = 1.0f / (float)max(n, 1);
  const float mx = sx * rn, my = sy * rn, mz = sz * rn;
  float a00 = 0.f, a11 = 0.f, a22 = 0.f, a01 = 0.f, a02 = 0.f, a12 = 0.f;
  for (int s = 0; s < k; ++s) {
    const int j = row[s];
    if (j < 0 || j >= N) continue;
    const float ex = (pts[3 * (size_t)j] - px) - mx, ey = (pts[3 * (size_t)j + 1] - py) - my, ez = (pts[3 * (size_t)j + 2] - pz) - mz;
    a00 = fmaf(ex, ex, a00); a11 = fmaf(ey, ey, a11); a22 = fmaf(ez, ez, a22);
    a01 = fmaf(ex, ey, a01); a02 = fmaf(ex, ez, a02); a12 = fmaf(ey, ez, a12);
  }
  a00 *= rn; a11 *= rn; a22 *= rn; a01 *= rn; a02 *= rn; a12 *= rn;
  const float tr = (a00 + a11) + a22;
  const bool has = tr > 0.0f && tr < INFINITY;
  const float itr = has ? 1.0f / tr : 0.0f;      // (the unit-trace matrix: a cloud of extent 1e-4 behaves like one of extent 1)
  a00 *= itr; a11 *= itr; a22 *= itr; a01 *= itr; a02 *= itr; a12 *= itr;
  float v00 = 1.f, v10 = 0.f, v20 = 0.f, v01 = 0.f, v11 = 1.f, v21 = 0.f, v02 = 0.f, v12 = 0.f, v22 = 1.f;      // v[row][column]
  for (int sweep = 0; sweep < 8; ++sweep) {
    knn_jacobi(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);      // (0, 1), r = 2
    knn_jacobi(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);      // (0, 2), r = 1
    knn_jacobi(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);      // (1, 2), r = 0
  }
  float l0 = a00, l1 = a11, l2 = a22;
  knn_order(l0, v00, v10, v20, l1, v01, v11, v21);
  knn_order(l1, v01, v11, v21, l2, v02, v12, v22);
  knn_order(l0, v00, v10, v20, l1, v01, v11, v21);
  const float e0 = l0 * tr, e1 = l1 * tr, e2 = l2 * tr;
  eig[3 * i] = has ? e0 : 0.f; eig[3 * i + 1] = has ? e1 : 0.f; eig[3 * i + 2] = has ? e2 : 0.f;
  // degenerate: fewer than three neighbours, or a middle eigenvalue that an fp32 covariance of <= 32 terms cannot tell from
  // zero (64 * 2^-24 of the largest) -- decided on the values written to eig, so a caller can repeat the decision
  float4 qo = make_float4(1.f, 0.f, 0.f, 0.f);
  if (has && n >= 3 && e1 > 0x1p-18f * e2) {
    // n = column 0, t1 = column 2, made orthonormal once more (V is orthogonal to a few ulp)
    float nx = v00, ny = v10, nz = v20, tx = v02, ty = v12, tz = v22;
    float inv = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
    bool flip;
    if (toward) {
      const float *tw = toward + (toward_per_point ? 3 * i : 0);
      flip = (nx * (tw[0] - px) + ny * (tw[1] - py) + nz * (tw[2] - pz)) < 0.0f;
    } else {      // the component of largest magnitude is positive, the lowest index on a tie
      float best = nx;
      if (fabsf(ny) > fabsf(best)) best = ny;
      if (fabsf(nz) > fabsf(best)) best = nz;
      flip = best < 0.0f;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    const float along = tx * nx + ty * ny + tz * nz;
    tx -= along * nx; ty -= along * ny; tz -= along * nz;
    inv = 1.0f / sqrtf(tx * tx + ty * ty + tz * tz);
    tx *= inv; ty *= inv; tz *= inv;
    const float ux = ny * tz - nz * ty, uy = nz * tx - nx * tz, uz = nx * ty - ny * tx;      // t2 = n x t1
    // R = [t1 t2 n] (columns): m_rc
    const float m00 = tx, m01 = ux, m02 = nx, m10 = ty, m11 = uy, m12 = ny, m20 = tz, m21 = uz, m22 = nz;
    const float trace = m00 + m11 + m22;
    float w, x, y, z;
    if (trace > 0.0f) {
      const float s = 2.0f * sqrtf(trace + 1.0f);
      w = 0.25f * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
      const float s = 2.0f * sqrtf(1.0f + m00 - m11 - m22);
      w = (m21 - m12) / s; x = 0.25f * s; y = (m01 + m10) / s; z = (m02 + m20) / s;
    } else if (m11 > m22) {
      const float s = 2.0f * sqrtf(1.0f + m11 - m00 - m22);
      w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25f * s; z = (m12 + m21) / s;
    } else {
      const float s = 2.0f * sqrtf(1.0f + m22 - m00 - m11);
      w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25f * s;
    }
    const float qn = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    const float sg = w < 0.0f ? -qn : qn;
    const float4 cand = make_float4(w * sg, x * sg, y * sg, z * sg);
    if (cand.x == cand.x && cand.y == cand.y && cand.z == cand.z && cand.w == cand.w) qo = cand;      // (never a NaN out)
  }
  float *qd = quats + 4 * i;
  qd[0] = qo.x; qd[1] = qo.y; qd[2] = qo.z; qd[3] = qo.w;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static long knn_cells(const int gx, const int gy, const int gz) { return (long)gx * gy * gz; }

// the grid is one the host wrapper may have chosen: every axis in [1, 1024], the product <= max(8 N, 2^15)
static bool knn_grid_ok(const long N, const int gx, const int gy, const int gz) {
  if (gx < 1 || gy < 1 || gz < 1 || gx > kKnnMaxAxis || gy > kKnnMaxAxis || gz > kKnnMaxAxis) return false;
  const long cap = 8 * N > 32768l ? 8 * N : 32768l;
  return knn_cells(gx, gy, gz) <= cap && knn_cells(gx, gy, gz) < 2147483647l;
}

struct KnnLayout {
  size_t sorted, cellid, counts, start, bsum, total;
  int nb;
};
static KnnLayout knn_layout(const long N, const long G) {
  KnnLayout l;
  l.nb = (int)((G + kKnnScanBlock * kKnnScanItems - 1) / (kKnnScanBlock * kKnnScanItems));
  Carve c;
  l.sorted = c.take_exact((size_t)N * 16);
  l.cellid = c.take((size_t)N * 4);
  l.counts = c.take((size_t)G * 4);
  l.start = c.take((size_t)(G + 1) * 4);
  l.bsum = c.take((size_t)l.nb * 4);
  l.total = c.at;
  return l;
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_knn_workspace_bytes(long N, int gx, int gy, int gz) {
  if (N < 0 || N > 268435455l || !knn_grid_ok(N, gx, gy, gz)) return 0;
  return knn_layout(N, knn_cells(gx, gy, gz)).total;
}

extern "C" int voge_knn_points(const float *points, long N, int k, int include_self, float lo_x, float lo_y, float lo_z, float cell,
                               int gx, int gy, int gz, int32_t *idx, float *d2, void *workspace, size_t workspace_bytes,
                               voge_stream_t stream) {
  if (k < 1 || N < 0 || N > 268435455l) return VOGE_ERR_BAD_ARG;
  if (k > kKnnMaxK) return VOGE_ERR_K_TOO_LARGE;
  if (!(cell > 0.0f) || !(cell < INFINITY) || !(fabsf(lo_x) < INFINITY) || !(fabsf(lo_y) < INFINITY) || !(fabsf(lo_z) < INFINITY))
    return VOGE_ERR_BAD_ARG;
  const float inv = 1.0f / cell;
  if (!(inv > 0.0f) || !(inv < INFINITY) || !knn_grid_ok(N, gx, gy, gz)) return VOGE_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!points || !idx || !d2 || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const long G = knn_cells(gx, gy, gz);
  const KnnLayout l = knn_layout(N, G);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  float4 *sorted = reinterpret_cast<float4 *>(ws + l.sorted);
  int *cellid = reinterpret_cast<int *>(ws + l.cellid), *counts = reinterpret_cast<int *>(ws + l.counts),
      *start = reinterpret_cast<int *>(ws + l.start), *bsum = reinterpret_cast<int *>(ws + l.bsum);
  const KnnGrid g{lo_x, lo_y, lo_z, cell, inv, gx, gy, gz};
  hipStream_t st = (hipStream_t)stream;
  const unsigned nblk = blocks256(N);
  const hipError_t fe = voge_fill_async(counts, 0, (size_t)G * 4, st);
  if (fe != hipSuccess) return (int)fe;
  hipLaunchKernelGGL(knn_count_kernel, dim3(nblk), dim3(256), 0, st, points, (int)N, g, cellid, counts);
  grid_scan_launch(counts, (int)G, nullptr, bsum, l.nb, (int)N, start, st);
  hipLaunchKernelGGL(knn_fill_kernel, dim3(nblk), dim3(256), 0, st, points, (int)N, cellid, counts, start, sorted);
  const unsigned sblk = (unsigned)((N + kKnnSearchBlock - 1) / kKnnSearchBlock);
  const size_t lds = (size_t)k * kKnnSearchBlock * sizeof(uint64_t);
  if (include_self)
    hipLaunchKernelGGL(knn_search_kernel<true>, dim3(sblk), dim3(kKnnSearchBlock), lds, st, sorted, start, (int)N, k, g, idx, d2);
  else
    hipLaunchKernelGGL(knn_search_kernel<false>, dim3(sblk), dim3(kKnnSearchBlock), lds, st, sorted, start, (int)N, k, g, idx, d2);
  return launch_status();
}

extern "C" int voge_knn_frames(const float *points, const int32_t *idx, long N, int k, const float *toward, int toward_per_point,
                               float *quats, float *eig, voge_stream_t stream) {
  if (k < 1 || N < 0 || N > 268435455l) return VOGE_ERR_BAD_ARG;
  if (k > kKnnMaxK) return VOGE_ERR_K_TOO_LARGE;
  if (N == 0) return 0;
  if (!points || !idx || !quats || !eig) return VOGE_ERR_BAD_ARG;
  hipLaunchKernelGGL(knn_frames_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, points, idx, (int)N, k,
                     toward, toward_per_point != 0, quats, eig);
  return launch_status();
}
