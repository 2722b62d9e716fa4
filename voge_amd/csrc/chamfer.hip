// Chamfer distance (EXTENSION: the reference's demo/ShapeFitting.py imports chamfer_distance from PyTorch3D; the torch form is a
// cdist + min over all Nx Ny pairs): exact nearest points between TWO clouds, the loss over them and its backward.
//
// voge_nearest_points.  d2(q, p) = (dx*dx + dy*dy) + dz*dz with dx = xq - xp, ..., every operation one IEEE fp32 operation (the
// library is built with -ffp-contract=off); a query gets the lexicographically smallest (d2, index) over the points, held as ONE
// 64-bit key (d2 bits << 32 | index; d2 >= 0, so its bits order as the value does) in a register.  That is a property of the SET
// of candidates, so the two routes return the same bits:
//   brute  chamfer_brute_kernel, one launch a direction: 64 queries a workgroup, the points tiled through LDS 1024 at a time, the
//          four waves take a quarter of a tile each and the four keys of a query meet in LDS (a minimum: no order to depend on);
//   grid   the search of knn.hip between two clouds, over a grid chosen ON THE DEVICE -- nothing of the call depends on a value
//          the host would have to read, so it can be captured into a graph:
//     (a) grid_box_kernel / chamfer_grid_kernel: the bounding box of the UNION of the clouds, and one thread that runs the rule
//         of ops.knn_grid (grid_choose of knn_grid.h): about 2 n cubic cells (n = max(Nx, Ny)), cell >= max extent / 1023,
//         G_a = floor(extent_a / cell) + 1 <= 1024 on every axis, G = Gx Gy Gz <= max(8 n, 2^15); the loop that enlarges the cell has 64 trips at most, and a box that
//         is not finite or a loop that did not end gives the one-cell grid (every point a candidate of ring 0: a brute force).
//         The grid goes into the workspace's head, every later kernel reads it from there; the workspace and the launches are
//         sized for the cap on G, which depends on (Nx, Ny) alone, and the scan reads the real G from memory;
//     (b) both clouds binned in that one grid: integer atomic counts, the scan of knn_grid.h, the fill -- as knn.hip does;
//     (c) chamfer_search_kernel: one query per lane, in its OWN cloud's cell order (a wave's lanes share their candidate cells),
//         against the other cloud's cell-ordered array; rings r = 0, 1, 2, ... of cells around the query's cell.
// The stopping rule is knn.hip's at k = 1.  After ring r every cell within Chebyshev distance r of the query's has been visited,
// so an unvisited point p differs from the query q by >= r + 1 in the cell index of some axis.  With t(x) = (x - lo) / cell and
// u(x) = fl(fl(x - lo) * fl(1 / cell)) = t(x) (1 + e), |e| < 2^-22: floorf and the clamp are monotone and the clamp never widens a
// difference, so u_p - u_q > r, hence t_p - t_q > r - 2^-22 (t_p + t_q) > r - 2^-11 -- t < 1024 for EVERY point and EVERY query,
// which is why the box must be the union's: G_a <= 1024 is made from the box that holds both clouds.  So p is farther than
// cell (r - 2^-11) from q on that axis, and the search stops after ring r once it holds a candidate whose d2 <= b * b,
// b = cell (r - 2^-10) (1 - 2^-20) > 0 (the factor covers the roundings of b, b * b and of an fp32 d2 >= dx^2): every unvisited
// point has an fp32 d2 strictly above the kept one -- no tie can be missed.  A query whose own cell holds no point of the other
// cloud simply holds no candidate yet: the rule cannot fire (and never fires at r = 0, where b < 0), the rings go on until one
// does or until the cube covers the grid, which bounds every loop.  A NaN or an infinity lands on a valid cell (knn_axis_cell) and
// walks at most the whole grid; the values are then out of contract, the indices still in range (an index that is not is written
// as -1, and the backward skips it).
//
// voge_chamfer_fwd.  The two searches write d2 by the query's own index; chamfer_loss_partial_kernel (chamfer_loss.h) leaves one fp64 sum (and the
// largest d2) per 1024 queries, chamfer_loss_final_kernel -- ONE workgroup -- adds them in an order fixed by the shapes (the
// mesh_reg.hip pattern) and rounds sum_x / Nx + sum_y / Ny to fp32 once.
//
// voge_chamfer_bwd, three launches.  g_x[i] = g (2 / Nx) (x_i - y_nn(i)) + g (2 / Ny) sum_{j: nn(j) = i} (x_i - y_j): a gather and
// a scatter whose lists can be as long as the other cloud (coincident points all pick index 0).  The scatter is done in FIXED
// POINT: every fp32 difference is scaled by 2^s, rounded to an int64 and added with a 64-bit INTEGER atomic into a zero-filled
// [N][3] accumulator -- integer addition is exact, so the sum does not depend on the order and the bits are the same on every run,
// at a cost linear in the points.  s is chosen on the device by the forward's last kernel and saved in meta[0]: with
// D = sqrt(max d2 (1 + 2^-20) + 2^-148) < 2^e bounding every component of every scattered difference (they are the differences
// the d2 were made of) and n = max(Nx, Ny) <= 2^L bounding every list, s = 62 - L - e, so |sum| <= 2^62 cannot overflow.  The
// quantum is q = 2^-s <= 2^(L - 61) D: a list of m terms is off by at most m q / 2 <= m 2^(L - 62) D per component, 2^-34 D a
// term for the largest clouds this library holds (L = 28).  chamfer_finish_kernel turns the accumulators into fp64, adds
// the gather term (one fp32 difference), scales by the upstream gradient and writes EVERY element of g_x and g_y, rounded to fp32
// once.  No float atomics anywhere, no wait on another workgroup.
#include <math.h>

#include "chamfer_loss.h"
#include "knn_grid.h"

namespace voge {

constexpr long kChamferMaxN = 268435455l;
constexpr double kChamferBruteMaxPairs = 8388608.0;      // Nx Ny at or below this: the brute route (measured: profiles/r17_chamfer.txt)
constexpr int kChSearchBlock = 128;
constexpr int kChTile = 1024;           // points of a brute-force tile

struct ChamferHead {      // the workspace's first 64 bytes
  KnnGrid g;
  int G;
  int pad[7];
};
static_assert(sizeof(ChamferHead) == 64, "ChamferHead is 64 bytes");

// ---- the grid, chosen on the device -------------------------------------------------------------------------------------------

// ONE workgroup: the box of the partial boxes, then thread 0 chooses the grid (grid_choose with n = max(Nx, Ny) and no floor)
__global__ void __launch_bounds__(256)
chamfer_grid_kernel(const float *__restrict__ partial, const int nb, const long n, const float cell_size, ChamferHead *__restrict__ head) {
  float lo[3], hi[3];
  grid_box_reduce(partial, nb, lo, hi);
  if (threadIdx.x != 0) return;
  ChamferHead h;
  grid_choose(lo, hi, n, cell_size, 0.0, h.g, h.G);
  for (int k = 0; k < 7; ++k) h.pad[k] = 0;
  *head = h;
}

// ---- both clouds binned in the one grid ---------------------------------------------------------------------------------------

struct ChamferCloud {
  const float *pts;
  int N;
  int *cellid, *counts, *start;
  float4 *sorted;
};

__global__ void __launch_bounds__(256)
chamfer_count_kernel(const ChamferCloud a, const ChamferCloud b, const unsigned nba, const ChamferHead *__restrict__ head) {
  const bool first = blockIdx.x < nba;
  const size_t i = (size_t)(blockIdx.x - (first ? 0u : nba)) * 256 + threadIdx.x;
  const int N = first ? a.N : b.N;
  if (i >= (size_t)N) return;
  grid_count_point(head->g, first ? a.pts : b.pts, i, first ? a.cellid : b.cellid, first ? a.counts : b.counts);
}

__global__ void __launch_bounds__(256)
chamfer_fill_kernel(const ChamferCloud a, const ChamferCloud b, const unsigned nba, const ChamferHead *__restrict__ head) {
  const bool first = blockIdx.x < nba;
  const size_t i = (size_t)(blockIdx.x - (first ? 0u : nba)) * 256 + threadIdx.x;
  const int N = first ? a.N : b.N;
  if (i >= (size_t)N) return;
  const int c = (first ? a.cellid : b.cellid)[i];
  if (c < 0 || c >= head->G) return;      // (the count pass wrote a cell of this grid: a guard, not a route)
  grid_fill_point(first ? a.pts : b.pts, i, c, first ? a.counts : b.counts, first ? a.start : b.start, N, first ? a.sorted : b.sorted);
}

// ---- the two searches ---------------------------------------------------------------------------------------------------------

struct ChamferDir {      // Nq queries in their cloud's cell order against the Nd points of the other cloud in theirs
  const float4 *q;
  int Nq;
  const float4 *db;
  const int *start;
  int Nd;
  int32_t *idx;
  float *d2;
};

__device__ __forceinline__ void chamfer_store(const uint64_t best, const int Nd, int32_t *__restrict__ idx, float *__restrict__ d2,
                                              const size_t at) {
  const uint32_t pi = (uint32_t)(best & 0xffffffffull);
  const bool ok = best != ~0ull && pi < (uint32_t)Nd;
  idx[at] = ok ? (int32_t)pi : -1;
  d2[at] = ok ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
}

__global__ void __launch_bounds__(kChSearchBlock)
chamfer_search_kernel(const ChamferDir d0, const ChamferDir d1, const unsigned nb0, const ChamferHead *__restrict__ head) {
  const bool first = blockIdx.x < nb0;
  const size_t t = (size_t)(blockIdx.x - (first ? 0u : nb0)) * kChSearchBlock + threadIdx.x;
  const int Nq = first ? d0.Nq : d1.Nq, Nd = first ? d0.Nd : d1.Nd;
  if (t >= (size_t)Nq) return;      // (no barrier below)
  const float4 *__restrict__ sorted = first ? d0.db : d1.db;
  const int *__restrict__ start = first ? d0.start : d1.start;
  const float4 q = (first ? d0.q : d1.q)[t];
  const int qi = __float_as_int(q.w);
  if (qi < 0 || qi >= Nq) return;      // (every slot of the query array was filled with an index below Nq: a guard on the output row)
  const KnnGrid g = head->g;
  const int cx = knn_axis_cell(q.x, g.lox, g.inv, g.gx), cy = knn_axis_cell(q.y, g.loy, g.inv, g.gy),
            cz = knn_axis_cell(q.z, g.loz, g.inv, g.gz);
  uint64_t best = ~0ull;
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
          const int j0 = max(start[row + ca], 0), j1 = min(start[row + cb + 1], Nd);
          for (int j = j0; j < j1; ++j) {
            const float4 p = sorted[j];
            const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)__float_as_int(p.w);
            best = key < best ? key : best;
          }
        }
      }
    }
    if (best != ~0ull) {
      const float b = g.cell * ((float)r - 0x1p-10f) * (1.0f - 0x1p-20f);
      if (b > 0.0f && __uint_as_float((uint32_t)(best >> 32)) <= b * b) break;
    }
  }
  chamfer_store(best, Nd, first ? d0.idx : d1.idx, first ? d0.d2 : d1.d2, (size_t)qi);
}

// 64 queries a workgroup (lane = query), wave w takes entries [256 w, 256 w + 256) of every tile
__global__ void __launch_bounds__(256)
chamfer_brute_kernel(const float *__restrict__ qs, const int Nq, const float *__restrict__ db, const int Nd, int32_t *__restrict__ idx,
                     float *__restrict__ d2) {
  __shared__ float4 tile[kChTile];
  __shared__ uint64_t keys[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t qi = (size_t)blockIdx.x * 64 + lane;
  const size_t qr = qi < (size_t)Nq ? qi : (size_t)Nq - 1;      // (a lane past the end repeats the last query and writes nothing)
  const float qx = qs[3 * qr], qy = qs[3 * qr + 1], qz = qs[3 * qr + 2];
  uint64_t best = ~0ull;
  for (int t0 = 0; t0 < Nd; t0 += kChTile) {
    const int n = min(kChTile, Nd - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 256) {
      const float *p = db + 3 * ((size_t)t0 + k);
      tile[k] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    __syncthreads();
    const int k0 = wave * (kChTile / 4), k1 = min(k0 + kChTile / 4, n);
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
      const float4 p = tile[k];
      const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)(t0 + k);
      best = key < best ? key : best;
    }
  }
  keys[wave][lane] = best;
  __syncthreads();
  if (wave == 0 && qi < (size_t)Nq) {
    const uint64_t a = keys[0][lane], b = keys[1][lane], c = keys[2][lane], d = keys[3][lane];
    const uint64_t ab = a < b ? a : b, cd = c < d ? c : d;
    chamfer_store(ab < cd ? ab : cd, Nd, idx, d2, qi);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------

// workgroups [0, nbx): point i of x adds (y_nn(i) - x_i) 2^s to acc_y[nn(i)]; the rest: point j of y adds (x_nn(j) - y_j) 2^s to
// acc_x[nn(j)] (nn_y == nullptr, the single-directional form: no such workgroups)
__global__ void __launch_bounds__(256)
chamfer_scatter_kernel(const float *__restrict__ x, const int Nx, const float *__restrict__ y, const int Ny,
                       const int32_t *__restrict__ nn_x, const int32_t *__restrict__ nn_y, const int32_t *__restrict__ meta,
                       long long *__restrict__ acc_x, long long *__restrict__ acc_y, const unsigned nbx) {
  const bool first = blockIdx.x < nbx;
  const size_t i = (size_t)(blockIdx.x - (first ? 0u : nbx)) * 256 + threadIdx.x;
  const int Nown = first ? Nx : Ny, Nother = first ? Ny : Nx;
  if (i >= (size_t)Nown) return;
  const int j = (first ? nn_x : nn_y)[i];
  if (j < 0 || j >= Nother) return;
  const double scale = ldexp(1.0, meta[0]);
  const float *p = (first ? x : y) + 3 * i, *o = (first ? y : x) + 3 * (size_t)j;
  long long *acc = (first ? acc_y : acc_x) + 3 * (size_t)j;
  atomic_add_i64(acc, llrint((double)(o[0] - p[0]) * scale));
  atomic_add_i64(acc + 1, llrint((double)(o[1] - p[1]) * scale));
  atomic_add_i64(acc + 2, llrint((double)(o[2] - p[2]) * scale));
}

// one point a thread, x then y: g = G (w_gather (own - nearest) + w_scatter acc 2^-s), every element written
__global__ void __launch_bounds__(256)
chamfer_finish_kernel(const float *__restrict__ x, const int Nx, const float *__restrict__ y, const int Ny,
                      const int32_t *__restrict__ nn_x, const int32_t *__restrict__ nn_y, const int32_t *__restrict__ meta,
                      const long long *__restrict__ acc_x, const long long *__restrict__ acc_y, const float *__restrict__ g_loss,
                      const double w_x, const double w_y, float *__restrict__ g_x, float *__restrict__ g_y) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)Nx + (size_t)Ny) return;
  const bool first = t < (size_t)Nx;
  const size_t i = first ? t : t - (size_t)Nx;
  const int Nother = first ? Ny : Nx;
  const int32_t *nn = first ? nn_x : nn_y;
  const double G = (double)g_loss[0], unscale = ldexp(1.0, -meta[0]);
  const double w_gather = first ? w_x : w_y, w_scatter = first ? w_y : w_x;      // (a list into x holds points of y, weighted 2 / Ny)
  const float *p = (first ? x : y) + 3 * i;
  const long long *acc = (first ? acc_x : acc_y) + 3 * i;
  float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
  const int j = nn ? nn[i] : -1;
  if (j >= 0 && j < Nother) {
    const float *o = (first ? y : x) + 3 * (size_t)j;
    d0 = p[0] - o[0]; d1 = p[1] - o[1]; d2 = p[2] - o[2];
  }
  // (a member of the list added (its nearest - itself) = (this point - the member): the sign this point's gradient wants)
  float *g = (first ? g_x : g_y) + 3 * i;
  g[0] = (float)(G * (w_gather * (double)d0 + w_scatter * ((double)acc[0] * unscale)));
  g[1] = (float)(G * (w_gather * (double)d1 + w_scatter * ((double)acc[1] * unscale)));
  g[2] = (float)(G * (w_gather * (double)d2 + w_scatter * ((double)acc[2] * unscale)));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

enum { kChamferSum = 1, kChamferSingle = 2 };
enum { kRouteAuto = 0, kRouteBrute = 1, kRouteGrid = 2 };

struct ChamferLayout {
  size_t head, boxp, sorted[2], cellid[2], counts[2], start[2], bsum[2], d2[2], psum, pmax, total;
  long cap;
  int nb_scan, nb_box;
};
static ChamferLayout chamfer_layout(const long Nx, const long Ny) {
  ChamferLayout l;
  const long N[2] = {Nx, Ny}, n = Nx > Ny ? Nx : Ny;
  l.cap = grid_cell_cap(n);
  l.nb_scan = (int)((l.cap + kKnnScanBlock * kKnnScanItems - 1) / (kKnnScanBlock * kKnnScanItems));
  l.nb_box = (int)((Nx + Ny + 256 * kGridBoxItems - 1) / (256 * kGridBoxItems));
  const size_t nb_loss = chamfer_loss_blocks(Nx) + chamfer_loss_blocks(Ny);
  Carve c;
  l.head = c.take_exact(sizeof(ChamferHead));
  l.boxp = c.take((size_t)l.nb_box * 6 * sizeof(float));
  for (int k = 0; k < 2; ++k) {
    l.sorted[k] = c.take_exact((size_t)N[k] * 16);
    l.cellid[k] = c.take((size_t)N[k] * 4);
    l.counts[k] = c.take((size_t)l.cap * 4);
    l.start[k] = c.take((size_t)(l.cap + 1) * 4);
    l.bsum[k] = c.take((size_t)l.nb_scan * 4);
    l.d2[k] = c.take((size_t)N[k] * 4);
  }
  l.psum = c.take(nb_loss * sizeof(double));
  l.pmax = c.take(nb_loss * sizeof(float));
  const size_t bwd = (size_t)(Nx + Ny) * 3 * sizeof(long long);      // the backward's accumulators, a call of its own
  l.total = c.at > bwd ? c.at : bwd;
  return l;
}

static bool chamfer_sizes_ok(const long Nx, const long Ny) { return Nx >= 1 && Ny >= 1 && Nx <= kChamferMaxN && Ny <= kChamferMaxN; }

static bool chamfer_brute(const int route, const long Nx, const long Ny) {
  return route == kRouteBrute || (route == kRouteAuto && (double)Nx * (double)Ny <= kChamferBruteMaxPairs);
}

// the nearest point of y for every x (idx_x, d2_x) and -- both -- of x for every y; the pointers were validated by the caller
static void chamfer_searches(const float *x, const long Nx, const float *y, const long Ny, const bool brute, const float cell_size,
                             const bool both, int32_t *idx_x, float *d2_x, int32_t *idx_y, float *d2_y, char *ws, const ChamferLayout &l,
                             hipStream_t st) {
  if (brute) {
    hipLaunchKernelGGL(chamfer_brute_kernel, dim3((unsigned)((Nx + 63) / 64)), dim3(256), 0, st, x, (int)Nx, y, (int)Ny, idx_x, d2_x);
    if (both)
      hipLaunchKernelGGL(chamfer_brute_kernel, dim3((unsigned)((Ny + 63) / 64)), dim3(256), 0, st, y, (int)Ny, x, (int)Nx, idx_y, d2_y);
    return;
  }
  ChamferHead *head = reinterpret_cast<ChamferHead *>(ws + l.head);
  float *boxp = reinterpret_cast<float *>(ws + l.boxp);
  ChamferCloud c[2];
  const float *pts[2] = {x, y};
  const long N[2] = {Nx, Ny};
  int *bsum[2];
  for (int k = 0; k < 2; ++k) {
    c[k] = ChamferCloud{pts[k], (int)N[k], reinterpret_cast<int *>(ws + l.cellid[k]), reinterpret_cast<int *>(ws + l.counts[k]),
                        reinterpret_cast<int *>(ws + l.start[k]), reinterpret_cast<float4 *>(ws + l.sorted[k])};
    bsum[k] = reinterpret_cast<int *>(ws + l.bsum[k]);
  }
  const long n = Nx > Ny ? Nx : Ny;
  const unsigned nbx = blocks256(Nx), nby = blocks256(Ny);
  hipLaunchKernelGGL(grid_box_kernel, dim3((unsigned)l.nb_box), dim3(256), 0, st, x, (int)Nx, y, (int)Ny, boxp);
  hipLaunchKernelGGL(chamfer_grid_kernel, dim3(1), dim3(256), 0, st, boxp, l.nb_box, n, cell_size, head);
  hipLaunchKernelGGL(grid_zero_kernel, dim3(blocks256(l.cap)), dim3(256), 0, st, &head->G, c[0].counts, c[1].counts);
  hipLaunchKernelGGL(chamfer_count_kernel, dim3(nbx + nby), dim3(256), 0, st, c[0], c[1], nbx, head);
  for (int k = 0; k < 2; ++k) grid_scan_launch(c[k].counts, 0, &head->G, bsum[k], l.nb_scan, c[k].N, c[k].start, st);
  hipLaunchKernelGGL(chamfer_fill_kernel, dim3(nbx + nby), dim3(256), 0, st, c[0], c[1], nbx, head);
  const ChamferDir d0{c[0].sorted, (int)Nx, c[1].sorted, c[1].start, (int)Ny, idx_x, d2_x};
  const ChamferDir d1{c[1].sorted, (int)Ny, c[0].sorted, c[0].start, (int)Nx, idx_y, d2_y};
  const unsigned sb0 = (unsigned)((Nx + kChSearchBlock - 1) / kChSearchBlock);
  const unsigned sb1 = both ? (unsigned)((Ny + kChSearchBlock - 1) / kChSearchBlock) : 0u;
  hipLaunchKernelGGL(chamfer_search_kernel, dim3(sb0 + sb1), dim3(kChSearchBlock), 0, st, d0, d1, sb0, head);
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_chamfer_workspace_bytes(long Nx, long Ny) {
  if (!chamfer_sizes_ok(Nx, Ny)) return 0;
  return chamfer_layout(Nx, Ny).total;
}

extern "C" int voge_nearest_points(const float *queries, long Nq, const float *points, long Np, int route, float cell_size,
                                   int32_t *idx, float *d2, void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (Nq < 0 || Nq > kChamferMaxN || Np < 1 || Np > kChamferMaxN || route < kRouteAuto || route > kRouteGrid) return VOGE_ERR_BAD_ARG;
  if (!(cell_size >= 0.0f) || !(cell_size < INFINITY)) return VOGE_ERR_BAD_ARG;      // (0: the default cell)
  if (Nq == 0) return 0;
  if (!queries || !points || !idx || !d2 || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const ChamferLayout l = chamfer_layout(Nq, Np);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  chamfer_searches(queries, Nq, points, Np, chamfer_brute(route, Nq, Np), cell_size, false, idx, d2, nullptr, nullptr,
                   static_cast<char *>(workspace), l, (hipStream_t)stream);
  return launch_status();
}

extern "C" int voge_chamfer_fwd(const float *x, long Nx, const float *y, long Ny, int route, int flags, float *loss, int32_t *nn_x,
                                int32_t *nn_y, int32_t *meta, void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (!chamfer_sizes_ok(Nx, Ny) || route < kRouteAuto || route > kRouteGrid || (flags & ~3)) return VOGE_ERR_BAD_ARG;
  const bool both = !(flags & kChamferSingle);
  if (!x || !y || !loss || !nn_x || (both && !nn_y) || !meta || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const ChamferLayout l = chamfer_layout(Nx, Ny);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  float *d2x = reinterpret_cast<float *>(ws + l.d2[0]), *d2y = reinterpret_cast<float *>(ws + l.d2[1]);
  chamfer_searches(x, Nx, y, Ny, chamfer_brute(route, Nx, Ny), 0.0f, both, nn_x, d2x, nn_y, d2y, ws, l, st);
  // max(Nx, Ny): every scatter list of the backward -- the points of one cloud that name one point of the other
  chamfer_loss_launch(d2x, Nx, d2y, Ny, both, flags & kChamferSum, Nx > Ny ? Nx : Ny, reinterpret_cast<double *>(ws + l.psum),
                      reinterpret_cast<float *>(ws + l.pmax), loss, meta, st);
  return launch_status();
}

extern "C" int voge_chamfer_bwd(const float *x, long Nx, const float *y, long Ny, const int32_t *nn_x, const int32_t *nn_y,
                                const int32_t *meta, const float *g_loss, int flags, float *g_x, float *g_y, void *workspace,
                                size_t workspace_bytes, voge_stream_t stream) {
  if (!chamfer_sizes_ok(Nx, Ny) || (flags & ~3)) return VOGE_ERR_BAD_ARG;
  const bool both = !(flags & kChamferSingle);
  if (!x || !y || !nn_x || (both && !nn_y) || !meta || !g_loss || !g_x || !g_y || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const size_t acc_bytes = (size_t)(Nx + Ny) * 3 * sizeof(long long);
  if (workspace_bytes < acc_bytes) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  long long *acc_x = static_cast<long long *>(workspace), *acc_y = acc_x + 3 * (size_t)Nx;
  const hipError_t fe = voge_fill_async(workspace, 0, acc_bytes, st);
  if (fe != hipSuccess) return (int)fe;
  const unsigned nbx = blocks256(Nx), nby = both ? blocks256(Ny) : 0u;
  hipLaunchKernelGGL(chamfer_scatter_kernel, dim3(nbx + nby), dim3(256), 0, st, x, (int)Nx, y, (int)Ny, nn_x, both ? nn_y : nullptr, meta,
                     acc_x, acc_y, nbx);
  const bool sum = flags & kChamferSum;
  const double w_x = sum ? 2.0 : 2.0 / (double)Nx, w_y = both ? (sum ? 2.0 : 2.0 / (double)Ny) : 0.0;
  hipLaunchKernelGGL(chamfer_finish_kernel, dim3(blocks256(Nx + Ny)), dim3(256), 0, st, x, (int)Nx, y, (int)Ny, nn_x,
                     both ? nn_y : nullptr, meta, acc_x, acc_y, g_loss, w_x, w_y, g_x, g_y);
  return launch_status();
}
