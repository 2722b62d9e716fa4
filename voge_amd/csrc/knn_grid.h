// The uniform grid of the searches (knn.hip: neighbours inside one cloud; chamfer.hip: nearest points between two clouds;
// point_mesh_grid.h: points against triangles and back) -- everything but the walks over the rings of cells, which each file
// keeps next to the stopping rule its header derives:
//   the grid and a point's cell (KnnGrid, knn_axis_cell, grid_cell_of);
//   the grid chosen ON THE DEVICE (grid_box_kernel, grid_box_reduce, grid_choose: the rule of ops.knn_grid) and the cap on its cells
//   (grid_cell_cap), which sizes the workspaces and the launches;
//   binning: grid_zero_kernel, the count and fill steps of a point (grid_count_point, grid_claim_row, grid_fill_point) and the
//   exclusive scan of the per-cell counts in three launches (grid_scan_launch).
#pragma once
#include <math.h>

#include "voge_common.h"

namespace voge {

constexpr int kKnnMaxAxis = 1024;
constexpr int kKnnScanBlock = 256;
constexpr int kKnnScanItems = 8;          // cells a thread of the scan: 2048 a workgroup
constexpr int kGridBoxItems = 8;          // points a thread of the box pass: 2048 a workgroup
constexpr int kGridTrips = 64;            // enlargements of the cell grid_choose tries

struct KnnGrid {
  float lox, loy, loz, cell, inv;
  int gx, gy, gz;
};

// the most cells a grid for at most n items may have (ops.knn_grid's cap; G and G + 1 stay ints)
__host__ __device__ inline long grid_cell_cap(const long n) {
  const long cap = 8 * n > 32768l ? 8 * n : 32768l;
  return cap < 2147483646l ? cap : 2147483646l;
}

// (the clamp happens in float: the same value as clamping the converted integer for every in-range input, and a NaN or an
// infinity lands on a valid cell instead of an undefined conversion)
__device__ __forceinline__ int knn_axis_cell(const float x, const float lo, const float inv, const int g) {
  const float u = floorf((x - lo) * inv);
  return (int)fminf(fmaxf(u, 0.0f), (float)(g - 1));
}

// the cell of a position, x fastest
__device__ __forceinline__ int grid_cell_of(const KnnGrid &g, const float x, const float y, const float z) {
  const int cx = knn_axis_cell(x, g.lox, g.inv, g.gx), cy = knn_axis_cell(y, g.loy, g.inv, g.gy), cz = knn_axis_cell(z, g.loz, g.inv, g.gz);
  return (cz * g.gy + cy) * g.gx + cx;
}

// ---- the grid, chosen on the device -------------------------------------------------------------------------------------------

// the bounding box of x [Nx][3] and y [Ny][3] together, six floats a workgroup (fminf / fmaxf drop a NaN: a cloud with some NaN
// coordinates still gets the box of its numbers)
static __global__ void __launch_bounds__(256)
grid_box_kernel(const float *__restrict__ x, const int Nx, const float *__restrict__ y, const int Ny, float *__restrict__ partial) {
  const size_t n = (size_t)Nx + (size_t)Ny;
  float lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;
#pragma unroll
  for (int k = 0; k < kGridBoxItems; ++k) {
    const size_t i = ((size_t)blockIdx.x * kGridBoxItems + k) * 256 + threadIdx.x;
    if (i < n) {
      const float *p = i < (size_t)Nx ? x + 3 * i : y + 3 * (i - (size_t)Nx);
      const float a = p[0], b = p[1], c = p[2];
      lo0 = fminf(lo0, a); lo1 = fminf(lo1, b); lo2 = fminf(lo2, c);
      hi0 = fmaxf(hi0, a); hi1 = fmaxf(hi1, b); hi2 = fmaxf(hi2, c);
    }
  }
  lo0 = wave_min(lo0); lo1 = wave_min(lo1); lo2 = wave_min(lo2);
  hi0 = wave_max(hi0); hi1 = wave_max(hi1); hi2 = wave_max(hi2);
  __shared__ float red[4][6];
  if ((threadIdx.x & 63) == 0) {
    float *r = red[threadIdx.x >> 6];
    r[0] = lo0; r[1] = lo1; r[2] = lo2; r[3] = hi0; r[4] = hi1; r[5] = hi2;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    const float a = red[0][c], b = red[1][c], d = red[2][c], e = red[3][c];
    partial[(size_t)blockIdx.x * 6 + c] = c < 3 ? fminf(fminf(a, b), fminf(d, e)) : fmaxf(fmaxf(a, b), fmaxf(d, e));
  }
}

// ONE workgroup of 256, every thread calls (a barrier inside): the box of the nb partial boxes, in thread 0's lo / hi
__device__ __forceinline__ void grid_box_reduce(const float *__restrict__ partial, const int nb, float lo[3], float hi[3]) {
  float lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += 256) {
    const float *p = partial + (size_t)i * 6;
    lo0 = fminf(lo0, p[0]); lo1 = fminf(lo1, p[1]); lo2 = fminf(lo2, p[2]);
    hi0 = fmaxf(hi0, p[3]); hi1 = fmaxf(hi1, p[4]); hi2 = fmaxf(hi2, p[5]);
  }
  lo0 = wave_min(lo0); lo1 = wave_min(lo1); lo2 = wave_min(lo2);
  hi0 = wave_max(hi0); hi1 = wave_max(hi1); hi2 = wave_max(hi2);
  __shared__ float red[4][6];
  if ((threadIdx.x & 63) == 0) {
    float *r = red[threadIdx.x >> 6];
    r[0] = lo0; r[1] = lo1; r[2] = lo2; r[3] = hi0; r[4] = hi1; r[5] = hi2;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int c = 0; c < 3; ++c) {
    lo[c] = fminf(fminf(red[0][c], red[1][c]), fminf(red[2][c], red[3][c]));
    hi[c] = fmaxf(fmaxf(red[0][c + 3], red[1][c + 3]), fmaxf(red[2][c + 3], red[3][c + 3]));
  }
}

// The rule of ops.knn_grid, one thread: about 2 n cubic cells in the box lo .. hi, cell >= max extent / 1023, G_a = floor(extent_a /
// cell) + 1 <= 1024 on every axis, G = Gx Gy Gz <= grid_cell_cap(n); the loop that enlarges the cell has kGridTrips trips at most,
// and a box that is not finite or a loop that did not end gives the one-cell grid (every item a candidate of ring 0: a brute
// force).  cell_size > 0 asks for a cell of that size, which goes through the same enlargement; default_floor > 0 is a floor on
// the DEFAULT cell only.
__device__ __forceinline__ void grid_choose(const float lo[3], const float hi[3], const long n, const float cell_size,
                                            const double default_floor, KnnGrid &grid, int &G) {
  double ext[3], mx = 0.0;
  bool fin = true;
  for (int c = 0; c < 3; ++c) {
    const float e = hi[c] - lo[c];
    fin = fin && fabsf(lo[c]) < INFINITY && fabsf(hi[c]) < INFINITY && fabsf(e) < INFINITY;
    ext[c] = e > 0.0f ? (double)e : 0.0;
    mx = fmax(mx, ext[c]);
  }
  grid = KnnGrid{fin ? lo[0] : 0.0f, fin ? lo[1] : 0.0f, fin ? lo[2] : 0.0f, 1.0f, 1.0f, 1, 1, 1};      // the one-cell fallback
  G = 1;
  if (!fin) return;
  const double cap = (double)grid_cell_cap(n);
  double cell;
  if (cell_size > 0.0f && cell_size < INFINITY) {
    cell = (double)cell_size;
  } else {
    int np = 0;
    double vol = 1.0;
    for (int c = 0; c < 3; ++c)
      if (ext[c] > 0.0) { vol *= ext[c]; ++np; }
    cell = np ? pow(vol / (2.0 * (double)(n > 1 ? n : 1)), 1.0 / (double)np) : 1.0;
    if (default_floor > 0.0) cell = fmax(cell, default_floor);
  }
  cell = fmax(cell, fmax(mx / 1023.0, 1e-30));
  for (int trip = 0; trip < kGridTrips; ++trip) {
    const float cf = (float)cell;
    const float inv = 1.0f / cf;
    if (!(cf > 0.0f) || !(cf < INFINITY) || !(inv > 0.0f) || !(inv < INFINITY)) break;
    double cells = 1.0;
    bool fits = true;
    int g[3];
    for (int c = 0; c < 3; ++c) {
      const double q = floor(ext[c] / (double)cf) + 1.0;
      fits = fits && q <= (double)kKnnMaxAxis;
      g[c] = (int)fmin(q, (double)kKnnMaxAxis);
      cells *= q;
    }
    if (fits && cells <= cap) {
      grid.cell = cf; grid.inv = inv;
      grid.gx = g[0]; grid.gy = g[1]; grid.gz = g[2];
      G = g[0] * g[1] * g[2];
      break;
    }
    cell = (double)cf * fmax(1.05, cbrt(cells / cap));      // (every round grows the cell)
  }
}

// ---- binning ------------------------------------------------------------------------------------------------------------------

// the counts of two tables binned in one grid of *G cells (launched for the cap on G)
static __global__ void __launch_bounds__(256)
grid_zero_kernel(const int *__restrict__ G, int *__restrict__ c0, int *__restrict__ c1) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)*G) return;
  c0[i] = 0;
  c1[i] = 0;
}

// the count step of point i of pts [N][3]: its cell, kept per point, and an integer atomic count per cell
__device__ __forceinline__ void grid_count_point(const KnnGrid &g, const float *__restrict__ pts, const size_t i, int *__restrict__ cellid,
                                                 int *__restrict__ counts) {
  const float *p = pts + 3 * i;
  const int c = grid_cell_of(g, p[0], p[1], p[2]);
  cellid[i] = c;
  atomicAdd(counts + c, 1);
}

// the fill step's slot claim: counts[c] falls back to zero, one slot an item -- the value after the decrement, in [0, count) -- ->
// the item's row of the cell-ordered table of N rows, or -1 (cannot happen after the count pass over the same cells: a guard, not a
// route).  The order INSIDE a cell depends on the atomics' arrival: it decides which lane serves which query, never a result.
__device__ __forceinline__ int grid_claim_row(int *__restrict__ counts, const int *__restrict__ start, const int c, const int N) {
  const int slot = atomicSub(counts + c, 1) - 1;
  const int pos = start[c] + slot;
  return slot < 0 || pos < 0 || pos >= N ? -1 : pos;
}

// the fill step of point i, whose cell is c: (x, y, z, index bits) into its row
__device__ __forceinline__ void grid_fill_point(const float *__restrict__ pts, const size_t i, const int c, int *__restrict__ counts,
                                                const int *__restrict__ start, const int N, float4 *__restrict__ sorted) {
  const int pos = grid_claim_row(counts, start, c, N);
  if (pos < 0) return;
  const float *p = pts + 3 * i;
  sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));
}

// exclusive scan of one int per thread over a workgroup of full waves; total: the workgroup's sum.  red: one int per wave.
__device__ __forceinline__ int knn_block_excl_scan(const int v, int *red, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int incl = wave_incl_scan_i32(v);
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const int s = red[w];
    off += w < wave ? s : 0;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return off + incl - v;
}

// The scan kernels take the number of cells G as an argument, or -- Gdev != nullptr -- read it from device memory: a caller that
// chose its grid on the device sizes the launches for the most cells the grid can have, and the workgroups past the real G find
// nothing to add (their sums are zero, they write nothing).
__device__ __forceinline__ int knn_scan_cells(const int G, const int *__restrict__ Gdev) { return Gdev ? *Gdev : G; }

static __global__ void __launch_bounds__(kKnnScanBlock)
knn_scan_partial_kernel(const int *__restrict__ counts, const int Garg, const int *__restrict__ Gdev, int *__restrict__ bsum) {
  __shared__ int red[kKnnScanBlock / 64];
  const int G = knn_scan_cells(Garg, Gdev);
  const size_t base = ((size_t)blockIdx.x * kKnnScanBlock + threadIdx.x) * kKnnScanItems;
  int s = 0;
#pragma unroll
  for (int j = 0; j < kKnnScanItems; ++j) s += base + j < (size_t)G ? counts[base + j] : 0;
  int total;
  knn_block_excl_scan(s, red, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup of 1024: bsum [nb] -> its exclusive scan, in place, 1024 entries a step with the carry in a register
static __global__ void __launch_bounds__(1024)
knn_scan_sums_kernel(int *__restrict__ bsum, const int nb) {
  __shared__ int red[16];
  int carry = 0;
  for (int s0 = 0; s0 < nb; s0 += 1024) {
    const int i = s0 + (int)threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int total;
    const int ex = knn_block_excl_scan(v, red, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
}

static __global__ void __launch_bounds__(kKnnScanBlock)
knn_scan_final_kernel(const int *__restrict__ counts, const int Garg, const int *__restrict__ Gdev, const int *__restrict__ bsum,
                      const int N, int *__restrict__ start) {
  __shared__ int red[kKnnScanBlock / 64];
  const int G = knn_scan_cells(Garg, Gdev);
  const size_t base = ((size_t)blockIdx.x * kKnnScanBlock + threadIdx.x) * kKnnScanItems;
  int c[kKnnScanItems], s = 0;
#pragma unroll
  for (int j = 0; j < kKnnScanItems; ++j) {
    c[j] = base + j < (size_t)G ? counts[base + j] : 0;
    s += c[j];
  }
  int total;
  int run = knn_block_excl_scan(s, red, total) + bsum[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kKnnScanItems; ++j) {
    if (base + j < (size_t)G) start[base + j] = run;
    run += c[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) start[G] = N;
}

// the scan of one count table of N items: counts [G] -> start [G + 1]; nb workgroups of 2048 cells cover G, or the cap on *Gdev
static void grid_scan_launch(const int *counts, const int G, const int *Gdev, int *bsum, const int nb, const int N, int *start,
                             hipStream_t st) {
  hipLaunchKernelGGL(knn_scan_partial_kernel, dim3((unsigned)nb), dim3(kKnnScanBlock), 0, st, counts, G, Gdev, bsum);
  hipLaunchKernelGGL(knn_scan_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb);
  hipLaunchKernelGGL(knn_scan_final_kernel, dim3((unsigned)nb), dim3(kKnnScanBlock), 0, st, counts, G, Gdev, bsum, N, start);
}

}  // namespace voge
