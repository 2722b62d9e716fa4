// What the two grid searches share (knn.hip: neighbours inside one cloud; chamfer.hip: nearest points between two clouds): the
// uniform grid, a point's cell on an axis, and the exclusive scan of the per-cell counts in three launches.
#pragma once
#include <math.h>

#include "voge_common.h"

namespace voge {

constexpr int kKnnMaxAxis = 1024;
constexpr int kKnnScanBlock = 256;
constexpr int kKnnScanItems = 8;          // cells a thread of the scan: 2048 a workgroup

struct KnnGrid {
  float lox, loy, loz, cell, inv;
  int gx, gy, gz;
};

// (the clamp happens in float: the same value as clamping the converted integer for every in-range input, and a NaN or an
// infinity lands on a valid cell instead of an undefined conversion)
__device__ __forceinline__ int knn_axis_cell(const float x, const float lo, const float inv, const int g) {
  const float u = floorf((x - lo) * inv);
  return (int)fminf(fmaxf(u, 0.0f), (float)(g - 1));
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

}  // namespace voge
