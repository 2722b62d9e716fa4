// The loss of two lists of fp32 squared distances: fp64 partial sums, ONE workgroup that adds them in an order fixed by the
// shapes, one rounding -- and the scale exponent of the fixed-point backward that follows.  Shared by chamfer.hip (two clouds)
// and point_mesh.hip (a cloud and a mesh's faces).
#pragma once
#include <math.h>

#include "voge_common.h"
#include "fixed_point.h"

namespace voge {

constexpr int kChLossItems = 4;         // d2 a thread of the partial sums: 1024 a workgroup

__device__ __forceinline__ double chamfer_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// workgroups [0, nba): d2a, the rest: d2b; one fp64 sum and the largest d2 a workgroup
static __global__ void __launch_bounds__(256)
chamfer_loss_partial_kernel(const float *__restrict__ d2a, const int Na, const float *__restrict__ d2b, const int Nb, const unsigned nba,
                            double *__restrict__ psum, float *__restrict__ pmax) {
  const bool first = blockIdx.x < nba;
  const float *__restrict__ d = first ? d2a : d2b;
  const int N = first ? Na : Nb;
  const size_t base = (size_t)(blockIdx.x - (first ? 0u : nba)) * (256 * kChLossItems) + threadIdx.x;
  double s = 0.0;
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < kChLossItems; ++k) {
    const size_t i = base + (size_t)k * 256;
    const float v = i < (size_t)N ? d[i] : 0.0f;
    s += (double)v;
    m = fmaxf(m, v);
  }
  s = chamfer_wave_sum_f64(s);
  m = wave_max(m);
  __shared__ double rs[4];
  __shared__ float rm[4];
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rm[threadIdx.x >> 6] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
    pmax[blockIdx.x] = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
  }
}

// ONE workgroup: loss = sum_a / div_a + sum_b / div_b in fp64, rounded once; meta[0] = the backward's scale exponent s:
// with D = sqrt(max d2 (1 + 2^-20) + 2^-148) < 2^e and every scatter list at most 2^list_bits long, s = 62 - list_bits - e
// (fixed_point.h's rule on a double D, without the head and without the clamp)
static __global__ void __launch_bounds__(256)
chamfer_loss_final_kernel(const double *__restrict__ psum, const float *__restrict__ pmax, const unsigned nba, const unsigned nbb,
                          const double div_a, const double div_b, const int list_bits, float *__restrict__ loss,
                          int32_t *__restrict__ meta) {
  double sa = 0.0, sb = 0.0;
  float m = 0.0f;
  for (unsigned i = threadIdx.x; i < nba; i += 256) { sa += psum[i]; m = fmaxf(m, pmax[i]); }
  for (unsigned i = threadIdx.x; i < nbb; i += 256) { sb += psum[nba + i]; m = fmaxf(m, pmax[nba + i]); }
  __shared__ double red[2][256];
  __shared__ float redm[256];
  red[0][threadIdx.x] = sa; red[1][threadIdx.x] = sb; redm[threadIdx.x] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      redm[threadIdx.x] = fmaxf(redm[threadIdx.x], redm[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  loss[0] = (float)(red[0][0] / div_a + (nbb ? red[1][0] / div_b : 0.0));
  int s = 0;
  const double D = sqrt((double)redm[0] * (1.0 + 0x1p-20) + 0x1p-148);
  if (D < (double)INFINITY) s = fixed_exponent(D, list_bits);      // (false for a NaN too: s = 0, the values are out of contract)
  meta[0] = s; meta[1] = 0; meta[2] = 0; meta[3] = 0;
}

// workgroups of chamfer_loss_partial_kernel for a list of n distances: one psum and one pmax entry each
static inline unsigned chamfer_loss_blocks(const long n) { return (unsigned)((n + 256 * kChLossItems - 1) / (256 * kChLossItems)); }

// The loss tail of a forward, two launches: the partial sums of d2a [Na] and -- both -- d2b [Nb], then the one workgroup that writes
// loss = sum_a / Na + sum_b / Nb (sum: the plain sums) and meta.  list_bound: no scatter list of the backward is longer (the caller
// says why).  psum and pmax hold chamfer_loss_blocks(Na) + chamfer_loss_blocks(Nb) entries.
static inline void chamfer_loss_launch(const float *d2a, const long Na, const float *d2b, const long Nb, const bool both, const bool sum,
                                       const long list_bound, double *psum, float *pmax, float *loss, int32_t *meta, hipStream_t st) {
  const unsigned nba = chamfer_loss_blocks(Na), nbb = both ? chamfer_loss_blocks(Nb) : 0u;
  hipLaunchKernelGGL(chamfer_loss_partial_kernel, dim3(nba + nbb), dim3(256), 0, st, d2a, (int)Na, d2b, (int)Nb, nba, psum, pmax);
  hipLaunchKernelGGL(chamfer_loss_final_kernel, dim3(1), dim3(256), 0, st, psum, pmax, nba, nbb, sum ? 1.0 : (double)Na,
                     sum ? 1.0 : (double)Nb, ceil_log2(list_bound), loss, meta);
}

}  // namespace voge
