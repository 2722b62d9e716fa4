// The order-independent sum of the geometry units: fixed-point terms added with 64-bit INTEGER atomics (atomic_add_i64), so the
// bits depend on no order of arrival.  Largest |x| -> scale exponent -> scatter -> finish:
//   * a launch of the unit's own finds D = the largest |x| of the terms, as bits (|x| >= 0 orders as its bits do, a NaN lies above
//     the infinity, and a maximum has no order): every wave ends in fixed_commit_max;
//   * scatter and finish both derive s from D and from L, 2^L >= the longest list of terms one accumulator can receive
//     (ceil_log2 on the host; every site says which n bounds its lists): round(x 2^s) is added, the sum times 2^-s is the result.
// THE BOUND.  s = 62 - L - e with 2^e > D (frexp: D = f 2^e, f in [0.5, 1), e = 0 for D = 0).  A term |x| <= D rounds to
// |round(x 2^s)| <= D 2^s + 1/2 < 2^(62 - L) + 1, and at most n <= 2^L of them meet: |sum| < 2^62 + n, n <= 2^30 -- inside int64.
// One term is off by at most half a quantum, q = 2^-s <= 2^(L - 61) D.
// No kernels here: a `static __global__` in a header is emitted by every unit that includes it.
#pragma once
#include <math.h>

#include "voge_common.h"

namespace voge {

struct FixedHead {      // a fixed-point workspace's first 16 bytes, zero-filled with the accumulators
  uint32_t dmax_bits;
  uint32_t pad[3];
};

// the end of an absmax kernel: m = this lane's largest bits -> the wave's -> one atomic max a wave (none for 0: the fill's value)
__device__ __forceinline__ void fixed_commit_max(FixedHead *__restrict__ head, uint32_t m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(&head->dmax_bits, m);
}

// s = 62 - L - e, 2^e > D, for a finite D >= 0 (THE BOUND above)
__device__ __forceinline__ int fixed_exponent(const double D, const int list_bits) {
  int e;
  frexp(D, &e);      // D = f 2^e, f in [0.5, 1), e = 0 for D = 0
  return 62 - list_bits - e;
}

// s of a head's D; a D that is not finite: 0, the values are out of contract.  The clamp is unreachable -- a finite fp32 D has
// e in [-148, 128] and list_bits <= 30, so s is in [-96, 210] -- and stays: it is part of the kernels' code as measured.
__device__ __forceinline__ int fixed_scale_exponent(const FixedHead *__restrict__ head, const int list_bits) {
  const float D = __uint_as_float(head->dmax_bits);
  if (!(D < INFINITY)) return 0;
  const int s = fixed_exponent((double)D, list_bits);
  return s < -1000 ? -1000 : (s > 1000 ? 1000 : s);
}

}  // namespace voge
