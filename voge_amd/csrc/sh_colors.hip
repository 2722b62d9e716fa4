// View-dependent colours (EXTENSION: the reference has no spherical-harmonic code).  For view b and Gaussian n, with
// delta = v - c_b and d = delta / |delta| (d = 0 where |delta|^2 <= 1e-20):
//   pre[b,n,:] = sum_{m < (degree+1)^2} Y_m(d) sh[n,m,:] + 0.5,   out = max(pre, 0) (clamp) | pre
// with the sixteen orthonormal real SH of degree <= 3 in the order and with the signs of Aggregation.sh_colors.
// One thread owns one Gaussian and walks the views in order: the M * C coefficients (forward) and their gradient sums
// (backward) stay in registers, the coefficient row is read once however many views there are, and every sum over the views has
// a fixed association -- no atomics, the same bits on every run.  M and C are compile-time (every loop over them is unrolled:
// nothing is indexed at run time, nothing goes to scratch); the active degree is a run-time, wave-uniform argument.
#include "voge_common.h"

namespace voge {

constexpr float kShC0 = 0.28209479177387814f;
constexpr float kShC1 = 0.4886025119029199f;
constexpr float kShC2a = 1.0925484305920792f, kShC2b = 0.31539156525252005f, kShC2c = 0.5462742152960396f;
constexpr float kShC3a = 0.5900435899266435f, kShC3b = 2.890611442640554f, kShC3c = 0.4570457994644658f,
                kShC3d = 0.3731763325901154f, kShC3e = 1.445305721320277f;
constexpr float kShTiny = 1e-20f;      // |delta|^2 at or below this: no direction

// Y_0 .. Y_{M-1} at the unit vector (x, y, z)
template <int M>
__device__ __forceinline__ void sh_basis(const float x, const float y, const float z, float (&Y)[M]) {
  Y[0] = kShC0;
  if constexpr (M >= 4) {
    Y[1] = -kShC1 * y;
    Y[2] = kShC1 * z;
    Y[3] = -kShC1 * x;
  }
  if constexpr (M >= 9) {
    const float xx = x * x, yy = y * y, zz = z * z;
    Y[4] = kShC2a * (x * y);
    Y[5] = -kShC2a * (y * z);
    Y[6] = kShC2b * (fmaf(2.0f, zz, -xx) - yy);
    Y[7] = -kShC2a * (x * z);
    Y[8] = kShC2c * (xx - yy);
    if constexpr (M >= 16) {
      const float q = fmaf(4.0f, zz, -xx) - yy;      // 4zz - xx - yy
      Y[9] = -kShC3a * (y * fmaf(3.0f, xx, -yy));
      Y[10] = kShC3b * ((x * y) * z);
      Y[11] = -kShC3c * (y * q);
      Y[12] = kShC3d * (z * (fmaf(2.0f, zz, -3.0f * xx) - 3.0f * yy));
      Y[13] = -kShC3c * (x * q);
      Y[14] = kShC3e * (z * (xx - yy));
      Y[15] = -kShC3a * (x * fmaf(-3.0f, yy, xx));
    }
  }
}

// (gx, gy, gz) = sum_m G_m grad Y_m at (x, y, z): the gradient of the polynomials as written above (their radial part is removed
// by the projection in the caller)
template <int M>
__device__ __forceinline__ void sh_basis_grad(const float x, const float y, const float z, const float (&G)[M], float &gx, float &gy,
                                              float &gz) {
  gx = gy = gz = 0.0f;
  if constexpr (M >= 4) {
    gy = -kShC1 * G[1];
    gz = kShC1 * G[2];
    gx = -kShC1 * G[3];
  }
  if constexpr (M >= 9) {
    const float a4 = kShC2a * G[4], a5 = -kShC2a * G[5], a6 = kShC2b * G[6], a7 = -kShC2a * G[7], a8 = kShC2c * G[8];
    gx = fmaf(a4, y, gx);  gy = fmaf(a4, x, gy);
    gy = fmaf(a5, z, gy);  gz = fmaf(a5, y, gz);
    gx = fmaf(a6, -2.0f * x, gx);  gy = fmaf(a6, -2.0f * y, gy);  gz = fmaf(a6, 4.0f * z, gz);
    gx = fmaf(a7, z, gx);  gz = fmaf(a7, x, gz);
    gx = fmaf(a8, 2.0f * x, gx);  gy = fmaf(a8, -2.0f * y, gy);
    if constexpr (M >= 16) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
      const float a9 = -kShC3a * G[9], a10 = kShC3b * G[10], a11 = -kShC3c * G[11], a12 = kShC3d * G[12], a13 = -kShC3c * G[13],
                  a14 = kShC3e * G[14], a15 = -kShC3a * G[15];
      const float d3 = 3.0f * (xx - yy);
      gx = fmaf(a9, 6.0f * xy, gx);  gy = fmaf(a9, d3, gy);
      gx = fmaf(a10, yz, gx);  gy = fmaf(a10, xz, gy);  gz = fmaf(a10, xy, gz);
      gx = fmaf(a11, -2.0f * xy, gx);  gy = fmaf(a11, fmaf(4.0f, zz, -xx) - 3.0f * yy, gy);  gz = fmaf(a11, 8.0f * yz, gz);
      gx = fmaf(a12, -6.0f * xz, gx);  gy = fmaf(a12, -6.0f * yz, gy);  gz = fmaf(a12, fmaf(6.0f, zz, -3.0f * xx) - 3.0f * yy, gz);
      gx = fmaf(a13, fmaf(4.0f, zz, -3.0f * xx) - yy, gx);  gy = fmaf(a13, -2.0f * xy, gy);  gz = fmaf(a13, 8.0f * xz, gz);
      gx = fmaf(a14, 2.0f * xz, gx);  gy = fmaf(a14, -2.0f * yz, gy);  gz = fmaf(a14, xx - yy, gz);
      gx = fmaf(a15, d3, gx);  gy = fmaf(a15, -6.0f * xy, gy);
    }
  }
}

// a Gaussian's M * C coefficients: 16-byte loads where the row length allows it (rows are then 16-byte aligned: the entry checks the
// base), a scalar walk otherwise; the coefficients above the active degree read as zero whatever the array holds there
template <int M, int C>
__device__ __forceinline__ void sh_load_row(const float *__restrict__ row, const int active, float (&s)[M * C]) {
  constexpr int NF = M * C;
  if constexpr (NF % 4 == 0) {
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int i = 0; i < NF / 4; ++i) {
      const float4 v = r4[i];
      s[4 * i] = v.x; s[4 * i + 1] = v.y; s[4 * i + 2] = v.z; s[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NF; ++i) s[i] = row[i];
  }
#pragma unroll
  for (int m = 1; m < M; ++m)
#pragma unroll
    for (int c = 0; c < C; ++c) s[m * C + c] = m < active ? s[m * C + c] : 0.0f;
}

template <int M, int C>
__device__ __forceinline__ void sh_store_row(float *__restrict__ row, const float (&s)[M * C]) {
  constexpr int NF = M * C;
  if constexpr (NF % 4 == 0) {
    float4 *r4 = reinterpret_cast<float4 *>(row);
#pragma unroll
    for (int i = 0; i < NF / 4; ++i) r4[i] = make_float4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < NF; ++i) row[i] = s[i];
  }
}

// unit direction from the camera centre to the Gaussian and 1 / |delta| (both zero where there is no direction)
__device__ __forceinline__ void sh_direction(const float vx, const float vy, const float vz, const float *__restrict__ c, float &x,
                                             float &y, float &z, float &inv) {
  const float dx = vx - c[0], dy = vy - c[1], dz = vz - c[2];
  const float n2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  inv = n2 > kShTiny ? 1.0f / sqrtf(n2) : 0.0f;
  x = dx * inv; y = dy * inv; z = dz * inv;
}

template <int M, int C>
__global__ void __launch_bounds__(64)
sh_colors_fwd_kernel(const float *__restrict__ sh, const float *__restrict__ verts, const float *__restrict__ centres, const int B,
                     const int N, const int active, const int shared, const int clamp, float *__restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  float s[M * C];
  sh_load_row<M, C>(sh + (size_t)n * (M * C), active, s);
  for (int b = 0; b < B; ++b) {
    const float *v = verts + 3 * ((shared ? (size_t)0 : (size_t)b * N) + n);
    float x, y, z, inv, Y[M];
    sh_direction(v[0], v[1], v[2], centres + 3 * b, x, y, z, inv);
    sh_basis<M>(x, y, z, Y);
    float *o = out + ((size_t)b * N + n) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float pre = 0.0f;
#pragma unroll
      for (int m = M - 1; m >= 1; --m) pre = fmaf(Y[m], s[m * C + c], pre);      // highest degree first, the constant term last
      pre = fmaf(Y[0], s[c], pre) + 0.5f;
      o[c] = clamp ? fmaxf(pre, 0.0f) : pre;
    }
  }
}

template <int M, int C>
__global__ void __launch_bounds__(64)
sh_colors_bwd_kernel(const float *__restrict__ sh, const float *__restrict__ verts, const float *__restrict__ centres,
                     const float *__restrict__ g_out, const int B, const int N, const int active, const int shared, const int clamp,
                     float *__restrict__ g_sh, float *__restrict__ g_verts) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  float s[M * C], acc[M * C];
  sh_load_row<M, C>(sh + (size_t)n * (M * C), active, s);
#pragma unroll
  for (int i = 0; i < M * C; ++i) acc[i] = 0.0f;
  float svx = 0.0f, svy = 0.0f, svz = 0.0f;
  for (int b = 0; b < B; ++b) {
    const size_t row = (shared ? (size_t)0 : (size_t)b * N) + n;
    const float *v = verts + 3 * row;
    float x, y, z, inv, Y[M], G[M];
    sh_direction(v[0], v[1], v[2], centres + 3 * b, x, y, z, inv);
    sh_basis<M>(x, y, z, Y);
#pragma unroll
    for (int m = 0; m < M; ++m) G[m] = 0.0f;
    const float *go = g_out + ((size_t)b * N + n) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float pre = 0.0f;      // (the forward's own operations: the same clamp decision)
#pragma unroll
      for (int m = M - 1; m >= 1; --m) pre = fmaf(Y[m], s[m * C + c], pre);
      pre = fmaf(Y[0], s[c], pre) + 0.5f;
      const float g = (!clamp || pre > 0.0f) ? go[c] : 0.0f;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        acc[m * C + c] = fmaf(Y[m], g, acc[m * C + c]);
        G[m] = fmaf(g, s[m * C + c], G[m]);
      }
    }
    float gx, gy, gz;
    sh_basis_grad<M>(x, y, z, G, gx, gy, gz);
    const float along = fmaf(z, gz, fmaf(y, gy, x * gx));      // d d / d v = (I - d d^T) / |delta|
    gx = fmaf(-along, x, gx) * inv; gy = fmaf(-along, y, gy) * inv; gz = fmaf(-along, z, gz) * inv;
    if (shared) {
      svx += gx; svy += gy; svz += gz;
    } else {
      g_verts[3 * row] = gx; g_verts[3 * row + 1] = gy; g_verts[3 * row + 2] = gz;
    }
  }
  if (shared) {
    g_verts[3 * (size_t)n] = svx; g_verts[3 * (size_t)n + 1] = svy; g_verts[3 * (size_t)n + 2] = svz;
  }
#pragma unroll
  for (int m = 1; m < M; ++m)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[m * C + c] = m < active ? acc[m * C + c] : 0.0f;      // (Y_m of an inactive m is not zero: its sum is dropped here)
  sh_store_row<M, C>(g_sh + (size_t)n * (M * C), acc);
}

static bool sh_args_ok(const int B, const int N, const int M, const int C, const int degree) {
  if (B < 0 || N < 0 || C < 1 || C > 4 || degree < 0) return false;
  if (M != 1 && M != 4 && M != 9 && M != 16) return false;
  return (degree + 1) * (degree + 1) <= M;
}

static bool sh_row_aligned(const void *p, const int M, const int C) {      // the 16-byte loads of sh_load_row / sh_store_row
  return (M * C) % 4 != 0 || (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace voge

using namespace voge;

#define VOGE_SH_CASE(KERNEL, MM, CC, ...)                                                                                  \
  case (MM) * 8 + (CC):                                                                                                    \
    hipLaunchKernelGGL((KERNEL<MM, CC>), dim3(((unsigned)N + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, __VA_ARGS__);  \
    break;
#define VOGE_SH_DISPATCH(KERNEL, ...)                                                                                      \
  switch (M * 8 + C) {                                                                                                     \
    VOGE_SH_CASE(KERNEL, 1, 1, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 1, 2, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 1, 3, __VA_ARGS__) \
    VOGE_SH_CASE(KERNEL, 1, 4, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 4, 1, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 4, 2, __VA_ARGS__) \
    VOGE_SH_CASE(KERNEL, 4, 3, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 4, 4, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 9, 1, __VA_ARGS__) \
    VOGE_SH_CASE(KERNEL, 9, 2, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 9, 3, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 9, 4, __VA_ARGS__) \
    VOGE_SH_CASE(KERNEL, 16, 1, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 16, 2, __VA_ARGS__) VOGE_SH_CASE(KERNEL, 16, 3, __VA_ARGS__) \
    VOGE_SH_CASE(KERNEL, 16, 4, __VA_ARGS__)                                                                               \
    default: return VOGE_ERR_BAD_ARG;                                                                                      \
  }

extern "C" int voge_sh_colors_fwd(const float *sh, const float *verts, const float *centres, int B, int N, int M, int C, int degree,
                                  int shared_verts, int clamp, float *out, voge_stream_t stream) {
  if (!sh_args_ok(B, N, M, C, degree)) return VOGE_ERR_BAD_ARG;
  if (B == 0 || N == 0) return 0;
  if (!sh || !verts || !centres || !out || !sh_row_aligned(sh, M, C)) return VOGE_ERR_BAD_ARG;
  const int active = (degree + 1) * (degree + 1);
  VOGE_SH_DISPATCH(sh_colors_fwd_kernel, sh, verts, centres, B, N, active, shared_verts != 0, clamp != 0, out)
  return launch_status();
}

extern "C" int voge_sh_colors_bwd(const float *sh, const float *verts, const float *centres, const float *g_out, int B, int N, int M,
                                  int C, int degree, int shared_verts, int clamp, float *g_sh, float *g_verts, voge_stream_t stream) {
  if (!sh_args_ok(B, N, M, C, degree)) return VOGE_ERR_BAD_ARG;
  if (B == 0 || N == 0) return 0;
  if (!sh || !verts || !centres || !g_out || !g_sh || !g_verts || !sh_row_aligned(sh, M, C) || !sh_row_aligned(g_sh, M, C))
    return VOGE_ERR_BAD_ARG;
  const int active = (degree + 1) * (degree + 1);
  VOGE_SH_DISPATCH(sh_colors_bwd_kernel, sh, verts, centres, g_out, B, N, active, shared_verts != 0, clamp != 0, g_sh, g_verts)
  return launch_status();
}
