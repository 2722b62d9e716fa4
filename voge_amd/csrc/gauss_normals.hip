// Per-view normals of oriented Gaussians (EXTENSION: the reference has neither oriented Gaussians nor normals).  An oriented
// Gaussian S = R diag(s) R^T stands for a flat surface element whose normal is its thinnest axis, a COLUMN of R = R(q / |q|):
//   k* = 0; for j = 1, 2: k* = j if s_j > s_k* (inverse_sigma == 0: A = 2 S, a larger s is thinner) | s_j < s_k* (A = R diag(2 / s) R^T)
//        -- an exact tie keeps the lowest index, a NaN never wins, a NaN in s_0 stays chosen;
//   n0 = R[:, k*];   for view b, delta = v - c_b and t = n0 . delta:   out[b*N + n] = -n0 where t > 0, n0 otherwise
//        -- the side that faces the camera (n . delta <= 0); t == 0, delta == 0 and a NaN t keep n0.
// One thread owns a Gaussian and walks the views in order when the orientations are shared, one thread owns a (view, Gaussian)
// when they are per view; consecutive lanes write consecutive 12-byte rows.  The backward recomputes the axis and the signs from
// the inputs (the forward saves nothing), sums the views in order in fp64 and goes through the chosen column in fp64 -- no
// atomics, the same bits on every run.  The axis and the sign are constants of the gradient; only the quaternions get one.
#include "voge_common.h"

namespace voge {

struct GaussNormalsArgs {
  const float *scales, *quats, *verts, *centres;
  int B, N, shared_orient, shared_verts, inverse_sigma;
  int quats16;      // quats (and the backward's g_quats) start on a 16-byte boundary: one 16-byte access a row
};

// the thinnest axis of (s0, s1, s2) by the comparison rule above
__device__ __forceinline__ int gn_axis(const float s0, const float s1, const float s2, const int inverse) {
  int k = 0;
  float sk = s0;
  if (inverse ? s1 < sk : s1 > sk) { k = 1; sk = s1; }
  if (inverse ? s2 < sk : s2 > sk) k = 2;
  return k;
}

__device__ __forceinline__ float4 gn_load_quat(const float *__restrict__ quats, const size_t row, const int quats16) {
  if (quats16) return reinterpret_cast<const float4 *>(quats)[row];
  const float *q = quats + 4 * row;
  return make_float4(q[0], q[1], q[2], q[3]);
}

// column k of a row-major 3x3 (selects: nothing is indexed at run time, nothing goes to scratch)
template <typename T>
__device__ __forceinline__ void gn_column(const T (&R)[9], const int k, T &x, T &y, T &z) {
  const T r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5], r6 = R[6], r7 = R[7], r8 = R[8];
  x = k == 0 ? r0 : (k == 1 ? r1 : r2);
  y = k == 0 ? r3 : (k == 1 ? r4 : r5);
  z = k == 0 ? r6 : (k == 1 ? r7 : r8);
}

// whether view b sees the back of n0 at the vertex row `vrow` (t > 0: the output is -n0)
__device__ __forceinline__ bool gn_flipped(const float *__restrict__ verts, const size_t vrow, const float *__restrict__ c,
                                           const float nx, const float ny, const float nz) {
  const float *v = verts + 3 * vrow;
  const float dx = v[0] - c[0], dy = v[1] - c[1], dz = v[2] - c[2];
  return fmaf(nz, dz, fmaf(ny, dy, nx * dx)) > 0.0f;
}

// the thread's orientation row, Gaussian and views [b0, b1)
__device__ __forceinline__ bool gn_thread(const GaussNormalsArgs &a, size_t &row, int &n, int &b0, int &b1) {
  row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= (a.shared_orient ? (size_t)a.N : (size_t)a.B * a.N)) return false;
  if (a.shared_orient) {
    n = (int)row; b0 = 0; b1 = a.B;
  } else {
    b0 = (int)(row / (size_t)a.N); n = (int)(row - (size_t)b0 * a.N); b1 = b0 + 1;
  }
  return true;
}

__global__ void __launch_bounds__(256)
gauss_normals_fwd_kernel(const GaussNormalsArgs a, float *__restrict__ out) {
  size_t row;
  int n, b0, b1;
  if (!gn_thread(a, row, n, b0, b1)) return;
  const float *s = a.scales + 3 * row;
  const int k = gn_axis(s[0], s[1], s[2], a.inverse_sigma);
  const float4 q = gn_load_quat(a.quats, row, a.quats16);
  float R[9], qh[4], inv, nx, ny, nz;
  quat_rotation<float>(quat_usable(q.x, q.y, q.z, q.w), q.x, q.y, q.z, q.w, R, qh, inv);
  gn_column<float>(R, k, nx, ny, nz);
  for (int b = b0; b < b1; ++b) {
    const size_t orow = (size_t)b * a.N + n;
    const bool flip = gn_flipped(a.verts, a.shared_verts ? (size_t)n : orow, a.centres + 3 * b, nx, ny, nz);
    float *o = out + 3 * orow;
    o[0] = flip ? -nx : nx; o[1] = flip ? -ny : ny; o[2] = flip ? -nz : nz;
  }
}

__global__ void __launch_bounds__(256)
gauss_normals_bwd_kernel(const GaussNormalsArgs a, const float *__restrict__ g_out, float *__restrict__ g_quats) {
  size_t row;
  int n, b0, b1;
  if (!gn_thread(a, row, n, b0, b1)) return;
  const float *s = a.scales + 3 * row;
  const int k = gn_axis(s[0], s[1], s[2], a.inverse_sigma);
  const float4 q = gn_load_quat(a.quats, row, a.quats16);
  const bool ok = quat_usable(q.x, q.y, q.z, q.w);      // (the forward's own fp32 decision)
  float Rf[9], qf[4], invf, nx, ny, nz;
  quat_rotation<float>(ok, q.x, q.y, q.z, q.w, Rf, qf, invf);      // (the forward's own column: the same signs)
  gn_column<float>(Rf, k, nx, ny, nz);
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;      // g_n0 = sum_b sign_b g_out[b*N + n]
  for (int b = b0; b < b1; ++b) {
    const size_t orow = (size_t)b * a.N + n;
    const bool flip = gn_flipped(a.verts, a.shared_verts ? (size_t)n : orow, a.centres + 3 * b, nx, ny, nz);
    const float *g = g_out + 3 * orow;
    g0 += (double)(flip ? -g[0] : g[0]); g1 += (double)(flip ? -g[1] : g[1]); g2 += (double)(flip ? -g[2] : g[2]);
  }
  double R[9], qh[4], inv;
  quat_rotation<double>(ok, q.x, q.y, q.z, q.w, R, qh, inv);
  double gR[9];      // g_R: g_n0 in column k
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    gR[j] = k == j ? g0 : 0.0; gR[3 + j] = k == j ? g1 : 0.0; gR[6 + j] = k == j ? g2 : 0.0;
  }
  const double w = qh[0], x = qh[1], y = qh[2], z = qh[3];      // (the derivative of quat_rotation's matrix, as fragment_bwd_finish_ori_kernel)
  const double gw = 2.0 * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
  const double gx = 2.0 * (y * gR[1] + z * gR[2] + y * gR[3] - 2.0 * x * gR[4] - w * gR[5] + z * gR[6] + w * gR[7] - 2.0 * x * gR[8]);
  const double gy = 2.0 * (-2.0 * y * gR[0] + x * gR[1] + w * gR[2] + x * gR[3] + z * gR[5] - w * gR[6] + z * gR[7] - 2.0 * y * gR[8]);
  const double gz = 2.0 * (-2.0 * z * gR[0] - w * gR[1] + x * gR[2] + w * gR[3] - 2.0 * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
  const double along = w * gw + x * gx + y * gy + z * gz;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) o = make_float4((float)((gw - w * along) * inv), (float)((gx - x * along) * inv), (float)((gy - y * along) * inv),
                          (float)((gz - z * along) * inv));
  if (a.quats16) {
    reinterpret_cast<float4 *>(g_quats)[row] = o;
  } else {
    float *gq = g_quats + 4 * row;
    gq[0] = o.x; gq[1] = o.y; gq[2] = o.z; gq[3] = o.w;
  }
}

// 1: nothing to do; 0: launch; < 0: the error
static int gauss_normals_check(const int B, const int N, const bool pointers) {
  if (B < 0 || N < 0) return VOGE_ERR_BAD_ARG;
  if (B == 0 || N == 0) return 1;
  if (!pointers || (long)B * N * 3 > 2147483647l) return VOGE_ERR_BAD_ARG;
  return 0;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace voge

using namespace voge;

extern "C" int voge_gauss_normals_fwd(const float *scales, const float *quats, const float *verts, const float *centres, int B, int N,
                                      int shared_orient, int shared_verts, int inverse_sigma, float *out, voge_stream_t stream) {
  const int rc = gauss_normals_check(B, N, scales && quats && verts && centres && out);
  if (rc != 0) return rc < 0 ? rc : 0;
  const GaussNormalsArgs a{scales, quats, verts, centres, B, N, shared_orient != 0, shared_verts != 0, inverse_sigma != 0, aligned16(quats)};
  const long rows = shared_orient ? (long)N : (long)B * N;
  hipLaunchKernelGGL(gauss_normals_fwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, out);
  return launch_status();
}

extern "C" int voge_gauss_normals_bwd(const float *scales, const float *quats, const float *verts, const float *centres,
                                      const float *g_out, int B, int N, int shared_orient, int shared_verts, int inverse_sigma,
                                      float *g_quats, voge_stream_t stream) {
  const int rc = gauss_normals_check(B, N, scales && quats && verts && centres && g_out && g_quats);
  if (rc != 0) return rc < 0 ? rc : 0;
  const GaussNormalsArgs a{scales, quats, verts, centres, B, N, shared_orient != 0, shared_verts != 0, inverse_sigma != 0,
                           aligned16(quats) && aligned16(g_quats)};
  const long rows = shared_orient ? (long)N : (long)B * N;
  hipLaunchKernelGGL(gauss_normals_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, g_out,
                     g_quats);
  return launch_status();
}
