// Depth-distortion regulariser of composited fragments (EXTENSION: the reference has none): per pixel
//   L = sum_i sum_j w_i w_j |t_i - t_j|      over the n = min(max(valid_num, 0), K) live slots, w = weight, t = len,
// the term Mip-NeRF 360 and 2D Gaussian splatting use to pull a ray's mass onto one surface.  Aggregation.distortion is the
// definition.  Order the live slots by (t_k, k) -- ascending len, exact ties by slot position -- and let u_k = t_k - t_first with
// t_first the smallest live len (the loss is translation invariant; on u the fp32 closed form is good to 2e-7 at ANY offset, on t
// it loses 2e-4 at t = 1000).  With, for slot i, over the slots before / after it in that order,
//   W<_i = sum w_j,  X<_i = sum w_j u_j,   W>_i, X>_i likewise,   S = sum_k w_k:
//   L        = 2 sum_i w_i (u_i W<_i - X<_i)
//   dL/dw_i  = 2 [u_i (W<_i - W>_i) - (X<_i - X>_i)]
//   dL/dt_i  = 2 w_i (W<_i - W>_i)          (at an exact tie the POSITIONAL subgradient: the earlier slot counts as nearer)
//   normalize: out = L / S^2 where S > 0, else 0 with zero gradient.  With the incoming gradient g: a = g / S^2, b = -2 g out / S
//   (normalize) or a = g, b = 0;  g_w_i = a dL/dw_i + b,  g_t_i = a dL/dt_i;  zero in the dead slots.
//
// Streaming kernels in the shape of depth_fwd/bwd_kernel (merge_blend.hip): a pixel owns LP consecutive lanes of ONE wave (LP a
// power of two, at most 64).  A UNIT is V consecutive slots -- V = 4, one 16-byte access per array, where K % 4 == 0 and the
// arrays are 16-byte aligned; V = 1 otherwise.  Units are dealt to the pixel's lanes CYCLICALLY: round r gives lane q the unit
// q + r * LP, so a round is LP consecutive units in slot order and a wave's access is contiguous; K <= 256 makes that one round
// for V = 4 and up to four for V = 1.  Fragments are stored in ascending (len, index) order, so the prefix sums are a scan in
// slot order: the unit's own sums, a segmented inclusive scan of them over the pixel's lanes (__shfl_up), the exclusive value
// from the lane below, a running carry between rounds (broadcast from the pixel's last lane), then the V slots in order.  The
// pixel totals (S, sum w u, L) are an xor butterfly of the lanes' sums.  All of it is a fixed association: the same bits on every
// run and in every lane that holds a total.
// Each pixel checks that its live len are non-decreasing (one compare per slot with the slot before it: in the unit, from the
// lane below, or from the last lane of the round before).  A pixel that fails -- edited fragments, find_farest_k -- takes a
// pairwise walk in the same kernel: each of its lanes loops over all live j for each of its own slots and classes j as before or
// after by (t_j, j) < (t_i, i), with t_first = the minimum.  The branch is per pixel and holds no cross-lane operation: sorted
// pixels of the same wave keep the scan's values (the scan itself is run by every lane, its result dropped where it does not apply).
// Bytes moved per slot: 8 read forward; 8 read + 8 written backward (plus 4 + 8 or 20 per PIXEL).  The backward recomputes the scan
// from weight and len (with more than one round it reads them twice, the second time from the cache), writes EVERY element of
// g_weight and g_len, dead slots as zero: no fill launch, no atomics.
#include "voge_common.h"

#include <cmath>

namespace voge {

__device__ __forceinline__ int dist_live(const int64_t *__restrict__ valid_num, const long pix, const int K) {
  const int64_t v = valid_num[pix];
  return (int)(v < 0 ? 0 : (v > K ? K : v));
}

// slots k0 .. k0 + V - 1 of a pixel; zero in the dead ones (k >= n), which are never read
template <int V>
__device__ __forceinline__ void dist_load(const float *__restrict__ w, const float *__restrict__ t, const int k0, const int n,
                                          float (&wv)[V], float (&tv)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) wv[j] = tv[j] = 0.0f;
  if (k0 >= n) return;
  if (V == 4) {
    const float4 w4 = *reinterpret_cast<const float4 *>(w + k0), t4 = *reinterpret_cast<const float4 *>(t + k0);
    const float a[4] = {w4.x, w4.y, w4.z, w4.w}, b[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (k0 + j < n) { wv[j] = a[j]; tv[j] = b[j]; }
  } else {
    wv[0] = w[k0];
    tv[0] = t[k0];
  }
}

// is a live slot of this unit smaller than the slot before it?  t_wrap: the last slot of the round before (lane 0's neighbour)
template <int V>
__device__ __forceinline__ bool dist_unsorted(const float (&tv)[V], const int k0, const int n, const int q, const float t_wrap) {
  float tp = __shfl_up(tv[V - 1], 1, 64);
  if (q == 0) tp = t_wrap;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int k = k0 + j;
    if (k > 0 && k < n && !(tv[j] >= tp)) bad = true;
    tp = tv[j];
  }
  return bad;
}

// (uw, ux), a unit's sums -> the sums of every unit of this round BEFORE it (ew, ex); (uw, ux) become the inclusive values
__device__ __forceinline__ void dist_scan(float &uw, float &ux, const int q, const int LP, float &ew, float &ex) {
  for (int o = 1; o < LP; o <<= 1) {
    const float a = __shfl_up(uw, o, 64), b = __shfl_up(ux, o, 64);
    if (q >= o) { uw += a; ux += b; }
  }
  ew = __shfl_up(uw, 1, 64);
  ex = __shfl_up(ux, 1, 64);
  if (q == 0) ew = ex = 0.0f;
}

// does any lane of this lane's pixel hold `bad`?
__device__ __forceinline__ bool dist_pixel_any(const bool bad, const int lane, const int LP) {
  const unsigned long long m = __ballot(bad);
  const unsigned long long seg = (LP == 64 ? ~0ull : ((1ull << LP) - 1ull)) << (lane & ~(LP - 1));
  return (m & seg) != 0ull;
}

__device__ __forceinline__ float dist_min_len(const float *__restrict__ t, const int n) {
  float m = INFINITY;
  for (int j = 0; j < n; ++j) m = fminf(m, t[j]);
  return m;
}

template <int V>
__global__ void __launch_bounds__(256)
distortion_fwd_kernel(const float *__restrict__ weight, const float *__restrict__ len, const int64_t *__restrict__ valid_num,
                      const long npix, const int K, const int LP, const int R, const int normalize, float *__restrict__ dist,
                      float *__restrict__ wsum) {
  const int lane = threadIdx.x & 63, q = lane & (LP - 1), last = lane | (LP - 1);
  const long pix = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / LP) + lane / LP;
  const bool ok = pix < npix;      // (no early exit: every lane takes part in the scan and the butterfly)
  const int n = ok ? dist_live(valid_num, pix, K) : 0;
  const float *const w = weight + pix * K, *const t = len + pix * K;
  const float t0 = n > 0 ? t[0] : 0.0f;      // t_first of a sorted pixel
  float cw = 0.0f, cx = 0.0f, t_wrap = 0.0f, Lh = 0.0f, S = 0.0f;      // Lh: this lane's share of L / 2
  bool bad = false;
  for (int r = 0; r < R; ++r) {
    const int k0 = V * (q + r * LP);
    float wv[V], tv[V], x[V], u[V];
    dist_load<V>(w, t, k0, n, wv, tv);
    bad |= dist_unsorted<V>(tv, k0, n, q, t_wrap);
    float uw = 0.0f, ux = 0.0f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      u[j] = k0 + j < n ? tv[j] - t0 : 0.0f;
      x[j] = wv[j] * u[j];
      uw += wv[j];
      ux += x[j];
    }
    S += uw;
    float pw, px;
    dist_scan(uw, ux, q, LP, pw, px);
    pw += cw;
    px += cx;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      Lh = fmaf(wv[j], fmaf(u[j], pw, -px), Lh);
      pw += wv[j];
      px += x[j];
    }
    if (R > 1) {
      cw += __shfl(uw, last, 64);
      cx += __shfl(ux, last, 64);
      t_wrap = __shfl(tv[V - 1], last, 64);
    }
  }
  if (dist_pixel_any(bad, lane, LP)) {      // the pairwise walk of an unsorted pixel
    const float tmin = dist_min_len(t, n);
    Lh = 0.0f;
    for (int r = 0; r < R; ++r)
      for (int i = V * (q + r * LP); i < min(V * (q + r * LP) + V, n); ++i) {
        const float wi = w[i], ti = t[i];
        float wl = 0.0f, xl = 0.0f;
        for (int j = 0; j < n; ++j) {
          const float wj = w[j], tj = t[j];
          if (tj < ti || (tj == ti && j < i)) { wl += wj; xl = fmaf(wj, tj - tmin, xl); }
        }
        Lh = fmaf(wi, fmaf(ti - tmin, wl, -xl), Lh);
      }
  }
  for (int o = LP >> 1; o > 0; o >>= 1) { Lh += __shfl_xor(Lh, o, 64); S += __shfl_xor(S, o, 64); }
  if (ok && q == 0) {
    const float L = 2.0f * Lh;
    dist[pix] = normalize ? (S > 0.0f ? L / S / S : 0.0f) : L;
    wsum[pix] = S;
  }
}

template <int V>
__global__ void __launch_bounds__(256)
distortion_bwd_kernel(const float *__restrict__ weight, const float *__restrict__ len, const int64_t *__restrict__ valid_num,
                      const float *__restrict__ dist, const float *__restrict__ wsum, const float *__restrict__ g_dist,
                      const long npix, const int K, const int LP, const int R, const int normalize, float *__restrict__ g_weight,
                      float *__restrict__ g_len) {
  const int lane = threadIdx.x & 63, q = lane & (LP - 1), last = lane | (LP - 1);
  const long pix = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / LP) + lane / LP;
  const bool ok = pix < npix;
  const int n = ok ? dist_live(valid_num, pix, K) : 0;
  const long base = pix * K;
  const float *const w = weight + base, *const t = len + base;
  const float t0 = n > 0 ? t[0] : 0.0f;
  // pass 1: the order check and the pixel's totals S = sum w, X = sum w u
  float wv[V], tv[V], S = 0.0f, X = 0.0f, t_wrap = 0.0f;
  bool bad = false;
  for (int r = 0; r < R; ++r) {
    const int k0 = V * (q + r * LP);
    dist_load<V>(w, t, k0, n, wv, tv);
    bad |= dist_unsorted<V>(tv, k0, n, q, t_wrap);
    float uw = 0.0f, ux = 0.0f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      uw += wv[j];
      ux += wv[j] * (k0 + j < n ? tv[j] - t0 : 0.0f);
    }
    S += uw;
    X += ux;
    if (R > 1) t_wrap = __shfl(tv[V - 1], last, 64);
  }
  for (int o = LP >> 1; o > 0; o >>= 1) { S += __shfl_xor(S, o, 64); X += __shfl_xor(X, o, 64); }
  const bool walk = dist_pixel_any(bad, lane, LP);
  const float tmin = walk ? dist_min_len(t, n) : t0;
  float a2 = 0.0f, b = 0.0f;      // 2 a and b of the header
  if (ok) {
    a2 = 2.0f * g_dist[pix];
    if (normalize) {
      const float Sf = wsum[pix];
      b = Sf > 0.0f ? -a2 * dist[pix] / Sf : 0.0f;
      a2 = Sf > 0.0f ? a2 / Sf / Sf : 0.0f;
    }
  }
  // pass 2: the scan again, the gradients, the stores
  float cw = 0.0f, cx = 0.0f;
  for (int r = 0; r < R; ++r) {
    const int k0 = V * (q + r * LP);
    if (R > 1) dist_load<V>(w, t, k0, n, wv, tv);      // (one round: pass 1 left this lane's unit in the registers)
    float u[V], x[V], uw = 0.0f, ux = 0.0f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      u[j] = k0 + j < n ? tv[j] - t0 : 0.0f;
      x[j] = wv[j] * u[j];
      uw += wv[j];
      ux += x[j];
    }
    float pw, px;
    dist_scan(uw, ux, q, LP, pw, px);
    pw += cw;
    px += cx;
    float gw[V], gl[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float dw = pw - (S - pw - wv[j]);            // W< - W>
      const float dx = px - (X - px - x[j]);             // X< - X>
      const bool live = k0 + j < n;
      gw[j] = live ? fmaf(a2, fmaf(u[j], dw, -dx), b) : 0.0f;
      gl[j] = live ? a2 * wv[j] * dw : 0.0f;
      pw += wv[j];
      px += x[j];
    }
    if (R > 1) {
      cw += __shfl(uw, last, 64);
      cx += __shfl(ux, last, 64);
    }
    if (walk) {      // the pairwise walk of an unsorted pixel
#pragma unroll
      for (int jj = 0; jj < V; ++jj) {
        const int i = k0 + jj;
        if (i >= n) continue;
        const float ti = tv[jj];
        float wl = 0.0f, xl = 0.0f, wg = 0.0f, xg = 0.0f;
        for (int j = 0; j < n; ++j) {
          const float wj = w[j], tj = t[j];
          if (tj < ti || (tj == ti && j < i)) { wl += wj; xl = fmaf(wj, tj - tmin, xl); }
          else if (j != i) { wg += wj; xg = fmaf(wj, tj - tmin, xg); }
        }
        gw[jj] = fmaf(a2, fmaf(ti - tmin, wl - wg, -(xl - xg)), b);
        gl[jj] = a2 * wv[jj] * (wl - wg);
      }
    }
    if (ok && k0 < K) {
      if (V == 4) {
        *reinterpret_cast<float4 *>(g_weight + base + k0) = make_float4(gw[0], gw[1], gw[2], gw[V - 1]);
        *reinterpret_cast<float4 *>(g_len + base + k0) = make_float4(gl[0], gl[1], gl[2], gl[V - 1]);
      } else {
        g_weight[base + k0] = gw[0];
        g_len[base + k0] = gl[0];
      }
    }
  }
}

// lanes per pixel: the smallest power of two that holds the pixel's units, at most a wave
static inline int dist_lanes(const int units) {
  int lp = 1;
  while (lp < units && lp < 64) lp <<= 1;
  return lp;
}

static inline bool dist_aligned(const void *a, const void *b, const void *c = nullptr, const void *d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

struct DistShape {
  int LP, R;      // lanes per pixel, rounds
  long blocks;
};
static inline DistShape dist_shape(const long npix, const int K, const bool vec) {
  const int units = vec ? K / 4 : K;
  DistShape s;
  s.LP = dist_lanes(units);
  s.R = (units + s.LP - 1) / s.LP;
  const long per_wg = 4L * (64 / s.LP);
  s.blocks = (npix + per_wg - 1) / per_wg;
  return s;
}

}  // namespace voge

using namespace voge;

extern "C" int voge_distortion_fwd(const float *weight, const float *len, const int64_t *valid_num, long npix, int K,
                                   int normalize, float *dist, float *wsum, voge_stream_t stream) {
  if (npix < 0 || K < 1) return VOGE_ERR_BAD_ARG;
  if (K > VOGE_MAX_K) return VOGE_ERR_K_TOO_LARGE;
  if (npix == 0) return 0;
  if (!weight || !len || !valid_num || !dist || !wsum) return VOGE_ERR_BAD_ARG;
  const bool vec = (K & 3) == 0 && dist_aligned(weight, len);
  const DistShape s = dist_shape(npix, K, vec);
  if (s.blocks > 0x7fffffffL) return VOGE_ERR_BAD_ARG;
  const dim3 grid((unsigned)s.blocks);
  if (vec)
    hipLaunchKernelGGL(distortion_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, weight, len, valid_num, npix, K, s.LP,
                       s.R, normalize, dist, wsum);
  else
    hipLaunchKernelGGL(distortion_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, weight, len, valid_num, npix, K, s.LP,
                       s.R, normalize, dist, wsum);
  return launch_status();
}

extern "C" int voge_distortion_bwd(const float *weight, const float *len, const int64_t *valid_num, const float *dist,
                                   const float *wsum, const float *g_dist, long npix, int K, int normalize, float *g_weight,
                                   float *g_len, voge_stream_t stream) {
  if (npix < 0 || K < 1) return VOGE_ERR_BAD_ARG;
  if (K > VOGE_MAX_K) return VOGE_ERR_K_TOO_LARGE;
  if (npix == 0) return 0;
  if (!weight || !len || !valid_num || !g_dist || !g_weight || !g_len || (normalize && (!dist || !wsum))) return VOGE_ERR_BAD_ARG;
  const bool vec = (K & 3) == 0 && dist_aligned(weight, len, g_weight, g_len);
  const DistShape s = dist_shape(npix, K, vec);
  if (s.blocks > 0x7fffffffL) return VOGE_ERR_BAD_ARG;
  const dim3 grid((unsigned)s.blocks);
  if (vec)
    hipLaunchKernelGGL(distortion_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, weight, len, valid_num, dist, wsum,
                       g_dist, npix, K, s.LP, s.R, normalize, g_weight, g_len);
  else
    hipLaunchKernelGGL(distortion_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, weight, len, valid_num, dist, wsum,
                       g_dist, npix, K, s.LP, s.R, normalize, g_weight, g_len);
  return launch_status();
}
