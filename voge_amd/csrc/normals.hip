// Surface normals from a depth map (EXTENSION: the reference has neither a depth nor a normal output).  depth [B][h][W] is the
// distance along each pixel's unit ray (Renderer.get_depth); the normal of the RENDERED surface is the normalised cross product
// of finite differences of the back-projected points P = depth * ray, turned to face the camera -- Aggregation.depth_normals is
// the definition, rule by rule:
//   valid      = isfinite(depth) && depth > 0
//   usable(nb) = nb inside the band && valid(nb) && (edge < 0 || |depth_nb - depth| <= edge * depth)
//   D_x        = P(j+1) - P(j-1) | P(j+1) - P(j) | P(j) - P(j-1) by which neighbours are usable (none: undefined); D_y along i
//   c = D_x x D_y;  defined = valid && both differences exist && 0 < |c|^2 < inf;  n = +-c / |c| with n . ray <= 0, else 0.
// The kernels make the rays from the camera (cam_load; nrm_dir is cam_ray's direction BEFORE it is normalised): band row i is
// image row row0 + i, no ray bundle is read or written.  P is formed as t * w with w the unnormalised direction and
// t = depth / |w|, and a difference as
//   P_a - P_b = (t_a - t_b) * w_a + t_b * (w_a - w_b),
// where w_a - w_b is a constant vector of the view (one or two pixel steps: no cancellation at all) and t_a - t_b comes from the
// DEPTH difference -- exact for neighbouring depths -- and the difference of 1 / |w|, itself formed from that constant vector
// (nrm_axis): nothing this arithmetic rounds is amplified.  What is amplified, by depth / pixel footprint, is the rounding the
// fp32 depth values arrive with: the fp32 floor of the problem, which no kernel can take back.
// One thread per pixel, both ways.  The backward is a GATHER: the thread of pixel q recomputes the stencils of the up to five
// outputs that read depth(q) -- q and its four neighbours -- and sums their contributions in a fixed order: no atomics, every
// element of g_depth written, the same bits on every run.  Neighbours come straight from the cache (13 distinct depths a
// thread, all but the halo shared with the workgroup's other lanes).
#include "voge_common.h"

#include <cfloat>

namespace voge {

constexpr int kNrmBX = 64, kNrmBY = 4;      // a workgroup's pixels: one wave per row segment of 64

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ float dot3(const V3 a, const V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross3(const V3 a, const V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 scale3(const float s, const V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 axpy3(const float s, const V3 a, const V3 b) { return V3{fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z)}; }

// cam_ray's world-space direction of image pixel (row ir, column j) before the normalisation: w = [vx, vy, 1] @ R^-1
__device__ __forceinline__ V3 nrm_dir(const CamK &k, const int ir, const int j) {
  const float vx = (k.px - ((float)j + 0.5f)) * k.ifx;
  const float vy = (k.py - ((float)ir + 0.5f)) * k.ify;
  return V3{vx * k.Ri.m[0] + vy * k.Ri.m[3] + k.Ri.m[6], vx * k.Ri.m[1] + vy * k.Ri.m[4] + k.Ri.m[7],
            vx * k.Ri.m[2] + vy * k.Ri.m[5] + k.Ri.m[8]};
}

struct NrmView {      // what a thread needs of its view
  CamK k;
  V3 sx, sy;          // w(i, j+1) - w(i, j) and w(i+1, j) - w(i, j): the same for every pixel
  int row0, h, W;
  float edge;         // < 0: none
};
__device__ __forceinline__ NrmView nrm_view(const float *R, const float *focal, const float *pp, const int b, const int row0,
                                            const int h, const int W, const float edge) {
  const CamView cam{R, nullptr, focal, pp, row0, max(h, 1), 0, h, W, 0, nullptr, nullptr};
  NrmView v;
  v.k = cam_load(cam, b);
  v.sx = V3{-v.k.ifx * v.k.Ri.m[0], -v.k.ifx * v.k.Ri.m[1], -v.k.ifx * v.k.Ri.m[2]};
  v.sy = V3{-v.k.ify * v.k.Ri.m[3], -v.k.ify * v.k.Ri.m[4], -v.k.ify * v.k.Ri.m[5]};
  v.row0 = row0; v.h = h; v.W = W; v.edge = edge;
  return v;
}

struct NrmSample {      // one pixel of the depth map and its ray: P = d * r * w
  V3 w;
  float d, r;           // d = 0 where the pixel is outside the band or its depth is not valid; r = 1 / |w|
  bool ok;
};
__device__ __forceinline__ NrmSample nrm_sample(const float *__restrict__ db, const NrmView &v, const int i, const int j) {
  NrmSample s;
  const bool in = i >= 0 && i < v.h && j >= 0 && j < v.W;
  const float d = db[(size_t)min(max(i, 0), v.h - 1) * v.W + min(max(j, 0), v.W - 1)];      // (never read outside the band)
  s.ok = in && d > 0.0f && d <= FLT_MAX;      // (NaN fails the first comparison, +inf the second)
  s.w = nrm_dir(v.k, v.row0 + i, j);
  s.d = s.ok ? d : 0.0f;
  s.r = 1.0f / sqrtf(dot3(s.w, s.w));
  return s;
}

// one axis of the stencil at centre c with its neighbours p (+1) and m (-1); step = w_p - w_c.  -> does the difference exist
// With a the + side and b the - side of the difference, `steps` pixels apart (w_a - w_b = steps * step):
//   |w_b|^2 - |w_a|^2 = -steps * step . (w_a + w_b)                     (a small number, formed without cancellation)
//   r_a - r_b         = (|w_b|^2 - |w_a|^2) (r_a r_b)^2 / (r_a + r_b)
//   t_a - t_b         = (d_a - d_b) r_a + d_b (r_a - r_b)               (d_a - d_b is exact for depths within a factor of 2)
//   D = P_a - P_b     = (t_a - t_b) w_a + t_b steps * step
__device__ __forceinline__ bool nrm_axis(const NrmSample &c, const NrmSample &p, const NrmSample &m, const V3 step, const float edge,
                                         V3 &D, bool &up, bool &um) {
  up = p.ok && (edge < 0.0f || fabsf(p.d - c.d) <= edge * c.d);
  um = m.ok && (edge < 0.0f || fabsf(m.d - c.d) <= edge * c.d);
  const float da = up ? p.d : c.d, db = um ? m.d : c.d, ra = up ? p.r : c.r, rb = um ? m.r : c.r;
  const V3 wa = up ? p.w : c.w, wb = um ? m.w : c.w;
  const float steps = (up ? 1.0f : 0.0f) + (um ? 1.0f : 0.0f);
  const float rr = ra * rb;
  const float dr = -steps * dot3(step, V3{wa.x + wb.x, wa.y + wb.y, wa.z + wb.z}) * (rr * rr) / (ra + rb);
  const float dt = fmaf(da - db, ra, db * dr);
  D = axpy3(dt, wa, scale3(db * rb * steps, step));
  return up || um;
}

struct NrmStencil {
  V3 Dx, Dy, c, w;      // the differences, their cross product, the pixel's own direction
  float c2;
  bool xp, xm, yp, ym;      // which neighbours the differences use
};
// the whole stencil of pixel (i, j) (inside the band) -> is its normal defined
__device__ __forceinline__ bool nrm_stencil(const float *__restrict__ db, const NrmView &v, const int i, const int j, NrmStencil &s) {
  const NrmSample c = nrm_sample(db, v, i, j);
  const NrmSample xp = nrm_sample(db, v, i, j + 1), xm = nrm_sample(db, v, i, j - 1);
  const NrmSample yp = nrm_sample(db, v, i + 1, j), ym = nrm_sample(db, v, i - 1, j);
  const bool hx = nrm_axis(c, xp, xm, v.sx, v.edge, s.Dx, s.xp, s.xm);
  const bool hy = nrm_axis(c, yp, ym, v.sy, v.edge, s.Dy, s.yp, s.ym);
  s.c = cross3(s.Dx, s.Dy);
  s.c2 = dot3(s.c, s.c);
  s.w = c.w;
  return c.ok && hx && hy && s.c2 > 0.0f && s.c2 <= FLT_MAX;
}

__global__ void __launch_bounds__(kNrmBX * kNrmBY)
depth_normals_fwd_kernel(const float *__restrict__ depth, const float *__restrict__ R, const float *__restrict__ focal,
                         const float *__restrict__ pp, const int row0, const int h, const int W, const float edge,
                         const int view_space, float *__restrict__ normals) {
  const int b = blockIdx.z, j = blockIdx.x * kNrmBX + threadIdx.x, i = blockIdx.y * kNrmBY + threadIdx.y;
  if (i >= h || j >= W) return;
  const NrmView v = nrm_view(R, focal, pp, b, row0, h, W, edge);
  const size_t px = ((size_t)b * h + i) * W + j;
  NrmStencil s;
  V3 n{0.0f, 0.0f, 0.0f};
  if (nrm_stencil(depth + (size_t)b * h * W, v, i, j, s)) {
    const float inv = 1.0f / sqrtf(s.c2);
    n = scale3(dot3(s.c, s.w) > 0.0f ? -inv : inv, s.c);      // towards the camera
    if (view_space) {      // n_world @ R
      const float *Rb = R + 9 * b;
      n = V3{fmaf(n.z, Rb[6], fmaf(n.y, Rb[3], n.x * Rb[0])), fmaf(n.z, Rb[7], fmaf(n.y, Rb[4], n.x * Rb[1])),
             fmaf(n.z, Rb[8], fmaf(n.y, Rb[5], n.x * Rb[2]))};
    }
  }
  normals[3 * px] = n.x; normals[3 * px + 1] = n.y; normals[3 * px + 2] = n.z;
}

// sum_{D in {D_x, D_y}} (d D / d P_q) applied to the gradient of output pixel (i, j), for the pixel q that sits at ROLE in that
// output's stencil: 0 the centre, 1 / 2 its -x / +x neighbour's centre (q is that output's + / - neighbour), 3 / 4 the same in y.
// Added to G; d P_q / d depth_q = w_q / |w_q| is applied by the caller, once.
template <int ROLE>
__device__ __forceinline__ void nrm_gather(const float *__restrict__ db, const float *__restrict__ gb, const float *__restrict__ Rb,
                                           const NrmView &v, const int view_space, const int i, const int j, V3 &G) {
  if (i < 0 || i >= v.h || j < 0 || j >= v.W) return;
  NrmStencil s;
  if (!nrm_stencil(db, v, i, j, s)) return;
  const float *gp = gb + 3 * ((size_t)i * v.W + j);
  V3 g{gp[0], gp[1], gp[2]};
  if (view_space)      // the transpose of the forward's n_world @ R
    g = V3{fmaf(g.z, Rb[2], fmaf(g.y, Rb[1], g.x * Rb[0])), fmaf(g.z, Rb[5], fmaf(g.y, Rb[4], g.x * Rb[3])),
           fmaf(g.z, Rb[8], fmaf(g.y, Rb[7], g.x * Rb[6]))};
  // n = f c / |c| (f = +-1, a constant):  g_c = f (g - u (u . g)) / |c|  with u = c / |c|
  const float inv = 1.0f / sqrtf(s.c2);
  const V3 u = scale3(inv, s.c);
  const V3 gc = scale3(dot3(s.c, s.w) > 0.0f ? -inv : inv, axpy3(-dot3(u, g), u, g));
  // c = D_x x D_y:  g_Dx = D_y x g_c,  g_Dy = g_c x D_x
  float fx = 0.0f, fy = 0.0f;      // the coefficient of P_q in D_x / D_y
  if (ROLE == 0) {
    fx = (s.xp && s.xm) ? 0.0f : (s.xp ? -1.0f : 1.0f);
    fy = (s.yp && s.ym) ? 0.0f : (s.yp ? -1.0f : 1.0f);
  } else if (ROLE == 1) {
    fx = s.xp ? 1.0f : 0.0f;
  } else if (ROLE == 2) {
    fx = s.xm ? -1.0f : 0.0f;
  } else if (ROLE == 3) {
    fy = s.yp ? 1.0f : 0.0f;
  } else {
    fy = s.ym ? -1.0f : 0.0f;
  }
  if (ROLE <= 2) G = axpy3(fx, cross3(s.Dy, gc), G);
  if (ROLE == 0 || ROLE >= 3) G = axpy3(fy, cross3(gc, s.Dx), G);
}

__global__ void __launch_bounds__(kNrmBX * kNrmBY)
depth_normals_bwd_kernel(const float *__restrict__ depth, const float *__restrict__ R, const float *__restrict__ focal,
                         const float *__restrict__ pp, const float *__restrict__ g_normals, const int row0, const int h, const int W,
                         const float edge, const int view_space, float *__restrict__ g_depth) {
  const int b = blockIdx.z, j = blockIdx.x * kNrmBX + threadIdx.x, i = blockIdx.y * kNrmBY + threadIdx.y;
  if (i >= h || j >= W) return;
  const NrmView v = nrm_view(R, focal, pp, b, row0, h, W, edge);
  const float *db = depth + (size_t)b * h * W, *gb = g_normals + (size_t)b * h * W * 3, *Rb = R + 9 * b;
  const NrmSample q = nrm_sample(db, v, i, j);
  float out = 0.0f;
  if (q.ok) {      // (a depth that is not valid is in no stencil)
    V3 G{0.0f, 0.0f, 0.0f};
    nrm_gather<0>(db, gb, Rb, v, view_space, i, j, G);
    nrm_gather<1>(db, gb, Rb, v, view_space, i, j - 1, G);
    nrm_gather<2>(db, gb, Rb, v, view_space, i, j + 1, G);
    nrm_gather<3>(db, gb, Rb, v, view_space, i - 1, j, G);
    nrm_gather<4>(db, gb, Rb, v, view_space, i + 1, j, G);
    out = dot3(G, q.w) * q.r;
  }
  g_depth[((size_t)b * h + i) * W + j] = out;
}

static bool nrm_args_ok(const int B, const int row0, const int h, const int W, const float edge) {
  if (B < 0 || h < 0 || W < 0 || row0 < 0 || edge != edge) return false;
  return B <= 65535 && (h + kNrmBY - 1) / kNrmBY <= 65535;      // (the grid's y and z extents)
}

}  // namespace voge

using namespace voge;

extern "C" int voge_depth_normals_fwd(const float *depth, const float *R, const float *focal, const float *pp, int B, int row0, int h,
                                      int W, float edge, int view_space, float *normals, voge_stream_t stream) {
  if (!nrm_args_ok(B, row0, h, W, edge)) return VOGE_ERR_BAD_ARG;
  if (B == 0 || h == 0 || W == 0) return 0;
  if (!depth || !R || !focal || !pp || !normals) return VOGE_ERR_BAD_ARG;
  hipLaunchKernelGGL(depth_normals_fwd_kernel, dim3((W + kNrmBX - 1) / kNrmBX, (h + kNrmBY - 1) / kNrmBY, B), dim3(kNrmBX, kNrmBY), 0,
                     (hipStream_t)stream, depth, R, focal, pp, row0, h, W, edge, view_space != 0, normals);
  return launch_status();
}

extern "C" int voge_depth_normals_bwd(const float *depth, const float *R, const float *focal, const float *pp, const float *g_normals,
                                      int B, int row0, int h, int W, float edge, int view_space, float *g_depth,
                                      voge_stream_t stream) {
  if (!nrm_args_ok(B, row0, h, W, edge)) return VOGE_ERR_BAD_ARG;
  if (B == 0 || h == 0 || W == 0) return 0;
  if (!depth || !R || !focal || !pp || !g_normals || !g_depth) return VOGE_ERR_BAD_ARG;
  hipLaunchKernelGGL(depth_normals_bwd_kernel, dim3((W + kNrmBX - 1) / kNrmBX, (h + kNrmBY - 1) / kNrmBY, B), dim3(kNrmBX, kNrmBY), 0,
                     (hipStream_t)stream, depth, R, focal, pp, g_normals, row0, h, W, edge, view_space != 0, g_depth);
  return launch_status();
}
