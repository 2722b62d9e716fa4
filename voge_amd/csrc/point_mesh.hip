// Point-to-mesh distance (EXTENSION: PyTorch3D's point_mesh_face_distance, the mesh-fitting loss beside the chamfer distance the
// reference's demo/ShapeFitting.py imports; the torch form is Aggregation.point_mesh_term, a P x F matrix in chunks): the squared
// distance from every point to its nearest triangle and from every triangle to its nearest point, the loss over both and its
// backward.  Measured: profiles/r25_point_mesh.txt.
//
// The pair function, pm_pair: Aggregation.point_triangle_closest operation by operation in fp32 (the library is built with
// -ffp-contract=off).  Differences first (e0 = b - a, e1 = c - a, v = p - a), four candidates -- the interior one, which exists
// only if nn = |e0 x e1|^2 > 0 and its three weights are >= 0, and the segments ab, bc, ca with t clamped to [0, 1] --, the smallest
// d2 wins and an exact tie keeps the earlier candidate.  Every candidate is a point of the triangle, so one with poor weights
// (a sliver's interior) can only lose; there is no area threshold.  A triangle is a RECORD of sixteen floats, built once per
// triangle (pm_record): a, e0, e1, n, 1 / nn and the three 1 / (e.e), each reciprocal 0 where its argument is 0 or where it would
// not be finite -- so the pair function has no division and no special case: t = 0 on an edge of length 0, no interior candidate
// on a triangle without area.  A face that names a vertex outside [0, V) gets a record of NaNs and never wins.
//
// voge_closest_faces / the two searches of voge_point_mesh_fwd, one launch each.  Both are exact brute-force searches; the winner
// is the lexicographically smallest (d2, index), held as ONE 64-bit key (d2 bits << 32 | index; d2 >= 0, so its bits order as the
// value does): a property of the SET of candidates, not of the order they are met in.
//   pm_point_kernel  a point per lane, 64 points a workgroup; the workgroup's lanes build one record each while staging a tile of
//                    256 triangles (16 KB of LDS), every wave takes its share of the tile's records -- all lanes of a wave read
//                    the same record: a broadcast, four 128-bit LDS reads a pair --, the waves' keys of a point meet in LDS;
//   pm_face_kernel   a triangle per lane with its record in registers, 64 triangles a workgroup; the points tiled through LDS 1024
//                    at a time, every wave takes its share of a tile, the keys meet in LDS.
// A workgroup per 64 queries would leave most of the GPU idle at a small P or F, so the candidates of a query are split over the
// waves of its workgroup: 16 waves while the queries make fewer than 1 024 workgroups, 4 from there on (measured: one wave is
// 3.5 - 4.7 x slower than four at 5 000 points; sixteen are 1.2 - 1.3 x faster than four below 1 024 workgroups, equal at 1 024 and
// 1.04 x slower at 1 563).  The split cannot change a bit: the minimum of the keys has no order (tested against the unsplit form
// of the -DVOGE_AB build).  After the search wave 0 evaluates the winner's pair once more for the weights (bary) -- cheaper than
// carrying three weights through the loop.
//
// voge_point_mesh_fwd.  The searches write d2 by their own index into the workspace; chamfer_loss.h's two kernels leave fp64
// partial sums and add them in ONE workgroup in an order fixed by the shapes: loss = sum_p / P + sum_f / F, rounded to fp32 once,
// and meta[0] = s, the scale exponent of the backward: with D = sqrt(max d2 (1 + 2^-20) + 2^-148) < 2^e and P + F <= 2^L,
// s = 62 - L - e.
//
// voge_point_mesh_bwd, three launches.  With r = p - q the residual of a chosen pair and w the weights of q (the envelope theorem:
// q minimises over the triangle, so the weights' own derivative drops out),
//   g_points[i] = g (2 / P) r_i + g (2 / F) sum_{f: nn(f) = i} r_f,
//   g_verts[v]  = - g (2 / P) sum_{i, k: faces[f_i][k] = v} w_ik r_i - g (2 / F) sum_{f, k: faces[f][k] = v} w_fk r_f.
// r is the residual pm_pair itself ends with (the pair is evaluated again), so every component is bounded by D whatever the
// cancellation in q; the weights are the saved ones.  (1) a zero fill of the [V + P][3] int64 accumulators; (2) pm_scatter_kernel,
// one item -- a point or a face -- per thread: every term u fl(w r) (u = 1 / P or 1 / F, 1 for "sum"; |term| <= D) is scaled by 2^s,
// rounded to an int64 and added with a 64-bit INTEGER atomic: exact, so the order does not matter, the bits are the same on every
// run and the cost stays linear when every point picks one face or every face one point.  A vertex gets at most three terms an item
// whose weights sum to 1, so |sum| <= 2^L 2^e 2^s + 1.5 2^L < 2^63; a list of m terms is off by at most m 2^-s / 2 per component.
// (3) pm_finish_kernel adds a point's own term in fp64, scales by 2 g and writes EVERY element of g_verts and g_points, rounded once.
// No float atomics, no host read-back (capturable); an index outside its range is skipped.
//
// The pair cap.  A brute force over 2^28 x 2^28 pairs would hold a GPU for days, so the brute-force entries (voge_closest_faces,
// voge_point_mesh_fwd, and voge_point_mesh_bwd without its grid flag) refuse P F above kPmMaxPairs before any HIP call.
// kPmMaxPairs = 2^38 is the largest power of two at which the slower direction stays under one second on the MI355X:
// tools/point_mesh_time.py, 524 288 points x 524 287 triangles, measured points -> faces 0.752 s and faces -> points 0.720 s
// (2.7 ps a pair; twice that would take 1.5 s by proportion).  The cap does NOT bind the grid route (point_mesh_grid.h:
// voge_closest_faces_grid, voge_point_mesh_fwd_grid, and the backward with flag bit 2), a search over a uniform grid whose items
// are triangles and which returns the brute route's bits; its limits are the sizes (2^28 - 1) and its workspace.
#include <math.h>

#include "chamfer_loss.h"

namespace voge {

constexpr long kPmMaxN = 268435455l;
constexpr double kPmMaxPairs = 274877906944.0;      // 2^38 (profiles/r25_point_mesh.txt)
constexpr int kPmFaceTile = 256;        // triangle records of a tile: one a lane of the workgroup, 16 KB
constexpr int kPmPointTile = 1024;      // points of a tile: 16 KB

struct PmRec {
  float4 a;       // a, 1 / nn
  float4 e0;      // b - a, 1 / (e0.e0)
  float4 e1;      // c - a, 1 / (e1.e1)
  float4 n;       // e0 x e1, 1 / (eb.eb), eb = e1 - e0
};
static_assert(sizeof(PmRec) == 64, "PmRec is sixteen floats");

__device__ __forceinline__ float pm_recip(const float x) {
  const float r = 1.0f / x;
  return (x > 0.0f && r < INFINITY) ? r : 0.0f;
}

__device__ __forceinline__ float pm_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz) {
  return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ PmRec pm_record(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const size_t f) {
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  PmRec r;
  if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) {
    r.a = r.e0 = r.e1 = r.n = make_float4(NAN, NAN, NAN, 0.0f);
    return r;
  }
  const float *a = verts + 3 * (size_t)ia, *b = verts + 3 * (size_t)ib, *c = verts + 3 * (size_t)ic;
  const float ax = a[0], ay = a[1], az = a[2];
  const float e0x = b[0] - ax, e0y = b[1] - ay, e0z = b[2] - az;
  const float e1x = c[0] - ax, e1y = c[1] - ay, e1z = c[2] - az;
  const float nx = (e0y * e1z) - (e0z * e1y), ny = (e0z * e1x) - (e0x * e1z), nz = (e0x * e1y) - (e0y * e1x);
  const float ebx = e1x - e0x, eby = e1y - e0y, ebz = e1z - e0z;
  r.a = make_float4(ax, ay, az, pm_recip(pm_dot(nx, ny, nz, nx, ny, nz)));
  r.e0 = make_float4(e0x, e0y, e0z, pm_recip(pm_dot(e0x, e0y, e0z, e0x, e0y, e0z)));
  r.e1 = make_float4(e1x, e1y, e1z, pm_recip(pm_dot(e1x, e1y, e1z, e1x, e1y, e1z)));
  r.n = make_float4(nx, ny, nz, pm_recip(pm_dot(ebx, eby, ebz, ebx, eby, ebz)));
  return r;
}

__device__ __forceinline__ float pm_clamp01(const float t) { return fminf(fmaxf(t, 0.0f), 1.0f); }

// d2 of the point (px, py, pz) and the triangle t; kOut: w[3] = the weights of the closest point on (a, b, c), r[3] = p - q
template <bool kOut>
__device__ __forceinline__ float pm_pair(const PmRec &t, const float px, const float py, const float pz, float *__restrict__ w,
                                         float *__restrict__ r) {
  const float e0x = t.e0.x, e0y = t.e0.y, e0z = t.e0.z, e1x = t.e1.x, e1y = t.e1.y, e1z = t.e1.z;
  const float nx = t.n.x, ny = t.n.y, nz = t.n.z;
  const float vx = px - t.a.x, vy = py - t.a.y, vz = pz - t.a.z;
  // interior: w2 = ((e0 x v).n) / nn, w1 = ((v x e1).n) / nn
  const float w2 = pm_dot((e0y * vz) - (e0z * vy), (e0z * vx) - (e0x * vz), (e0x * vy) - (e0y * vx), nx, ny, nz) * t.a.w;
  const float w1 = pm_dot((vy * e1z) - (vz * e1y), (vz * e1x) - (vx * e1z), (vx * e1y) - (vy * e1x), nx, ny, nz) * t.a.w;
  const float w0 = (1.0f - w1) - w2;
  const bool inside = t.a.w > 0.0f && w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f;
  const float ix = vx - (w1 * e0x + w2 * e1x), iy = vy - (w1 * e0y + w2 * e1y), iz = vz - (w1 * e0z + w2 * e1z);
  const float d_in = pm_dot(ix, iy, iz, ix, iy, iz);
  // ab
  const float t_ab = pm_clamp01(pm_dot(vx, vy, vz, e0x, e0y, e0z) * t.e0.w);
  const float abx = vx - t_ab * e0x, aby = vy - t_ab * e0y, abz = vz - t_ab * e0z;
  const float d_ab = pm_dot(abx, aby, abz, abx, aby, abz);
  // bc
  const float ux = vx - e0x, uy = vy - e0y, uz = vz - e0z;
  const float ebx = e1x - e0x, eby = e1y - e0y, ebz = e1z - e0z;
  const float t_bc = pm_clamp01(pm_dot(ux, uy, uz, ebx, eby, ebz) * t.n.w);
  const float bcx = ux - t_bc * ebx, bcy = uy - t_bc * eby, bcz = uz - t_bc * ebz;
  const float d_bc = pm_dot(bcx, bcy, bcz, bcx, bcy, bcz);
  // ca, walked from a
  const float t_ca = pm_clamp01(pm_dot(vx, vy, vz, e1x, e1y, e1z) * t.e1.w);
  const float cax = vx - t_ca * e1x, cay = vy - t_ca * e1y, caz = vz - t_ca * e1z;
  const float d_ca = pm_dot(cax, cay, caz, cax, cay, caz);
  const bool s_ab = !inside || d_ab < d_in;
  float d = s_ab ? d_ab : d_in;
  const bool s_bc = d_bc < d;
  d = s_bc ? d_bc : d;
  const bool s_ca = d_ca < d;
  d = s_ca ? d_ca : d;
  if (kOut) {
    w[0] = s_ca ? 1.0f - t_ca : s_bc ? 0.0f : s_ab ? 1.0f - t_ab : w0;
    w[1] = s_ca ? 0.0f : s_bc ? 1.0f - t_bc : s_ab ? t_ab : w1;
    w[2] = s_ca ? t_ca : s_bc ? t_bc : s_ab ? 0.0f : w2;
    r[0] = s_ca ? cax : s_bc ? bcx : s_ab ? abx : ix;
    r[1] = s_ca ? cay : s_bc ? bcy : s_ab ? aby : iy;
    r[2] = s_ca ? caz : s_bc ? bcz : s_ab ? abz : iz;
  }
  return d;
}

__device__ __forceinline__ uint64_t pm_key(const float d, const uint32_t index) { return ((uint64_t)__float_as_uint(d) << 32) | index; }

template <int kWaves>
__device__ __forceinline__ uint64_t pm_min_keys(const uint64_t (*keys)[64], const int lane) {
  uint64_t best = keys[0][lane];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = keys[w][lane] < best ? keys[w][lane] : best;
  return best;
}

// ---- the two searches ---------------------------------------------------------------------------------------------------------

// 64 points a workgroup (lane = point), wave w of kWaves takes records [w T / kWaves, (w + 1) T / kWaves) of every tile of T = 256
// (kWaves = 1: the -DVOGE_AB build's unsplit form, what the split is measured against)
template <int kWaves>
__global__ void __launch_bounds__(64 * kWaves)
pm_point_kernel(const float *__restrict__ points, const int P, const float *__restrict__ verts, const int V,
                const int32_t *__restrict__ faces, const int F, int32_t *__restrict__ face_idx, float *__restrict__ d2,
                float *__restrict__ bary) {
  __shared__ PmRec tile[kPmFaceTile];
  __shared__ uint64_t keys[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t qi = (size_t)blockIdx.x * 64 + lane;
  const size_t qr = qi < (size_t)P ? qi : (size_t)P - 1;      // (a lane past the end repeats the last point and writes nothing)
  const float px = points[3 * qr], py = points[3 * qr + 1], pz = points[3 * qr + 2];
  uint64_t best = ~0ull;
  for (int t0 = 0; t0 < F; t0 += kPmFaceTile) {
    const int n = min(kPmFaceTile, F - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 64 * kWaves) tile[k] = pm_record(verts, V, faces, (size_t)t0 + k);
    __syncthreads();
    const int k0 = wave * (kPmFaceTile / kWaves), k1 = min(k0 + kPmFaceTile / kWaves, n);
#pragma unroll 2
    for (int k = k0; k < k1; ++k) {
      const PmRec t = tile[k];
      const uint64_t key = pm_key(pm_pair<false>(t, px, py, pz, nullptr, nullptr), (uint32_t)(t0 + k));
      best = key < best ? key : best;
    }
  }
  keys[wave][lane] = best;
  __syncthreads();
  if (wave != 0 || qi >= (size_t)P) return;
  best = pm_min_keys<kWaves>(keys, lane);
  const uint32_t fi = (uint32_t)(best & 0xffffffffull);
  const bool ok = best != ~0ull && fi < (uint32_t)F;
  float w[3] = {0.0f, 0.0f, 0.0f}, r[3];
  if (ok) pm_pair<true>(pm_record(verts, V, faces, fi), px, py, pz, w, r);
  face_idx[qi] = ok ? (int32_t)fi : -1;
  d2[qi] = ok ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
  bary[3 * qi] = w[0]; bary[3 * qi + 1] = w[1]; bary[3 * qi + 2] = w[2];
}

// 64 triangles a workgroup (lane = triangle, its record in registers), wave w of kWaves takes its share of every tile of 1024 points
template <int kWaves>
__global__ void __launch_bounds__(64 * kWaves)
pm_face_kernel(const float *__restrict__ points, const int P, const float *__restrict__ verts, const int V,
               const int32_t *__restrict__ faces, const int F, int32_t *__restrict__ point_idx, float *__restrict__ d2,
               float *__restrict__ bary) {
  __shared__ float4 tile[kPmPointTile];
  __shared__ uint64_t keys[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t fi = (size_t)blockIdx.x * 64 + lane;
  const PmRec t = pm_record(verts, V, faces, fi < (size_t)F ? fi : (size_t)F - 1);
  uint64_t best = ~0ull;
  for (int t0 = 0; t0 < P; t0 += kPmPointTile) {
    const int n = min(kPmPointTile, P - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 64 * kWaves) {
      const float *p = points + 3 * ((size_t)t0 + k);
      tile[k] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    __syncthreads();
    const int k0 = wave * (kPmPointTile / kWaves), k1 = min(k0 + kPmPointTile / kWaves, n);
#pragma unroll 2
    for (int k = k0; k < k1; ++k) {
      const float4 p = tile[k];
      const uint64_t key = pm_key(pm_pair<false>(t, p.x, p.y, p.z, nullptr, nullptr), (uint32_t)(t0 + k));
      best = key < best ? key : best;
    }
  }
  keys[wave][lane] = best;
  __syncthreads();
  if (wave != 0 || fi >= (size_t)F) return;
  best = pm_min_keys<kWaves>(keys, lane);
  const uint32_t pi = (uint32_t)(best & 0xffffffffull);
  const bool ok = best != ~0ull && pi < (uint32_t)P;
  float w[3] = {0.0f, 0.0f, 0.0f}, r[3];
  if (ok) pm_pair<true>(t, points[3 * (size_t)pi], points[3 * (size_t)pi + 1], points[3 * (size_t)pi + 2], w, r);
  point_idx[fi] = ok ? (int32_t)pi : -1;
  d2[fi] = ok ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
  bary[3 * fi] = w[0]; bary[3 * fi + 1] = w[1]; bary[3 * fi + 2] = w[2];
}

// ---- backward -----------------------------------------------------------------------------------------------------------------

// item t < P: point t with its face; item P + f: face f with its point (point_idx == nullptr, the single-directional form: no such
// items).  Adds - u fl(w_k r) 2^s to the three vertices of the face and, for a face item, u r 2^s to the point
__global__ void __launch_bounds__(256)
pm_scatter_kernel(const float *__restrict__ points, const int P, const float *__restrict__ verts, const int V,
                  const int32_t *__restrict__ faces, const int F, const int32_t *__restrict__ face_idx, const float *__restrict__ bary_p,
                  const int32_t *__restrict__ point_idx, const float *__restrict__ bary_f, const int32_t *__restrict__ meta,
                  const double u_p, const double u_f, long long *__restrict__ acc_v, long long *__restrict__ acc_p) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool first = t < (size_t)P;
  if (!first && (!point_idx || t >= (size_t)P + (size_t)F)) return;
  const size_t own = first ? t : t - (size_t)P;
  const int other = (first ? face_idx : point_idx)[own];
  if (other < 0 || other >= (first ? F : P)) return;
  const size_t f = first ? (size_t)other : own, i = first ? own : (size_t)other;
  const int iv[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  if ((unsigned)iv[0] >= (unsigned)V || (unsigned)iv[1] >= (unsigned)V || (unsigned)iv[2] >= (unsigned)V) return;
  float w[3], r[3];
  pm_pair<true>(pm_record(verts, V, faces, f), points[3 * i], points[3 * i + 1], points[3 * i + 2], w, r);
  const float *b = (first ? bary_p : bary_f) + 3 * own;
  const double scale = ldexp(first ? u_p : u_f, meta[0]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float wk = b[k];
    if (wk == 0.0f) continue;      // (an edge or a corner: the vertex across gets nothing)
    long long *acc = acc_v + 3 * (size_t)iv[k];
    atomic_add_i64(acc, llrint((double)(-(wk * r[0])) * scale));
    atomic_add_i64(acc + 1, llrint((double)(-(wk * r[1])) * scale));
    atomic_add_i64(acc + 2, llrint((double)(-(wk * r[2])) * scale));
  }
  if (!first) {
    long long *acc = acc_p + 3 * i;
    atomic_add_i64(acc, llrint((double)r[0] * scale));
    atomic_add_i64(acc + 1, llrint((double)r[1] * scale));
    atomic_add_i64(acc + 2, llrint((double)r[2] * scale));
  }
}

// one row a thread, the V vertices then the P points: g = 2 G (acc 2^-s [+ u_p r_i]), every element written
__global__ void __launch_bounds__(256)
pm_finish_kernel(const float *__restrict__ points, const int P, const float *__restrict__ verts, const int V,
                 const int32_t *__restrict__ faces, const int F, const int32_t *__restrict__ face_idx, const int32_t *__restrict__ meta,
                 const long long *__restrict__ acc, const float *__restrict__ g_loss, const double u_p, float *__restrict__ g_verts,
                 float *__restrict__ g_points) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)V + (size_t)P) return;
  const double G = 2.0 * (double)g_loss[0], unscale = ldexp(1.0, -meta[0]);
  double own[3] = {0.0, 0.0, 0.0};
  float *g = g_verts + 3 * t;
  if (t >= (size_t)V) {
    const size_t i = t - (size_t)V;
    g = g_points + 3 * i;
    const int f = face_idx[i];
    if (f >= 0 && f < F) {
      const PmRec rec = pm_record(verts, V, faces, (size_t)f);
      float w[3], r[3];
      pm_pair<true>(rec, points[3 * i], points[3 * i + 1], points[3 * i + 2], w, r);
      if (rec.a.x == rec.a.x)      // (not the record of a face with a vertex out of range)
        for (int k = 0; k < 3; ++k) own[k] = u_p * (double)r[k];
    }
  }
  g[0] = (float)(G * ((double)acc[3 * t] * unscale + own[0]));
  g[1] = (float)(G * ((double)acc[3 * t + 1] * unscale + own[1]));
  g[2] = (float)(G * ((double)acc[3 * t + 2] * unscale + own[2]));
}

}  // namespace voge

#include "point_mesh_grid.h"      // the grid route: kernels, layout and pm_grid_searches

namespace voge {

// ---- host ---------------------------------------------------------------------------------------------------------------------

enum { kPmSum = 1, kPmSingle = 2, kPmGridPairs = 4 };      // (bit 2, the backward only: the pairs came from the grid route, no pair cap)

struct PmLayout {
  size_t d2p, d2f, psum, pmax, total;
};
static PmLayout pm_layout(const long V, const long F, const long P) {
  PmLayout l;
  const size_t nb_loss = chamfer_loss_blocks(P) + chamfer_loss_blocks(F);
  Carve c;
  l.d2p = c.take((size_t)P * 4);
  l.d2f = c.take((size_t)F * 4);
  l.psum = c.take(nb_loss * sizeof(double));
  l.pmax = c.take(nb_loss * sizeof(float));
  const size_t bwd = (size_t)(V + P) * 3 * sizeof(long long);      // the backward's accumulators, a call of its own
  l.total = c.at > bwd ? c.at : bwd;
  return l;
}

// The waves of a workgroup: 16 while the queries make fewer than kPmWideBelow workgroups (at 4 waves each they would leave SIMDs
// idle: the MI355X has 1024), else 4 -- measured, profiles/r25_point_mesh.txt.  The winner is the minimum of the keys: no bit
// depends on the choice.  -DVOGE_AB builds can force 1, 4 or 16 (voge_debug_point_mesh_waves; 0: this rule).
constexpr long kPmWideBelow = 1024;
#ifdef VOGE_AB
static int pm_waves = 0;
#endif

static int pm_choose_waves(const long queries) {
#ifdef VOGE_AB
  if (pm_waves) return pm_waves;
#endif
  return (queries + 63) / 64 < kPmWideBelow ? 16 : 4;
}

template <int kWaves>
static void pm_launch(const bool by_face, const float *points, const long P, const float *verts, const long V, const int32_t *faces,
                      const long F, int32_t *idx, float *d2, float *bary, hipStream_t st) {
  const dim3 grid((unsigned)(((by_face ? F : P) + 63) / 64)), block(64 * kWaves);
  if (by_face)
    hipLaunchKernelGGL(pm_face_kernel<kWaves>, grid, block, 0, st, points, (int)P, verts, (int)V, faces, (int)F, idx, d2, bary);
  else
    hipLaunchKernelGGL(pm_point_kernel<kWaves>, grid, block, 0, st, points, (int)P, verts, (int)V, faces, (int)F, idx, d2, bary);
}

// by_face false: the nearest face of every point; true: the nearest point of every face
static void pm_search(const bool by_face, const float *points, const long P, const float *verts, const long V, const int32_t *faces,
                      const long F, int32_t *idx, float *d2, float *bary, hipStream_t st) {
  const int waves = pm_choose_waves(by_face ? F : P);
#ifdef VOGE_AB
  if (waves == 1) return pm_launch<1>(by_face, points, P, verts, V, faces, F, idx, d2, bary, st);
#endif
  if (waves == 16) return pm_launch<16>(by_face, points, P, verts, V, faces, F, idx, d2, bary, st);
  pm_launch<4>(by_face, points, P, verts, V, faces, F, idx, d2, bary, st);
}

static bool pm_size_ok(const long n) { return n >= 1 && n <= kPmMaxN; }
static bool pm_pairs_ok(const long F, const long P) { return (double)F * (double)P <= kPmMaxPairs; }

}  // namespace voge

using namespace voge;

#ifdef VOGE_AB
// (not part of the ABI: the -DVOGE_AB build only, like voge_debug_sweep_variant) 0: the rule; 1, 4, 16: that many waves a workgroup
extern "C" int voge_debug_point_mesh_waves(int waves) {
  if (waves != 0 && waves != 1 && waves != 4 && waves != 16) return VOGE_ERR_BAD_ARG;
  pm_waves = waves;
  return 0;
}
#endif

extern "C" size_t voge_point_mesh_workspace_bytes(long V, long F, long P) {
  if (!pm_size_ok(V) || !pm_size_ok(F) || !pm_size_ok(P)) return 0;
  return pm_layout(V, F, P).total;
}

extern "C" int voge_closest_faces(const float *points, long P, const float *verts, long V, const int32_t *faces, long F,
                                  int32_t *face_idx, float *d2, float *bary, voge_stream_t stream) {
  if (P < 0 || P > kPmMaxN || !pm_size_ok(V) || !pm_size_ok(F)) return VOGE_ERR_BAD_ARG;
  if (!pm_pairs_ok(F, P)) return VOGE_ERR_K_TOO_LARGE;
  if (P == 0) return 0;
  if (!points || !verts || !faces || !face_idx || !d2 || !bary) return VOGE_ERR_BAD_ARG;
  pm_search(false, points, P, verts, V, faces, F, face_idx, d2, bary, (hipStream_t)stream);
  return launch_status();
}

extern "C" int voge_point_mesh_fwd(const float *verts, long V, const int32_t *faces, long F, const float *points, long P, int flags,
                                   float *loss, int32_t *face_idx, float *bary_p, int32_t *point_idx, float *bary_f, int32_t *meta,
                                   void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (!pm_size_ok(V) || !pm_size_ok(F) || !pm_size_ok(P) || (flags & ~3)) return VOGE_ERR_BAD_ARG;
  if (!pm_pairs_ok(F, P)) return VOGE_ERR_K_TOO_LARGE;
  const bool both = !(flags & kPmSingle);
  if (!verts || !faces || !points || !loss || !face_idx || !bary_p || (both && (!point_idx || !bary_f)) || !meta || bad_workspace(workspace))
    return VOGE_ERR_BAD_ARG;
  const PmLayout l = pm_layout(V, F, P);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  float *d2p = reinterpret_cast<float *>(ws + l.d2p), *d2f = reinterpret_cast<float *>(ws + l.d2f);
  pm_search(false, points, P, verts, V, faces, F, face_idx, d2p, bary_p, st);
  if (both) pm_search(true, points, P, verts, V, faces, F, point_idx, d2f, bary_f, st);
  // P + F, the items of the backward's scatter (a point or a face each): no scatter list is longer
  chamfer_loss_launch(d2p, P, d2f, F, both, flags & kPmSum, P + F, reinterpret_cast<double *>(ws + l.psum),
                      reinterpret_cast<float *>(ws + l.pmax), loss, meta, st);
  return launch_status();
}

extern "C" size_t voge_point_mesh_grid_workspace_bytes(long V, long F, long P) {
  if (!pm_size_ok(V) || !pm_size_ok(F) || !pm_size_ok(P)) return 0;
  return pm_grid_layout(V, F, P).total;
}

static bool pm_cell_size_ok(const float cell_size) { return cell_size >= 0.0f && cell_size < INFINITY; }      // (0: the default cell)

extern "C" int voge_closest_faces_grid(const float *points, long P, const float *verts, long V, const int32_t *faces, long F,
                                       float cell_size, int32_t *face_idx, float *d2, float *bary, void *workspace,
                                       size_t workspace_bytes, voge_stream_t stream) {
  if (P < 0 || P > kPmMaxN || !pm_size_ok(V) || !pm_size_ok(F) || !pm_cell_size_ok(cell_size)) return VOGE_ERR_BAD_ARG;
  if (P == 0) return 0;
  if (!points || !verts || !faces || !face_idx || !d2 || !bary || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const PmGridLayout l = pm_grid_layout(V, F, P);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  pm_grid_searches(points, P, verts, V, faces, F, cell_size, false, face_idx, d2, bary, nullptr, nullptr, nullptr,
                   static_cast<char *>(workspace), l, (hipStream_t)stream);
  return launch_status();
}

extern "C" int voge_point_mesh_fwd_grid(const float *verts, long V, const int32_t *faces, long F, const float *points, long P, int flags,
                                        float cell_size, float *loss, int32_t *face_idx, float *bary_p, int32_t *point_idx,
                                        float *bary_f, int32_t *meta, void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (!pm_size_ok(V) || !pm_size_ok(F) || !pm_size_ok(P) || (flags & ~3) || !pm_cell_size_ok(cell_size)) return VOGE_ERR_BAD_ARG;
  const bool both = !(flags & kPmSingle);
  if (!verts || !faces || !points || !loss || !face_idx || !bary_p || (both && (!point_idx || !bary_f)) || !meta || bad_workspace(workspace))
    return VOGE_ERR_BAD_ARG;
  const PmGridLayout l = pm_grid_layout(V, F, P);
  if (workspace_bytes < l.total) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  float *d2p = reinterpret_cast<float *>(ws + l.d2p), *d2f = reinterpret_cast<float *>(ws + l.d2f);
  pm_grid_searches(points, P, verts, V, faces, F, cell_size, both, face_idx, d2p, bary_p, point_idx, d2f, bary_f, ws, l, st);
  // P + F: every scatter list of the backward, as in voge_point_mesh_fwd -- the two routes share it
  chamfer_loss_launch(d2p, P, d2f, F, both, flags & kPmSum, P + F, reinterpret_cast<double *>(ws + l.psum),
                      reinterpret_cast<float *>(ws + l.pmax), loss, meta, st);
  return launch_status();
}

extern "C" int voge_point_mesh_bwd(const float *verts, long V, const int32_t *faces, long F, const float *points, long P,
                                   const int32_t *face_idx, const float *bary_p, const int32_t *point_idx, const float *bary_f,
                                   const int32_t *meta, const float *g_loss, int flags, float *g_verts, float *g_points,
                                   void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (!pm_size_ok(V) || !pm_size_ok(F) || !pm_size_ok(P) || (flags & ~7)) return VOGE_ERR_BAD_ARG;
  if (!(flags & kPmGridPairs) && !pm_pairs_ok(F, P)) return VOGE_ERR_K_TOO_LARGE;
  const bool both = !(flags & kPmSingle);
  if (!verts || !faces || !points || !face_idx || !bary_p || (both && (!point_idx || !bary_f)) || !meta || !g_loss || !g_verts ||
      !g_points || bad_workspace(workspace))
    return VOGE_ERR_BAD_ARG;
  const size_t acc_bytes = (size_t)(V + P) * 3 * sizeof(long long);
  if (workspace_bytes < acc_bytes) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  long long *acc_v = static_cast<long long *>(workspace), *acc_p = acc_v + 3 * (size_t)V;
  const hipError_t fe = voge_fill_async(workspace, 0, acc_bytes, st);
  if (fe != hipSuccess) return (int)fe;
  const bool sum = flags & kPmSum;
  const double u_p = sum ? 1.0 : 1.0 / (double)P, u_f = sum ? 1.0 : 1.0 / (double)F;
  const long items = P + (both ? F : 0);
  hipLaunchKernelGGL(pm_scatter_kernel, dim3(blocks256(items)), dim3(256), 0, st, points, (int)P, verts, (int)V, faces,
                     (int)F, face_idx, bary_p, both ? point_idx : nullptr, bary_f, meta, u_p, u_f, acc_v, acc_p);
  hipLaunchKernelGGL(pm_finish_kernel, dim3(blocks256(V + P)), dim3(256), 0, st, points, (int)P, verts, (int)V, faces,
                     (int)F, face_idx, meta, acc_v, g_loss, u_p, g_verts, g_points);
  return launch_status();
}
