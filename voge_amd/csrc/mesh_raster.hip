// Mesh depth maps (EXTENSION: PyTorch3D's rasterize_meshes with one face a pixel): the nearest face under every pixel by an exact
// ray-triangle test, its barycentric weights and get_depth's depth.  Aggregation.mesh_rasterize IS the definition, seven steps;
// this file follows them operation for operation (-ffp-contract=off, IEEE division and square root), so pix_to_face, bary and depth
// carry the definition's fp32 bits.
//
// RECORDS, one thread per (view, face) (mr_records_kernel): the corners in view space, p = ((x0 R0k + x1 R1k) + x2 R2k) + Tk; the
// record n_a = b x c, n_b = c x a, n_c = a x b, each component (p q) - (r s), and the corners' z: 12 floats; and a conservative
// screen box (x0, x1, y0, y1, inclusive; x0 > x1: empty), 64 bytes in all.  A face that names a vertex outside [0, V) gets NaN
// records and an empty box: it hits nothing (the definition raises instead; nothing is read back here to do that).
//
// THE BOX.  u = 2^-24.  Let a, b, c be the stored corners (exact fp32 numbers), d = (d0, d1, 1) the ray a lane computes, n^ = the
// exact cross products of the stored corners and w^_i = d . n^_i.  Then sum_i w^_i p_i = vol d with vol = a . (b x c): the z and x
// rows give sum_i w^_i z_i = vol and d0 = sum_i mu_i delta_i, mu_i = w^_i z_i / vol, sum mu_i = 1, delta_i = x_i / z_i the corner's
// own direction -- the ray is an affine combination of the projected corners.  The lane's w_i differs from w^_i by at most
//     E = 8 u M |d|,      M = the largest squared corner norm:
// a component of n is fl(fl(p q) - fl(r s)), off by 2 u (|p q| + |r s|) <= 2 u M, which d spreads to (|d0| + |d1| + 1) 2 u M
// <= 2 sqrt(3) u M |d|; the three roundings of (d0 n0 + d1 n1) + n2 add 3 u |d| |n| <= 3 u M |d|: 6.5 u M |d| in all.  A hit has
// w_i >= 0 (or all <= 0), so w^_i >= -E (<= E), and with every z_i > 0: mu_i >= -nu where vol has the arm's sign, mu_i in
// [1 - 2 nu, nu] where it has not, nu = E zmax / |vol|.  Either way the negative weights sum to at most 4 nu, and
//     d0 in [dmin - 4 nu (dmax - dmin), dmax + 4 nu (dmax - dmin)],      dmin, dmax over the three corners.
// The lane's d0 = fl(fl(px - (j + 0.5)) / fx) is within 2 u |d0| of the pixel centre's, so the centre j + 0.5 = px - fx d0 lies in the
// interval above widened by 4 u max|d0|, mapped through px - fx d; 2^-10 pixel is added on top for the fp64 arithmetic this is
// evaluated in (ten orders above its roundings).  Rows alike.  The box is the WHOLE IMAGE when a corner has z <= 2^-16 sqrt(M)
// (its direction is meaningless), when vol = 0 (the face's plane holds the camera centre: every ray is "near" it) or when anything
// above is not finite (a NaN corner: such a face hits nothing anyway); it is EMPTY when every corner has z <= 0: then
// z = (bary_a a_z + bary_b b_z) + bary_c c_z <= 0 exactly, the computed bary being >= 0 exactly.  tests/test_gpu_mesh_raster.py
// holds the two routes to the same bits on every case: a box that is too small shows there.
//
// RASTER, ONE kernel for both routes (mr_raster_kernel): a workgroup of 256 lanes is a tile of 16 x 16 pixels, one pixel a lane.
// The candidates -- all F records (route "brute") or the tile's own list (route "bins") -- go through LDS in chunks
// of 256: lane t reads candidate c0 + t and stages its 12 floats and its index when its box meets the tile (a ballot compacts
// them; the order inside a chunk is arbitrary).  Every lane then runs steps 4 - 5 on the staged records and keeps its best hit as
// ONE 64-bit key, the bits of z (positive: its bits order as it does) above the face index, under min: the lexicographically
// smallest (z, index) whatever the order of the faces or the split of the list.  At the end the lane reads the winner's record
// again and evaluates bary and depth = z sqrt((d0 d0 + d1 d1) + 1) with the same function the walk used.
//   brute: records, raster -- two launches, nothing read back (capturable): the meshes of a fitting loop.
//   bins:  records; zero fill of the tables; mr_count_kernel (integer atomics on the tile counters, and the 64-bit total); the
//          two-level integer scan of mesh_scan.h; the host reads ONE number, the total, to size the list (one synchronisation);
//          mr_fill_kernel (an atomic cursor a tile: arbitrary order, which the key does not see); raster over each tile's list.
//
// ACCURACY against the definition in fp64 on the same fp32 inputs, where both choose the same face.  P = the largest
// |x0 R0k| + |x1 R1k| + |x2 R2k| + |Tk| over the face's corners, rM = sqrt(M), zr = zmax - zmin:
//   e_p = 4 u P                                   a view-space coordinate (three products, three sums);
//   e_n = 2 u M + 2 sqrt(2) e_p rM                a component of n: its own roundings and the corners' (|b1| + |b2| <= sqrt(2) |b|);
//   e_w = |d| (5 u M + sqrt(3) e_n)               w: its three roundings, the two of d0 / d1, and n's error spread by d;
//   e_b = 4 e_w / |det| + 3 u                     bary_i = w_i / det, det off by 3 e_w + 2 u |det| (the w share one sign);
//   e_z = 2 e_b zr + e_p + 8 u zmax               z: the bary sum to 1 within 5 u, so only the SPREAD of the corners' z meets e_b;
//   depth: |d| (e_z + 3 u z).
// Derived, not fitted; tests/mesh_raster_cases.py restates them.  They are first order in u: the marks of step 7 take out the
// pixels where |det| is so small that the second order counts.
//
// BACKWARD, depth -> verts (pix_to_face and bary carry none, the cameras none).  For a covered pixel z = vol / det, and
//     d depth / d p_i = |d| bary_i N / det,      N = n_a + n_b + n_c = (b - a) x (c - a),  p_i the corner in view space:
// d z / d a = (n_a - z d x (c - b)) / det = (b - q) x (c - q) / det with q = z d the hit point, and (b - q) x (c - q) = bary_a N for
// a point of the face's plane.  The nine terms g |d| bary_i N_k / det are evaluated in fp64 from the fp32 inputs at the forward's
// face and summed in FIXED POINT (fixed_point.h): zero fill of the head and of acc [B][V][4]; mr_bwd_absmax_kernel (D = the largest
// finite |term|, rounded up to fp32); mr_bwd_scatter_kernel (round(term 2^s) with 64-bit INTEGER atomics into the view's own
// accumulators, 2^L >= B H W; a term that is not finite adds 1 to the fourth slot instead); mr_bwd_finish_kernel, one thread a
// vertex: g_x_j = sum_b sum_k R_b[j][k] acc[b][v][k] 2^-s in fp64 -- the rotation back through R^T -- rounded once; NaN where a term
// was not finite.  No float atomics, nothing read back, the same bits on every run and in every order of the faces.  Error: m
// terms at a vertex are off by m q / 2 per view-space component, q = 2^-s <= 2^(L - 61) D.  Lanes of a wave that hold the same
// face (a face under many pixels) add their terms in the wave first -- integer sums, the same bits -- and commit them once.
#include <math.h>

#include "voge_common.h"
#include "fixed_point.h"
#include "mesh_scan.h"

namespace voge {

constexpr int kMrTile = 16;                 // a tile's edge in pixels; 256 lanes = one workgroup (ops.MESH_RASTER_TILE)
constexpr int kMrChunk = 256;               // records of one LDS chunk
constexpr long kMrMaxPixels = 2147483647l;  // B H W < 2^31
constexpr long kMrMaxPairs = 1l << 36;      // B F: the grid of the records launch

struct __attribute__((aligned(16))) MrRec {
  float n[9];      // n_a, n_b, n_c
  float z[3];      // a_z, b_z, c_z
  int x0, x1, y0, y1;
};
static_assert(sizeof(MrRec) == 64, "MrRec is four 16-byte words");

struct MrHit {
  float w[3], det;
  bool hit;      // step 5 without z > 0
};

// steps 4 and 5 (the signs) of one ray against one record
__device__ __forceinline__ MrHit mr_edges(const float *__restrict__ n, const float d0, const float d1, const int cull) {
  MrHit h;
#pragma unroll
  for (int i = 0; i < 3; ++i) h.w[i] = (d0 * n[3 * i] + d1 * n[3 * i + 1]) + n[3 * i + 2];
  h.det = (h.w[0] + h.w[1]) + h.w[2];
  const bool front = h.w[0] >= 0.0f && h.w[1] >= 0.0f && h.w[2] >= 0.0f && h.det > 0.0f;
  const bool back = h.w[0] <= 0.0f && h.w[1] <= 0.0f && h.w[2] <= 0.0f && h.det < 0.0f;
  h.hit = back || (front && !cull);
  return h;
}

// bary_i = w_i / det, z = (bary_a a_z + bary_b b_z) + bary_c c_z
__device__ __forceinline__ float mr_depth_z(const MrHit &h, const float *__restrict__ z, float (&bary)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) bary[i] = h.w[i] / h.det;
  return (bary[0] * z[0] + bary[1] * z[1]) + bary[2] * z[2];
}

// step 2: the ray of pixel column j (row i with the second focal length and principal point)
__device__ __forceinline__ float mr_dir(const float pp, const float f, const int j) { return (pp - ((float)j + 0.5f)) / f; }

// step 1, T = float: the records; T = double: the backward
template <typename T>
__device__ __forceinline__ void mr_view_point(const float *__restrict__ x, const float *__restrict__ R, const float *__restrict__ t, T (&p)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = (((T)x[0] * (T)R[k] + (T)x[1] * (T)R[3 + k]) + (T)x[2] * (T)R[6 + k]) + (T)t[k];
}

// step 3: u x v, each component (p q) - (r s)
template <typename T>
__device__ __forceinline__ void mr_cross(const T (&u)[3], const T (&v)[3], T *__restrict__ o) {
  o[0] = (u[1] * v[2]) - (u[2] * v[1]);
  o[1] = (u[2] * v[0]) - (u[0] * v[2]);
  o[2] = (u[0] * v[1]) - (u[1] * v[0]);
}

// ---- records ------------------------------------------------------------------------------------------------------------------

// the pixel interval [lo, hi] (inclusive, clamped to [0, n - 1]; lo > hi: empty) whose centres j + 0.5 = pp - f d can have d in
// [dlo, dhi] (THE BOX in the header); anything not finite: the whole axis
__device__ __forceinline__ void mr_axis_box(const double dlo, const double dhi, const double pp, const double f, const int n, int &lo, int &hi) {
  const double ua = pp - f * dhi, ub = pp - f * dlo;
  const double ulo = fmin(ua, ub) - 0.5 - 0x1p-10, uhi = fmax(ua, ub) - 0.5 + 0x1p-10;
  lo = 0; hi = n - 1;
  if (!(ulo > -1e300 && uhi < 1e300)) return;      // (a NaN or an infinity)
  lo = (int)fmin(fmax(ceil(ulo), 0.0), (double)n);
  hi = (int)fmax(fmin(floor(uhi), (double)(n - 1)), -1.0);
}

__global__ void __launch_bounds__(256)
mr_records_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F, const float *__restrict__ R,
                  const float *__restrict__ T, const float *__restrict__ focal, const float *__restrict__ pp, const int B, const int H,
                  const int W, MrRec *__restrict__ recs) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * (size_t)F) return;
  const int b = (int)(i / (size_t)F), f = (int)(i - (size_t)b * (size_t)F);
  const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
  MrRec r;
  if (!face_in_range(ia, ib, ic, V)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r.n[k] = NAN;
    r.z[0] = r.z[1] = r.z[2] = NAN;
    r.x0 = r.y0 = 0; r.x1 = r.y1 = -1;
    recs[i] = r;
    return;
  }
  float p[3][3];
  mr_view_point<float>(verts + 3 * (size_t)ia, R + 9 * b, T + 3 * b, p[0]);
  mr_view_point<float>(verts + 3 * (size_t)ib, R + 9 * b, T + 3 * b, p[1]);
  mr_view_point<float>(verts + 3 * (size_t)ic, R + 9 * b, T + 3 * b, p[2]);
  mr_cross<float>(p[1], p[2], r.n);
  mr_cross<float>(p[2], p[0], r.n + 3);
  mr_cross<float>(p[0], p[1], r.n + 6);
  r.z[0] = p[0][2]; r.z[1] = p[1][2]; r.z[2] = p[2][2];
  // the box, in fp64 (the header's derivation)
  const double fx = focal[2 * b], fy = focal[2 * b + 1], px = pp[2 * b], py = pp[2 * b + 1];
  double M = 0.0, zmin = INFINITY, zmax = -INFINITY, dlo[2] = {INFINITY, INFINITY}, dhi[2] = {-INFINITY, -INFINITY};
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double x = p[c][0], y = p[c][1], z = p[c][2];
    M = fmax(M, (x * x + y * y) + z * z);
    zmin = fmin(zmin, z); zmax = fmax(zmax, z);
    finite = finite && fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY;
    const double e0 = x / z, e1 = y / z;
    dlo[0] = fmin(dlo[0], e0); dhi[0] = fmax(dhi[0], e0);
    dlo[1] = fmin(dlo[1], e1); dhi[1] = fmax(dhi[1], e1);
  }
  r.x0 = 0; r.x1 = W - 1; r.y0 = 0; r.y1 = H - 1;
  if (finite && zmax <= 0.0) {      // behind the camera: z <= 0 exactly, no hit
    r.x1 = -1; r.y1 = -1;
  } else if (finite && zmin > 0x1p-16 * sqrt(M)) {
    const double a0 = p[0][0], a1 = p[0][1], a2 = p[0][2], b0 = p[1][0], b1 = p[1][1], b2 = p[1][2], c0 = p[2][0], c1 = p[2][1], c2 = p[2][2];
    const double vol = fabs(a0 * (b1 * c2 - b2 * c1) + a1 * (b2 * c0 - b0 * c2) + a2 * (b0 * c1 - b1 * c0));
    const double m0 = fmax(fabs(px - 0.5), fabs(px - ((double)W - 0.5))) / fabs(fx), m1 = fmax(fabs(py - 0.5), fabs(py - ((double)H - 0.5))) / fabs(fy);
    const double E = 0x1p-21 * M * sqrt((m0 * m0 + m1 * m1) + 1.0);      // 8 u M |d|
    const double nu = E * zmax / vol;                                   // (vol = 0: not finite, the whole image)
    if (nu >= 0.0 && nu < 1e300) {
      const double pad0 = 4.0 * nu * (dhi[0] - dlo[0]) + 0x1p-22 * m0, pad1 = 4.0 * nu * (dhi[1] - dlo[1]) + 0x1p-22 * m1;
      mr_axis_box(dlo[0] - pad0, dhi[0] + pad0, px, fx, W, r.x0, r.x1);
      mr_axis_box(dlo[1] - pad1, dhi[1] + pad1, py, fy, H, r.y0, r.y1);
    }
  }
  recs[i] = r;
}

// ---- the bins route's lists ---------------------------------------------------------------------------------------------------

struct MrTiles {
  int tx0, tx1, ty0, ty1;      // the tiles a box meets, inclusive (tx0 > tx1: none)
};
__device__ __forceinline__ MrTiles mr_box_tiles(const MrRec &r) {
  MrTiles t;
  const bool any = r.x0 <= r.x1 && r.y0 <= r.y1;
  t.tx0 = r.x0 / kMrTile; t.tx1 = any ? r.x1 / kMrTile : -1;
  t.ty0 = r.y0 / kMrTile; t.ty1 = any ? r.y1 / kMrTile : -1;
  return t;
}

__global__ void __launch_bounds__(256)
mr_count_kernel(const MrRec *__restrict__ recs, const int F, const int B, const int tiles_x, const int tiles_y, uint32_t *__restrict__ count,
                unsigned long long *__restrict__ total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * (size_t)F) return;
  const int b = (int)(i / (size_t)F);
  const MrTiles t = mr_box_tiles(recs[i]);
  if (t.tx0 > t.tx1 || t.ty0 > t.ty1) return;
  uint32_t *c = count + (size_t)b * tiles_x * tiles_y;
  for (int ty = t.ty0; ty <= t.ty1 && ty < tiles_y; ++ty)
    for (int tx = t.tx0; tx <= t.tx1 && tx < tiles_x; ++tx) atomicAdd(c + (size_t)ty * tiles_x + tx, 1u);
  atomicAdd(total, (unsigned long long)(t.tx1 - t.tx0 + 1) * (unsigned long long)(t.ty1 - t.ty0 + 1));
}

// the exclusive prefix of every tile's count inside its block of kMcBlock tiles, and the block's total
__global__ void __launch_bounds__(kMcBlock)
mr_scan_local_kernel(const uint32_t *__restrict__ count, const long n, uint32_t *__restrict__ loc, uint32_t *__restrict__ blocks) {
  const long i = (long)blockIdx.x * kMcBlock + threadIdx.x;
  uint32_t upto;
  const uint32_t excl = mesh_scan_local(i < n ? count[i] : 0u, upto);
  if (i < n) loc[i] = excl;
  if (threadIdx.x == kMcBlock - 1) blocks[blockIdx.x] = upto;
}

__global__ void __launch_bounds__(kMcTop)
mr_scan_top_kernel(uint32_t *__restrict__ blocks, const long nb, const unsigned long long *__restrict__ total, long long *__restrict__ total_out) {
  mesh_scan_top(blocks, nb);
  if (threadIdx.x == 0) *total_out = (long long)*total;      // what the host reads: the 64-bit total of the count launch
}

__global__ void __launch_bounds__(256)
mr_fill_kernel(const MrRec *__restrict__ recs, const int F, const int B, const int tiles_x, const int tiles_y, const uint32_t *__restrict__ count,
               const uint32_t *__restrict__ loc, const uint32_t *__restrict__ blocks, uint32_t *__restrict__ cursor, int32_t *__restrict__ list,
               const long list_len) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * (size_t)F) return;
  const int b = (int)(i / (size_t)F), f = (int)(i - (size_t)b * (size_t)F);
  const MrTiles t = mr_box_tiles(recs[i]);
  for (int ty = t.ty0; ty <= t.ty1 && ty < tiles_y; ++ty)
    for (int tx = t.tx0; tx <= t.tx1 && tx < tiles_x; ++tx) {
      const size_t bt = ((size_t)b * tiles_y + ty) * tiles_x + tx;
      const uint32_t slot = atomicAdd(cursor + bt, 1u);
      const size_t at = (size_t)blocks[bt / kMcBlock] + loc[bt] + slot;
      if (slot < count[bt] && at < (size_t)list_len) list[at] = f;      // (always: the counts were made from the same boxes)
    }
}

// ---- raster -------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
mr_raster_kernel(const MrRec *__restrict__ recs, const int F, const float *__restrict__ focal, const float *__restrict__ pp, const int H,
                 const int W, const int tiles_x, const int tiles_y, const int cull, const int binned, const int32_t *__restrict__ list, const long list_len,
                 const uint32_t *__restrict__ count, const uint32_t *__restrict__ loc, const uint32_t *__restrict__ blocks,
                 int32_t *__restrict__ pix_to_face, float *__restrict__ bary_out, float *__restrict__ depth_out) {
  __shared__ float4 srec[kMrChunk][3];
  __shared__ int sidx[kMrChunk];
  __shared__ int scount;
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t bt = blockIdx.x;
  const int per = tiles_x * tiles_y;
  const int b = (int)(bt / (size_t)per), t = (int)(bt - (size_t)b * per);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int px0 = tx * kMrTile, py0 = ty * kMrTile;
  const int j = px0 + (tid & (kMrTile - 1)), i = py0 + (tid >> 4);
  const float d0 = mr_dir(pp[2 * b], focal[2 * b], j), d1 = mr_dir(pp[2 * b + 1], focal[2 * b + 1], i);
  const MrRec *__restrict__ vrec = recs + (size_t)b * (size_t)F;
  size_t start = 0;
  long n = F;
  if (binned) {
    start = (size_t)blocks[bt / kMcBlock] + loc[bt];
    n = count[bt];
    if (start + (size_t)n > (size_t)list_len) n = 0;      // (never: the total the host read covers every list)
  }
  unsigned long long best = ~0ull;
  for (long c0 = 0; c0 < n; c0 += kMrChunk) {
    __syncthreads();      // (the chunk before is done with)
    if (tid == 0) scount = 0;
    __syncthreads();
    const long c = c0 + tid;
    int f = -1;
    if (c < n) f = binned ? list[start + c] : (int)c;
    bool stage = false;
    const float4 *src = nullptr;
    if ((unsigned)f < (unsigned)F) {
      src = reinterpret_cast<const float4 *>(vrec + f);
      const int4 box = *reinterpret_cast<const int4 *>(src + 3);
      stage = box.x <= px0 + kMrTile - 1 && box.y >= px0 && box.z <= py0 + kMrTile - 1 && box.w >= py0;
    }
    const unsigned long long mask = __ballot(stage);
    int base = 0;
    if (lane == 0 && mask) base = atomicAdd(&scount, __popcll(mask));
    base = __shfl(base, 0, 64);
    if (stage) {
      const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
      srec[slot][0] = src[0]; srec[slot][1] = src[1]; srec[slot][2] = src[2];
      sidx[slot] = f;
    }
    __syncthreads();
    const int m = scount;
    for (int k = 0; k < m; ++k) {
      const float4 r0 = srec[k][0], r1 = srec[k][1], r2 = srec[k][2];
      const float rn[9] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
      const float rz[3] = {r2.y, r2.z, r2.w};
      const MrHit h = mr_edges(rn, d0, d1, cull);
      if (h.hit) {
        float bary[3];
        const float z = mr_depth_z(h, rz, bary);
        if (z > 0.0f) {
          const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)sidx[k];
          best = key < best ? key : best;
        }
      }
    }
  }
  if (i >= H || j >= W) return;
  const size_t pix = ((size_t)b * H + i) * W + j;
  int face = -1;
  float bary[3] = {0.0f, 0.0f, 0.0f}, depth = 0.0f;
  if (best != ~0ull) {
    face = (int)(unsigned)(best & 0xffffffffull);
    const MrRec r = vrec[face];
    const MrHit h = mr_edges(r.n, d0, d1, cull);
    const float z = mr_depth_z(h, r.z, bary);
    depth = z * sqrtf((d0 * d0 + d1 * d1) + 1.0f);
  }
  pix_to_face[pix] = face;
  bary_out[3 * pix] = bary[0]; bary_out[3 * pix + 1] = bary[1]; bary_out[3 * pix + 2] = bary[2];
  depth_out[pix] = depth;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------

struct MrTerms {
  double t[9];      // g |d| bary_i N_k / det at [3 i + k], view space
  int iv[3];
  bool any;         // the pixel is covered by a face whose indices are inside the tables
};

// the nine terms of one pixel in fp64 from the fp32 inputs (the header's closed form)
__device__ __forceinline__ MrTerms mr_bwd_terms(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                                                const float *__restrict__ R, const float *__restrict__ T, const float *__restrict__ focal,
                                                const float *__restrict__ pp, const int H, const int W, const int32_t *__restrict__ pix_to_face,
                                                const float *__restrict__ g_depth, const size_t pix) {
  MrTerms o;
  o.any = false;
  o.iv[0] = o.iv[1] = o.iv[2] = 0;
  const int f = pix_to_face[pix];
  if ((unsigned)f >= (unsigned)F) return o;
  o.iv[0] = faces[3 * (size_t)f]; o.iv[1] = faces[3 * (size_t)f + 1]; o.iv[2] = faces[3 * (size_t)f + 2];
  if (!face_in_range(o.iv[0], o.iv[1], o.iv[2], V)) return o;
  const size_t hw = (size_t)H * W;
  const int b = (int)(pix / hw);
  const size_t rem = pix - (size_t)b * hw;
  const int i = (int)(rem / W), j = (int)(rem - (size_t)i * W);
  const double d0 = ((double)pp[2 * b] - ((double)j + 0.5)) / (double)focal[2 * b];
  const double d1 = ((double)pp[2 * b + 1] - ((double)i + 0.5)) / (double)focal[2 * b + 1];
  double p[3][3], n[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) mr_view_point<double>(verts + 3 * (size_t)o.iv[c], R + 9 * b, T + 3 * b, p[c]);
  mr_cross<double>(p[1], p[2], n);
  mr_cross<double>(p[2], p[0], n + 3);
  mr_cross<double>(p[0], p[1], n + 6);
  double w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = (d0 * n[3 * c] + d1 * n[3 * c + 1]) + n[3 * c + 2];
  const double det = (w[0] + w[1]) + w[2];
  const double G = (double)g_depth[pix] * sqrt((d0 * d0 + d1 * d1) + 1.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = G * (w[c] / det);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[3 * c + k] = s * (((n[k] + n[3 + k]) + n[6 + k]) / det);
  }
  o.any = true;
  return o;
}

__global__ void __launch_bounds__(256)
mr_bwd_absmax_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F, const float *__restrict__ R,
                     const float *__restrict__ T, const float *__restrict__ focal, const float *__restrict__ pp, const int H, const int W,
                     const size_t npix, const int32_t *__restrict__ pix_to_face, const float *__restrict__ g_depth, FixedHead *__restrict__ head) {
  uint32_t m = 0u;
  for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * 256) {
    const MrTerms o = mr_bwd_terms(verts, V, faces, F, R, T, focal, pp, H, W, pix_to_face, g_depth, pix);
    if (!o.any) continue;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double a = fabs(o.t[k]);
      if (a < 3.0e38) {      // (finite, and finite as fp32 after the rounding up)
        float x = (float)a;
        if ((double)x < a) x = __uint_as_float(__float_as_uint(x) + 1u);      // D >= every |term|
        m = max(m, __float_as_uint(x));
      }
    }
  }
  fixed_commit_max(head, m);
}

// the sum of a 64-bit integer over the wave (in every lane)
__device__ __forceinline__ long long mr_wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)v, o, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), o, 64);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

__global__ void __launch_bounds__(256)
mr_bwd_scatter_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F, const float *__restrict__ R,
                      const float *__restrict__ T, const float *__restrict__ focal, const float *__restrict__ pp, const int H, const int W,
                      const size_t npix, const int32_t *__restrict__ pix_to_face, const float *__restrict__ g_depth,
                      const FixedHead *__restrict__ head, const int list_bits, long long *__restrict__ acc) {
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  MrTerms o;
  o.any = false;
  if (pix < npix) o = mr_bwd_terms(verts, V, faces, F, R, T, focal, pp, H, W, pix_to_face, g_depth, pix);
  const double scale = ldexp(1.0, fixed_scale_exponent(head, list_bits));
  long long q[9];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const bool fin = o.any && fabs(o.t[k]) < 3.0e38;
    bad = bad || (o.any && !fin);
    q[k] = fin ? llrint(o.t[k] * scale) : 0ll;
  }
  const int b = pix < npix ? (int)(pix / ((size_t)H * W)) : 0;
  // the wave's lanes all on one face of one view (a face under many pixels): add in the wave, commit once
  const int f = o.any ? pix_to_face[pix] : -1;
  const int f0 = __builtin_amdgcn_readfirstlane(f), b0 = __builtin_amdgcn_readfirstlane(b);
  const bool uniform = __all(f == f0 && b == b0 && !bad) && f0 >= 0 && __popcll(__ballot(1)) == 64;
  if (uniform) {
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = mr_wave_sum_i64(q[k]);
    if ((threadIdx.x & 63) != 0) return;
  } else if (!o.any) {
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    long long *a = acc + 4 * ((size_t)b * V + (size_t)o.iv[c]);
    if (bad) {
      atomic_add_i64(a + 3, 1ll);
      continue;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (q[3 * c + k]) atomic_add_i64(a + k, q[3 * c + k]);
  }
}

__global__ void __launch_bounds__(256)
mr_bwd_finish_kernel(const int V, const int B, const float *__restrict__ R, const FixedHead *__restrict__ head, const int list_bits,
                     const long long *__restrict__ acc, float *__restrict__ g_verts) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  const double inv = ldexp(1.0, -fixed_scale_exponent(head, list_bits));
  double g[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  for (int b = 0; b < B; ++b) {
    const long long *a = acc + 4 * ((size_t)b * V + v);
    bad = bad || a[3] != 0;
    const double s0 = (double)a[0], s1 = (double)a[1], s2 = (double)a[2];
    const float *r = R + 9 * b;
#pragma unroll
    for (int jx = 0; jx < 3; ++jx) g[jx] += ((double)r[3 * jx] * s0 + (double)r[3 * jx + 1] * s1) + (double)r[3 * jx + 2] * s2;
  }
#pragma unroll
  for (int jx = 0; jx < 3; ++jx) g_verts[3 * v + jx] = bad ? NAN : (float)(g[jx] * inv);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct MrLayout {
  size_t recs, count, cursor, loc, blocks, total, fwd;      // forward: records [B F], then the bins route's tables
  size_t head, acc, bwd;                                    // backward, from the front again
  long tiles_x, tiles_y, nt, nb;
};
static MrLayout mr_layout(const long B, const long V, const long F, const long H, const long W) {
  MrLayout l;
  l.tiles_x = (W + kMrTile - 1) / kMrTile;
  l.tiles_y = (H + kMrTile - 1) / kMrTile;
  l.nt = B * l.tiles_x * l.tiles_y;
  l.nb = (l.nt + kMcBlock - 1) / kMcBlock;
  Carve fwd, bwd;      // (two calls on one workspace: each starts at its front)
  l.recs = fwd.take_exact((size_t)B * (size_t)F * sizeof(MrRec));
  l.count = fwd.take((size_t)l.nt * sizeof(uint32_t));      // count, cursor and total are adjacent: one zero fill
  l.cursor = fwd.take((size_t)l.nt * sizeof(uint32_t));
  l.total = fwd.take_exact(16);
  l.loc = fwd.take((size_t)l.nt * sizeof(uint32_t));
  l.blocks = fwd.take((size_t)l.nb * sizeof(uint32_t));
  l.fwd = fwd.at;
  l.head = bwd.take_exact(sizeof(FixedHead));
  l.acc = bwd.take_exact((size_t)B * (size_t)V * 4 * sizeof(long long));
  l.bwd = bwd.at;
  return l;
}

static bool mr_sizes_ok(const long B, const long V, const long F, const long H, const long W) {
  if (B < 0 || V < 0 || F < 0 || H < 1 || W < 1 || V > kMcMax || F > kMcMax || H > kMrMaxPixels || W > kMrMaxPixels) return false;
  if (B > 0 && (H * W > kMrMaxPixels / B || (F > 0 && B > kMrMaxPairs / F) || (V > 0 && B > kMrMaxPairs / V))) return false;
  return true;
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_mesh_raster_workspace_bytes(long B, long V, long F, long H, long W) {
  if (!mr_sizes_ok(B, V, F, H, W) || B < 1) return 0;
  const MrLayout l = mr_layout(B, V, F, H, W);
  return l.fwd > l.bwd ? l.fwd : l.bwd;
}

extern "C" int voge_mesh_raster_fwd(const float *verts, long V, const int32_t *faces, long F, const float *R, const float *T, const float *focal,
                                    const float *pp, long B, long H, long W, int cull_backfaces, int stages, int32_t *list, long list_len,
                                    int32_t *pix_to_face, float *bary, float *depth, long long *total, void *workspace,
                                    size_t workspace_bytes, voge_stream_t stream) {
  if (!mr_sizes_ok(B, V, F, H, W) || B < 1 || (stages & ~15) || !stages || list_len < 0 || list_len > 2147483647l) return VOGE_ERR_BAD_ARG;
  if (!R || !T || !focal || !pp || bad_workspace(workspace) || (F > 0 && (!faces || !verts))) return VOGE_ERR_BAD_ARG;
  if ((stages & 8) && (!pix_to_face || !bary || !depth)) return VOGE_ERR_BAD_ARG;
  if ((stages & 2) && !total) return VOGE_ERR_BAD_ARG;
  if ((stages & 4) && list_len > 0 && !list) return VOGE_ERR_BAD_ARG;
  const MrLayout l = mr_layout(B, V, F, H, W);
  if (workspace_bytes < l.fwd) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  MrRec *recs = reinterpret_cast<MrRec *>(ws + l.recs);
  uint32_t *count = reinterpret_cast<uint32_t *>(ws + l.count), *cursor = reinterpret_cast<uint32_t *>(ws + l.cursor);
  uint32_t *loc = reinterpret_cast<uint32_t *>(ws + l.loc), *blocks = reinterpret_cast<uint32_t *>(ws + l.blocks);
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(ws + l.total);
  const long pairs = B * F;
  if ((stages & 1) && pairs > 0)
    hipLaunchKernelGGL(mr_records_kernel, dim3(blocks256(pairs)), dim3(256), 0, st, verts, (int)V, faces, (int)F, R, T, focal, pp, (int)B, (int)H,
                       (int)W, recs);
  if (stages & 2) {
    const hipError_t fe = voge_fill_async(ws + l.count, 0, l.loc - l.count, st);      // count, cursor, total
    if (fe != hipSuccess) return (int)fe;
    if (pairs > 0)
      hipLaunchKernelGGL(mr_count_kernel, dim3(blocks256(pairs)), dim3(256), 0, st, recs, (int)F, (int)B, (int)l.tiles_x, (int)l.tiles_y, count, tot);
    hipLaunchKernelGGL(mr_scan_local_kernel, dim3((unsigned)l.nb), dim3(kMcBlock), 0, st, count, l.nt, loc, blocks);
    hipLaunchKernelGGL(mr_scan_top_kernel, dim3(1), dim3(kMcTop), 0, st, blocks, l.nb, tot, total);
  }
  if ((stages & 4) && pairs > 0 && list_len > 0)
    hipLaunchKernelGGL(mr_fill_kernel, dim3(blocks256(pairs)), dim3(256), 0, st, recs, (int)F, (int)B, (int)l.tiles_x, (int)l.tiles_y, count, loc,
                       blocks, cursor, list, list_len);
  if (stages & 8) {
    hipLaunchKernelGGL(mr_raster_kernel, dim3((unsigned)l.nt), dim3(256), 0, st, recs, (int)F, focal, pp, (int)H, (int)W, (int)l.tiles_x,
                       (int)l.tiles_y, cull_backfaces ? 1 : 0, (stages & 4) ? 1 : 0 /* the lists of stage 4 */, list, list_len, count, loc, blocks, pix_to_face, bary, depth);
  }
  return launch_status();
}

extern "C" int voge_mesh_raster_bwd(const float *verts, long V, const int32_t *faces, long F, const float *R, const float *T, const float *focal,
                                    const float *pp, long B, long H, long W, const int32_t *pix_to_face, const float *g_depth, float *g_verts,
                                    void *workspace, size_t workspace_bytes, voge_stream_t stream) {
  if (!mr_sizes_ok(B, V, F, H, W) || B < 1 || V < 1) return VOGE_ERR_BAD_ARG;
  if (!verts || !R || !T || !focal || !pp || !pix_to_face || !g_depth || !g_verts || (F > 0 && !faces) || bad_workspace(workspace))
    return VOGE_ERR_BAD_ARG;
  const MrLayout l = mr_layout(B, V, F, H, W);
  if (workspace_bytes < l.bwd) return VOGE_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  FixedHead *head = reinterpret_cast<FixedHead *>(ws + l.head);
  long long *acc = reinterpret_cast<long long *>(ws + l.acc);
  const hipError_t fe = voge_fill_async(workspace, 0, l.bwd, st);
  if (fe != hipSuccess) return (int)fe;
  const size_t npix = (size_t)B * (size_t)H * (size_t)W;
  const int bits = ceil_log2((long)npix);      // B H W <= 2^bits: every list of the scatter
  if (F > 0) {
    hipLaunchKernelGGL(mr_bwd_absmax_kernel, dim3(blocks256_capped(npix)), dim3(256), 0, st, verts, (int)V, faces, (int)F, R, T, focal, pp, (int)H,
                       (int)W, npix, pix_to_face, g_depth, head);
    hipLaunchKernelGGL(mr_bwd_scatter_kernel, dim3(blocks256((long)npix)), dim3(256), 0, st, verts, (int)V, faces, (int)F, R, T, focal, pp, (int)H,
                       (int)W, npix, pix_to_face, g_depth, head, bits, acc);
  }
  hipLaunchKernelGGL(mr_bwd_finish_kernel, dim3(blocks256(V)), dim3(256), 0, st, (int)V, (int)B, R, head, bits, acc, g_verts);
  return launch_status();
}
