// Mesh extraction (EXTENSION: the reference has none; the step the 2D Gaussian splatting pipeline ends with): depth maps fused into
// a truncated signed distance volume, and marching tetrahedra on Kuhn's split of every cell.  Aggregation.tsdf_integrate and
// Aggregation.marching_tets are the definitions; neither step is differentiable.  No float atomics anywhere.
//
// voge_tsdf_integrate, one launch.  tsdf_integrate_kernel: one grid point per thread, x fastest, so the two 4-byte reads and the
//   two 4-byte writes of a wave are one contiguous 256 bytes each: 16 bytes a grid point, however many views the call has, because
//   the loop over the views runs INSIDE the kernel with tsdf and w in registers.  A view's constants (R, T, centre, focal, pp: 20
//   floats) are indexed by the loop counter alone, wave-uniform, so they arrive by scalar loads; the depth gathers of neighbouring
//   grid points hit neighbouring pixels (nearest pixel, no interpolation) and live in L2.  A wave none of whose lanes projects
//   into the image (or has a valid pixel) skips the rest of the view: every step below sits under its predecessor's condition, so
//   the compiler's branch on an empty execution mask is the skip.  The arithmetic is the definition's, operation by operation in
//   fp32 (-ffp-contract=off; x = lo + i h from the index, never an incremental p(x + 1) = p(x) + h R, whose roundings would
//   differ):  p = x @ R + T as ((x0 R0k + x1 R1k) + x2 R2k) + Tk, skipped unless p_z > 0; u = px - (fx p_x) / p_z, v likewise,
//   skipped unless 0 <= u < W and 0 <= v < H (tested on the floats: no conversion of a wild value); d = depth[b][floor v][floor u],
//   skipped unless finite and > 0; sdf = d - sqrt((dx dx + dy dy) + dz dz), dx = x - c, skipped if sdf < -trunc;
//   tsdf <- (tsdf w + min(1, sdf / trunc)) / (w + 1); w <- w + 1 or min(w + 1, max_weight).  Sequential in the views: the same
//   bits on every run, and one call with three views gives the bits of three calls with one view each.
//
// Extraction: count, scan, emit; the mesh is sized on the host between scan and emit (the caller reads totals back: the one
// synchronisation of an extraction, a one-off step).
//   voge_mtet_count, one launch, a grid point per thread, kMtBlock points a workgroup.  The point reads the (up to) eight corners of
//     the cell it is the low corner of: observed = finite (and weight > 0), inside = value < level, strictly; a corner beyond the
//     grid counts as unobserved.  It writes edge_mask (bit d - 1: the edge of direction d = 1 .. 7 -- bit 0 = +x, bit 1 = +y,
//     bit 2 = +z -- carries a vertex: both ends observed, exactly one inside), face_count (0 .. 12: the triangles of the cell's six
//     tetrahedra whose four corners are observed: 1 with one or three corners inside, 2 with two) and the EXCLUSIVE prefixes of the
//     vertex and the face counts inside its workgroup as 16-bit numbers (at most 256 x 7 and 256 x 12), and the workgroup its two
//     totals: 6 bytes a grid point, not 28.
//   voge_mtet_scan, ONE workgroup of kMtTop: the exclusive scan of the workgroups' totals in place, kMtTop entries a round with the
//     running totals carried from round to round, and totals[0] = V, totals[1] = F as 64-bit numbers.  Integer sums: no order.
//   voge_mtet_emit, one launch, a grid point per thread.  The vertex of edge (q, d) has the id
//     voff[q] + popcount(edge_mask[q] & ((1 << (d - 1)) - 1)), voff[q] = block_v[q / kMtBlock] + vloc[q]: the vertices ascend by
//     (q, d), the faces by (cell, tetrahedron, triangle) from block_f[q / kMtBlock] + floc[q].  A point with neither (two bytes
//     read) returns.  Vertex: p_a + t (p_b - p_a), t = (level - v_a) / (v_b - v_a), p = lo + i h, a the owner q: the definition's
//     operations in fp32.  Tetrahedra and the 16 cases: kMtCorner and kMtEdge below, derived by Aggregation._mtet_tables.
//     Every write is guarded by V and F, the sizes the caller allocated.
// Indices are 32-bit: nx ny nz 7 < 2^31 (the vertex ids), so a face offset, at most 12 nx ny nz < 2^32, fits an unsigned one.
//
// Attributes (colour, or any C floats a pixel carries), fused beside the distance and carried to the vertices; C is a compile-time
// number, 1 .. 8, the volume [nz,ny,nx,C] and the images [B,H,W,C] are channel last.  Both kernels are gathers: no atomics.
//   voge_tsdf_integrate_attr, one launch.  tsdf_integrate_attr_kernel<C> is tsdf_integrate_kernel's loop, operation by operation
//     (tsdf and weight come out with that kernel's bits), with C more accumulators in registers: a grid point's C floats are read
//     once and written once, a wave's rows are one contiguous span of 256 C bytes, 16 + 8 C bytes a grid point however many
//     views.  The attribute pixel -- the depth's own nearest pixel -- is read only under the last condition, where the view
//     updates the point, so a wave that skips a view still skips all of it:  attr <- (attr w + pixel) / (w + 1) per channel,
//     with the weight BEFORE its own update, every operation separate.  The values of the pixel are not examined.
//   voge_mtet_attr, one launch after voge_mtet_emit, a grid point per thread, on emit's tables (edge_mask, vloc, block_v).  A point
//     whose mask is zero returns after one byte.  For every set bit d it recomputes t = (level - v_a) / (v_b - v_a) and writes the
//     C floats attr_a + t (attr_b - attr_a) of vertex voff[q] + popcount(mask & ((1 << (d - 1)) - 1)): emit's numbering.  Every
//     write is guarded by V.
#include <math.h>

#include "mesh_scan.h"      // the two scan levels, shared with mesh_clean.hip and mesh_simplify.hip

namespace voge {

constexpr int kMtBlock = kMcBlock;      // grid points of a scan block (= threads of the count launch); ops.MTET_BLOCK
constexpr int kMtTop = kMcTop;          // block totals one round of the top level takes (= its threads); ops.MTET_TOP
constexpr long kMtMaxKeys = 2147483647l;      // nx ny nz 7 <= 2^31 - 1

// the six tetrahedra of a cell as corner masks (c0, c1, c2, c3), positively oriented: one per permutation of the axes
__constant__ unsigned char kMtCorner[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
// the triangles of a case (bit j: local corner j inside): every vertex as the local edge 4 m + n, 255 where there is none
__constant__ unsigned char kMtEdge[16][6] = {
    {255, 255, 255, 255, 255, 255}, {1, 2, 3, 255, 255, 255}, {1, 7, 6, 255, 255, 255}, {2, 3, 7, 2, 7, 6},
    {2, 6, 11, 255, 255, 255},      {3, 1, 6, 3, 6, 11},      {1, 7, 11, 1, 11, 2},     {3, 7, 11, 255, 255, 255},
    {3, 11, 7, 255, 255, 255},      {1, 2, 11, 1, 11, 7},     {6, 1, 3, 6, 3, 11},      {2, 11, 6, 255, 255, 255},
    {2, 6, 7, 2, 7, 3},             {1, 6, 7, 255, 255, 255}, {1, 3, 2, 255, 255, 255}, {255, 255, 255, 255, 255, 255}};

struct MtGrid {
  int nx, ny, nz;
  float lox, loy, loz, hx, hy, hz;
};

// ---- fusion -------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
tsdf_integrate_kernel(float *__restrict__ tsdf, float *__restrict__ weight, const MtGrid g, const float *__restrict__ depth, const int B,
                      const int H, const int W, const float *__restrict__ R, const float *__restrict__ T,
                      const float *__restrict__ centre, const float *__restrict__ focal, const float *__restrict__ pp, const float trunc,
                      const float max_weight) {
  const uint32_t n = (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;      // (below 2^31 / 7: the host's mt_dims -- 32-bit index arithmetic)
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const uint32_t row = q / (uint32_t)g.nx;
  const int ix = (int)(q - row * (uint32_t)g.nx), iz = (int)(row / (uint32_t)g.ny), iy = (int)(row - (uint32_t)iz * (uint32_t)g.ny);
  const float x0 = g.lox + (float)ix * g.hx, x1 = g.loy + (float)iy * g.hy, x2 = g.loz + (float)iz * g.hz;
  float val = tsdf[q], w = weight[q];
  const float fW = (float)W, fH = (float)H;
  for (int b = 0; b < B; ++b) {
    const float *Rb = R + 9 * (size_t)b, *Tb = T + 3 * (size_t)b, *cb = centre + 3 * (size_t)b;
    const float pz = ((x0 * Rb[2] + x1 * Rb[5]) + x2 * Rb[8]) + Tb[2];
    if (!(pz > 0.0f)) continue;
    const float px = ((x0 * Rb[0] + x1 * Rb[3]) + x2 * Rb[6]) + Tb[0];
    const float py = ((x0 * Rb[1] + x1 * Rb[4]) + x2 * Rb[7]) + Tb[1];
    const float u = pp[2 * b] - (focal[2 * b] * px) / pz;
    const float v = pp[2 * b + 1] - (focal[2 * b + 1] * py) / pz;
    if (!(u >= 0.0f && u < fW && v >= 0.0f && v < fH)) continue;      // (a NaN fails: the definition's comparisons)
    const int j = (int)floorf(u), i = (int)floorf(v);                  // in [0, W) x [0, H) by the test above
    const float d = depth[((size_t)b * H + i) * W + j];
    if (!(d > 0.0f && d < INFINITY)) continue;
    const float dx = x0 - cb[0], dy = x1 - cb[1], dz = x2 - cb[2];
    const float sdf = d - sqrtf((dx * dx + dy * dy) + dz * dz);
    if (sdf < -trunc) continue;
    val = (val * w + fminf(1.0f, sdf / trunc)) / (w + 1.0f);
    w = max_weight > 0.0f ? fminf(w + 1.0f, max_weight) : w + 1.0f;
  }
  tsdf[q] = val;
  weight[q] = w;
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t mt_offset(const int c, const int nx, const int ny) {
  return (uint32_t)(c & 1) + (uint32_t)((c >> 1) & 1) * (uint32_t)nx + (uint32_t)(c >> 2) * (uint32_t)nx * (uint32_t)ny;
}

// observed / inside of the eight corners of the cell whose low corner is q = (ix, iy, iz), bit c for the corner of mask c; a corner
// beyond the grid is unobserved
__device__ __forceinline__ void mt_corners(const float *__restrict__ values, const float *__restrict__ weight, const int nx, const int ny,
                                           const int nz, const int ix, const int iy, const int iz, const uint32_t q, const float level,
                                           uint32_t &obs, uint32_t &ins) {
  obs = 0u;
  ins = 0u;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (ix + (c & 1) < nx && iy + ((c >> 1) & 1) < ny && iz + (c >> 2) < nz) {
      const uint32_t p = q + mt_offset(c, nx, ny);
      const float v = values[p];
      bool o = fabsf(v) < INFINITY;      // finite: false for a NaN as well
      if (weight) o = o && weight[p] > 0.0f;
      obs |= (uint32_t)o << c;
      ins |= (uint32_t)(v < level) << c;
    }
  }
}

// the case of tetrahedron `tet` (bit j: local corner j inside), -1 unless its four corners are observed
__device__ __forceinline__ int mt_case(const int tet, const uint32_t obs, const uint32_t ins) {
  const int c1 = kMtCorner[tet][1], c2 = kMtCorner[tet][2];
  const uint32_t need = 1u | (1u << c1) | (1u << c2) | 128u;
  if ((obs & need) != need) return -1;
  return (int)((ins & 1u) | (((ins >> c1) & 1u) << 1) | (((ins >> c2) & 1u) << 2) | (((ins >> 7) & 1u) << 3));
}

__device__ __forceinline__ int mt_case_faces(const int cs) {
  const int k = __popc((unsigned)cs);
  return k == 2 ? 2 : (k == 1 || k == 3 ? 1 : 0);
}

__global__ void __launch_bounds__(kMtBlock)
mtet_count_kernel(const float *__restrict__ values, const float *__restrict__ weight, const int nx, const int ny, const int nz,
                  const float level, uint8_t *__restrict__ edge_mask, uint8_t *__restrict__ face_count, uint16_t *__restrict__ vloc,
                  uint16_t *__restrict__ floc, uint32_t *__restrict__ block_v, uint32_t *__restrict__ block_f) {
  const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;      // (below 2^31 / 7: the host's mt_dims -- 32-bit index arithmetic)
  const int tid = threadIdx.x;
  const uint32_t q = blockIdx.x * (uint32_t)kMtBlock + (uint32_t)tid;
  uint32_t mask = 0u, fc = 0u;
  if (q < n) {
    const uint32_t row = q / (uint32_t)nx;
    const int ix = (int)(q - row * (uint32_t)nx), iz = (int)(row / (uint32_t)ny), iy = (int)(row - (uint32_t)iz * (uint32_t)ny);
    uint32_t obs, ins;
    mt_corners(values, weight, nx, ny, nz, ix, iy, iz, q, level, obs, ins);
    if (obs & 1u) {
#pragma unroll
      for (int d = 1; d < 8; ++d)
        if (((obs >> d) & 1u) && (((ins >> d) ^ ins) & 1u)) mask |= 1u << (d - 1);
    }
    if (obs & 128u) {
#pragma unroll
      for (int tet = 0; tet < 6; ++tet) {
        const int cs = mt_case(tet, obs, ins);
        if (cs >= 0) fc += (uint32_t)mt_case_faces(cs);
      }
    }
  }
  // both counts in one number (vertices below bit 16: at most 256 x 7; faces above: at most 256 x 12), scanned over the workgroup
  const uint32_t x = (uint32_t)__popc(mask) | (fc << 16);
  uint32_t upto;
  const uint32_t excl = mesh_scan_local(x, upto);
  if (q < n) {
    edge_mask[q] = (uint8_t)mask;
    face_count[q] = (uint8_t)fc;
    vloc[q] = (uint16_t)(excl & 0xffffu);
    floc[q] = (uint16_t)(excl >> 16);
  }
  if (tid == kMtBlock - 1) {      // (the last thread's inclusive prefix: the block's totals)
    block_v[blockIdx.x] = upto & 0xffffu;
    block_f[blockIdx.x] = upto >> 16;
  }
}

// ONE workgroup: the exclusive scan of block_v / block_f in place, kMtTop entries a round (mesh_scan.h's top level on the pair:
// vertices in the low 32 bits: below 2^31 in all; faces in the high 32: below 2^32 in all -- no carry between the halves)
__global__ void __launch_bounds__(kMtTop)
mtet_scan_kernel(uint32_t *__restrict__ block_v, uint32_t *__restrict__ block_f, const long nb, long long *__restrict__ totals) {
  const unsigned long long carry = mesh_scan_top<unsigned long long>(block_v, block_f, nb);
  if (threadIdx.x == 0) {
    totals[0] = (long long)(carry & 0xffffffffull);
    totals[1] = (long long)(carry >> 32);
  }
}

__global__ void __launch_bounds__(256)
mtet_emit_kernel(const float *__restrict__ values, const float *__restrict__ weight, const MtGrid g, const float level,
                 const uint8_t *__restrict__ edge_mask, const uint8_t *__restrict__ face_count, const uint16_t *__restrict__ vloc,
                 const uint16_t *__restrict__ floc, const uint32_t *__restrict__ block_v, const uint32_t *__restrict__ block_f,
                 const long V, const long F, float *__restrict__ verts, int32_t *__restrict__ faces) {
  const int nx = g.nx, ny = g.ny, nz = g.nz;
  const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;      // (below 2^31 / 7: the host's mt_dims -- 32-bit index arithmetic)
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const uint32_t mask = edge_mask[q], fc = face_count[q];
  if (!(mask | fc)) return;
  const uint32_t row = q / (uint32_t)nx;
  const int ix = (int)(q - row * (uint32_t)nx), iz = (int)(row / (uint32_t)ny), iy = (int)(row - (uint32_t)iz * (uint32_t)ny);
  if (mask) {
    const float va = values[q];
    const float pax = g.lox + (float)ix * g.hx, pay = g.loy + (float)iy * g.hy, paz = g.loz + (float)iz * g.hz;
    long id = (long)block_v[q / kMtBlock] + (long)vloc[q];
#pragma unroll
    for (int d = 1; d < 8; ++d) {
      if (!((mask >> (d - 1)) & 1u)) continue;      // (a set bit: the other end is inside the grid -- the count kernel's test)
      const float vb = values[q + mt_offset(d, nx, ny)];
      const float t = (level - va) / (vb - va);
      const float pbx = g.lox + (float)(ix + (d & 1)) * g.hx, pby = g.loy + (float)(iy + ((d >> 1) & 1)) * g.hy,
                  pbz = g.loz + (float)(iz + (d >> 2)) * g.hz;
      if (id < V) {
        float *o = verts + 3 * (size_t)id;
        o[0] = pax + t * (pbx - pax);
        o[1] = pay + t * (pby - pay);
        o[2] = paz + t * (pbz - paz);
      }
      ++id;
    }
  }
  if (fc) {
    uint32_t obs, ins;
    mt_corners(values, weight, nx, ny, nz, ix, iy, iz, q, level, obs, ins);
    long f = (long)block_f[q / kMtBlock] + (long)floc[q];
    for (int tet = 0; tet < 6; ++tet) {
      const int cs = mt_case(tet, obs, ins);
      if (cs < 0) continue;
      const int cnt = mt_case_faces(cs);
      for (int k = 0; k < cnt; ++k, ++f) {
        if (f >= F) continue;
        int32_t *o = faces + 3 * (size_t)f;
        for (int r = 0; r < 3; ++r) {
          const int e = kMtEdge[cs][3 * k + r];
          const int ca = kMtCorner[tet][(e >> 2) & 3], cb = kMtCorner[tet][e & 3];      // (one's bits contain the other's)
          const int low = ca < cb ? ca : cb, d = ca ^ cb;
          const uint32_t ql = q + mt_offset(low, nx, ny);      // (inside the grid: the tetrahedron's corners are observed)
          o[r] = (int32_t)(block_v[ql / kMtBlock] + (uint32_t)vloc[ql] + (uint32_t)__popc((uint32_t)edge_mask[ql] & ((1u << (d - 1)) - 1u)));
        }
      }
    }
  }
}

// ---- attributes ---------------------------------------------------------------------------------------------------------------

constexpr int kMtMaxChannels = 8;      // the channels of one launch; ops.MTET_MAX_CHANNELS

// tsdf_integrate_kernel with C attribute accumulators: the projection, the decisions and the update of tsdf and w are that kernel's,
// line by line; only the block under the last condition is new
template <int C>
__global__ void __launch_bounds__(256)
tsdf_integrate_attr_kernel(float *__restrict__ tsdf, float *__restrict__ weight, float *__restrict__ attr, const MtGrid g,
                           const float *__restrict__ depth, const float *__restrict__ image, const int B, const int H, const int W,
                           const float *__restrict__ R, const float *__restrict__ T, const float *__restrict__ centre,
                           const float *__restrict__ focal, const float *__restrict__ pp, const float trunc, const float max_weight) {
  const uint32_t n = (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;      // (below 2^31 / 7: the host's mt_dims -- 32-bit index arithmetic)
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const uint32_t row = q / (uint32_t)g.nx;
  const int ix = (int)(q - row * (uint32_t)g.nx), iz = (int)(row / (uint32_t)g.ny), iy = (int)(row - (uint32_t)iz * (uint32_t)g.ny);
  const float x0 = g.lox + (float)ix * g.hx, x1 = g.loy + (float)iy * g.hy, x2 = g.loz + (float)iz * g.hz;
  float val = tsdf[q], w = weight[q];
  float *const arow = attr + (size_t)q * C;
  float a[C];
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = arow[c];
  const float fW = (float)W, fH = (float)H;
  for (int b = 0; b < B; ++b) {
    const float *Rb = R + 9 * (size_t)b, *Tb = T + 3 * (size_t)b, *cb = centre + 3 * (size_t)b;
    const float pz = ((x0 * Rb[2] + x1 * Rb[5]) + x2 * Rb[8]) + Tb[2];
    if (!(pz > 0.0f)) continue;
    const float px = ((x0 * Rb[0] + x1 * Rb[3]) + x2 * Rb[6]) + Tb[0];
    const float py = ((x0 * Rb[1] + x1 * Rb[4]) + x2 * Rb[7]) + Tb[1];
    const float u = pp[2 * b] - (focal[2 * b] * px) / pz;
    const float v = pp[2 * b + 1] - (focal[2 * b + 1] * py) / pz;
    if (!(u >= 0.0f && u < fW && v >= 0.0f && v < fH)) continue;      // (a NaN fails: the definition's comparisons)
    const int j = (int)floorf(u), i = (int)floorf(v);                  // in [0, W) x [0, H) by the test above
    const size_t pixel = ((size_t)b * H + i) * W + j;
    const float d = depth[pixel];
    if (!(d > 0.0f && d < INFINITY)) continue;
    const float dx = x0 - cb[0], dy = x1 - cb[1], dz = x2 - cb[2];
    const float sdf = d - sqrtf((dx * dx + dy * dy) + dz * dz);
    if (sdf < -trunc) continue;
    const float *prow = image + pixel * C;      // (the view updates the point: only now is the pixel's attribute read)
    const float w1 = w + 1.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = (a[c] * w + prow[c]) / w1;
    val = (val * w + fminf(1.0f, sdf / trunc)) / (w + 1.0f);
    w = max_weight > 0.0f ? fminf(w + 1.0f, max_weight) : w + 1.0f;
  }
  tsdf[q] = val;
  weight[q] = w;
#pragma unroll
  for (int c = 0; c < C; ++c) arow[c] = a[c];
}

// the attribute of every vertex mtet_emit_kernel numbered, from the tables it numbered them by
template <int C>
__global__ void __launch_bounds__(256)
mtet_attr_kernel(const float *__restrict__ values, const int nx, const int ny, const int nz, const float level,
                 const float *__restrict__ attr, const uint8_t *__restrict__ edge_mask, const uint16_t *__restrict__ vloc,
                 const uint32_t *__restrict__ block_v, const long V, float *__restrict__ vert_attr) {
  const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;      // (below 2^31 / 7: the host's mt_dims -- 32-bit index arithmetic)
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const uint32_t mask = edge_mask[q];
  if (!mask) return;
  const float va = values[q];
  const float *const arow = attr + (size_t)q * C;
  float aa[C];
#pragma unroll
  for (int c = 0; c < C; ++c) aa[c] = arow[c];
  const long voff = (long)block_v[q / kMtBlock] + (long)vloc[q];
#pragma unroll
  for (int d = 1; d < 8; ++d) {
    if (!((mask >> (d - 1)) & 1u)) continue;      // (a set bit: the other end is inside the grid -- the count kernel's test)
    const long id = voff + (long)__popc(mask & ((1u << (d - 1)) - 1u));
    if (id >= V) continue;
    const uint32_t qb = q + mt_offset(d, nx, ny);
    const float vb = values[qb];
    const float t = (level - va) / (vb - va);
    const float *const brow = attr + (size_t)qb * C;
    float *const o = vert_attr + (size_t)id * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = aa[c] + t * (brow[c] - aa[c]);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

// 0, or the error of a grid's dimensions: every one >= 2, nx ny nz 7 < 2^31
static int mt_dims(const int nx, const int ny, const int nz) {
  if (nx < 2 || ny < 2 || nz < 2) return VOGE_ERR_BAD_ARG;
  if ((long)nx * (long)ny > kMtMaxKeys || (long)nx * (long)ny * (long)nz > kMtMaxKeys / 7) return VOGE_ERR_K_TOO_LARGE;
  return 0;
}
static bool mt_pos(const float v) { return v > 0.0f && v < INFINITY; }
static bool mt_fin(const float v) { return fabsf(v) < INFINITY; }

}  // namespace voge

using namespace voge;

extern "C" int voge_tsdf_integrate(float *tsdf, float *weight, int nx, int ny, int nz, float lox, float loy, float loz, float hx,
                                   float hy, float hz, const float *depth, int B, int H, int W, const float *R, const float *T,
                                   const float *centre, const float *focal, const float *pp, float trunc, float max_weight,
                                   voge_stream_t stream) {
  const int de = mt_dims(nx, ny, nz);
  if (de) return de;
  if (B < 0 || H < 1 || W < 1 || !mt_pos(trunc) || !mt_pos(hx) || !mt_pos(hy) || !mt_pos(hz) || !mt_fin(lox) || !mt_fin(loy) ||
      !mt_fin(loz) || max_weight != max_weight)
    return VOGE_ERR_BAD_ARG;
  if (!tsdf || !weight) return VOGE_ERR_BAD_ARG;
  if (B == 0) return 0;
  if (!depth || !R || !T || !centre || !focal || !pp) return VOGE_ERR_BAD_ARG;
  const MtGrid g = {nx, ny, nz, lox, loy, loz, hx, hy, hz};
  const size_t n = (size_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, g, depth, B,
                     H, W, R, T, centre, focal, pp, trunc, max_weight);
  return launch_status();
}

extern "C" int voge_mtet_count(const float *values, const float *weight, int nx, int ny, int nz, float level, uint8_t *edge_mask,
                               uint8_t *face_count, uint16_t *vloc, uint16_t *floc, uint32_t *block_v, uint32_t *block_f,
                               voge_stream_t stream) {
  const int de = mt_dims(nx, ny, nz);
  if (de) return de;
  if (!values || !edge_mask || !face_count || !vloc || !floc || !block_v || !block_f || level != level) return VOGE_ERR_BAD_ARG;
  const size_t n = (size_t)nx * ny * nz;
  hipLaunchKernelGGL(mtet_count_kernel, dim3((unsigned)((n + kMtBlock - 1) / kMtBlock)), dim3(kMtBlock), 0, (hipStream_t)stream, values, weight,
                     nx, ny, nz, level, edge_mask, face_count, vloc, floc, block_v, block_f);
  return launch_status();
}

extern "C" int voge_mtet_scan(uint32_t *block_v, uint32_t *block_f, long nblocks, long long *totals, voge_stream_t stream) {
  if (nblocks < 1 || !block_v || !block_f || !totals) return VOGE_ERR_BAD_ARG;
  if (nblocks > kMtMaxKeys / 7 / kMtBlock + 1) return VOGE_ERR_K_TOO_LARGE;
  hipLaunchKernelGGL(mtet_scan_kernel, dim3(1), dim3(kMtTop), 0, (hipStream_t)stream, block_v, block_f, nblocks, totals);
  return launch_status();
}

extern "C" int voge_mtet_emit(const float *values, const float *weight, int nx, int ny, int nz, float level, float lox, float loy,
                              float loz, float hx, float hy, float hz, const uint8_t *edge_mask, const uint8_t *face_count,
                              const uint16_t *vloc, const uint16_t *floc, const uint32_t *block_v, const uint32_t *block_f, long V, long F,
                              float *verts, int32_t *faces, voge_stream_t stream) {
  const int de = mt_dims(nx, ny, nz);
  if (de) return de;
  if (V < 0 || F < 0) return VOGE_ERR_BAD_ARG;
  if (V > kMtMaxKeys || F > kMtMaxKeys) return VOGE_ERR_K_TOO_LARGE;
  if (!values || !edge_mask || !face_count || !vloc || !floc || !block_v || !block_f || level != level || !mt_pos(hx) || !mt_pos(hy) ||
      !mt_pos(hz) || !mt_fin(lox) || !mt_fin(loy) || !mt_fin(loz) || (V > 0 && !verts) || (F > 0 && !faces))
    return VOGE_ERR_BAD_ARG;
  if (V == 0 && F == 0) return 0;
  const MtGrid g = {nx, ny, nz, lox, loy, loz, hx, hy, hz};
  const size_t n = (size_t)nx * ny * nz;
  hipLaunchKernelGGL(mtet_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values, weight, g, level, edge_mask,
                     face_count, vloc, floc, block_v, block_f, V, F, verts, faces);
  return launch_status();
}

// one case of the switch over the channels: kernel<C>
#define VOGE_MT_CHANNELS(c, launch) \
  switch (c) {                      \
    case 1: launch(1); break;       \
    case 2: launch(2); break;       \
    case 3: launch(3); break;       \
    case 4: launch(4); break;       \
    case 5: launch(5); break;       \
    case 6: launch(6); break;       \
    case 7: launch(7); break;       \
    default: launch(8); break;      \
  }

extern "C" int voge_tsdf_integrate_attr(float *tsdf, float *weight, float *attr, int C, int nx, int ny, int nz, float lox, float loy,
                                        float loz, float hx, float hy, float hz, const float *depth, const float *attr_image, int B, int H,
                                        int W, const float *R, const float *T, const float *centre, const float *focal, const float *pp,
                                        float trunc, float max_weight, voge_stream_t stream) {
  const int de = mt_dims(nx, ny, nz);
  if (de) return de;
  if (C < 1 || C > kMtMaxChannels || B < 0 || H < 1 || W < 1 || !mt_pos(trunc) || !mt_pos(hx) || !mt_pos(hy) || !mt_pos(hz) ||
      !mt_fin(lox) || !mt_fin(loy) || !mt_fin(loz) || max_weight != max_weight)
    return VOGE_ERR_BAD_ARG;
  if (!tsdf || !weight || !attr) return VOGE_ERR_BAD_ARG;
  if (B == 0) return 0;
  if (!depth || !attr_image || !R || !T || !centre || !focal || !pp) return VOGE_ERR_BAD_ARG;
  const MtGrid g = {nx, ny, nz, lox, loy, loz, hx, hy, hz};
  const size_t n = (size_t)nx * ny * nz;
#define VOGE_MT_LAUNCH(c)                                                                                                                  \
  hipLaunchKernelGGL(tsdf_integrate_attr_kernel<c>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, attr, \
                     g, depth, attr_image, B, H, W, R, T, centre, focal, pp, trunc, max_weight)
  VOGE_MT_CHANNELS(C, VOGE_MT_LAUNCH)
#undef VOGE_MT_LAUNCH
  return launch_status();
}

extern "C" int voge_mtet_attr(const float *values, int nx, int ny, int nz, float level, const float *attr, int C, const uint8_t *edge_mask,
                              const uint16_t *vloc, const uint32_t *block_v, long V, float *vert_attr, voge_stream_t stream) {
  const int de = mt_dims(nx, ny, nz);
  if (de) return de;
  if (C < 1 || C > kMtMaxChannels || V < 0) return VOGE_ERR_BAD_ARG;
  if (V > kMtMaxKeys) return VOGE_ERR_K_TOO_LARGE;
  if (!values || !attr || !edge_mask || !vloc || !block_v || level != level || (V > 0 && !vert_attr)) return VOGE_ERR_BAD_ARG;
  if (V == 0) return 0;
  const size_t n = (size_t)nx * ny * nz;
#define VOGE_MT_LAUNCH(c)                                                                                                                  \
  hipLaunchKernelGGL(mtet_attr_kernel<c>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values, nx, ny, nz, level, \
                     attr, edge_mask, vloc, block_v, V, vert_attr)
  VOGE_MT_CHANNELS(C, VOGE_MT_LAUNCH)
#undef VOGE_MT_LAUNCH
  return launch_status();
}
