// The grid route of the point-to-mesh searches (included by point_mesh.hip, whose pair function, records and keys it uses): the
// same winners as the brute-force kernels -- the smallest key (d2 bits << 32 | index) over the candidates, d2 from pm_pair on the
// record of pm_record --, found without meeting every pair, so the pair cap of the brute route does not bind it.  What a search
// has to prove is that it never skips an item that could hold the smallest key.
//
// (a) The grid, chosen on the device.  grid_box_kernel (knn_grid.h): the bounding box of the UNION of verts and points;
//     pm_grid_extent_kernel: the sum over the faces of 2 h_f (below: the largest extent of a face's bounding box), fp64 partial
//     sums in an order fixed by the shapes; pm_grid_choose_kernel, one workgroup: the rule of ops.knn_grid with n = max(F, P) --
//     about 2 n cubic cells, cell >= max extent / 1023, G_a <= 1024, G <= max(8 n, 2^15), at most 64 enlargements, the one-cell grid
//     for a box that is not finite or a loop that did not end -- with one more floor: cell >= kPmGridFloor x the mean of 2 h_f, so
//     that a typical triangle does not span many cells.  cell_size > 0 asks for a cell of that size (no floor, the same
//     enlargement).  The grid, H = kPmGridBig cell and the large list's counter live in the workspace's first 64 bytes; the
//     workspace and every launch are sized by (V, F, P) alone and nothing is read back: the call can be captured.
// (b) ONE cell per triangle.  A triangle is binned by the cell of the centre c_f of its bounding box and carries its half-extent
//     h_f = max_a max(hi_a - c_a, c_a - lo_a), rounded UP (x (1 + 2^-22) after the fp32 subtraction): every point of the triangle
//     is within h_f of c_f on every axis.  Triangles with h_f <= H are SMALL: count -> scan (knn_grid.h) -> fill, which writes
//     each one's record and index in cell order into [0, nsmall).  The others -- and every record that is not finite: a NaN or
//     infinite vertex, a vertex index out of range -- are LARGE: an integer atomic counter hands out the slots F - 1, F - 2, ...
//     of the same table (order inside the list is free, the key decides).  A table of exactly F entries: no total to read back.
//     The points are binned in the same grid, as chamfer.hip bins its queries.
// (c) pm_grid_point_kernel, a point per lane in the points' cell order: first the whole large list, tiled through LDS, then rings
//     r = 0, 1, 2, ... of cells around the point's cell over the cell-ordered records.  After ring r an unvisited small triangle
//     has its centre in a cell whose index differs by >= r + 1 on some axis, so by knn.hip's argument (both the point and the
//     centre lie in the union's box, t < 1024) |c_a - p_a| > cell (r - 2^-11) on that axis, and every point of the triangle is
//     farther than B = cell (r - 2^-11) - H from p.  The walk stops after ring r once the kept d2 <= b b, with
//         X = fl(fl(cell (r - 2^-10)) - H),      b = X (1 - 2^-8) - 2^-7 H,      b > 2^-50.
//     Derivation.  r - 2^-10 is exact (r <= 1023); the product and the difference round by at most 2^-24 (cell r + X) <=
//     2^-13 cell, so X < B.  For an unvisited triangle at true distance d > B > X the fp32 d2 of pm_pair is, by the module's value
//     bound (tests/point_mesh_cases.py), >= d^2 - e (d + L)^2 with e = 32 2^-23 = 2^-18 and L its longest edge, at most the
//     diagonal of its bounding box: L <= 2 sqrt(3) h_f < 3.47 H.  d^2 - e (d + L)^2 >= (d - 2^-9 (d + L))^2 while d >= 2^-9 (d + L),
//     so sqrt(fp32 d2) >= d (1 - 2^-9) - 2^-9 3.47 H > X (1 - 2^-9) - 3.47 2^-9 H.  That exceeds b (1 + 2^-23) -- the roundings of
//     b and b b -- because X (2^-8 - 2^-9) > 2^-22 X and 2^-7 H = 4 2^-9 H > 3.47 2^-9 H (1 + 2^-22): every unvisited triangle has an
//     fp32 d2 STRICTLY above b b >= the kept d2, so no tie can be missed either.  b > 2^-50 keeps b b a normal number (a relative
//     bound says nothing once d2 underflows).  With kPmGridBig = 1 the rule first fires at r = 2, b = 0.987 cell.  The walk also
//     ends when the cube covers the grid, which bounds every loop.  The winner's pair is evaluated once more for the weights.
// (d) pm_grid_face_kernel, a triangle per lane (its record in registers) in the table's order -- the small ones by cell, the large
//     ones behind them --, rings around its centre's cell over the cell-ordered points.  The same rule with the lane's OWN h_f in
//     H's place: an unvisited point is farther than cell (r - 2^-11) - h_f from the triangle, L <= 2 sqrt(3) h_f.  A large
//     triangle needs no list here, it walks more rings -- at worst the whole grid (a record that is not finite has h_f = inf and
//     never fires the rule).  The known weak cases, all correct and bounded: ONE huge triangle idles the other lanes of its wave
//     for its walk; a mesh of mostly large triangles is a brute force with extra steps in (c); lopsided pairs (a few faces against
//     many points or the reverse) choose the grid for the larger side.  A hierarchy for wildly mixed sizes is out of scope.
//
//     Also weak: points FAR from the mesh (many cells away) walk rings of empty cells, two dependent loads a cell, and lose to the
//     brute force below the pair cap; a distance transform or a summed-volume table over the cell counts would skip them (not taken).
//
// Measured on the MI355X (tools/point_mesh_grid_time.py, profiles/r28_point_mesh_grid.txt): the 256^3 sphere's level set
// (1 011 432 faces) against 438 544 points within 0.02 of it 7.6 ms (809 pairs a point, 2.4 rings), both directions 7.9 ms;
// against demo/RenderPointClouds.py's cloud as it lies (18 rings a point) 1.12 s and 1.31 s.  kPmGridBig = 1, the floor at 1 x the
// mean extent and 128 queries a workgroup are the settings measured; cells 1.5 - 6 x larger lose 1.5 - 13 x near the surface and
// gain at most 3 x far from it.  See kPmGridMinPairs below.
#pragma once
#include "knn_grid.h"

namespace voge {

constexpr float kPmGridBig = 1.0f;          // a triangle is small while h_f <= kPmGridBig cell
constexpr double kPmGridFloor = 1.0;        // cell >= kPmGridFloor x the mean largest bounding-box extent of a face
constexpr int kPmGridBlock = 128;           // queries a workgroup of the two searches
constexpr int kPmGridLargeTile = 256;       // records of a tile of the large list: 16 KB of LDS
constexpr int kPmGridItems = 8;             // faces a thread of the extent pass: 2048 a workgroup
// Route None takes the grid from this many pairs P F on (ops.POINT_MESH_GRID_MIN_PAIRS chooses; profiles/r28_point_mesh_grid.txt).
// Measured: with the points near the surface the grid route wins from 10^7 pairs on (2 000 x 5 120: 247 against 258 us,
// 200 000 x 81 920: 0.43 against 48.3 ms; 2^24 by the rule), with the points spread through the box it loses at EVERY size below the pair cap (its
// walks run 5 - 19 rings of mostly empty cells, a microsecond a cell) and first draws level at the cap itself (524 288 x 524 287:
// 0.74 against 0.74 s one way, 0.75 against 1.46 s both).  The shapes cannot tell the two apart, so None stays on the brute force
// up to the cap: the crossover is the cap.
constexpr double kPmGridMinPairs = 274877906944.0;      // 2^38 = kPmMaxPairs

struct PmGridHead {      // the workspace's first 64 bytes
  KnnGrid g;
  int G;
  int nlarge;            // the length of the large list (an integer atomic counter, zeroed with the grid)
  float H;               // kPmGridBig cell
  int pad[5];
};
static_assert(sizeof(PmGridHead) == 64, "PmGridHead is 64 bytes");

// the centre of a face's bounding box and its half-extent, rounded up; fin false (h = inf, centre 0): a vertex index out of
// range or a coordinate that is not finite
struct PmTriBox {
  float cx, cy, cz, h;
  bool fin;
};

__device__ __forceinline__ void pm_grid_axis(const float a, const float b, const float c, float &mid, float &h) {
  const float lo = fminf(fminf(a, b), c), hi = fmaxf(fmaxf(a, b), c);
  mid = fminf(fmaxf(0.5f * lo + 0.5f * hi, lo), hi);
  h = fmaxf(h, fmaxf(hi - mid, mid - lo));
}

__device__ __forceinline__ PmTriBox pm_grid_tribox(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces,
                                                   const size_t f) {
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  PmTriBox t{0.0f, 0.0f, 0.0f, INFINITY, false};
  if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return t;
  const float *a = verts + 3 * (size_t)ia, *b = verts + 3 * (size_t)ib, *c = verts + 3 * (size_t)ic;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && fabsf(a[k]) < INFINITY && fabsf(b[k]) < INFINITY && fabsf(c[k]) < INFINITY;
  if (!fin) return t;
  float h = 0.0f;
  pm_grid_axis(a[0], b[0], c[0], t.cx, h);
  pm_grid_axis(a[1], b[1], c[1], t.cy, h);
  pm_grid_axis(a[2], b[2], c[2], t.cz, h);
  h *= 0x1.000004p0f;      // 1 + 2^-22: above the exact half-extent whatever the subtraction rounded
  if (!(h < INFINITY)) {
    t.cx = t.cy = t.cz = 0.0f;
    return t;
  }
  t.h = h;
  t.fin = true;
  return t;
}

// ---- the grid, chosen on the device -------------------------------------------------------------------------------------------

// one fp64 sum of 2 h_f per 2048 faces (a face that is not finite adds nothing), added in an order fixed by the shapes
__global__ void __launch_bounds__(256)
pm_grid_extent_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                      double *__restrict__ partial) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kPmGridItems; ++k) {
    const size_t f = ((size_t)blockIdx.x * kPmGridItems + k) * 256 + threadIdx.x;
    if (f < (size_t)F) {
      const PmTriBox t = pm_grid_tribox(verts, V, faces, f);
      s += t.fin ? 2.0 * (double)t.h : 0.0;
    }
  }
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// ONE workgroup: the box of the partial boxes, the mean extent, then thread 0 chooses the grid (grid_choose with the floor on the
// default cell), H, and zeroes the large list's counter
__global__ void __launch_bounds__(256)
pm_grid_choose_kernel(const float *__restrict__ boxp, const int nb_box, const double *__restrict__ extp, const int nb_ext, const long F,
                      const long n, const float cell_size, PmGridHead *__restrict__ head) {
  float lo[3], hi[3];
  grid_box_reduce(boxp, nb_box, lo, hi);
  double es = 0.0;
  for (int i = threadIdx.x; i < nb_ext; i += 256) es += extp[i];
  __shared__ double rede[256];
  rede[threadIdx.x] = es;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) rede[threadIdx.x] += rede[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double mean = rede[0] / (double)F;
  PmGridHead h;
  grid_choose(lo, hi, n, cell_size, mean > 0.0 && mean < (double)INFINITY ? kPmGridFloor * mean : 0.0, h.g, h.G);
  h.nlarge = 0;
  h.H = kPmGridBig * h.g.cell;
  for (int k = 0; k < 5; ++k) h.pad[k] = 0;
  *head = h;
}

// ---- the faces and the points binned in the one grid --------------------------------------------------------------------------

struct PmGridTables {
  const float *verts;
  int V;
  const int32_t *faces;
  int F;
  const float *points;
  int P;
  PmRec *rec;             // [F] records: the small triangles in cell order, then the large list
  int32_t *fidx;          // [F] their face indices
  int *fcell, *fcounts, *fstart;
  float4 *psorted;        // [P] the points in cell order, w = the index
  int *pcell, *pcounts, *pstart;
};

// workgroups [0, nbf): a face a thread -- its cell's count, or a slot of the large list (fcell = -1 - slot); the rest: a point a thread
__global__ void __launch_bounds__(256)
pm_grid_count_kernel(const PmGridTables t, const unsigned nbf, PmGridHead *__restrict__ head) {
  const bool first = blockIdx.x < nbf;
  const size_t i = (size_t)(blockIdx.x - (first ? 0u : nbf)) * 256 + threadIdx.x;
  if (i >= (size_t)(first ? t.F : t.P)) return;
  const KnnGrid g = head->g;
  if (first) {
    const PmTriBox b = pm_grid_tribox(t.verts, t.V, t.faces, i);
    if (b.fin && b.h <= head->H) {
      const int c = grid_cell_of(g, b.cx, b.cy, b.cz);
      t.fcell[i] = c;
      atomicAdd(t.fcounts + c, 1);
    } else {
      t.fcell[i] = -1 - atomicAdd(&head->nlarge, 1);
    }
    return;
  }
  grid_count_point(g, t.points, i, t.pcell, t.pcounts);
}

// a point takes its row as chamfer.hip's do; a small triangle claims its row the same way, a large one takes slot F - 1 - k of the table
__global__ void __launch_bounds__(256)
pm_grid_fill_kernel(const PmGridTables t, const unsigned nbf, const PmGridHead *__restrict__ head) {
  const bool first = blockIdx.x < nbf;
  const size_t i = (size_t)(blockIdx.x - (first ? 0u : nbf)) * 256 + threadIdx.x;
  const int N = first ? t.F : t.P;
  if (i >= (size_t)N) return;
  const int c = (first ? t.fcell : t.pcell)[i];
  const bool large = first && c < 0;
  if (!large && (c < 0 || c >= head->G)) return;      // (the count pass wrote a cell of this grid: a guard, not a route)
  if (!first) {
    grid_fill_point(t.points, i, c, t.pcounts, t.pstart, N, t.psorted);
    return;
  }
  const int pos = large ? N + c : grid_claim_row(t.fcounts, t.fstart, c, N);      // N - 1 - k, k = -1 - c
  if (pos < 0 || pos >= N) return;      // (cannot happen after the count pass over the same table: a guard, not a route)
  t.rec[pos] = pm_record(t.verts, t.V, t.faces, i);
  t.fidx[pos] = (int32_t)i;
}

// ---- the two searches ---------------------------------------------------------------------------------------------------------

// Rings r = 0, 1, ... of cells around (cx, cy, cz); eval(j0, j1) meets the entries [j0, j1) of the cell-ordered table (start, at
// most Nd entries) and lowers best.  hq: H, or the lane's own h_f.  The stopping rule of the header.
template <class Eval>
__device__ __forceinline__ void pm_grid_walk(const KnnGrid &g, const int cx, const int cy, const int cz, const int *__restrict__ start,
                                             const int Nd, const float hq, uint64_t &best, Eval eval) {
  // the ring at which the cube covers the grid
  const int rmax = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
  for (int r = 0; r <= rmax; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.gx - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, g.gy - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.gz - 1);
    for (int zz = z0; zz <= z1; ++zz) {
      for (int yy = y0; yy <= y1; ++yy) {
        const int row = (zz * g.gy + yy) * g.gx;
        // a row of the shell's faces in y or z: cells x0 .. x1 are one range of the table; an inner row: the two cells at cx -+ r
        const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
#pragma unroll
        for (int part = 0; part < 2; ++part) {
          int ca, cb;
          if (face) {
            if (part == 1) break;
            ca = x0; cb = x1;
          } else {
            ca = cb = part == 0 ? cx - r : cx + r;
            if (ca < 0 || ca >= g.gx) continue;
          }
          eval(max(start[row + ca], 0), min(start[row + cb + 1], Nd));
        }
      }
    }
    if (best != ~0ull) {
      const float X = g.cell * ((float)r - 0x1p-10f) - hq;
      const float b = X * (1.0f - 0x1p-8f) - 0x1p-7f * hq;
      if (b > 0x1p-50f && __uint_as_float((uint32_t)(best >> 32)) <= b * b) break;
    }
  }
}

__global__ void __launch_bounds__(kPmGridBlock)
pm_grid_point_kernel(const PmGridTables t, const PmGridHead *__restrict__ head, int32_t *__restrict__ face_idx, float *__restrict__ d2,
                     float *__restrict__ bary) {
  __shared__ PmRec tile[kPmGridLargeTile];
  __shared__ int32_t tidx[kPmGridLargeTile];
  const size_t at = (size_t)blockIdx.x * kPmGridBlock + threadIdx.x;
  bool active = at < (size_t)t.P;
  const float4 q = t.psorted[active ? at : (size_t)t.P - 1];      // (a lane past the end repeats the last point and writes nothing)
  const int qi = __float_as_int(q.w);
  active = active && qi >= 0 && qi < t.P;      // (every slot was filled with an index below P: a guard on the output row)
  const int nlarge = min(max(head->nlarge, 0), t.F), nsmall = t.F - nlarge;
  uint64_t best = ~0ull;
  for (int t0 = 0; t0 < nlarge; t0 += kPmGridLargeTile) {
    const int n = min(kPmGridLargeTile, nlarge - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kPmGridBlock) {
      tile[k] = t.rec[(size_t)nsmall + t0 + k];
      tidx[k] = t.fidx[(size_t)nsmall + t0 + k];
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < n; ++k) {
      const PmRec rec = tile[k];
      const uint64_t key = pm_key(pm_pair<false>(rec, q.x, q.y, q.z, nullptr, nullptr), (uint32_t)tidx[k]);
      best = key < best ? key : best;
    }
  }
  if (!active) return;      // (no barrier below)
  const KnnGrid g = head->g;
  if (nsmall > 0) {
    const PmRec *__restrict__ rec = t.rec;
    const int32_t *__restrict__ fidx = t.fidx;
    pm_grid_walk(g, knn_axis_cell(q.x, g.lox, g.inv, g.gx), knn_axis_cell(q.y, g.loy, g.inv, g.gy),
                 knn_axis_cell(q.z, g.loz, g.inv, g.gz), t.fstart, nsmall, head->H, best, [&](const int j0, const int j1) {
                   for (int j = j0; j < j1; ++j) {
                     const PmRec r = rec[j];
                     const uint64_t key = pm_key(pm_pair<false>(r, q.x, q.y, q.z, nullptr, nullptr), (uint32_t)fidx[j]);
                     best = key < best ? key : best;
                   }
                 });
  }
  const uint32_t fi = (uint32_t)(best & 0xffffffffull);
  const bool ok = best != ~0ull && fi < (uint32_t)t.F;
  float w[3] = {0.0f, 0.0f, 0.0f}, r[3];
  if (ok) pm_pair<true>(pm_record(t.verts, t.V, t.faces, fi), q.x, q.y, q.z, w, r);
  face_idx[qi] = ok ? (int32_t)fi : -1;
  d2[qi] = ok ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
  bary[3 * (size_t)qi] = w[0]; bary[3 * (size_t)qi + 1] = w[1]; bary[3 * (size_t)qi + 2] = w[2];
}

__global__ void __launch_bounds__(kPmGridBlock)
pm_grid_face_kernel(const PmGridTables t, const PmGridHead *__restrict__ head, int32_t *__restrict__ point_idx, float *__restrict__ d2,
                    float *__restrict__ bary) {
  const size_t at = (size_t)blockIdx.x * kPmGridBlock + threadIdx.x;
  if (at >= (size_t)t.F) return;      // (no barrier below)
  const int fi = t.fidx[at];
  if (fi < 0 || fi >= t.F) return;      // (every slot of the table was filled with an index below F: a guard on the output row)
  const PmRec rec = pm_record(t.verts, t.V, t.faces, (size_t)fi);
  const PmTriBox b = pm_grid_tribox(t.verts, t.V, t.faces, (size_t)fi);
  const KnnGrid g = head->g;
  const float4 *__restrict__ sorted = t.psorted;
  uint64_t best = ~0ull;
  pm_grid_walk(g, knn_axis_cell(b.cx, g.lox, g.inv, g.gx), knn_axis_cell(b.cy, g.loy, g.inv, g.gy),
               knn_axis_cell(b.cz, g.loz, g.inv, g.gz), t.pstart, t.P, b.h, best, [&](const int j0, const int j1) {
                 for (int j = j0; j < j1; ++j) {
                   const float4 p = sorted[j];
                   const uint64_t key = pm_key(pm_pair<false>(rec, p.x, p.y, p.z, nullptr, nullptr), (uint32_t)__float_as_int(p.w));
                   best = key < best ? key : best;
                 }
               });
  const uint32_t pi = (uint32_t)(best & 0xffffffffull);
  const bool ok = best != ~0ull && pi < (uint32_t)t.P;
  float w[3] = {0.0f, 0.0f, 0.0f}, r[3];
  if (ok) pm_pair<true>(rec, t.points[3 * (size_t)pi], t.points[3 * (size_t)pi + 1], t.points[3 * (size_t)pi + 2], w, r);
  point_idx[fi] = ok ? (int32_t)pi : -1;
  d2[fi] = ok ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
  bary[3 * (size_t)fi] = w[0]; bary[3 * (size_t)fi + 1] = w[1]; bary[3 * (size_t)fi + 2] = w[2];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct PmGridLayout {
  size_t head, boxp, extp, rec, fidx, fcell, fcounts, fstart, fbsum, psorted, pcell, pcounts, pstart, pbsum, d2p, d2f, psum, pmax, total;
  long cap;
  int nb_scan, nb_box, nb_ext;
};
static PmGridLayout pm_grid_layout(const long V, const long F, const long P) {
  PmGridLayout l;
  const long n = F > P ? F : P;
  l.cap = grid_cell_cap(n);
  l.nb_scan = (int)((l.cap + kKnnScanBlock * kKnnScanItems - 1) / (kKnnScanBlock * kKnnScanItems));
  l.nb_box = (int)((V + P + 256 * kGridBoxItems - 1) / (256 * kGridBoxItems));
  l.nb_ext = (int)((F + 256 * kPmGridItems - 1) / (256 * kPmGridItems));
  const size_t nb_loss = chamfer_loss_blocks(P) + chamfer_loss_blocks(F);
  Carve c;
  l.head = c.take_exact(sizeof(PmGridHead));
  l.boxp = c.take((size_t)l.nb_box * 6 * sizeof(float));
  l.extp = c.take((size_t)l.nb_ext * sizeof(double));
  l.rec = c.take_exact((size_t)F * sizeof(PmRec));
  l.fidx = c.take((size_t)F * 4);
  l.fcell = c.take((size_t)F * 4);
  l.fcounts = c.take((size_t)l.cap * 4);
  l.fstart = c.take((size_t)(l.cap + 1) * 4);
  l.fbsum = c.take((size_t)l.nb_scan * 4);
  l.psorted = c.take_exact((size_t)P * 16);
  l.pcell = c.take((size_t)P * 4);
  l.pcounts = c.take((size_t)l.cap * 4);
  l.pstart = c.take((size_t)(l.cap + 1) * 4);
  l.pbsum = c.take((size_t)l.nb_scan * 4);
  l.d2p = c.take((size_t)P * 4);
  l.d2f = c.take((size_t)F * 4);
  l.psum = c.take(nb_loss * sizeof(double));
  l.pmax = c.take(nb_loss * sizeof(float));
  const size_t bwd = (size_t)(V + P) * 3 * sizeof(long long);      // the backward's accumulators, a call of its own
  l.total = c.at > bwd ? c.at : bwd;
  return l;
}

// the nearest face of every point (face_idx, d2p, bary_p) and -- both -- the nearest point of every face; the pointers were
// validated by the caller
static void pm_grid_searches(const float *points, const long P, const float *verts, const long V, const int32_t *faces, const long F,
                             const float cell_size, const bool both, int32_t *face_idx, float *d2p, float *bary_p, int32_t *point_idx,
                             float *d2f, float *bary_f, char *ws, const PmGridLayout &l, hipStream_t st) {
  PmGridHead *head = reinterpret_cast<PmGridHead *>(ws + l.head);
  float *boxp = reinterpret_cast<float *>(ws + l.boxp);
  double *extp = reinterpret_cast<double *>(ws + l.extp);
  const auto ints = [ws](const size_t off) { return reinterpret_cast<int *>(ws + off); };
  const PmGridTables t{verts, (int)V, faces, (int)F, points, (int)P, reinterpret_cast<PmRec *>(ws + l.rec), ints(l.fidx), ints(l.fcell),
                       ints(l.fcounts), ints(l.fstart), reinterpret_cast<float4 *>(ws + l.psorted), ints(l.pcell), ints(l.pcounts),
                       ints(l.pstart)};
  const unsigned nbf = blocks256(F), nbp = blocks256(P);
  hipLaunchKernelGGL(grid_box_kernel, dim3((unsigned)l.nb_box), dim3(256), 0, st, verts, (int)V, points, (int)P, boxp);
  hipLaunchKernelGGL(pm_grid_extent_kernel, dim3((unsigned)l.nb_ext), dim3(256), 0, st, verts, (int)V, faces, (int)F, extp);
  hipLaunchKernelGGL(pm_grid_choose_kernel, dim3(1), dim3(256), 0, st, boxp, l.nb_box, extp, l.nb_ext, F, F > P ? F : P, cell_size, head);
  hipLaunchKernelGGL(grid_zero_kernel, dim3(blocks256(l.cap)), dim3(256), 0, st, &head->G, t.fcounts, t.pcounts);
  hipLaunchKernelGGL(pm_grid_count_kernel, dim3(nbf + nbp), dim3(256), 0, st, t, nbf, head);
  int *counts[2] = {t.fcounts, t.pcounts}, *start[2] = {t.fstart, t.pstart}, *bsum[2] = {ints(l.fbsum), ints(l.pbsum)};
  const int N[2] = {(int)F, (int)P};
  for (int k = 0; k < 2; ++k) grid_scan_launch(counts[k], 0, &head->G, bsum[k], l.nb_scan, N[k], start[k], st);
  hipLaunchKernelGGL(pm_grid_fill_kernel, dim3(nbf + nbp), dim3(256), 0, st, t, nbf, head);
  hipLaunchKernelGGL(pm_grid_point_kernel, dim3((unsigned)((P + kPmGridBlock - 1) / kPmGridBlock)), dim3(kPmGridBlock), 0, st, t, head,
                     face_idx, d2p, bary_p);
  if (both)
    hipLaunchKernelGGL(pm_grid_face_kernel, dim3((unsigned)((F + kPmGridBlock - 1) / kPmGridBlock)), dim3(kPmGridBlock), 0, st, t, head,
                       point_idx, d2f, bary_f);
}

}  // namespace voge
