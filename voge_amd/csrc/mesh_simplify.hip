// Mesh simplification (EXTENSION: the reference has none; the decimation step every mesh toolkit has between extracting a mesh and
// using it): vertex clustering on a uniform grid (Rossignac-Borrel) with mean or quadric placement (Lindstrom).  One mesh per call:
// verts [V,3] fp32, faces [F,3] int32, a cell size (hx, hy, hz).  Aggregation.mesh_simplify is the definition and states the rule in
// five steps; the launches below follow it step for step.  Nothing here is differentiable.  No float atomics anywhere, no thread
// ever waits for another, every loop has a trip cap a correct run cannot reach, and a thread that meets one sets a bit of the
// error word, which the caller reads back with the two output sizes: ONE synchronisation per call.
//
// voge_mesh_simplify_scan, steps 1 to 4 up to the sizes (fills aside, eight launches):
//   simp_bbox_kernel         lo = the per-axis minimum, an integer atomic min on the ORDERED bits of the floats (sign bit flipped for
//                          x >= 0, all bits for x < 0: the unsigned order is the floats'; a minimum has no order of arrival).  It
//                          stays in device memory; every later kernel reads it there.  A vertex that is not finite sets bit 2.
//   simp_cell_insert_kernel  cell(v) = floor((v - lo) / h), three IEEE fp32 operations (-ffp-contract=off, correctly rounded
//                          division): the bits of the definition's, also for the thousands of vertices extract_mesh puts exactly on
//                          cell boundaries.  A cell index above 2^21 - 2 sets bit 3.  Then THE TABLE (below) with key = the cell.
//   simp_cell_label_kernel   looks every vertex's cell up: vlabel [V], the smallest vertex index of the cell (step 2).
//   simp_triple_kernel       one face per thread: the three labels; two equal: dropped (-1, -1, -1); else rotated so that the smallest
//                          comes first, which names the triple -> tri [F][3].  An index outside [0, V) sets bit 1 and drops the face.
//   simp_face_insert_kernel  THE TABLE again (refilled), key = the rotated triple, read from tri.
//   simp_face_mark_kernel    looks every face's triple up: the face stays when the smallest face index of the triple is its own ->
//                          fkeep [F]; a face that stays marks vflag of its three labels, plain byte stores of the same 1 (step 3).
//   simp_local_scan_kernel, simp_top_scan_kernel   mesh_scan.h's two levels over vflag and fkeep: the row of every kept label and face,
//                          totals = (V', F', error word) (step 4).
// THE TABLE: smallest index per key, open addressing over 32-bit entries, capacity a power of two >= 2 max(V, F), filled with -1.
// The key of an occupied slot is THE KEY OF THE ITEM WHOSE INDEX IT HOLDS (a cell: recomputed from that vertex; a triple: read from
// tri, which an earlier launch wrote).  Item i probes from a fixed hash of its key: old = atomicCAS(slot, -1, i); old == -1: the
// slot is i's; key(old) == key(i): atomicMin(slot, i) (skipped when old < i: entries only decrease), done; else the next slot.
//   * a slot never becomes empty again, and its key never changes: only items of the same key lower it;
//   * every decision is made on the value an ATOMIC returned from memory, never on a cached load, so a stale L1 on another XCD
//     cannot mislead it; the keys behind the indices are inputs of the launch;
//   * an item therefore ends in the first slot of its probe sequence that holds its key, all items of a key in the same one, and
//     the slot ends as their minimum: the result does not depend on the hash, the order of arrival or the capacity;
//   * the probe cap is the capacity (the table is at most half full); reaching it, or meeting an entry outside [0, n), sets bit 0.
// The look-ups run in a later launch, on a table nobody writes any more, with plain loads.
//
// voge_mesh_simplify_emit, step 5 and the outputs, on acc [V'][4 or 14] int64, zero-filled first:
//   simp_emit_kernel         one vertex and one face per thread: vert_index[v] = the row of v's label or -1; a vertex of a kept
//                          cluster adds 1 and round(x 2^sp), x = (v - c) / h in fp64 with c = lo + (cell + 1/2) h, to its row with
//                          64-bit INTEGER atomics; a kept face writes its corners' rows, in its own corner order, and face_index.
//   simp_quadric_kernel      ("quadric") one face per thread, all F of them: n = e1 x e2 normalised, e1 = (b - a) / h, e2 = (c - a) / h,
//                          fp64; zero or not finite: nothing; else per corner whose cluster is kept: 1, the six n n^T and the three
//                          n d terms, d = -n . x_corner, as round(t 2^sq), to that cluster's row.  (d^2, the quadric's constant,
//                          does not enter the solve and is not kept.)
//   simp_finish_kernel       one thread a kept label, fp64: count == 1: the vertex's own bits; "mean" or m == 0: c + h (sum / count);
//                          else (A + lambda m I) x = -b + lambda m mu by Cramer's rule, x clamped to [-1/2, 1/2]^3, c + x h; ONE
//                          rounding to fp32.
// voge_mesh_simplify_attr, up to eight channels a call, on its own accumulators [V'][9] int64 behind a 16-byte head:
//   simp_attr_absmax_kernel (D = the largest finite |value| of the slice, an integer atomic max on the bits), simp_attr_scatter_kernel
//   (round(a 2^sa) to the row; a value that is not finite sets the channel's bit in the row's ninth word instead),
//   simp_attr_finish_kernel (count == 1: the row's own bits; a flagged channel: NaN; else sum / count, one rounding).
// SCALES.  A cell index is decided in fp32 and may be off the fp64 quotient by 2^-23 of it, at most 3/8 below 2^21: |x| < 1 per axis,
// |x| < 2 as a vector, |d| < 2, |n_i n_j| <= 1.  With 2^Lv >= V and 2^Lf >= 3 F (the items that can meet in one row):
// sp = 60 - Lv, sq = 60 - Lf: |term| < 2^(s + 2), |sum| < 2^62.  sa = 62 - Lv - e with 2^e > D, clamped to +-1000: fixed_point.h's rule, as vn_scatter_kernel's.
// Integer addition is exact: the same bits on every run and under any permutation of the faces.
//
// BOUNDS against the definition (eps = 2^-24, u = 2^-53, M = max |coordinate|, q = 2^-s; a cluster of n vertices, m contributions):
//   mean     both are one fp32 rounding of c + h mean(x) resp. mean(p), equal in exact arithmetic.  The kernel's sum is off by at
//            most n qp / 2, its mean by qp / 2 cells; the fp64 steps (c, x, the definition's sum of n numbers) by (n + 8) u (M + h).
//            |v' - def| <= 2 eps |def| + h qp / 2 + (n + 8) u (M + h)             per axis.
//   quadric  the system is SPD with eigenvalues in [lambda m, (1 + lambda) m].  The kernel's matrix is off by E, |E_ij| <= m Q / 2,
//            Q = qq + 2 m u (fixed point, and the definition's fp64 sums in another order), |E|_2 <= 3 m Q / 2; its right side by e,
//            |e| <= sqrt(3) m (Q + lambda P) / 2, P = qp + 2 n u.  |x| <= X = 2 (1 + lambda) / lambda before the clamp (|b| <= 2 m,
//            |mu| <= 2).  |dx| <= (|e| + |E|_2 X) / (lambda m) = (sqrt(3) (Q + lambda P) + 3 Q X) / (2 lambda): the condition bound
//            (1 + lambda) / lambda times the quantum, twice over.  The clamp does not increase it.  2^-28 covers Cramer's rule in fp64.
//            |v' - def| <= the mean's bound + h (|dx| + 2^-28)                     per axis.
//   attr     |a' - def| <= 2 eps |def| + qa / 2 + (n + 8) u D,   qa = 2^-sa <= 2^(Lv - 61) D.
// tests/mesh_simplify_cases.py evaluates these and logs the share used.
#include <math.h>

#include "voge_common.h"
#include "fixed_point.h"
#include "mesh_scan.h"

namespace voge {

constexpr int kSimpErrCap = 1, kSimpErrIndex = 2, kSimpErrFinite = 4, kSimpErrCells = 8;
constexpr float kSimpMaxCell = 2097150.0f;      // 2^21 - 2: at most 2^21 - 1 cells on an axis
constexpr double kSimpLambda = 1e-3;            // Aggregation.MESH_SIMPLIFY_LAMBDA
constexpr int kSimpChannels = 8;                // attribute channels of one voge_mesh_simplify_attr call; ops.MESH_SIMPLIFY_CHANNELS
constexpr int kSimpRowMean = 4, kSimpRowQuadric = 14;      // int64 words of an accumulator row: n, x sums[, m, A (6), b (3)]
constexpr int kSimpRowAttr = kSimpChannels + 1;

struct SimpGrid {
  const float *verts;
  const uint32_t *lo_bits;      // ordered bits, in device memory
  float hx, hy, hz;
};

__device__ __forceinline__ uint32_t simp_ordered(const float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float simp_float(const uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// step 1 for vertex v; false when a cell index is negative, above the cap or not a number
__device__ __forceinline__ bool simp_cell(const SimpGrid &g, const size_t v, int (&c)[3]) {
  const float fx = floorf((g.verts[3 * v] - simp_float(g.lo_bits[0])) / g.hx);
  const float fy = floorf((g.verts[3 * v + 1] - simp_float(g.lo_bits[1])) / g.hy);
  const float fz = floorf((g.verts[3 * v + 2] - simp_float(g.lo_bits[2])) / g.hz);
  if (!(fx >= 0.0f && fx <= kSimpMaxCell && fy >= 0.0f && fy <= kSimpMaxCell && fz >= 0.0f && fz <= kSimpMaxCell)) return false;
  c[0] = (int)fx; c[1] = (int)fy; c[2] = (int)fz;
  return true;
}

// x = (v - c) / h of vertex v in the cell `c`, fp64
__device__ __forceinline__ void simp_local(const SimpGrid &g, const size_t v, const int (&c)[3], double (&x)[3]) {
  const double h[3] = {(double)g.hx, (double)g.hy, (double)g.hz};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double centre = (double)simp_float(g.lo_bits[k]) + ((double)c[k] + 0.5) * h[k];
    x[k] = ((double)g.verts[3 * v + k] - centre) / h[k];
  }
}

struct SimpCellKeys {      // key(i) = the cell of vertex i
  SimpGrid g;
  __device__ __forceinline__ bool get(const int i, int (&k)[3]) const { return simp_cell(g, (size_t)i, k); }
};
struct SimpTripleKeys {      // key(i) = the rotated triple of face i; a dropped face has none
  const int32_t *tri;
  __device__ __forceinline__ bool get(const int i, int (&k)[3]) const {
    k[0] = tri[3 * (size_t)i]; k[1] = tri[3 * (size_t)i + 1]; k[2] = tri[3 * (size_t)i + 2];
    return k[0] >= 0;
  }
};

__device__ __forceinline__ uint32_t simp_hash(const int (&k)[3]) {
  uint32_t x = (uint32_t)k[0] * 73856093u ^ (uint32_t)k[1] * 19349663u ^ (uint32_t)k[2] * 83492791u;
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ bool simp_same(const int (&a)[3], const int (&b)[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// THE TABLE's insert (header); false: the probe cap, or an entry that is no item
template <class Keys>
__device__ __forceinline__ bool simp_insert(int32_t *__restrict__ table, const uint32_t mask, const int i, const int n, const int (&key)[3],
                                          const Keys &keys) {
  uint32_t slot = simp_hash(key) & mask;
  for (uint32_t trips = 0; trips <= mask; ++trips) {
    const int old = atomicCAS(table + slot, -1, i);
    if (old == -1) return true;
    if ((unsigned)old >= (unsigned)n) return false;
    int other[3];
    if (keys.get(old, other) && simp_same(other, key)) {
      if (old > i) atomicMin(table + slot, i);
      return true;
    }
    slot = (slot + 1u) & mask;
  }
  return false;
}

// the smallest index of `key` in a table nobody writes; -1: not there, the probe cap, or an entry that is no item
template <class Keys>
__device__ __forceinline__ int simp_lookup(const int32_t *__restrict__ table, const uint32_t mask, const int n, const int (&key)[3],
                                         const Keys &keys) {
  uint32_t slot = simp_hash(key) & mask;
  for (uint32_t trips = 0; trips <= mask; ++trips) {
    const int e = table[slot];
    if ((unsigned)e >= (unsigned)n) return -1;      // (an empty slot too)
    int other[3];
    if (keys.get(e, other) && simp_same(other, key)) return e;
    slot = (slot + 1u) & mask;
  }
  return -1;
}

// ---- steps 1 and 2 ------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
simp_bbox_kernel(const float *__restrict__ verts, const int V, uint32_t *__restrict__ lo_bits, int32_t *__restrict__ err) {
  uint32_t m[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
  bool bad = false;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)V; v += (size_t)gridDim.x * 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = verts[3 * v + k];
      if (fabsf(x) < INFINITY) m[k] = min(m[k], simp_ordered(x)); else bad = true;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m[k] = min(m[k], (uint32_t)__shfl_xor((int)m[k], o, 64));
    if ((threadIdx.x & 63) == 0 && m[k] != 0xffffffffu) atomicMin(lo_bits + k, m[k]);
  }
  if (bad) atomicOr(err, kSimpErrFinite);
}

__global__ void __launch_bounds__(256)
simp_cell_insert_kernel(const SimpGrid g, const int V, int32_t *__restrict__ table, const uint32_t mask, int32_t *__restrict__ err) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  int c[3];
  if (!simp_cell(g, v, c)) {
    atomicOr(err, kSimpErrCells);
    return;
  }
  if (!simp_insert(table, mask, (int)v, V, c, SimpCellKeys{g})) atomicOr(err, kSimpErrCap);
}

__global__ void __launch_bounds__(256)
simp_cell_label_kernel(const SimpGrid g, const int V, const int32_t *__restrict__ table, const uint32_t mask, int32_t *__restrict__ vlabel,
                     int32_t *__restrict__ err) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  int c[3], label = (int)v;      // (its own index where step 1 failed: every later read stays inside the arrays)
  if (simp_cell(g, v, c)) {
    const int l = simp_lookup(table, mask, V, c, SimpCellKeys{g});
    if (l < 0) atomicOr(err, kSimpErrCap); else label = l;
  }
  vlabel[v] = label;
}

// ---- step 3 -------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
simp_triple_kernel(const int32_t *__restrict__ faces, const int F, const int V, const int32_t *__restrict__ vlabel, int32_t *__restrict__ tri,
                 int32_t *__restrict__ err) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  int a = -1, b = -1, c = -1;
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
    atomicOr(err, kSimpErrIndex);
  } else {
    const int l0 = vlabel[i0], l1 = vlabel[i1], l2 = vlabel[i2];
    if (l0 != l1 && l1 != l2 && l2 != l0) {
      if (l0 < l1 && l0 < l2) { a = l0; b = l1; c = l2; }
      else if (l1 < l2) { a = l1; b = l2; c = l0; }
      else { a = l2; b = l0; c = l1; }
    }
  }
  tri[3 * f] = a; tri[3 * f + 1] = b; tri[3 * f + 2] = c;
}

__global__ void __launch_bounds__(256)
simp_face_insert_kernel(const int32_t *__restrict__ tri, const int F, int32_t *__restrict__ table, const uint32_t mask, int32_t *__restrict__ err) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const SimpTripleKeys keys{tri};
  int key[3];
  if (!keys.get((int)f, key)) return;
  if (!simp_insert(table, mask, (int)f, F, key, keys)) atomicOr(err, kSimpErrCap);
}

__global__ void __launch_bounds__(256)
simp_face_mark_kernel(const int32_t *__restrict__ tri, const int F, const int V, const int32_t *__restrict__ table, const uint32_t mask,
                    uint8_t *__restrict__ fkeep, uint8_t *__restrict__ vflag, int32_t *__restrict__ err) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const SimpTripleKeys keys{tri};
  int key[3];
  bool keep = false;
  if (keys.get((int)f, key)) {
    const int first = simp_lookup(table, mask, F, key, keys);
    if (first < 0) atomicOr(err, kSimpErrCap);
    keep = first == (int)f && (unsigned)key[0] < (unsigned)V && (unsigned)key[1] < (unsigned)V && (unsigned)key[2] < (unsigned)V;
  }
  fkeep[f] = keep ? 1 : 0;
  if (keep) {
    vflag[key[0]] = 1; vflag[key[1]] = 1; vflag[key[2]] = 1;
  }
}

// ---- step 4 -------------------------------------------------------------------------------------------------------------------

// blocks [0, nbv): the labels' flags; blocks [nbv, nbv + nbf): the faces'.  loc and btot are laid out the same way (loc: V then F).
__global__ void __launch_bounds__(kMcBlock)
simp_local_scan_kernel(const int F, const int V, const uint8_t *__restrict__ fkeep, const uint8_t *__restrict__ vflag, const int nbv,
                     uint16_t *__restrict__ loc, uint32_t *__restrict__ btot) {
  const bool is_v = (int)blockIdx.x < nbv;
  const size_t i = (size_t)(is_v ? blockIdx.x : blockIdx.x - nbv) * kMcBlock + threadIdx.x;
  const bool in = i < (size_t)(is_v ? V : F);
  uint32_t x = 0u;
  if (in) x = (is_v ? vflag[i] : fkeep[i]) != 0;
  uint32_t upto;
  const uint32_t excl = mesh_scan_local(x, upto);
  if (in) loc[(is_v ? (size_t)0 : (size_t)V) + i] = (uint16_t)excl;
  if ((int)threadIdx.x == kMcBlock - 1) btot[blockIdx.x] = upto;      // (the last thread's inclusive prefix: the block's total)
}

__global__ void __launch_bounds__(kMcTop)
simp_top_scan_kernel(uint32_t *__restrict__ btot, const long nbv, const long nbf, const int32_t *__restrict__ err, long long *__restrict__ totals) {
  const uint32_t nv = mesh_scan_top(btot, nbv), nf = mesh_scan_top(btot + nbv, nbf);
  if (threadIdx.x == 0) {
    totals[0] = (long long)nv;
    totals[1] = (long long)nf;
    totals[2] = (long long)err[0];
  }
}

// ---- step 5 -------------------------------------------------------------------------------------------------------------------

struct SimpRows {      // the scan's tables: label l is output row blocks[l / 256] + loc[l] when vflag[l]
  const uint8_t *vflag;
  const uint16_t *loc;
  const uint32_t *blocks;
  long Vk;
  __device__ __forceinline__ long of(const int l) const {      // -1: dropped (or outside what the caller allocated)
    if (!vflag[l]) return -1;
    const long row = (long)blocks[l / kMcBlock] + (long)loc[l];
    return row < Vk ? row : -1;
  }
};

__global__ void __launch_bounds__(256)
simp_emit_kernel(const SimpGrid g, const int V, const int32_t *__restrict__ faces, const int F, const int32_t *__restrict__ vlabel,
               const uint8_t *__restrict__ fkeep, const SimpRows rows, const int nbv, const long Fk, const int sp, const int row_words,
               long long *__restrict__ acc, int32_t *__restrict__ faces_out, int32_t *__restrict__ vert_index, int32_t *__restrict__ face_index) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)V) {
    const int l = vlabel[i];
    const long row = (unsigned)l < (unsigned)V ? rows.of(l) : -1;
    vert_index[i] = (int32_t)row;
    int c[3];
    if (row >= 0 && simp_cell(g, i, c)) {
      double x[3];
      simp_local(g, i, c, x);
      const double scale = ldexp(1.0, sp);
      long long *a = acc + (size_t)row * row_words;
      atomic_add_i64(a, 1ll);
#pragma unroll
      for (int k = 0; k < 3; ++k) atomic_add_i64(a + 1 + k, llrint(x[k] * scale));
    }
  }
  if (i < (size_t)F && fkeep[i]) {
    const long row = (long)rows.blocks[nbv + i / kMcBlock] + (long)rows.loc[(size_t)V + i];
    if (row < Fk) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * i + k];      // (the face's own corner order: the rotation only names the triple)
        faces_out[3 * row + k] = (unsigned)v < (unsigned)V && (unsigned)vlabel[v] < (unsigned)V ? (int32_t)rows.of(vlabel[v]) : -1;
      }
      face_index[row] = (int32_t)i;
    }
  }
}

__global__ void __launch_bounds__(256)
simp_quadric_kernel(const SimpGrid g, const int V, const int32_t *__restrict__ faces, const int F, const int32_t *__restrict__ vlabel,
                  const SimpRows rows, const int sq, long long *__restrict__ acc) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const int iv[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  if ((unsigned)iv[0] >= (unsigned)V || (unsigned)iv[1] >= (unsigned)V || (unsigned)iv[2] >= (unsigned)V) return;
  const double h[3] = {(double)g.hx, (double)g.hy, (double)g.hz};
  double e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = (double)g.verts[3 * (size_t)iv[0] + k];
    e1[k] = ((double)g.verts[3 * (size_t)iv[1] + k] - a) / h[k];
    e2[k] = ((double)g.verts[3 * (size_t)iv[2] + k] - a) / h[k];
  }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  const double norm = sqrt((cx * cx + cy * cy) + cz * cz);
  if (!(norm > 0.0 && norm < (double)INFINITY)) return;
  const double n[3] = {cx / norm, cy / norm, cz / norm};
  const double scale = ldexp(1.0, sq);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int l = vlabel[iv[r]];
    const long row = (unsigned)l < (unsigned)V ? rows.of(l) : -1;
    int c[3];
    if (row < 0 || !simp_cell(g, (size_t)iv[r], c)) continue;
    double x[3];
    simp_local(g, (size_t)iv[r], c, x);
    const double d = -((n[0] * x[0] + n[1] * x[1]) + n[2] * x[2]);
    long long *a = acc + (size_t)row * kSimpRowQuadric + kSimpRowMean;
    atomic_add_i64(a, 1ll);
    atomic_add_i64(a + 1, llrint(n[0] * n[0] * scale));
    atomic_add_i64(a + 2, llrint(n[0] * n[1] * scale));
    atomic_add_i64(a + 3, llrint(n[0] * n[2] * scale));
    atomic_add_i64(a + 4, llrint(n[1] * n[1] * scale));
    atomic_add_i64(a + 5, llrint(n[1] * n[2] * scale));
    atomic_add_i64(a + 6, llrint(n[2] * n[2] * scale));
    atomic_add_i64(a + 7, llrint(n[0] * d * scale));
    atomic_add_i64(a + 8, llrint(n[1] * d * scale));
    atomic_add_i64(a + 9, llrint(n[2] * d * scale));
  }
}

__device__ __forceinline__ double simp_det3(const double m00, const double m01, const double m02, const double m10, const double m11,
                                          const double m12, const double m20, const double m21, const double m22) {
  return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20);
}

__global__ void __launch_bounds__(256)
simp_finish_kernel(const SimpGrid g, const int V, const SimpRows rows, const int sp, const int sq, const int row_words,
                 const long long *__restrict__ acc, float *__restrict__ verts_out) {
  const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= (size_t)V) return;
  const long row = rows.of((int)l);
  int c[3];
  if (row < 0 || !simp_cell(g, l, c)) return;
  float *out = verts_out + 3 * row;
  const long long *a = acc + (size_t)row * row_words;
  if (a[0] <= 1) {      // (the label is the cluster's only vertex)
    out[0] = g.verts[3 * l]; out[1] = g.verts[3 * l + 1]; out[2] = g.verts[3 * l + 2];
    return;
  }
  const double count = (double)a[0], unit = ldexp(1.0, -sp);
  double x[3] = {(double)a[1] * unit / count, (double)a[2] * unit / count, (double)a[3] * unit / count};
  if (row_words == kSimpRowQuadric && a[kSimpRowMean] > 0) {
    const long long *q = a + kSimpRowMean;
    const double uq = ldexp(1.0, -sq), lm = kSimpLambda * (double)q[0];
    const double a00 = (double)q[1] * uq + lm, a01 = (double)q[2] * uq, a02 = (double)q[3] * uq, a11 = (double)q[4] * uq + lm,
                 a12 = (double)q[5] * uq, a22 = (double)q[6] * uq + lm;
    const double r0 = lm * x[0] - (double)q[7] * uq, r1 = lm * x[1] - (double)q[8] * uq, r2 = lm * x[2] - (double)q[9] * uq;
    const double det = simp_det3(a00, a01, a02, a01, a11, a12, a02, a12, a22);
    x[0] = simp_det3(r0, a01, a02, r1, a11, a12, r2, a12, a22) / det;
    x[1] = simp_det3(a00, r0, a02, a01, r1, a12, a02, r2, a22) / det;
    x[2] = simp_det3(a00, a01, r0, a01, a11, r1, a02, a12, r2) / det;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = fmin(fmax(x[k], -0.5), 0.5);
  }
  const double h[3] = {(double)g.hx, (double)g.hy, (double)g.hz};
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = (float)(((double)simp_float(g.lo_bits[k]) + ((double)c[k] + 0.5) * h[k]) + x[k] * h[k]);
}

// ---- attributes ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
simp_attr_absmax_kernel(const float *__restrict__ attr, const int V, const int C, const int c0, const int nc, FixedHead *__restrict__ head) {
  uint32_t m = 0u;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)V; v += (size_t)gridDim.x * 256)
    for (int k = 0; k < nc; ++k) {
      const float x = attr[v * C + c0 + k];
      if (fabsf(x) < INFINITY) m = max(m, __float_as_uint(x) & 0x7fffffffu);
    }
  fixed_commit_max(head, m);      // (D is finite by construction)
}

__global__ void __launch_bounds__(256)
simp_attr_scatter_kernel(const float *__restrict__ attr, const int V, const int C, const int c0, const int nc, const int32_t *__restrict__ vlabel,
                       const SimpRows rows, const FixedHead *__restrict__ head, const int list_bits, long long *__restrict__ acc) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  const int l = vlabel[v];
  const long row = (unsigned)l < (unsigned)V ? rows.of(l) : -1;
  if (row < 0) return;
  const double scale = ldexp(1.0, fixed_scale_exponent(head, list_bits));
  long long *a = acc + (size_t)row * kSimpRowAttr;
  unsigned long long bad = 0ull;
  for (int k = 0; k < nc; ++k) {
    const float x = attr[v * C + c0 + k];
    if (fabsf(x) < INFINITY) {
      const long long t = llrint((double)x * scale);
      if (t) atomic_add_i64(a + k, t);
    } else {
      bad |= 1ull << k;
    }
  }
  if (bad) atomicOr(reinterpret_cast<unsigned long long *>(a + kSimpChannels), bad);
}

__global__ void __launch_bounds__(256)
simp_attr_finish_kernel(const float *__restrict__ attr, const int V, const int C, const int c0, const int nc, const SimpRows rows,
                      const FixedHead *__restrict__ head, const int list_bits, const long long *__restrict__ acc,
                      const long long *__restrict__ count, const int count_words, float *__restrict__ attr_out) {
  const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= (size_t)V) return;
  const long row = rows.of((int)l);
  if (row < 0) return;
  const long long n = count[(size_t)row * count_words];
  const long long *a = acc + (size_t)row * kSimpRowAttr;
  const double unit = ldexp(1.0, -fixed_scale_exponent(head, list_bits));
  for (int k = 0; k < nc; ++k) {
    float y;
    if (n <= 1) y = attr[l * C + c0 + k];      // (the label is the cluster's only vertex)
    else if ((a[kSimpChannels] >> k) & 1) y = NAN;
    else y = (float)((double)a[k] * unit / (double)n);
    attr_out[(size_t)row * C + c0 + k] = y;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool simp_sizes_ok(const long V, const long F) { return V >= 1 && F >= 1 && V <= kMcMax && F <= kMcMax; }
static size_t simp_capacity(const long V, const long F) { return (size_t)1 << ceil_log2(2 * (V > F ? V : F)); }

struct SimpLayout {      // the scan's workspace: [err 16 | vflag] is zero-filled as one range, [lo 16 | table] with 0xFF as one
  size_t err, vflag, lo, table, vlabel, tri, fkeep, loc, blocks, bytes;
  long nbv, nbf;
  size_t cap;
};
static SimpLayout simp_layout(const long V, const long F) {
  SimpLayout w;
  w.nbv = (V + kMcBlock - 1) / kMcBlock;
  w.nbf = (F + kMcBlock - 1) / kMcBlock;
  w.cap = simp_capacity(V, F);
  Carve c;
  w.err = c.take(16);
  w.vflag = c.take((size_t)V);
  w.lo = c.take(16);
  w.table = c.take_exact(w.cap * 4);      // (a power of two >= 2 entries: 8 bytes for V = F = 1, a multiple of 16 otherwise)
  w.vlabel = c.take((size_t)V * 4);
  w.tri = c.take((size_t)F * 12);
  w.fkeep = c.take((size_t)F);
  w.loc = c.take((size_t)(V + F) * 2);
  w.blocks = c.take((size_t)(w.nbv + w.nbf) * 4);
  w.bytes = c.at;
  return w;
}
static bool simp_cell_size_ok(const float hx, const float hy, const float hz) {
  return hx > 0.0f && hy > 0.0f && hz > 0.0f && hx < INFINITY && hy < INFINITY && hz < INFINITY;
}
static size_t simp_attr_bytes(const long Vk) { return sizeof(FixedHead) + (size_t)Vk * kSimpRowAttr * sizeof(long long); }

template <class T>
static T *simp_at(void *workspace, const size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + offset); }

static SimpRows simp_rows(void *workspace, const SimpLayout &w, const long Vk) {
  return SimpRows{simp_at<uint8_t>(workspace, w.vflag), simp_at<uint16_t>(workspace, w.loc), simp_at<uint32_t>(workspace, w.blocks), Vk};
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_mesh_simplify_workspace_bytes(long V, long F) {
  if (!simp_sizes_ok(V, F)) return 0;
  return simp_layout(V, F).bytes;
}

extern "C" size_t voge_mesh_simplify_acc_bytes(long Vk, int quadric) {
  if (Vk < 1 || Vk > kMcMax) return 0;
  return (size_t)Vk * (quadric ? kSimpRowQuadric : kSimpRowMean) * sizeof(long long);
}

extern "C" size_t voge_mesh_simplify_attr_workspace_bytes(long Vk) {
  if (Vk < 1 || Vk > kMcMax) return 0;
  return simp_attr_bytes(Vk);
}

extern "C" int voge_mesh_simplify_scan(const float *verts, long V, const int32_t *faces, long F, float hx, float hy, float hz,
                                       void *workspace, size_t workspace_bytes, long long *totals, int stages, voge_stream_t stream) {
  if (!simp_sizes_ok(V, F) || !simp_cell_size_ok(hx, hy, hz) || (stages & ~255) || !stages) return VOGE_ERR_BAD_ARG;
  if (!verts || !faces || !totals || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  const SimpLayout w = simp_layout(V, F);
  if (workspace_bytes < w.bytes) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t *err = simp_at<int32_t>(workspace, w.err), *table = simp_at<int32_t>(workspace, w.table);
  int32_t *vlabel = simp_at<int32_t>(workspace, w.vlabel), *tri = simp_at<int32_t>(workspace, w.tri);
  uint8_t *vflag = simp_at<uint8_t>(workspace, w.vflag), *fkeep = simp_at<uint8_t>(workspace, w.fkeep);
  const SimpGrid g{verts, simp_at<uint32_t>(workspace, w.lo), hx, hy, hz};
  const uint32_t mask = (uint32_t)(w.cap - 1);
  if (stages & 1) {      // err and vflag: 0; lo and the table: 0xFF (the largest ordered bits; -1, an empty slot)
    hipError_t fe = voge_fill_async(err, 0, w.lo - w.err, st);
    if (fe == hipSuccess) fe = voge_fill_async(simp_at<void>(workspace, w.lo), 0xff, 16 + w.cap * 4, st);
    if (fe != hipSuccess) return (int)fe;
    hipLaunchKernelGGL(simp_bbox_kernel, dim3(blocks256_capped((size_t)V)), dim3(256), 0, st, verts, (int)V, simp_at<uint32_t>(workspace, w.lo), err);
  }
  if (stages & 2) hipLaunchKernelGGL(simp_cell_insert_kernel, dim3(blocks256(V)), dim3(256), 0, st, g, (int)V, table, mask, err);
  if (stages & 4) hipLaunchKernelGGL(simp_cell_label_kernel, dim3(blocks256(V)), dim3(256), 0, st, g, (int)V, table, mask, vlabel, err);
  if (stages & 8) hipLaunchKernelGGL(simp_triple_kernel, dim3(blocks256(F)), dim3(256), 0, st, faces, (int)F, (int)V, vlabel, tri, err);
  if (stages & 16) {
    const hipError_t fe = voge_fill_async(table, 0xff, w.cap * 4, st);
    if (fe != hipSuccess) return (int)fe;
    hipLaunchKernelGGL(simp_face_insert_kernel, dim3(blocks256(F)), dim3(256), 0, st, tri, (int)F, table, mask, err);
  }
  if (stages & 32) hipLaunchKernelGGL(simp_face_mark_kernel, dim3(blocks256(F)), dim3(256), 0, st, tri, (int)F, (int)V, table, mask, fkeep, vflag, err);
  if (stages & 64)
    hipLaunchKernelGGL(simp_local_scan_kernel, dim3((unsigned)(w.nbv + w.nbf)), dim3(kMcBlock), 0, st, (int)F, (int)V, fkeep, vflag, (int)w.nbv,
                       simp_at<uint16_t>(workspace, w.loc), simp_at<uint32_t>(workspace, w.blocks));
  if (stages & 128)
    hipLaunchKernelGGL(simp_top_scan_kernel, dim3(1), dim3(kMcTop), 0, st, simp_at<uint32_t>(workspace, w.blocks), w.nbv, w.nbf, err, totals);
  return launch_status();
}

extern "C" int voge_mesh_simplify_emit(const float *verts, long V, const int32_t *faces, long F, float hx, float hy, float hz, int quadric,
                                       void *workspace, size_t workspace_bytes, long Vk, long Fk, void *acc, size_t acc_bytes,
                                       float *verts_out, int32_t *faces_out, int32_t *vert_index, int32_t *face_index, int stages,
                                       voge_stream_t stream) {
  if (!simp_sizes_ok(V, F) || !simp_cell_size_ok(hx, hy, hz) || Vk < 1 || Fk < 1 || Vk > V || Fk > F || (stages & ~15) || !stages)
    return VOGE_ERR_BAD_ARG;
  if (!verts || !faces || bad_workspace(workspace) || !acc || !verts_out || !faces_out || !vert_index || !face_index ||
      (reinterpret_cast<uintptr_t>(acc) & 7) != 0)
    return VOGE_ERR_BAD_ARG;
  const SimpLayout w = simp_layout(V, F);
  const int words = quadric ? kSimpRowQuadric : kSimpRowMean;
  if (workspace_bytes < w.bytes || acc_bytes < (size_t)Vk * words * sizeof(long long)) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const SimpGrid g{verts, simp_at<uint32_t>(workspace, w.lo), hx, hy, hz};
  const SimpRows rows = simp_rows(workspace, w, Vk);
  const int32_t *vlabel = simp_at<int32_t>(workspace, w.vlabel);
  long long *sums = static_cast<long long *>(acc);
  const int sp = 60 - ceil_log2(V), sq = 60 - ceil_log2(3 * F);      // the vertices, the corners that can meet in one row (SCALES)
  if (stages & 1) {
    const hipError_t fe = voge_fill_async(acc, 0, (size_t)Vk * words * sizeof(long long), st);
    if (fe != hipSuccess) return (int)fe;
  }
  if (stages & 2)
    hipLaunchKernelGGL(simp_emit_kernel, dim3(blocks256(V > F ? V : F)), dim3(256), 0, st, g, (int)V, faces, (int)F, vlabel,
                       simp_at<uint8_t>(workspace, w.fkeep), rows, (int)w.nbv, Fk, sp, words, sums, faces_out, vert_index, face_index);
  if ((stages & 4) && quadric) hipLaunchKernelGGL(simp_quadric_kernel, dim3(blocks256(F)), dim3(256), 0, st, g, (int)V, faces, (int)F, vlabel, rows, sq, sums);
  if (stages & 8) hipLaunchKernelGGL(simp_finish_kernel, dim3(blocks256(V)), dim3(256), 0, st, g, (int)V, rows, sp, sq, words, sums, verts_out);
  return launch_status();
}

extern "C" int voge_mesh_simplify_attr(const float *attr, long V, long F, int C, int c0, int nc, const void *workspace, size_t workspace_bytes,
                                       long Vk, const void *acc, int quadric, void *attr_workspace, size_t attr_workspace_bytes,
                                       float *attr_out, int stages, voge_stream_t stream) {
  if (!simp_sizes_ok(V, F) || Vk < 1 || Vk > V || C < 1 || c0 < 0 || nc < 1 || nc > kSimpChannels || c0 + nc > C || (stages & ~15) || !stages)
    return VOGE_ERR_BAD_ARG;
  if (!attr || bad_workspace(workspace) || !acc || bad_workspace(attr_workspace) || !attr_out) return VOGE_ERR_BAD_ARG;
  const SimpLayout w = simp_layout(V, F);
  if (workspace_bytes < w.bytes || attr_workspace_bytes < simp_attr_bytes(Vk)) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const SimpRows rows = simp_rows(const_cast<void *>(workspace), w, Vk);
  const int32_t *vlabel = simp_at<int32_t>(const_cast<void *>(workspace), w.vlabel);
  FixedHead *head = static_cast<FixedHead *>(attr_workspace);
  long long *sums = simp_at<long long>(attr_workspace, sizeof(FixedHead));
  const int bits = ceil_log2(V);      // V <= 2^bits: the vertices that can meet in one row
  if (stages & 1) {
    const hipError_t fe = voge_fill_async(attr_workspace, 0, simp_attr_bytes(Vk), st);
    if (fe != hipSuccess) return (int)fe;
  }
  if (stages & 2) hipLaunchKernelGGL(simp_attr_absmax_kernel, dim3(blocks256_capped((size_t)V)), dim3(256), 0, st, attr, (int)V, C, c0, nc, head);
  if (stages & 4) hipLaunchKernelGGL(simp_attr_scatter_kernel, dim3(blocks256(V)), dim3(256), 0, st, attr, (int)V, C, c0, nc, vlabel, rows, head, bits, sums);
  if (stages & 8)
    hipLaunchKernelGGL(simp_attr_finish_kernel, dim3(blocks256(V)), dim3(256), 0, st, attr, (int)V, C, c0, nc, rows, head, bits, sums,
                       static_cast<const long long *>(acc), quadric ? kSimpRowQuadric : kSimpRowMean, attr_out);
  return launch_status();
}
