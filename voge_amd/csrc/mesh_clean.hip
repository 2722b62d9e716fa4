// Mesh clean-up (EXTENSION: the reference has none; what the 2D Gaussian splatting pipeline does between extracting a mesh and scoring
// or saving it): connected components of a triangle mesh, the filter that keeps the largest of them, and area-weighted vertex
// normals.  One mesh per call: verts [V,3] fp32, faces [F,3] int32.  Aggregation.mesh_components, Aggregation.mesh_clean and
// Aggregation.mesh_vertex_normals are the definitions; nothing here is differentiable.  No float atomics anywhere.
//
// voge_mesh_components, three launches.  Two vertices are connected when a chain of faces links them; a component's label is its
// smallest vertex index.  A lock-free union-find over parent [V]:
//   (1) mc_init_kernel: parent[x] = x, count[x] = 0, meta = 0.
//   (2) mc_link_kernel, one face per thread: unite(i0, i1), unite(i0, i2).
//   (3) mc_label_kernel, one vertex and one face per thread, after (2) has finished: the root of a walk along parent is the label;
//       a face takes the label of its first vertex and adds 1 to count[label] with a 32-bit integer atomic (exact: the same
//       numbers on every run; the lanes of a wave that share a label add once, together), and the add that finds 0 adds 1 to
//       meta[1], the number of components.
// INVARIANT of (2): parent[x] <= x at all times, and an entry only ever decreases.  Every write to parent is a device-scope atomic
// of one of two kinds:
//   link      atomicCAS(&parent[a], a, b) with b < a: it succeeds only while a is a root, and then hangs a under b;
//   shorten   atomicMin(&parent[x], g) with g = parent[parent[x]] as read: it replaces a pointer by a pointer further up.
// Call the edges the successful links made the LINK FOREST: an edge always leads to a lower index, so it is a forest, a node gets
// its edge once and keeps it (after the link parent[a] != a for good, so no later CAS on a succeeds), and "y is an ancestor of x in
// the link forest" can therefore only become true, never false again.  Every value parent[x] ever holds is such an ancestor of x:
// x itself at the start, the link's b, and a shortening writes parent[p] for an ancestor p of x, an ancestor of an ancestor.  So:
//   * STALE READS ARE HARMLESS.  The loads of parent are relaxed workgroup-scope atomic loads -- whole words, not re-ordered or
//     invented by the compiler, but served from the CU's L1, and a workgroup on another XCD need not see a store made during the
//     launch.  Whatever value a load returns is one parent[x] HAS held: an ancestor of x in the link forest, in x's component, not
//     above x.  A walk along stale pointers is a walk up the link forest that may stop below the true root ("a root as last
//     seen"); the CAS that follows operates on memory, not on a cached copy, fails when its a is no root any more, and returns
//     what parent[a] holds -- an ancestor of a, below a -- from where the thread goes on.  A b that is no root any more is no
//     error either: a root hung under ANY lower node of the other tree joins the two trees.
//   * EVERY LOOP TRIP STRICTLY LOWERS AN INDEX.  A trip of the walk replaces x by parent[x] < x (the walk ends at parent[x] == x);
//     a trip of unite's loop either ends it (same node reached from both sides: one tree for good; or the link succeeded) or
//     replaces a by the CAS's return value < a.  a and b are non-negative and below V, so one unite makes fewer than 2 V trips
//     in all, whatever the other threads do: NO THREAD EVER WAITS FOR ANOTHER, there is no lock and no spin on a value.
//   * AFTER THE LAUNCH every face's three vertices are in one tree of the link forest, a tree's root is its smallest index, and
//     parent's pointers lead to it: launch (3) reads labels off a forest nobody writes any more.
// Every loop carries a trip cap a correct run cannot reach (2 V for a unite, V for a walk of (3)) and checks that the index it
// moves to is lower than the one it leaves (which also keeps every read inside parent); a thread that meets either sets bit 0 of
// meta[0] and leaves.  A face that names a vertex outside [0, V) sets bit 1 and joins nothing.  The caller reads meta back.
//
// voge_mesh_clean_scan / _emit: the filter.  keep_root [V] (bytes) says which labels stay -- the ranking is the caller's.
//   scan, four launches: the zero fill of vflag [V]; mc_mark_kernel (a kept face sets vflag of its three vertices: plain byte
//     stores of the same 1); mc_local_scan_kernel (kMcBlock flags a workgroup, vertices' blocks first, then the faces': the
//     exclusive prefix inside the block as a 16-bit number and the block's total); mc_top_scan_kernel, ONE workgroup of kMcTop:
//     both tables of block totals become their exclusive scans in place, kMcTop entries a round with the total carried, and
//     totals = (V', F', error word) -- what the caller reads back to size the outputs: the one synchronisation of the filter.
//   emit, one launch: a kept vertex v goes to row blocks[v / 256] + loc[v] with its bits and writes vert_index there; a kept
//     face goes to its row with its three indices renumbered the same way and writes face_index.  Order is kept on both sides.
// Integer sums only: the same bits on every run.
//
// voge_vertex_normals, four launches, nothing read back (capturable): PyTorch3D's verts_normals_packed, the normalised sum over the
// faces at a vertex of cr = (b - a) x (c - a), which weights them by area.  cr is mesh_sample.hip's ms_face: differences first,
// every component (p q) - (r s), one IEEE fp32 operation each (-ffp-contract=off): the bits of Aggregation._face_cross.  The sum is
// made in FIXED POINT (fixed_point.h: the head, the exponent rule and its bound): the zero fill of acc [V][4] and the head;
// vn_absmax_kernel (D = the largest finite |cr| component, by an integer atomic max on the float's bits: a maximum has no order);
// vn_scatter_kernel (s = 62 - L - e with 2^L >= 3 F -- a vertex is named by at most 3 F corners -- and 2^e > D, chosen by every
// thread from D, clamped to +-1000; round(cr 2^s) added to the face's three vertices with 64-bit INTEGER atomics: |term| <= 2^(62 - L),
// so |sum| <= 2^62 cannot overflow; a face whose cr is not finite adds 1 to the fourth slot of its vertices instead); vn_finish_kernel,
// one thread a vertex: the sum as fp64, its norm in fp64, one rounding to fp32; (0, 0, 0) where the sum is zero, where a term was
// not finite, and for a vertex no face names.  Integer addition is exact, so the bits do not depend on the order of the faces.
// Error: with q = 2^-s <= 2^(L - 61) D a vertex that m corners name is off by at most m q / 2 per component before it is normalised.
// A face that names a vertex outside [0, V) is skipped.
#include <math.h>

#include "voge_common.h"
#include "fixed_point.h"
#include "mesh_scan.h"      // kMcBlock, kMcTop, kMcMax and the two scan levels, shared with mesh_simplify.hip

namespace voge {

constexpr int kMcErrCap = 1, kMcErrIndex = 2;
constexpr int kMcPeel = 4;             // rounds in which the label launch counts a root once for all the lanes of a wave that have it

// ---- components ---------------------------------------------------------------------------------------------------------------

// (header: a whole word, possibly stale)
__device__ __forceinline__ int mc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root above x as this thread sees it, shortening the path on the way; -1 when the trip cap or the invariant fails
__device__ __forceinline__ int mc_find(int32_t *__restrict__ parent, int x, int &budget) {
  int p = mc_load(parent + x);
  while (p != x) {
    if (--budget < 0 || (unsigned)p > (unsigned)x) return -1;
    const int g = mc_load(parent + p);      // (p < x < V: inside the table)
    if ((unsigned)g > (unsigned)p) return -1;
    if (g < p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ bool mc_unite(int32_t *__restrict__ parent, int a, int b, int budget) {
  for (;;) {
    a = mc_find(parent, a, budget);
    if (a < 0) return false;
    b = mc_find(parent, b, budget);
    if (b < 0) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return true;
    if (--budget < 0 || (unsigned)old >= (unsigned)a) return false;
    a = old;
  }
}

__global__ void __launch_bounds__(256)
mc_init_kernel(int32_t *__restrict__ parent, int32_t *__restrict__ count, const int V, int32_t *__restrict__ meta) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < 4) meta[i] = 0;
  if (i < (size_t)V) {
    parent[i] = (int32_t)i;
    count[i] = 0;
  }
}

__global__ void __launch_bounds__(256)
mc_link_kernel(const int32_t *__restrict__ faces, const int F, const int V, int32_t *__restrict__ parent, int32_t *__restrict__ meta) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
    atomicOr(meta, kMcErrIndex);
    return;
  }
  const int budget = 2 * V;      // (V < 2^28)
  bool ok = true;
  if (i1 != i0) ok = mc_unite(parent, i0, i1, budget);
  if (ok && i2 != i0 && i2 != i1) ok = mc_unite(parent, i0, i2, budget);
  if (!ok) atomicOr(meta, kMcErrCap);
}

// the root above x in a table nobody writes; -1 when the trip cap or the invariant fails
__device__ __forceinline__ int mc_root(const int32_t *__restrict__ parent, int x, const int V) {
  for (int trips = 0; trips <= V; ++trips) {
    const int p = parent[x];
    if (p == x) return x;
    if ((unsigned)p > (unsigned)x) return -1;
    x = p;
  }
  return -1;
}

__global__ void __launch_bounds__(256)
mc_label_kernel(const int32_t *__restrict__ faces, const int F, const int V, const int32_t *__restrict__ parent,
                int32_t *__restrict__ vert_label, int32_t *__restrict__ face_label, int32_t *__restrict__ count, int32_t *__restrict__ meta) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)V) {
    const int r = mc_root(parent, (int)i, V);
    if (r < 0) atomicOr(meta, kMcErrCap);
    vert_label[i] = r < 0 ? (int32_t)i : r;
  }
  int r = -1;
  if (i < (size_t)F) {
    const int i0 = faces[3 * i];
    if ((unsigned)i0 < (unsigned)V) {
      r = mc_root(parent, i0, V);
      if (r < 0) atomicOr(meta, kMcErrCap);
    }
    face_label[i] = r;
  }
  // The faces of a wave mostly share their root, and a million adds to ONE address serialise (11.5 ms of this launch's 11.5 at the
  // 256^3 sphere): up to kMcPeel times the first pending lane's root is counted once for every lane that has it; whoever is left
  // adds for itself.  Integer sums: the grouping does not show.  (No lane has left the kernel: every wave is whole here.)
  bool pending = r >= 0;
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int round = 0; round < kMcPeel; ++round) {
    const unsigned long long act = __ballot(pending);
    if (!act) break;      // (the same in every lane)
    const int leader = __ffsll(act) - 1;
    const int r0 = __shfl(r, leader, 64);
    const bool mine = pending && r == r0;
    const unsigned long long same = __ballot(mine);
    if (lane == leader && atomicAdd(count + r0, (int)__popcll(same)) == 0) atomicAdd(meta + 1, 1);
    pending = pending && !mine;
  }
  if (pending && atomicAdd(count + r, 1) == 0) atomicAdd(meta + 1, 1);
}

// ---- the filter ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool mc_face_kept(const int32_t *__restrict__ face_label, const uint8_t *__restrict__ keep_root, const size_t f,
                                             const int V) {
  const int l = face_label[f];
  return (unsigned)l < (unsigned)V && keep_root[l] != 0;
}

__global__ void __launch_bounds__(256)
mc_mark_kernel(const int32_t *__restrict__ faces, const int F, const int V, const int32_t *__restrict__ face_label,
               const uint8_t *__restrict__ keep_root, uint8_t *__restrict__ vflag, int32_t *__restrict__ err) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  if ((unsigned)face_label[f] >= (unsigned)V) {
    atomicOr(err, kMcErrIndex);
    return;
  }
  if (!mc_face_kept(face_label, keep_root, f, V)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = faces[3 * f + k];
    if ((unsigned)v < (unsigned)V) vflag[v] = 1; else atomicOr(err, kMcErrIndex);
  }
}

// blocks [0, nbv): the vertices' flags; blocks [nbv, nbv + nbf): the faces'.  loc and btot are laid out the same way (loc: V then F).
__global__ void __launch_bounds__(kMcBlock)
mc_local_scan_kernel(const int F, const int V, const int32_t *__restrict__ face_label, const uint8_t *__restrict__ keep_root,
                     const uint8_t *__restrict__ vflag, const int nbv, uint16_t *__restrict__ loc, uint32_t *__restrict__ btot) {
  const int tid = threadIdx.x;
  const bool is_v = (int)blockIdx.x < nbv;
  const size_t i = (size_t)(is_v ? blockIdx.x : blockIdx.x - nbv) * kMcBlock + tid;
  const bool in = i < (size_t)(is_v ? V : F);
  uint32_t x = 0u;
  if (in) x = is_v ? (vflag[i] != 0) : mc_face_kept(face_label, keep_root, i, V);
  uint32_t upto;
  const uint32_t excl = mesh_scan_local(x, upto);
  if (in) loc[(is_v ? (size_t)0 : (size_t)V) + i] = (uint16_t)excl;
  if (tid == kMcBlock - 1) btot[blockIdx.x] = upto;      // (the last thread's inclusive prefix: the block's total)
}

// ONE workgroup: the exclusive scans of btot[0, nbv) and btot[nbv, nbv + nbf) in place; totals = (V', F', error word)
__global__ void __launch_bounds__(kMcTop)
mc_top_scan_kernel(uint32_t *__restrict__ btot, const long nbv, const long nbf, const int32_t *__restrict__ err, long long *__restrict__ totals) {
  const int tid = threadIdx.x;
  const uint32_t nv = mesh_scan_top(btot, nbv), nf = mesh_scan_top(btot + nbv, nbf);
  if (tid == 0) totals[0] = (long long)nv;
  if (tid == 0) totals[1] = (long long)nf;
  if (tid == 0) totals[2] = (long long)err[0];
}

__global__ void __launch_bounds__(256)
mc_emit_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, const int F, const int V,
               const int32_t *__restrict__ face_label, const uint8_t *__restrict__ keep_root, const uint8_t *__restrict__ vflag,
               const uint16_t *__restrict__ loc, const uint32_t *__restrict__ blocks, const int nbv, const long Vk, const long Fk,
               float *__restrict__ verts_out, int32_t *__restrict__ faces_out, int32_t *__restrict__ vert_index,
               int32_t *__restrict__ face_index) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)V && vflag[i]) {
    const long row = (long)blocks[i / kMcBlock] + (long)loc[i];
    if (row < Vk) {      // (the sizes the caller allocated)
      verts_out[3 * row] = verts[3 * i];
      verts_out[3 * row + 1] = verts[3 * i + 1];
      verts_out[3 * row + 2] = verts[3 * i + 2];
      vert_index[row] = (int32_t)i;
    }
  }
  if (i < (size_t)F && mc_face_kept(face_label, keep_root, i, V)) {
    const long row = (long)blocks[nbv + i / kMcBlock] + (long)loc[(size_t)V + i];
    if (row < Fk) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * i + k];
        faces_out[3 * row + k] = (unsigned)v < (unsigned)V ? (int32_t)(blocks[v / kMcBlock] + (uint32_t)loc[v]) : -1;
      }
      face_index[row] = (int32_t)i;
    }
  }
}

// ---- vertex normals -----------------------------------------------------------------------------------------------------------

struct VnCross {
  float x, y, z;
  bool ok;      // the face's indices are inside the table
};

// mesh_sample.hip's ms_face: differences first, every component (p q) - (r s)
__device__ __forceinline__ VnCross vn_cross(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const size_t f,
                                            int (&iv)[3]) {
  VnCross c = {0.0f, 0.0f, 0.0f, false};
  iv[0] = faces[3 * f]; iv[1] = faces[3 * f + 1]; iv[2] = faces[3 * f + 2];
  if (!face_in_range(iv[0], iv[1], iv[2], V)) return c;
  const float *a = verts + 3 * (size_t)iv[0], *b = verts + 3 * (size_t)iv[1], *cc = verts + 3 * (size_t)iv[2];
  const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const float e2x = cc[0] - a[0], e2y = cc[1] - a[1], e2z = cc[2] - a[2];
  c.x = (e1y * e2z) - (e1z * e2y);
  c.y = (e1z * e2x) - (e1x * e2z);
  c.z = (e1x * e2y) - (e1y * e2x);
  c.ok = true;
  return c;
}

__device__ __forceinline__ bool vn_finite(const VnCross &c) { return fabsf(c.x) < INFINITY && fabsf(c.y) < INFINITY && fabsf(c.z) < INFINITY; }

__global__ void __launch_bounds__(256)
vn_absmax_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F, FixedHead *__restrict__ head) {
  uint32_t m = 0u;
  for (size_t f = (size_t)blockIdx.x * 256 + threadIdx.x; f < (size_t)F; f += (size_t)gridDim.x * 256) {
    int iv[3];
    const VnCross c = vn_cross(verts, V, faces, f, iv);
    if (c.ok && vn_finite(c))
      m = max(m, max(__float_as_uint(c.x) & 0x7fffffffu, max(__float_as_uint(c.y) & 0x7fffffffu, __float_as_uint(c.z) & 0x7fffffffu)));
  }
  fixed_commit_max(head, m);      // (D is finite by construction)
}

__global__ void __launch_bounds__(256)
vn_scatter_kernel(const float *__restrict__ verts, const int V, const int32_t *__restrict__ faces, const int F,
                  const FixedHead *__restrict__ head, const int list_bits, long long *__restrict__ acc) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  int iv[3];
  const VnCross c = vn_cross(verts, V, faces, f, iv);
  if (!c.ok) return;
  if (!vn_finite(c)) {
#pragma unroll
    for (int r = 0; r < 3; ++r) atomic_add_i64(acc + 4 * (size_t)iv[r] + 3, 1ll);
    return;
  }
  const double scale = ldexp(1.0, fixed_scale_exponent(head, list_bits));
  const long long tx = llrint((double)c.x * scale), ty = llrint((double)c.y * scale), tz = llrint((double)c.z * scale);
  if ((tx | ty | tz) == 0) return;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    long long *a = acc + 4 * (size_t)iv[r];
    atomic_add_i64(a, tx);
    atomic_add_i64(a + 1, ty);
    atomic_add_i64(a + 2, tz);
  }
}

__global__ void __launch_bounds__(256)
vn_finish_kernel(const int V, const long long *__restrict__ acc, float *__restrict__ normals) {
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (size_t)V) return;
  const long long *a = acc + 4 * v;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (a[3] == 0 && (a[0] | a[1] | a[2]) != 0) {
    // (the common factor 2^-s drops out of the quotient: the accumulators as they are, below 2^62 each, their squares below 2^124)
    const double x = (double)a[0], y = (double)a[1], z = (double)a[2];
    const double n = sqrt((x * x + y * y) + z * z);
    nx = (float)(x / n); ny = (float)(y / n); nz = (float)(z / n);
  }
  normals[3 * v] = nx; normals[3 * v + 1] = ny; normals[3 * v + 2] = nz;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool mc_sizes_ok(const long V, const long F) { return V >= 0 && F >= 0 && V <= kMcMax && F <= kMcMax; }
static size_t vn_bytes(const long V) { return sizeof(FixedHead) + (size_t)V * 4 * sizeof(long long); }

}  // namespace voge

using namespace voge;

extern "C" int voge_mesh_components(const int32_t *faces, long F, long V, int32_t *parent, int32_t *vert_label, int32_t *face_label,
                                    int32_t *count, int32_t *meta, int stages, voge_stream_t stream) {
  if (!mc_sizes_ok(V, F) || !meta || (stages & ~7) || !stages) return VOGE_ERR_BAD_ARG;
  if ((F > 0 && (!faces || !face_label)) || (V > 0 && (!parent || !vert_label || !count))) return VOGE_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (stages & 1) hipLaunchKernelGGL(mc_init_kernel, dim3(blocks256(V > 4 ? V : 4)), dim3(256), 0, st, parent, count, (int)V, meta);
  if ((stages & 2) && F > 0) hipLaunchKernelGGL(mc_link_kernel, dim3(blocks256(F)), dim3(256), 0, st, faces, (int)F, (int)V, parent, meta);
  if ((stages & 4) && (V > 0 || F > 0))
    hipLaunchKernelGGL(mc_label_kernel, dim3(blocks256(V > F ? V : F)), dim3(256), 0, st, faces, (int)F, (int)V, parent, vert_label, face_label,
                       count, meta);
  return launch_status();
}

extern "C" int voge_mesh_clean_scan(const int32_t *faces, long F, long V, const int32_t *face_label, const uint8_t *keep_root,
                                    uint8_t *vflag, uint16_t *loc, uint32_t *blocks, int32_t *err, long long *totals, int stages,
                                    voge_stream_t stream) {
  if (!mc_sizes_ok(V, F) || V < 1 || F < 1 || (stages & ~15) || !stages) return VOGE_ERR_BAD_ARG;
  if (!faces || !face_label || !keep_root || !vflag || !loc || !blocks || !err || !totals) return VOGE_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long nbv = (V + kMcBlock - 1) / kMcBlock, nbf = (F + kMcBlock - 1) / kMcBlock;
  if (stages & 1) {
    hipError_t fe = voge_fill_async(vflag, 0, ((size_t)V + 3) & ~(size_t)3, st);      // (vflag holds V rounded up to 4 bytes)
    if (fe == hipSuccess) fe = voge_fill_async(err, 0, 4, st);
    if (fe != hipSuccess) return (int)fe;
  }
  if (stages & 2) hipLaunchKernelGGL(mc_mark_kernel, dim3(blocks256(F)), dim3(256), 0, st, faces, (int)F, (int)V, face_label, keep_root, vflag, err);
  if (stages & 4)
    hipLaunchKernelGGL(mc_local_scan_kernel, dim3((unsigned)(nbv + nbf)), dim3(kMcBlock), 0, st, (int)F, (int)V, face_label, keep_root, vflag,
                       (int)nbv, loc, blocks);
  if (stages & 8) hipLaunchKernelGGL(mc_top_scan_kernel, dim3(1), dim3(kMcTop), 0, st, blocks, nbv, nbf, err, totals);
  return launch_status();
}

extern "C" int voge_mesh_clean_emit(const float *verts, const int32_t *faces, long F, long V, const int32_t *face_label,
                                    const uint8_t *keep_root, const uint8_t *vflag, const uint16_t *loc, const uint32_t *blocks, long Vk,
                                    long Fk, float *verts_out, int32_t *faces_out, int32_t *vert_index, int32_t *face_index,
                                    voge_stream_t stream) {
  if (!mc_sizes_ok(V, F) || V < 1 || F < 1 || Vk < 0 || Fk < 0 || Vk > V || Fk > F) return VOGE_ERR_BAD_ARG;
  if (!verts || !faces || !face_label || !keep_root || !vflag || !loc || !blocks || (Vk > 0 && (!verts_out || !vert_index)) ||
      (Fk > 0 && (!faces_out || !face_index)))
    return VOGE_ERR_BAD_ARG;
  if (Vk == 0 && Fk == 0) return 0;
  const long nbv = (V + kMcBlock - 1) / kMcBlock;
  hipLaunchKernelGGL(mc_emit_kernel, dim3(blocks256(V > F ? V : F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (int)F, (int)V, face_label,
                     keep_root, vflag, loc, blocks, (int)nbv, Vk, Fk, verts_out, faces_out, vert_index, face_index);
  return launch_status();
}

extern "C" size_t voge_vertex_normals_workspace_bytes(long V) {
  if (V < 1 || V > kMcMax) return 0;
  return vn_bytes(V);
}

extern "C" int voge_vertex_normals(const float *verts, long V, const int32_t *faces, long F, float *normals, void *workspace,
                                   size_t workspace_bytes, int stages, voge_stream_t stream) {
  if (!mc_sizes_ok(V, F) || V < 1 || (stages & ~15) || !stages) return VOGE_ERR_BAD_ARG;
  if (!verts || !normals || (F > 0 && !faces) || bad_workspace(workspace)) return VOGE_ERR_BAD_ARG;
  if (workspace_bytes < vn_bytes(V)) return VOGE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  FixedHead *head = reinterpret_cast<FixedHead *>(workspace);
  long long *acc = reinterpret_cast<long long *>(static_cast<char *>(workspace) + sizeof(FixedHead));
  const int bits = ceil_log2(3 * F);      // 3 F <= 2^bits: the corners that can name one vertex
  if (stages & 1) {
    const hipError_t fe = voge_fill_async(workspace, 0, vn_bytes(V), st);
    if (fe != hipSuccess) return (int)fe;
  }
  if (F > 0) {
    if (stages & 2) hipLaunchKernelGGL(vn_absmax_kernel, dim3(blocks256_capped((size_t)F)), dim3(256), 0, st, verts, (int)V, faces, (int)F, head);
    if (stages & 4) hipLaunchKernelGGL(vn_scatter_kernel, dim3(blocks256(F)), dim3(256), 0, st, verts, (int)V, faces, (int)F, head, bits, acc);
  }
  if (stages & 8) hipLaunchKernelGGL(vn_finish_kernel, dim3(blocks256(V)), dim3(256), 0, st, (int)V, acc, normals);
  return launch_status();
}
