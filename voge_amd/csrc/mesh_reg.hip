// Mesh regularisers (EXTENSION: the reference takes them from PyTorch3D): the edge-length, uniform-Laplacian and normal-consistency
// terms of a vertex set [B][V][3] over ONE shared topology, the int32 tables of voge_amd/Losses.py MeshTopology:
//   edges [E][2] (i < j, sorted), nbr_off [V+1] / nbr [2E] (CSR adjacency), pairs [P][4] = (v0, v1, a, b), inc_off [V+1] / inc [4P]
//   (per vertex the entries pair * 4 + role it takes part in).
//   edge      (1 / BE) sum_b sum_e (|v_i - v_j| - t)^2                                   -- a zero length counts t^2, no gradient
//   laplacian (1 / BV) sum_b sum_i |L_i|,  L_i = (1 / d_i) sum_{j in N(i)} (v_j - v_i)   -- L_i == 0 (or d_i == 0): no gradient
//   normal    (1 / BP) sum_b sum_p (1 - n0 . n1 / (|n0| |n1|)),  n0 = (v1 - v0) x (a - v0),  n1 = -(v1 - v0) x (b - v0)
//                                                                -- a pair with a zero-area face counts 1, no gradient
// Every term works on DIFFERENCES of positions (exact, or one rounding of a small number), so a fine mesh far from the origin
// loses nothing to cancellation.  The edge term is fp32.  The Laplacian and the pairs widen the positions to fp64 BEFORE they
// difference them and stay there: a sliver face's normal and a small |L_i| amplify the rounding of an fp32 difference by
// 1 / sin(angle) and by edge / |L_i|, which the fan around a vertex of degree 300 turns into 1e-4 of the gradient; in fp64 both
// terms are the definition's to the last rounding of the result.  The items are bound by their gathers, not by this arithmetic.
// Forward: one launch over the E + V + P items of each mesh, one item a thread; a workgroup leaves three partial sums (a
// butterfly over the wave, the four waves in order), and a second launch of ONE workgroup adds the partials in fp64 in an order
// that depends on the shapes alone (thread t takes partials t, t + 256, ..; then a tree over the threads) and divides.  The
// vertex items also leave dir_i = L_i / (|L_i| d_i) for the backward.  Backward: one launch, one thread a vertex, a gather: its
// neighbours' edge terms, -d_i dir_i + sum_{j in N(i)} dir_j, and for every `inc` entry the pair's gradient recomputed for the
// vertex's own role; sums in fp64.  No atomics of any kind, nothing zero-filled: the same bits on every run.
#include "voge_common.h"

namespace voge {

enum { kMeshEdge = 1, kMeshLaplacian = 2, kMeshNormal = 4 };

struct MeshRegArgs {
  const float *verts;
  const int32_t *edges, *nbr_off, *nbr, *pairs, *inc_off, *inc;
  int B, V;
  int nE, nV, nP;      // the items of a mesh: E, V, P, each 0 where its term is off
  float t;
};

template <typename T>
struct Vec3 {
  T x, y, z;
};
typedef Vec3<float> V3;
typedef Vec3<double> D3;
__device__ __forceinline__ V3 mr_load(const float *__restrict__ v, const int i) {
  const float *p = v + 3 * (size_t)i;
  return V3{p[0], p[1], p[2]};
}
__device__ __forceinline__ D3 mr_wide(const V3 a) { return D3{(double)a.x, (double)a.y, (double)a.z}; }
template <typename T>
__device__ __forceinline__ Vec3<T> mr_sub(const Vec3<T> a, const Vec3<T> b) { return Vec3<T>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T>
__device__ __forceinline__ Vec3<T> mr_cross(const Vec3<T> a, const Vec3<T> b) {
  return Vec3<T>{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename T>
__device__ __forceinline__ T mr_dot(const Vec3<T> a, const Vec3<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the pair's two face normals (unnormalised), their lengths and the cosine, in fp64; false: a zero-area face
struct MeshPair {
  D3 e, p, q, n0, n1;
  double l0, l1, c;
};
struct MeshCorners {      // the pair's four positions as loaded: v0, v1, a, b
  V3 v0, v1, a, b;
};
__device__ __forceinline__ MeshCorners mr_corners(const float *__restrict__ v, const int4 row) {
  return MeshCorners{mr_load(v, row.x), mr_load(v, row.y), mr_load(v, row.z), mr_load(v, row.w)};
}
__device__ __forceinline__ bool mr_pair(const MeshCorners k, MeshPair &m) {
  const D3 v0 = mr_wide(k.v0);
  m.e = mr_sub(mr_wide(k.v1), v0);
  m.p = mr_sub(mr_wide(k.a), v0);
  m.q = mr_sub(mr_wide(k.b), v0);
  m.n0 = mr_cross(m.e, m.p);
  m.n1 = mr_cross(m.q, m.e);
  m.l0 = sqrt(mr_dot(m.n0, m.n0));
  m.l1 = sqrt(mr_dot(m.n1, m.n1));
  if (!(m.l0 > 0.0 && m.l1 > 0.0)) return false;
  m.c = mr_dot(m.n0, m.n1) / (m.l0 * m.l1);
  return true;
}

__global__ void __launch_bounds__(256)
mesh_reg_fwd_kernel(const MeshRegArgs a, const unsigned nblk, float *__restrict__ lap_dir, float *__restrict__ partial) {
  const unsigned b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  const long item = (long)blk * 256 + threadIdx.x;
  const float *v = a.verts + (size_t)b * a.V * 3;
  float se = 0.0f, sl = 0.0f, sn = 0.0f;
  if (item < a.nE) {
    const int2 ij = reinterpret_cast<const int2 *>(a.edges)[item];
    const V3 d = mr_sub(mr_load(v, ij.x), mr_load(v, ij.y));
    const float r = sqrtf(mr_dot(d, d)) - a.t;      // (a zero length: (0 - t)^2 = t^2)
    se = r * r;
  } else if (item < (long)a.nE + a.nV) {
    const int i = (int)(item - a.nE);
    const int o0 = a.nbr_off[i], o1 = a.nbr_off[i + 1];
    const D3 vi = mr_wide(mr_load(v, i));
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int o = o0; o < o1; ++o) {
      const D3 d = mr_sub(mr_wide(mr_load(v, a.nbr[o])), vi);
      sx += d.x; sy += d.y; sz += d.z;
    }
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    const double n2 = sx * sx + sy * sy + sz * sz;      // (|sum| = d_i |L_i|)
    if (n2 > 0.0) {
      const double n = sqrt(n2), deg = (double)(o1 - o0);
      sl = (float)(n / deg);
      ux = (float)(sx / (n * deg)); uy = (float)(sy / (n * deg)); uz = (float)(sz / (n * deg));
    }
    float *u = lap_dir + ((size_t)b * a.V + i) * 3;
    u[0] = ux; u[1] = uy; u[2] = uz;
  } else if (item < (long)a.nE + a.nV + a.nP) {
    MeshPair m;
    sn = mr_pair(mr_corners(v, reinterpret_cast<const int4 *>(a.pairs)[item - a.nE - a.nV]), m) ? (float)(1.0 - m.c) : 1.0f;
  }
  se = wave_sum(se); sl = wave_sum(sl); sn = wave_sum(sn);
  __shared__ float red[3][4];
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = se; red[1][w] = sl; red[2][w] = sn;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float *r = red[threadIdx.x];
    partial[(size_t)blockIdx.x * 3 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// out[k] = (sum of the n partials of term k) / count_k, 0 where count_k == 0.  One workgroup.
__global__ void __launch_bounds__(256)
mesh_reg_sum_kernel(const float *__restrict__ partial, const unsigned n, const double cE, const double cV, const double cP,
                    float *__restrict__ out) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4      // (the loads of four rounds in flight; the additions keep their order)
  for (unsigned i = threadIdx.x; i < n; i += 256) {
    const float *p = partial + (size_t)i * 3;
    s0 += (double)p[0]; s1 += (double)p[1]; s2 += (double)p[2];
  }
  __shared__ double red[3][256];
  red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    const double c = threadIdx.x == 0 ? cE : (threadIdx.x == 1 ? cV : cP);
    out[threadIdx.x] = c > 0.0 ? (float)(red[threadIdx.x][0] / c) : 0.0f;
  }
}

__global__ void __launch_bounds__(256)
mesh_reg_bwd_kernel(const MeshRegArgs a, const float *__restrict__ lap_dir, const float *__restrict__ g_edge,
                    const float *__restrict__ g_lap, const float *__restrict__ g_normal, const double cE, const double cV,
                    const double cP, float *__restrict__ g_verts) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= (size_t)a.B * a.V) return;
  const size_t b = r / (size_t)a.V;
  const int i = (int)(r - b * a.V);
  const float *v = a.verts + b * a.V * 3;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  if (a.nE | a.nV) {
    const double we = a.nE && g_edge ? 2.0 * (double)g_edge[0] / cE : 0.0;      // d (len - t)^2 = 2 (len - t) d len
    const double wl = a.nV && g_lap ? (double)g_lap[0] / cV : 0.0;
    const int o0 = a.nbr_off[i], o1 = a.nbr_off[i + 1];
    const V3 vi = mr_load(v, i);
    const float *dir = lap_dir + b * a.V * 3;
    double ex = 0.0, ey = 0.0, ez = 0.0, lx = 0.0, ly = 0.0, lz = 0.0;
    for (int o = o0; o < o1; ++o) {
      const int j = a.nbr[o];
      if (a.nE) {
        const V3 d = mr_sub(vi, mr_load(v, j));
        const float len = sqrtf(mr_dot(d, d));
        if (len > 0.0f) {
          const double k = (double)((len - a.t) / len);
          ex += k * (double)d.x; ey += k * (double)d.y; ez += k * (double)d.z;
        }
      }
      if (a.nV) {
        const V3 u = mr_load(dir, j);
        lx += (double)u.x; ly += (double)u.y; lz += (double)u.z;
      }
    }
    if (a.nV) {
      const V3 u = mr_load(dir, i);
      const double deg = (double)(o1 - o0);
      lx -= deg * (double)u.x; ly -= deg * (double)u.y; lz -= deg * (double)u.z;
    }
    gx = we * ex + wl * lx; gy = we * ey + wl * ly; gz = we * ez + wl * lz;
  }
  if (a.nP) {
    const double wn = g_normal ? (double)g_normal[0] / cP : 0.0;
    double px = 0.0, py = 0.0, pz = 0.0;
    const int o0 = a.inc_off[i], o1 = a.inc_off[i + 1];
    // an entry is a chain of three dependent loads (inc, the pair's row, its corners): the next entry's are requested before this
    // one's arithmetic, or a vertex of 24 entries waits for 72 round trips one after the other
    const int4 *rows = reinterpret_cast<const int4 *>(a.pairs);
    int ent_next = 0;
    MeshCorners next{};
    if (o0 < o1) {
      ent_next = a.inc[o0];
      next = mr_corners(v, rows[ent_next >> 2]);
    }
    for (int o = o0; o < o1; ++o) {
      const int role = ent_next & 3;
      const MeshCorners now = next;
      if (o + 1 < o1) {
        ent_next = a.inc[o + 1];
        next = mr_corners(v, rows[ent_next >> 2]);
      }
      MeshPair m;
      if (!mr_pair(now, m)) continue;
      // d (1 - c): g0 = -(n1 / |n1| - c n0 / |n0|) / |n0| on n0, g1 likewise on n1
      const double i0 = 1.0 / m.l0, i1 = 1.0 / m.l1;
      const D3 h0{m.n0.x * i0, m.n0.y * i0, m.n0.z * i0}, h1{m.n1.x * i1, m.n1.y * i1, m.n1.z * i1};
      const D3 g0{(m.c * h0.x - h1.x) * i0, (m.c * h0.y - h1.y) * i0, (m.c * h0.z - h1.z) * i0};
      const D3 g1{(m.c * h1.x - h0.x) * i1, (m.c * h1.y - h0.y) * i1, (m.c * h1.z - h0.z) * i1};
      // n0 = e x p, n1 = q x e:  g_e = p x g0 + g1 x q,  g_p = g0 x e,  g_q = e x g1;  v1, a, b carry e, p, q and v0 minus all
      const D3 t0 = mr_cross(m.p, g0), t1 = mr_cross(g1, m.q);
      const D3 ge{t0.x + t1.x, t0.y + t1.y, t0.z + t1.z}, gp = mr_cross(g0, m.e), gq = mr_cross(m.e, g1);
      D3 g;
      if (role == 0) g = D3{-(ge.x + gp.x + gq.x), -(ge.y + gp.y + gq.y), -(ge.z + gp.z + gq.z)};
      else g = role == 1 ? ge : (role == 2 ? gp : gq);
      px += g.x; py += g.y; pz += g.z;
    }
    gx += wn * px; gy += wn * py; gz += wn * pz;
  }
  float *g = g_verts + r * 3;
  g[0] = (float)gx; g[1] = (float)gy; g[2] = (float)gz;
}

// 1: nothing to do; 0: launch; < 0: the error
static int mesh_reg_check(const int B, const int V, const int E, const int P, const int terms) {
  if (B < 0 || V < 0 || E < 0 || P < 0 || (terms & ~7)) return VOGE_ERR_BAD_ARG;
  if (B == 0 || V == 0) return 1;
  if ((long)B * V * 3 > 2147483647l || E > 1073741823 || P > 536870911) return VOGE_ERR_BAD_ARG;      // (nbr holds 2E, inc entries 4P + 3)
  return 0;
}

static bool mesh_reg_aligned(const void *p, const uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

static long mesh_reg_blocks(const int V, const int E, const int P) { return ((long)E + V + P + 255) / 256; }

static MeshRegArgs mesh_reg_args(const float *verts, const int32_t *edges, const int32_t *nbr_off, const int32_t *nbr,
                                 const int32_t *pairs, const int32_t *inc_off, const int32_t *inc, const int B, const int V,
                                 const int E, const int P, const int terms, const float t) {
  return MeshRegArgs{verts, edges, nbr_off, nbr, pairs, inc_off, inc, B, V, (terms & kMeshEdge) ? E : 0,
                     (terms & kMeshLaplacian) ? V : 0, (terms & kMeshNormal) ? P : 0, t};
}

}  // namespace voge

using namespace voge;

extern "C" size_t voge_mesh_reg_workspace_bytes(int B, int V, int E, int P) {
  if (B <= 0 || V <= 0 || E < 0 || P < 0) return 0;
  return (size_t)B * (size_t)mesh_reg_blocks(V, E, P) * 3 * sizeof(float);
}

extern "C" int voge_mesh_reg_fwd(const float *verts, const int32_t *edges, const int32_t *nbr_off, const int32_t *nbr,
                                 const int32_t *pairs, int B, int V, int E, int P, int terms, float target_length, float *lap_dir,
                                 void *workspace, size_t workspace_bytes, float *out, voge_stream_t stream) {
  const int rc = mesh_reg_check(B, V, E, P, terms);
  if (rc != 0) return rc < 0 ? rc : 0;
  const MeshRegArgs a = mesh_reg_args(verts, edges, nbr_off, nbr, pairs, nullptr, nullptr, B, V, E, P, terms, target_length);
  if (!verts || !out || (a.nE && !edges) || (a.nV && !(nbr_off && nbr && lap_dir)) || (a.nP && !pairs)) return VOGE_ERR_BAD_ARG;
  if (!mesh_reg_aligned(edges, 8) || !mesh_reg_aligned(pairs, 16)) return VOGE_ERR_BAD_ARG;      // (rows are read whole)
  const long nblk = mesh_reg_blocks(a.nV, a.nE, a.nP), total = nblk * B;
  if (total > 2147483647l) return VOGE_ERR_BAD_ARG;
  if (total > 0 && (!workspace || workspace_bytes < (size_t)total * 3 * sizeof(float))) return VOGE_ERR_WORKSPACE;
  float *partial = static_cast<float *>(workspace);
  if (total > 0)
    hipLaunchKernelGGL(mesh_reg_fwd_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a, (unsigned)nblk, lap_dir,
                       partial);
  hipLaunchKernelGGL(mesh_reg_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, (unsigned)total,
                     (double)a.nE * B, (double)a.nV * B, (double)a.nP * B, out);
  return launch_status();
}

extern "C" int voge_mesh_reg_bwd(const float *verts, const int32_t *nbr_off, const int32_t *nbr, const int32_t *pairs,
                                 const int32_t *inc_off, const int32_t *inc, const float *lap_dir, const float *g_edge,
                                 const float *g_lap, const float *g_normal, int B, int V, int E, int P, int terms,
                                 float target_length, float *g_verts, voge_stream_t stream) {
  const int rc = mesh_reg_check(B, V, E, P, terms);
  if (rc != 0) return rc < 0 ? rc : 0;
  const MeshRegArgs a = mesh_reg_args(verts, nullptr, nbr_off, nbr, pairs, inc_off, inc, B, V, E, P, terms, target_length);
  if (!verts || !g_verts || ((a.nE || a.nV) && !(nbr_off && nbr)) || (a.nV && !lap_dir) || (a.nP && !(pairs && inc_off && inc)))
    return VOGE_ERR_BAD_ARG;
  if (!mesh_reg_aligned(pairs, 16)) return VOGE_ERR_BAD_ARG;
  const long rows = (long)B * V;
  hipLaunchKernelGGL(mesh_reg_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, lap_dir, g_edge,
                     g_lap, g_normal, (double)a.nE * B, (double)a.nV * B, (double)a.nP * B, g_verts);
  return launch_status();
}
