// Round 3's sweep, kept as an ORACLE: the kernel the product launched until round 5, cut down to the one form that still runs --
// a single wave on an 8x8-pixel tile, no instrumentation, no composite inside the epilogue.  It exists in -DVOGE_AB builds only
// (libvoge_hip_ab.so, never the product library: trace_fwd.hip includes this file under that macro), where a process-wide switch
// (voge_debug_sweep_variant) sends launch_trace here instead of to sweep_iso_kernel: tests/test_gpu_configs.py compares the two
// bit for bit, scalar-sigma and general forms, and tools/needle_scene_ab.py times one against the other.  What was removed, and how
// the removal was checked: HISTORY.md, "sweep_r3.h".
// (One input on which the two differ: a scalar form with a == 0.  This kernel evaluates it through pair_eval_iso -- a finite len and
//  act = 0, a hit --, sweep_iso_kernel stages it as never hit, as the reference's 0 / 0 has it: DESIGN.md section 3.)
//
// One workgroup = one wave = an 8x8 pixel tile, one ray per lane.  Its candidate stream is the tile's own sorted list (binB;
// pooled when long) or, if that overflowed, its quad's list, or else every Gaussian of the batch element, read in chunks of 64:
//   fill   : lane i takes stream entry base + i; an entry of the tile's own list was tested against the tile's cone by binB,
//            any other is tested here.  Survivors are compacted IN ORDER into LDS: (mu, a | NaN), id, len bound, and the full
//            eval record of an anisotropic one;
//   consume: for every staged candidate all 64 lanes evaluate their ray against it (record broadcast from LDS) and insert
//            into their LDS top-K list of 64-bit (ord(len) << 32 | id) keys;
//   exit   : once every lane holds K hits and the next candidate's len bound exceeds the wave's largest kept len, nothing
//            later in the (sorted) stream can enter.
// The cull and the exit test are conservative, so the result equals the brute-force sweep.  The epilogue re-maps lanes to
// (pixel, slot) so that the outputs are written as contiguous runs of K floats per pixel.
// (Included by trace_fwd.hip behind TraceWs, unpack_eval and trace_bin.h's lists, which it uses.)
#pragma once
#include <atomic>

#include "voge_common.h"

namespace voge {

static std::atomic<int> g_sweep_variant{0};      // 0: sweep_iso_kernel, 1: this file's kernel
static bool ab_round3_selected() { return g_sweep_variant.load(std::memory_order_relaxed) == 1; }

constexpr int kTrip = 4;   // candidates evaluated per trip of the sweep's inner loop
constexpr int kEpiU = 4;   // vec4 epilogue: items (4 slots of a pixel each) a thread takes through its stages together
constexpr int kR3TP = 65;  // key row stride: the transposed epilogue read stays conflict-light

template <bool ISO>
struct TraceLds {
  // layout inside dynamic LDS, after the [K + 1][65] key array.  ISO (the scalar-sigma entry points: every candidate is
  // isotropic) stages no full records.
  float4 ms[64];         // (mu, s00 | NaN): all an isotropic evaluation needs
  float4 ev[ISO ? 1 : 64 * 3];    // full eval record, staged for anisotropic candidates only
  int32_t id[64];        // candidate ids of the staged chunk; per-ray hit counts during the epilogue
  float lb[64];
};
__host__ __device__ constexpr size_t sweep_r3_key_bytes(const int K) { return (sizeof(uint64_t) * (size_t)(K + 1) * kR3TP + 15) & ~(size_t)15; }
template <bool ISO>
constexpr size_t sweep_r3_lds_bytes(const int K) { return sweep_r3_key_bytes(K) + ((sizeof(TraceLds<ISO>) + 15) & ~(size_t)15); }
static_assert(sweep_r3_lds_bytes<true>(VOGE_MAX_K) <= 160 * 1024 && sweep_r3_lds_bytes<false>(VOGE_MAX_K) <= 160 * 1024,
              "sweep_r3_kernel's LDS at VOGE_MAX_K");

template <bool ISO>
__global__ void __launch_bounds__(64)
sweep_r3_kernel(const float4 *__restrict__ cull, const float4 *__restrict__ evr, const float4 *__restrict__ ms,
                const float *__restrict__ rays, const int *__restrict__ bin_count, const int32_t *__restrict__ bin_id,
                const float *__restrict__ bin_lb, const int32_t *__restrict__ tl_id, const float *__restrict__ tl_lb,
                const int32_t *__restrict__ pool_id, const float *__restrict__ pool_lb, const int *__restrict__ tl_off,
                const int2 *__restrict__ order, const int tiles_per_img, const int nstx, const int nst, const int N, const int H,
                const int W, const int K, const float thr_act, int32_t *__restrict__ out_idx, float *__restrict__ out_len,
                float *__restrict__ out_act, float *__restrict__ out_dsd, int32_t *__restrict__ out_cnt) {
  constexpr int T = 64, TP = kR3TP, TW = 8, TH = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint64_t *keys = reinterpret_cast<uint64_t *>(smem_raw);
  TraceLds<ISO> &L = *reinterpret_cast<TraceLds<ISO> *>(smem_raw + sweep_r3_key_bytes(K));

  const int lane = threadIdx.x;
  const int tiles_x = (W + TW - 1) / TW;
  // Heavy tiles first: workgroup i takes slot i % 16 of the super-tile with launch rank i / 16 (binB: super-tiles by
  // descending candidate count, inside them quad by quad, a quad's tiles by descending list length).  The sweep lasts as long as its longest
  // tile, so that one must not start late; everything shorter fills in behind it.
  const int2 slot = order[blockIdx.x];               // (tile [| kPoolFlag], length of its list | -1 = overflowed)
  if (slot.x < 0 || slot.y == 0) return;             // outside the image | nothing can hit it: binB wrote its outputs
  const bool pooled = (slot.x & kPoolFlag) != 0;     // a long list (binB's long path): it lives in the pool
  const int lin = slot.x & ~kPoolFlag;
  const int b = lin / tiles_per_img, bx = lin - b * tiles_per_img;
  const int tx = bx % tiles_x, ty = bx / tiles_x;
  const int px = tx * TW + (lane & 7);
  const int py = ty * TH + (lane >> 3);
  const bool valid = (px < W) && (py < H);
  const int cpx = min(px, W - 1), cpy = min(py, H - 1);
  const size_t ray_id = ((size_t)b * H + cpy) * W + cpx;
  const float dx = rays[3 * ray_id + 0], dy = rays[3 * ray_id + 1], dz = rays[3 * ray_id + 2];
  const float qxx = dx * dx, qyy = dy * dy, qzz = dz * dz, qxy = dx * dy, qxz = dx * dz, qyz = dy * dz;

  // ---- the tile's bounding cone ------------------------------------------------------------
  const RayDir u = ray_dir(dx, dy, dz);
  const bool wave_dirs_ok = __all(u.ok);
  const bool unit_rays = __all(!u.ok || u.unit);
  const float wsx = wave_sum_dpp(u.ok ? u.ux : 0.f), wsy = wave_sum_dpp(u.ok ? u.uy : 0.f), wsz = wave_sum_dpp(u.ok ? u.uz : 0.f);
  Cone cone;
  {
    const float n = sqrtf(fmaf(wsz, wsz, fmaf(wsy, wsy, wsx * wsx)));
    const float ax = wsx / n, ay = wsy / n, az = wsz / n;
    float smax = 0.f, cmin = 1.f;
    cone_partial(u, ax, ay, az, smax, cmin);
    cone = cone_finish(ax, ay, az, n, wave_max(smax), wave_min(cmin), wave_dirs_ok);
  }

  // ---- candidate stream of this tile -----------------------------------------------------
  // tile list (bin2) -> super-tile list (bin) -> every Gaussian of the batch element
  const int tile = lin;
  // (fallback of an overflowed tile list: the ordered list of the tile's 16x16-pixel quad, which binB then spilled)
  const int bin = (b * nst + ((ty * TH) / kST) * nstx + (tx * TW) / kST) * 4 + (((ty * TH) / kQuad) & 1) * 2 + (((tx * TW) / kQuad) & 1);
  const int tc = slot.y;
  const int bc = (tc >= 0) ? tc : ((bin_count != nullptr) ? bin_count[bin] : -1);
  const bool binned = bc >= 0;
  const int src_n = binned ? bc : N;
  const size_t list_at = pooled ? (size_t)tl_off[tile] : (size_t)tile * kTileCap;
  const int32_t *src_id = (tc >= 0) ? (pooled ? pool_id : tl_id) + list_at : (binned ? bin_id + (size_t)bin * kQCap : nullptr);
  const float *src_lb = (tc >= 0) ? (pooled ? pool_lb : tl_lb) + list_at : (binned ? bin_lb + (size_t)bin * kQCap : nullptr);
  const float4 *cullb = cull + (size_t)b * N;
  const float4 *evrb = evr + (size_t)b * N * 3;
  const float4 cull_none = make_float4(0.f, 0.f, 0.f, -1.f);
  auto load_id = [&](int g) { return (g < src_n) ? (binned ? src_id[g] : g) : -1; };
  auto load_lb = [&](int g) { return (binned && g < src_n) ? src_lb[g] : -INFINITY; };
  auto load_rec = [&](int id) { return (id >= 0) ? cullb[id] : cull_none; };
  const float4 *msb = ms + (size_t)b * N;
  auto load_ms = [&](int id) { return (id >= 0) ? msb[id] : cull_none; };
  // the tile's own list was already filtered with this tile's cone (bin2): no second test
  const bool prefiltered = tc >= 0;

  uint64_t *mykeys = keys + lane;
  int cnt = 0;
  uint64_t worst = valid ? ((uint64_t)f2ord(VOGE_SENT_LEN) << 32) : 0ull, tail = 0ull;
  bool wdone = false;

  int base = 0;
  // two-deep software pipeline: ids two chunks ahead, cull / ms records one chunk ahead
  int id0 = load_id(lane);
  float lb0 = load_lb(lane);
  float4 c0r = prefiltered ? cull_none : load_rec(id0);
  float4 m0r = load_ms(id0);
  int id1 = load_id(T + lane);
  float lb1 = load_lb(T + lane);
  bool tile_gen = false;      // an anisotropic candidate was staged at some point (wave-uniform)
  // Barriers: one wave's LDS operations complete in order, but a lane reads what OTHER lanes staged, which the compiler only
  // orders across a barrier.  Two per chunk -- the staged chunk before its reads, those reads before the next chunk overwrites
  // it -- and one in front of the epilogue's hit counts.
  while (base < src_n) {
    bool chunk_iso = true;   // every staged candidate of this chunk is isotropic (wave-uniform)
    bool chunk_gen = !ISO;   // ... or every one is anisotropic
    // fill: one chunk of 64 stream entries
    int nbuf;
    {
      const int id = id0;
      const float lbv = lb0;
      const float4 c = c0r;
      const float4 mrec = m0r;
      id0 = id1; lb0 = lb1;
      c0r = prefiltered ? cull_none : load_rec(id0);
      m0r = load_ms(id0);
      id1 = load_id(base + 2 * T + lane);
      lb1 = load_lb(base + 2 * T + lane);
      const bool keep = prefiltered ? (id >= 0) : cone_keep(c, cone);
      const unsigned long long m = __ballot(keep);
      if (!ISO) {
        chunk_iso = chunk_iso && __all(!keep || (mrec.w == mrec.w));
        chunk_gen = chunk_gen && __all(!keep || !(mrec.w == mrec.w));
      }
      if (keep) {
        const int slot = __popcll(m & ((1ull << lane) - 1ull));
        L.ms[slot] = mrec;
        L.id[slot] = id;
        L.lb[slot] = lbv;
        if (!ISO && !(mrec.w == mrec.w)) {   // anisotropic: the full record (dependent gather, not prefetched)
          L.ev[slot * 3 + 0] = evrb[(size_t)id * 3 + 0];
          L.ev[slot * 3 + 1] = evrb[(size_t)id * 3 + 1];
          L.ev[slot * 3 + 2] = evrb[(size_t)id * 3 + 2];
        }
      }
      nbuf = __popcll(m);
      base += T;
    }
    tile_gen = tile_gen || !chunk_iso;
    __syncthreads();      // the staged chunk is in LDS before any lane reads it
    // consume: the chunk's survivors are the contiguous range [0, nbuf) -- one batch
    unsigned long long m = __ballot(lane < nbuf);
    // Exit test, once per chunk.  The bound is refreshed here only: a stale
    // (larger) bound merely delays the exit, because a lane's worst key only ever decreases.
    // The list bounds are monotone, so "first candidate past the bound" cuts the chunk.
    if (binned && unit_rays && __all(!valid || cnt == K)) {
      const float wmax = wave_max(valid ? ord2f((uint32_t)(worst >> 32)) : -INFINITY);
      const unsigned long long ex = __ballot(lane < nbuf && L.lb[lane] > wmax);
      if (ex) {
        m &= (1ull << __builtin_ctzll(ex)) - 1ull;
        wdone = true;      // (this chunk's candidates in front of the cut are still taken)
      }
    }
    // (gid = the candidate's global id, read from L.id by the caller: the fast loops fetch the ids of a
    // trip together with its records, so no LDS latency sits between two commits)
    auto commit = [&](const PairOut &o, const int gid, const bool on) {
      const uint64_t key = ((uint64_t)f2ord(o.len) << 32) | (uint32_t)gid;
      // (rays outside the image start with worst = 0, the others with the key of len = 1e10: `key < worst`
      // also says "a ray of the image" and "len below the sentinel")
      const bool take = on & (o.act < thr_act) & (key < worst);
      topk_commit<!ISO>(mykeys, TP, K, cnt, worst, tail, key, take);
    };
    if (chunk_iso) {
      // All-isotropic chunk (the common case): the candidates up to the exit cut are the contiguous
      // range [0, n) -- no bit scanning, no per-candidate isotropy test.
      const int s_end = __popcll(m);
      for (int s0 = 0; s0 < s_end; s0 += kTrip) {
        float4 cc[kTrip];
        int gid[kTrip];
        PairOut o[kTrip];
#pragma unroll
        for (int q = 0; q < kTrip; ++q) {
          cc[q] = L.ms[min(s0 + q, s_end - 1)];
          gid[q] = L.id[min(s0 + q, s_end - 1)] + b * N;
        }
#pragma unroll
        for (int q = 0; q < kTrip; ++q)
          o[q] = pair_eval_iso(cc[q].x, cc[q].y, cc[q].z, cc[q].w, dx, dy, dz, qxx, qyy, qzz);
        // The evaluations must finish as one block of four interleaved chains: without this
        // the compiler sinks each one behind its own commit's predicate and the wave (alone on
        // its SIMD) runs four dependent chains back to back.
#pragma unroll
        for (int q = 0; q < kTrip; ++q) asm volatile("" : "+v"(o[q].len), "+v"(o[q].act));
#pragma unroll
        for (int q = 0; q < kTrip; ++q) commit(o[q], gid[q], s0 + q < s_end);
      }
      m = 0ull;
    } else if (!ISO && chunk_gen) {
      // the same contiguous-range loop for an all-anisotropic chunk (full records from LDS)
      const int s_end = __popcll(m);
      for (int s0 = 0; s0 < s_end; s0 += kTrip) {
        PairOut o[kTrip];
        int gid[kTrip];
#pragma unroll
        for (int q = 0; q < kTrip; ++q) {
          const int sidx = min(s0 + q, s_end - 1);
          const float4 cc = L.ms[sidx];
          gid[q] = L.id[sidx] + b * N;
          o[q] = pair_eval_gen(cc.x, cc.y, cc.z, unpack_eval(L.ev[sidx * 3], L.ev[sidx * 3 + 1], L.ev[sidx * 3 + 2]), dx, dy,
                               dz, qxx, qyy, qzz, qxy, qxz, qyz);
        }
#pragma unroll
        for (int q = 0; q < kTrip; ++q) asm volatile("" : "+v"(o[q].len), "+v"(o[q].act));
#pragma unroll
        for (int q = 0; q < kTrip; ++q) commit(o[q], gid[q], s0 + q < s_end);
      }
      m = 0ull;
    }
    while (m) {
      // four candidates per trip: their evaluations are independent instruction streams
      int sq[kTrip];
      int nt = 0;
#pragma unroll
      for (int q = 0; q < kTrip; ++q) {
        sq[q] = m ? __builtin_ctzll(m) : 0;
        if (m) { ++nt; m &= m - 1ull; }
      }
      // The four evaluations form ONE straight-line block (the isotropic / general choice is
      // made per batch, on scalar registers), so the scheduler interleaves their chains.
      PairOut o[kTrip];
      float4 cc[kTrip], e0[kTrip];
      int gid[kTrip];
      bool iso = true, any_iso = false;
      bool fiso[kTrip];
#pragma unroll
      for (int q = 0; q < kTrip; ++q) {
        cc[q] = L.ms[sq[q]];
        gid[q] = L.id[sq[q]] + b * N;
        const bool f = fiso[q] = (__builtin_amdgcn_readfirstlane(__float_as_uint(cc[q].w)) & 0x7fffffffu) <= 0x7f800000u;
        iso = iso && f;
        any_iso = any_iso || f;
      }
      if (ISO || iso) {
#pragma unroll
        for (int q = 0; q < kTrip; ++q)
          o[q] = pair_eval_iso(cc[q].x, cc[q].y, cc[q].z, cc[q].w, dx, dy, dz, qxx, qyy, qzz);
      } else {
        float4 e1[kTrip], e2[kTrip];
#pragma unroll
        for (int q = 0; q < kTrip; ++q) {
          e0[q] = L.ev[sq[q] * 3]; e1[q] = L.ev[sq[q] * 3 + 1]; e2[q] = L.ev[sq[q] * 3 + 2];
        }
        if (!any_iso) {
#pragma unroll
          for (int q = 0; q < kTrip; ++q)
            o[q] = pair_eval_gen(cc[q].x, cc[q].y, cc[q].z, unpack_eval(e0[q], e1[q], e2[q]), dx, dy, dz, qxx, qyy,
                                 qzz, qxy, qxz, qyz);
        } else {  // mixed batch: per-candidate dispatch (same arithmetic, just not interleaved)
#pragma unroll
          for (int q = 0; q < kTrip; ++q) {
            if (fiso[q])   // uniform: the flag came through readfirstlane
              o[q] = pair_eval_iso(cc[q].x, cc[q].y, cc[q].z, cc[q].w, dx, dy, dz, qxx, qyy, qzz);
            else
              o[q] = pair_eval_gen(cc[q].x, cc[q].y, cc[q].z, unpack_eval(e0[q], e1[q], e2[q]), dx, dy, dz, qxx, qyy,
                                   qzz, qxy, qxz, qyz);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kTrip; ++q) commit(o[q], gid[q], q < nt);
    }
    __syncthreads();      // every lane's reads of the chunk are over before the next one is staged
    if (wdone) break;
  }

  // ---- epilogue: lanes re-mapped to (pixel, slot); act / dsd recomputed with pair_eval ------
  L.id[lane] = cnt;           // (the staged ids are done with: the array now holds the hit counts)
  if (out_cnt != nullptr && valid) out_cnt[((size_t)b * H + py) * W + px] = cnt;
  __syncthreads();            // the hit counts are in LDS before the re-mapped lanes read them
  const int tw = min(TW, W - tx * TW);
  const int row_items = tw * K;
  auto slot_value = [&](const int r, const int x, const int s, const size_t pix, int32_t &oi, float &ol, float &oa,
                        float &od) {
    const int owner = 8 * r + x;      // the lane that swept pixel (x, r) of the tile
    oi = -1; ol = VOGE_SENT_LEN; oa = VOGE_SENT_ACT; od = 0.0f;
    if (s < L.id[owner]) {
      const uint64_t key = keys[(size_t)s * TP + owner];
      oi = (int32_t)(uint32_t)key;
      const float *ry = rays + pix * 3;
      const float ex = ry[0], ey = ry[1], ez = ry[2];
      const float4 cc = ms[oi];      // (centre, a | NaN): an isotropic Gaussian needs nothing else
      PairOut o;
      if (ISO || cc.w == cc.w) {
        o = pair_eval_iso(cc.x, cc.y, cc.z, cc.w, ex, ey, ez, ex * ex, ey * ey, ez * ez);
      } else {
        const EvalRec e = unpack_eval(evr[(size_t)oi * 3 + 0], evr[(size_t)oi * 3 + 1], evr[(size_t)oi * 3 + 2]);
        o = pair_eval(cc.x, cc.y, cc.z, e, ex, ey, ez, ex * ex, ey * ey, ez * ez, ex * ey, ex * ez, ey * ez);
      }
      ol = ord2f((uint32_t)(key >> 32));
      oa = o.act;
      od = o.dsd;
    }
  };
  const bool vec4 = ((K & 3) == 0);   // rows of K floats stay 16-byte aligned: 16-byte stores
  if (vec4) {
    // All rows of the tile as one item space; an item = 4 consecutive slots of one pixel.  kEpiU
    // items per thread go through the stages together -- LDS keys, then one 16-byte gather per
    // slot (isotropic Gaussians need nothing more), then arithmetic and the 16-byte stores -- so
    // a thread has up to 4 * kEpiU gathers in flight instead of one dependent chain per slot.
    const int th = min(TH, H - ty * TH);
    const int ipr = row_items >> 2;
    const int nitem = th * ipr;
    const float inv_ipr = 1.0f / (float)ipr, invK = 1.0f / (float)K;
    // Tiles that staged anisotropic candidates: centre and full record (4 gathers per slot) are issued
    // together for kEpiG items -- one round trip per round instead of "centre, then 3 more per slot".
    // (pair_eval dispatches on the record, so an isotropic entry in such a tile is still exact.)
    constexpr int kEpiG = 2;
    const bool want_ad = out_act != nullptr;
    for (int it0 = lane; tile_gen && want_ad && it0 < nitem; it0 += T * kEpiG) {
      uint64_t key[kEpiG][4];
      float4 rc[kEpiG][4], g0[kEpiG][4], g1[kEpiG][4], g2[kEpiG][4];
      float ex[kEpiG], ey[kEpiG], ez[kEpiG];
      size_t ob[kEpiG];
      int nv[kEpiG];
#pragma unroll
      for (int u = 0; u < kEpiG; ++u) {
        const int it = it0 + u * T;
        nv[u] = -1;
        ob[u] = 0;
        ex[u] = ey[u] = ez[u] = 0.0f;
        if (it < nitem) {
          const int r = __float2int_rz(((float)it + 0.5f) * inv_ipr);
          const int j = (it - r * ipr) * 4;
          const int x = __float2int_rz(((float)j + 0.5f) * invK);
          const int sl = j - x * K;
          const int owner = 8 * r + x;      // the lane that swept pixel (x, r) of the tile
          const size_t pix = ((size_t)b * H + ty * TH + r) * W + (size_t)tx * TW + x;
          ob[u] = pix * K + sl;
          nv[u] = max(0, min(4, L.id[owner] - sl));
#pragma unroll
          for (int q = 0; q < 4; ++q) key[u][q] = (q < nv[u]) ? keys[(size_t)(sl + q) * TP + owner] : 0ull;
          if (nv[u] > 0) { ex[u] = rays[pix * 3]; ey[u] = rays[pix * 3 + 1]; ez[u] = rays[pix * 3 + 2]; }
        }
      }
#pragma unroll
      for (int u = 0; u < kEpiG; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rc[u][q] = g0[u][q] = g1[u][q] = g2[u][q] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (q < nv[u]) {
            const size_t gi = (uint32_t)key[u][q];
            rc[u][q] = ms[gi]; g0[u][q] = evr[gi * 3]; g1[u][q] = evr[gi * 3 + 1]; g2[u][q] = evr[gi * 3 + 2];
          }
        }
#pragma unroll
      for (int u = 0; u < kEpiG; ++u) {
        if (nv[u] < 0) continue;
        int32_t oi[4];
        float ol[4], oa[4], od[4];
        const float qxx = ex[u] * ex[u], qyy = ey[u] * ey[u], qzz = ez[u] * ez[u];
        const float qxy = ex[u] * ey[u], qxz = ex[u] * ez[u], qyz = ey[u] * ez[u];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          oi[q] = -1; ol[q] = VOGE_SENT_LEN; oa[q] = VOGE_SENT_ACT; od[q] = 0.0f;
          if (q < nv[u]) {
            oi[q] = (int32_t)(uint32_t)key[u][q];
            ol[q] = ord2f((uint32_t)(key[u][q] >> 32));
            const PairOut o = pair_eval(rc[u][q].x, rc[u][q].y, rc[u][q].z, unpack_eval(g0[u][q], g1[u][q], g2[u][q]),
                                        ex[u], ey[u], ez[u], qxx, qyy, qzz, qxy, qxz, qyz);
            oa[q] = o.act;
            od[q] = o.dsd;
          }
        }
        st16i<true>(out_idx + ob[u], oi[0], oi[1], oi[2], oi[3]);      // (write-once, 16 B per slot: non-temporal, voge_common.h)
        st16f<true>(out_len + ob[u], ol[0], ol[1], ol[2], ol[3]);
        st16f<true>(out_act + ob[u], oa[0], oa[1], oa[2], oa[3]);
        st16f<true>(out_dsd + ob[u], od[0], od[1], od[2], od[3]);
      }
    }
    // Fragment mode without act / dsd (out_act == NULL; voge_fragments_fwd_iso*): index and len are the key itself --
    // no gather, no ray, no arithmetic; the composite kernel behind the sweep derives act / dsd from the same
    // records with the same operations (composite.hip), at its own, much higher residency.
    for (int it0 = lane; !want_ad && it0 < nitem; it0 += T * kEpiU) {
#pragma unroll
      for (int u = 0; u < kEpiU; ++u) {
        const int it = it0 + u * T;
        if (it >= nitem) break;
        const int r = __float2int_rz(((float)it + 0.5f) * inv_ipr);
        const int j = (it - r * ipr) * 4;
        const int x = __float2int_rz(((float)j + 0.5f) * invK);
        const int sl = j - x * K;
        const int owner = 8 * r + x;      // the lane that swept pixel (x, r) of the tile
        const size_t pix = ((size_t)b * H + ty * TH + r) * W + (size_t)tx * TW + x;
        const int nv = max(0, min(4, L.id[owner] - sl));
        int32_t oi[4];
        float ol[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint64_t key = (q < nv) ? keys[(size_t)(sl + q) * TP + owner] : 0ull;
          oi[q] = (q < nv) ? (int32_t)(uint32_t)key : -1;
          ol[q] = (q < nv) ? ord2f((uint32_t)(key >> 32)) : VOGE_SENT_LEN;
        }
        *reinterpret_cast<int4 *>(out_idx + pix * K + sl) = make_int4(oi[0], oi[1], oi[2], oi[3]);
        *reinterpret_cast<float4 *>(out_len + pix * K + sl) = make_float4(ol[0], ol[1], ol[2], ol[3]);
      }
    }
    for (int it0 = lane; !tile_gen && want_ad && it0 < nitem; it0 += T * kEpiU) {
      uint64_t key[kEpiU][4];
      float4 rec[kEpiU][4];
      float ex[kEpiU], ey[kEpiU], ez[kEpiU];
      size_t ob[kEpiU];
      int nv[kEpiU];
#pragma unroll
      for (int u = 0; u < kEpiU; ++u) {
        const int it = it0 + u * T;
        nv[u] = -1;
        ob[u] = 0;
        ex[u] = ey[u] = ez[u] = 0.0f;
        if (it < nitem) {
          const int r = __float2int_rz(((float)it + 0.5f) * inv_ipr);
          const int j = (it - r * ipr) * 4;
          const int x = __float2int_rz(((float)j + 0.5f) * invK);
          const int sl = j - x * K;
          const int owner = 8 * r + x;      // the lane that swept pixel (x, r) of the tile
          const size_t pix = ((size_t)b * H + ty * TH + r) * W + (size_t)tx * TW + x;
          ob[u] = pix * K + sl;
          nv[u] = max(0, min(4, L.id[owner] - sl));
#pragma unroll
          for (int q = 0; q < 4; ++q) key[u][q] = (q < nv[u]) ? keys[(size_t)(sl + q) * TP + owner] : 0ull;
          if (nv[u] > 0) { ex[u] = rays[pix * 3]; ey[u] = rays[pix * 3 + 1]; ez[u] = rays[pix * 3 + 2]; }
        }
      }
#pragma unroll
      for (int u = 0; u < kEpiU; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          rec[u][q] = (q < nv[u]) ? ms[(uint32_t)key[u][q]] : make_float4(0.f, 0.f, 0.f, 0.f);
      // anisotropic entries (w = NaN) need their full record: 3 more gathers each.  They are issued for
      // all four slots of an item before any is used (12 in flight per lane instead of 3).
      bool gen_any = false;
#pragma unroll
      for (int u = 0; u < kEpiU; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) gen_any = gen_any || ((q < nv[u]) && !(rec[u][q].w == rec[u][q].w));
      gen_any = __any(gen_any);
#pragma unroll
      for (int u = 0; u < kEpiU; ++u) {
        if (nv[u] < 0) continue;
        int32_t oi[4];
        float ol[4], oa[4], od[4];
        const float qxx = ex[u] * ex[u], qyy = ey[u] * ey[u], qzz = ez[u] * ez[u];
        float4 g0[4], g1[4], g2[4];
        if (gen_any) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            g0[q] = g1[q] = g2[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((q < nv[u]) && !(rec[u][q].w == rec[u][q].w)) {
              const size_t eo = (size_t)(uint32_t)key[u][q] * 3;
              g0[q] = evr[eo]; g1[q] = evr[eo + 1]; g2[q] = evr[eo + 2];
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          oi[q] = -1; ol[q] = VOGE_SENT_LEN; oa[q] = VOGE_SENT_ACT; od[q] = 0.0f;
          if (q < nv[u]) {
            oi[q] = (int32_t)(uint32_t)key[u][q];
            ol[q] = ord2f((uint32_t)(key[u][q] >> 32));
            PairOut o;
            if (rec[u][q].w == rec[u][q].w) {
              o = pair_eval_iso_at(rec[u][q].x, rec[u][q].y, rec[u][q].z, rec[u][q].w, ol[q], ex[u], ey[u], ez[u],
                                   (qxx + qyy) + qzz);     // len is in the key: no second division
            } else {
              const EvalRec e = unpack_eval(g0[q], g1[q], g2[q]);
              o = pair_eval(rec[u][q].x, rec[u][q].y, rec[u][q].z, e, ex[u], ey[u], ez[u], qxx, qyy, qzz, ex[u] * ey[u],
                            ex[u] * ez[u], ey[u] * ez[u]);
            }
            oa[q] = o.act;
            od[q] = o.dsd;
          }
        }
        st16i<true>(out_idx + ob[u], oi[0], oi[1], oi[2], oi[3]);      // (write-once, 16 B per slot: non-temporal, voge_common.h)
        st16f<true>(out_len + ob[u], ol[0], ol[1], ol[2], ol[3]);
        st16f<true>(out_act + ob[u], oa[0], oa[1], oa[2], oa[3]);
        st16f<true>(out_dsd + ob[u], od[0], od[1], od[2], od[3]);
      }
    }
  }
  if (!vec4 && out_act == nullptr) {
    // K not a multiple of four, fragments without act / dsd (ShapeFitting's max_assign = 25): index and len are the keys
    // themselves -- every slot of the tile is one independent LDS read and two 4-byte stores, no gather, no arithmetic
    const int th = min(TH, H - ty * TH);
    const float inv_ri = 1.0f / (float)row_items;
    for (int it = lane; it < th * row_items; it += T) {
      const int r = __float2int_rz(((float)it + 0.5f) * inv_ri);
      const int j = it - r * row_items;
      const int x = j / K, sl = j - x * K;
      const int owner = 8 * r + x;      // the lane that swept pixel (x, r) of the tile
      const bool in = sl < L.id[owner];
      const uint64_t key = in ? keys[(size_t)sl * TP + owner] : 0ull;
      const size_t o = (((size_t)b * H + ty * TH + r) * W + (size_t)tx * TW) * K + j;
      out_idx[o] = in ? (int32_t)(uint32_t)key : -1;
      out_len[o] = in ? ord2f((uint32_t)(key >> 32)) : VOGE_SENT_LEN;
    }
  }
  if (!vec4 && out_act != nullptr) {
    // K not a multiple of four, act / dsd wanted: one slot per lane and trip over the whole tile (rows x pixels x slots
    // flattened, so a wave makes th * tw * K / 64 trips instead of th * ceil(tw * K / 64)), four trips in flight
    const int th = min(TH, H - ty * TH);
    const float inv_ri = 1.0f / (float)row_items;
    const int nit = th * row_items;
    for (int it0 = lane; it0 < nit; it0 += 4 * T) {
      int32_t oi[4];
      float ol[4], oa[4], od[4];
      size_t oo[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int it = it0 + u * T;
        oo[u] = 0; oi[u] = -1; ol[u] = VOGE_SENT_LEN; oa[u] = VOGE_SENT_ACT; od[u] = 0.0f;
        if (it < nit) {
          const int r = __float2int_rz(((float)it + 0.5f) * inv_ri);
          const int j = it - r * row_items;
          const int x = j / K, sl = j - x * K;
          const size_t pix = ((size_t)b * H + ty * TH + r) * W + (size_t)tx * TW + x;
          slot_value(r, x, sl, pix, oi[u], ol[u], oa[u], od[u]);
          oo[u] = pix * K + sl;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (it0 + u * T < nit) { out_idx[oo[u]] = oi[u]; out_len[oo[u]] = ol[u]; out_act[oo[u]] = oa[u]; out_dsd[oo[u]] = od[u]; }
      }
    }
  }
}

// What launch_trace does in place of its sweep_iso_kernel launch while the switch says 1 (binB has run: same lists, same order)
template <bool ISO>
static int launch_sweep_r3(const TraceWs &ws, const float *rays, const dim3 grid, int N, int H, int W, int K, float thr_act, int32_t *idx,
                           float *len, float *act, float *dsd, int32_t *cnt, hipStream_t st, const CamView &cam) {
  if (cam.R != nullptr) return VOGE_ERR_BAD_ARG;      // (round 3's sweep reads the ray bundle: no camera form)
  const size_t lds = sweep_r3_lds_bytes<ISO>(K);
  static DynLdsCache cache;
  const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(sweep_r3_kernel<ISO>), lds, cache);
  if (rc) return rc;
  hipLaunchKernelGGL(sweep_r3_kernel<ISO>, grid, dim3(64), lds, st, ws.cull, ws.evr, ws.ms, rays, ws.q_count, ws.q_id, ws.q_lb, ws.tl_id,
                     ws.tl_lb, ws.pool_id, ws.pool_lb, ws.tl_off, ws.order, ((W + 7) / 8) * ((H + 7) / 8), ws.nstx, ws.nstx * ws.nsty, N, H,
                     W, K, thr_act, idx, len, act, dsd, cnt);
  return launch_status();
}

}  // namespace voge

// the process-wide switch (tests/test_gpu_configs.py, tools/needle_scene_ab.py, tools/stress_render_case.py)
extern "C" int voge_debug_sweep_variant(int variant) {
  if (variant < 0 || variant > 1) return VOGE_ERR_BAD_ARG;
  voge::g_sweep_variant.store(variant, std::memory_order_relaxed);
  return 0;
}
