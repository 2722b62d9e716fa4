// Fused backward of the fragment pipeline for gfx950: shade (merge + silhouette + blend) -> composite -> fine trace,
// ONE pass over the fragments.
//
// Reference behaviour being reproduced (all by autograd there):
//   VoGE/Renderer.py:157-171 (get_silhouette, to_colored_background) and VoGE/Aggregation.py:111-141 (merge_final),
//   VoGE/Aggregation.py:30-107 (aggregation), VoGE/csrc/ray_trace_voge/ray_trace_voge.cu:283-332 (trace backward),
// for the renderer's common case: isotropic Gaussians (one scalar each), <= 4 colour channels, fixed cameras.
//
// The three stand-alone backward kernels (voge_shade_bwd, voge_composite_bwd, voge_trace_bwd_iso) exchange g_weight
// and g_len / g_act / g_dsd through memory (336 MB at cfg3), each reads the index lists again, and two of them build a
// per-Gaussian accumulation table of their own.  Here a lane owns two consecutive slots of a pixel (the composite
// backward's layout, composite_core.h); for them it
//   1. gathers the slots' colours:       g_w[k] = <g_rgb, colour[idx_k]> + g_sum_w          (shade backward)
//   2. runs the composite's closed-form backward on u = g_w * w:  g_act, g_len, g_dsd        (registers)
//   3. gathers the slots' (mu, a) and forms the trace's per-slot terms for g_mu (3) and g_a  (trace backward)
//   4. adds (g_mu, g_a | w g_rgb) -- EIGHT sums -- to ONE wave-private LDS table entry per Gaussian,
// and the table is flushed with lane-coalesced atomics into acc[P][8].  A finishing pass turns acc into the
// gradients of what the caller passed in (verts / sigmas through the view's chain rule, colours).
// Everything a stage hands to the next stays in registers; by linearity in g_weight, gradients reaching the weights
// from other consumers (e.g. a silhouette loss) still take the stand-alone kernels and simply add up.
#include "composite_core.h"

namespace voge {

#ifndef VOGE_FB_NE
#define VOGE_FB_NE 128
#endif
constexpr int kFbNE = VOGE_FB_NE;  // table entries per wave (four slots per lane: WaveTable, one array of keys and values)
// Two slots per lane: WaveDirTable (voge_common.h) -- a directory of kFbND keys probed by double hashing over kFbNEV dense value
// entries.  A 4x3 group holds 45 distinct Gaussians on average and 81 at most at cfg3, 71 at most at cfg4 (the whole frames:
// tools/table_probe_sim.py --gpu, profiles/r13_fb_table.txt); a group with more takes the straight-to-memory path for the
// keys that come late.  96 entries + 256 keys keep every instantiation's LDS at or under what the 128-slot table took (as many
// workgroups per CU by LDS as before, or more).  The frame's own kernel -- scalar sigmas, three colour channels through the
// shade stage -- takes 512 keys: 1.5-2 us faster at cfg3 (2.0 loop iterations per round instead of 2.5), 9552 bytes, 17
// workgroups per CU by LDS where its registers allow 16.
#ifndef VOGE_FB_ND
#define VOGE_FB_ND 256
#endif
#ifndef VOGE_FB_ND_FRAME
#define VOGE_FB_ND_FRAME 512
#endif
#ifndef VOGE_FB_NEV
#define VOGE_FB_NEV 96
#endif
constexpr int kFbND = VOGE_FB_ND, kFbNDFrame = VOGE_FB_ND_FRAME, kFbNEV = VOGE_FB_NEV;
// A wave's group of pixels: GW x GH (<= 64 pixels; lane g of the wave holds pixel (g % GW, g / GW)'s hit count).  The
// lanes are handed out by those counts (composite_core.h, "Lane packing by hit count"): ceil(count / 2) lanes per
// pixel, as many consecutive pixels per round as fit the wave.
#ifndef VOGE_FB_GW
#define VOGE_FB_GW 4
#endif
#ifndef VOGE_FB_GH
#define VOGE_FB_GH 3
#endif
constexpr int kFbGW = VOGE_FB_GW, kFbGH = VOGE_FB_GH, kFbG = kFbGW * kFbGH;
static_assert(kFbG <= 64 && (kFbGW & (kFbGW - 1)) == 0, "a group's pixels are the lanes of one wave; GW a power of two");
// -DVOGE_FB_TIMES: per-section cycle counters of the fused backward (tools/fb_sections.py).  Sections: 0 set-up + lane
// packing, 1 streams + gathers + shade terms, 2 LDS rows + composite backward, 3 trace terms, 4 table, 5 flush.
#ifdef VOGE_FB_TIMES
constexpr int kFbTimesWaves = 1 << 16;
__device__ unsigned long long g_fb_times[kFbTimesWaves][8];      // one row per workgroup (plain stores: no same-address atomics)
__device__ unsigned long long g_fb_tab[kFbTimesWaves][4];       // accumulations (wave-wide calls), their election rounds, lanes taking part
__device__ unsigned long long g_fb_wall[kFbTimesWaves][2];       // its first and last stamp (s_memrealtime, 100 MHz): tools/fb_wall.py
#define FB_T0() const unsigned long long fb_w0_ = __builtin_amdgcn_s_memrealtime(); unsigned long long fb_t_ = __builtin_readcyclecounter(), fb_acc_[6] = {0, 0, 0, 0, 0, 0}
#define FB_TICK(i) do { const unsigned long long n_ = __builtin_readcyclecounter(); fb_acc_[i] += n_ - fb_t_; fb_t_ = n_; } while (0)
#define FB_TOUT() do { if (threadIdx.x == 0 && blockIdx.x < kFbTimesWaves) { for (int i_ = 0; i_ < 6; ++i_) g_fb_times[blockIdx.x][i_] = fb_acc_[i_]; g_fb_times[blockIdx.x][6] = 1ull; g_fb_wall[blockIdx.x][0] = fb_w0_; g_fb_wall[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define FB_T0() do {} while (0)
#define FB_TICK(i) do {} while (0)
#define FB_TOUT() do {} while (0)
#endif

template <int NV4, int NS, int ND>
struct FragBwdLds {
  // key = Gaussian index; values: (g_mu, g_a), (w g_rgb, -) for A = a I [NV4 = 2];
  //                               (g_mu, g_A[0]), g_A[1..4], g_A[5..8], (w g_rgb, -) for a full 3x3 A [NV4 = 4];
  //                               without the colour term (SRC = 1): NV4 = 1 | 3
  static constexpr int kRows = NS * 64 + 4 * kFbG;      // a round's padded rows: 64 lanes' slots + two sentinel pairs per pixel
  std::conditional_t<NS == 2, WaveDirTable<ND, kFbNEV, NV4>, WaveTable<kFbNE, NV4>> tab;
  float len[kRows], sp[kRows], E[kRows], u[kRows];
  float r[kRows];                 // row sums of the composite backward, accumulated by the column walks (compn_bwd_wave)
};

#ifndef VOGE_FB_ABL
#define VOGE_FB_ABL 0
#endif
#ifndef VOGE_FB_WPE
#define VOGE_FB_WPE 4      // capping the registers for 5 / 6 waves per SIMD spills and is slower
#endif
// SRC: where the gradient of the weights comes from.
//   0: the shade stage is part of the pass (colours, rgb, wsum, bg, g_img given): g_w = <g_rgb, colour> + g_sum_w, and the
//      colours' own gradient w g_rgb rides in the table (C: colour channels, 1..4);
//   1: g_weight [pix][K] is given by whoever consumed the weights (merge_final, get_silhouette, any torch expression),
//      element (p, k) at g_weight[p * gw_stride_pix + k * gw_stride_k] (K, 1 contiguous; (1, 0) for a per-pixel value
//      broadcast over the slots, which is what a silhouette loss alone produces), plus the gradient of vert_hit_length
//      (g_hitlen, contiguous or NULL) added to the trace's g_len; C = 0, no colour term.
//   2: the DEPTH form (voge_frame_depth_bwd_iso; C = 0, no colour term, the weights-driven form's table): the gradient of the
//      weights is g_w[k] = a len_k + b with two per-pixel scalars, formed here from operands the other forms do not use in this
//      combination -- `rgb` = the forward's depth [pix], `wsum` = its weight sums [pix], g_img = the depth's gradient (element p at
//      g_img[p * gs_pix]; NULL: none), `bg` = the SILHOUETTE's gradient [pix] | NULL, thr > 0: the normalised depth
//      (a = g_D / S, b = -a D where S > 0) else the plain sum (a = g_D, b = 0); the silhouette's pass-through adds to b, and
//      a w_k is added to the trace's g_len.  No kernel argument of its own.
// NS: slots per lane (2; 4 for lists of more than 128 slots, so that a pixel's lanes still fit one wave).
// OffT: uint32_t when every BYTE offset the kernel forms in it fits 32 bits -- into the [pix][K] arrays (4 K bytes per pixel),
// the rays (12), the shade form's rgb (4 C) and the per-pixel scalars (4): fb_launch's test -- (the loads then take scalar base +
// 32-bit lane offset and the address arithmetic leaves the vector unit), else size_t.
// ISO: every Gaussian is A = a I (rec = [P] (mu, a)); otherwise rec = [P][3] packed (mu, A) as in trace_bwd.hip.
// NOAD: the forward kept no act / dsd (voge_fragments_fwd_iso* with act = dsd = NULL, voge_trace_lean_fwd); they are re-derived
// from the records, the ray and len with the forward's own operations (pair_eval_iso_at / pair_eval): 8 bytes per slot less to read.
// K need not be a multiple of NS: `vec` (uniform) says whether a lane's group is aligned and inside its pixel's row
// (wide loads) or is read slot by slot.
// DIAG (round 6; !ISO, NOAD): rec = [P][2] compact per-axis records (mu, a0 | a1, a2, 0, 0) of voge_frame_trace_fwd_gen (kind 1):
// em / sm from pair_eval_diag, the trace terms of the diagonal alone (the general terms' bits on such a form: their other
// coefficients multiply zeros), table entries of 12 | 8 floats instead of 16 | 12 -- (g_mu, g_A00), (g_A11, g_A22, w g_rgb ...).
template <int SRC, int C, int NS, typename OffT, bool ISO, bool NOAD, bool DIAG = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NS == 4 ? 2 : (ISO ? VOGE_FB_WPE : 3))))
fragment_bwd_kernel(const float4 *__restrict__ rec, const float *__restrict__ rays,
                        const float *__restrict__ colors, const int32_t *__restrict__ idx, const int32_t *__restrict__ cnt,
                        const float *__restrict__ weight, const float *__restrict__ act, const float *__restrict__ len,
                        const float *__restrict__ dsd, const float *__restrict__ rgb, const float *__restrict__ wsum,
                        const float *__restrict__ bg, const float thr, const float *__restrict__ g_img, const long gs_pix,
                        const long gs_c, const float *__restrict__ g_hitlen, const float occ,
                        const int P, const long nrows, const int W, const int K, const long Nattr,
                        float *__restrict__ acc /* [P][NACC], zeroed */) {
  static_assert(NS == 2 || NS == 4, "a lane owns one or two aligned pairs of slots");
  static_assert(!DIAG || (!ISO && NOAD && C <= 4), "the per-axis form keeps no act / dsd");
  constexpr int NV4 = SRC == 0 ? (ISO ? 2 : (DIAG ? 3 : 4)) : (ISO ? 1 : (DIAG ? 2 : 3)), NACC = 4 * NV4;
  constexpr int NRC = ISO ? 1 : (DIAG ? 2 : 3);      // float4s per record
  // sum c (0 .. NACC - 1) of Gaussian `key`.  (Round 6 tried adding the table straight into the caller's gradient arrays --
  // g_verts [N][3], g_sigmas [N], g_colors [N][C], zeroed by the forward -- instead of acc [P][8] + a finishing pass: one launch
  // less, and the kernel went from 107 to 137 us.  An entry's eight sums are ONE 32-byte atomic request here and three requests
  // into three arrays there; the kernel's tail is bound by those requests.  acc stays; the forward zeroes it on its way.)
  auto sum_add = [&](const int key, const int c, const float v) { unsafeAtomicAdd(acc + NACC * (size_t)key + c, v); };
  constexpr int ND = (SRC == 0 && ISO && C == 3) ? kFbNDFrame : kFbND;      // directory keys (NS == 2)
  __shared__ __attribute__((aligned(16))) FragBwdLds<NV4, NS, ND> L;
  float *const Llen = L.len, *const Lsp = L.sp, *const LE = L.E, *const Lu = L.u, *const LR = L.r;
  const int lane = threadIdx.x;
  FB_T0();
  const int blocks_x = (W + kFbGW - 1) / kFbGW;
  const long blk = blockIdx.x;
  const int x0 = (int)(blk % blocks_x) * kFbGW;
  const long y0 = (blk / blocks_x) * kFbGH;
  const bool vec = (K % NS) == 0;
  // the group's hit counts -> lanes per pixel
  const int gx = x0 + (lane & (kFbGW - 1));
  const long gy = y0 + lane / kFbGW;
  const bool pv = lane < kFbG && gx < W && gy < nrows;
  const int lead_g = pv ? min(K, max(0, cnt[gy * W + gx])) : 0;
  const int need = (lead_g + NS - 1) / NS;
  const int incl = wave_incl_scan(need, lane);
  if (__builtin_amdgcn_readlane(incl, 63) == 0) return;     // nothing was hit in these pixels
  if constexpr (NS == 2) wd_clear(L.tab, lane); else wt_clear(L.tab, lane);
  int pc = 0, off = 0;
  while (pc < kFbG) {
    PackLane pk;
    int npm;
    const int pe = pack_round(need, incl, kFbG, lane, pc, off, pk, npm);
    off = __builtin_amdgcn_readlane(incl, pe - 1);
    pc = pe;
    if (npm == 0) continue;       // (uniform) a run of empty pixels
    FB_TICK(0);
    const bool on = pk.p >= 0;
    const int q = on ? lane - pk.s0 : 0, LP = on ? pk.np : 1;
    const int lead = __shfl(lead_g, on ? pk.p : 0, 64);
    const int k0 = NS * q;
    const OffT pix = on ? (OffT)((y0 + pk.p / kFbGW) * W + x0 + (pk.p & (kFbGW - 1))) : (OffT)0;
    const OffT fb = (pix * (OffT)K + (OffT)k0) * (OffT)4;      // byte offset of the lane's group in the [pix][K] arrays
    const int r0 = NS * pk.s0 + 4 * pk.ord, RS = NS * LP + 4;
    const int d0 = on ? r0 + 2 + k0 : 2;
    // ---- the lane's slots ----
    // Round 5: the loads of a round go out in TWO waves of requests -- everything addressed by the pixel (ray, the slots'
    // idx / weight / len [/ act / dsd / g_weight], the pixel's forward sums and upstream gradient), then everything addressed
    // by the slots' Gaussian ids (records, colours) -- each unconditional at a clamped address, masks applied to the VALUES
    // afterwards.  As `if (on) load ...; if (live) load ...` the compiler had to join every exec-mask region before the next:
    // ray -> wait -> streams -> wait -> record 0 -> wait -> record 1 -> wait -> colours -> pixel data, six dependent round trips
    // per round (SQ_WAIT_ANY: 46 % of the kernel's wave cycles, profiles/r5_pmc_sq_counters_head.txt).
    int id[NS];
    float wv[NS], lm[NS], sm[NS], em[NS], gwv[NS];
    bool live[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      id[a] = -1; wv[a] = 0.f; lm[a] = VOGE_SENT_LEN; sm[a] = 1e-5f; em[a] = 0.f; gwv[a] = 0.f;
      live[a] = on && (k0 + a < lead);
    }
    // (a lane that is off reads pixel 0, slot 0: pix = 0 and q = 0 there)
    const float3 dv = at_bytes<float3>(rays, pix * (OffT)12);
    const float dx = on ? dv.x : 0.f, dy = on ? dv.y : 0.f, dz = on ? dv.z : 0.f;
    float4 rc[NS][NRC];
    float av[NS], dv2[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) { av[a] = 0.f; dv2[a] = 0.f; }
    {
      int idr[NS];
      float wr[NS], lr[NS], ar[NS], dr[NS], gr_[NS];
#pragma unroll
      for (int a = 0; a < NS; ++a) { idr[a] = -1; wr[a] = 0.f; lr[a] = VOGE_SENT_LEN; ar[a] = 0.f; dr[a] = 0.f; gr_[a] = 0.f; }
      const bool gw_wide = SRC == 1 && g_img != nullptr && vec && gs_c == 1 && gs_pix == (long)K;
      if (vec) {                // (uniform) wide accesses: the group is aligned and inside the pixel's row
#pragma unroll
        for (int h2 = 0; h2 < NS / 2; ++h2) {
          const OffT fo = fb + (OffT)(8 * h2);
          const int2 i2 = at_bytes<int2>(idx, fo);
          const v2f w2 = at_bytes<v2f>(weight, fo), l2 = at_bytes<v2f>(len, fo);
          idr[2 * h2] = i2.x; idr[2 * h2 + 1] = i2.y; wr[2 * h2] = w2.x; wr[2 * h2 + 1] = w2.y; lr[2 * h2] = l2.x; lr[2 * h2 + 1] = l2.y;
          if (!NOAD) {
            const v2f a2 = at_bytes<v2f>(act, fo), d2 = at_bytes<v2f>(dsd, fo);
            ar[2 * h2] = a2.x; ar[2 * h2 + 1] = a2.y; dr[2 * h2] = d2.x; dr[2 * h2 + 1] = d2.y;
          }
          if (gw_wide) {        // (uniform)
            const v2f g2 = at_bytes<v2f>(g_img, fo);
            gr_[2 * h2] = g2.x; gr_[2 * h2 + 1] = g2.y;
          }
        }
      } else {                  // slot by slot; a slot behind the pixel's row re-reads the row's last one (never live)
#pragma unroll
        for (int a = 0; a < NS; ++a) {
          const OffT fo = (pix * (OffT)K + (OffT)min(k0 + a, K - 1)) * (OffT)4;
          idr[a] = at_bytes<int>(idx, fo); wr[a] = at_bytes<float>(weight, fo); lr[a] = at_bytes<float>(len, fo);
          if (!NOAD) { ar[a] = at_bytes<float>(act, fo); dr[a] = at_bytes<float>(dsd, fo); }
        }
      }
      if (SRC == 1 && g_img != nullptr && !gw_wide) {      // (uniform) the consumers' gradient of the weights, any strides
#pragma unroll
        for (int a = 0; a < NS; ++a) gr_[a] = g_img[(long)pix * gs_pix + (long)min(k0 + a, K - 1) * gs_c];
      }
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        if (live[a]) { id[a] = idr[a]; wv[a] = wr[a]; lm[a] = lr[a]; av[a] = ar[a]; dv2[a] = dr[a]; gwv[a] = gr_[a]; }
      }
    }
    // the pixel's forward sums and upstream gradient (the shade stage), requested with the slots
    float gr[4] = {0.f, 0.f, 0.f, 0.f}, g_sum_w = 0.0f;
    float px_ws = 0.f, px_rgb[4] = {0.f, 0.f, 0.f, 0.f}, px_g[4] = {0.f, 0.f, 0.f, 0.f};
    if (SRC == 2) {      // (depth form: the gradient of the depth, the forward's weight sum and depth, the silhouette's gradient)
      if (g_img != nullptr) px_g[0] = g_img[(long)pix * gs_pix];
      px_ws = at_bytes<float>(wsum, pix * (OffT)4);
      px_rgb[0] = at_bytes<float>(rgb, pix * (OffT)4);
      if (bg != nullptr) px_g[1] = at_bytes<float>(bg, pix * (OffT)4);
    }
    if (SRC == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) px_g[c] = g_img[(long)pix * gs_pix + c * gs_c];
      if (wsum != nullptr) px_ws = at_bytes<float>(wsum, pix * (OffT)4);
      if (bg != nullptr) {
#pragma unroll
        for (int c = 0; c < C; ++c) px_rgb[c] = at_bytes<float>(rgb, pix * (OffT)(4 * C) + (OffT)(4 * c));
      } else if (rgb != nullptr) {      // (merge form, round 6: `rgb` = the forward's weight sums [pix], `wsum` = the SILHOUETTE's gradient)
        px_rgb[0] = at_bytes<float>(rgb, pix * (OffT)4);
      }
    }
    // ---- second wave of requests: what the slots' Gaussians carry (records, colours), at clamped ids ----
    bool okv[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) okv[a] = live[a] && id[a] >= 0 && id[a] < P;
    if (NOAD) {      // (act / dsd re-derived from the records; with act / dsd given the records are only needed by the trace terms)
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const uint32_t ro = (uint32_t)(okv[a] ? id[a] : 0) * (16u * NRC);      // (P < 2^26: host)
#pragma unroll
        for (int r = 0; r < NRC; ++r) rc[a][r] = !(VOGE_FB_ABL & 8) ? at_bytes<float4>(rec, ro + 16u * r) : make_float4(0.f, 0.f, 0.f, 0.f);      // (P >= 1, Nattr >= 1 here: host)
      }
    }
    float col[NS][4];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      col[a][0] = col[a][1] = col[a][2] = col[a][3] = 0.0f;
      if (SRC == 0 && !(VOGE_FB_ABL & 4)) {
        const bool cok = okv[a] && id[a] < Nattr;
        const uint32_t o = (uint32_t)(cok ? id[a] : 0) * (uint32_t)(4 * C);      // (bytes; Nattr * C < 2^30: host)
        if (C == 3) {
          const float3 v = at_bytes<float3>(colors, o);
          col[a][0] = cok ? v.x : 0.f; col[a][1] = cok ? v.y : 0.f; col[a][2] = cok ? v.z : 0.f;
        } else if (C == 4) {
          const float4 v = at_bytes<float4>(colors, o);
          col[a][0] = cok ? v.x : 0.f; col[a][1] = cok ? v.y : 0.f; col[a][2] = cok ? v.z : 0.f; col[a][3] = cok ? v.w : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) { const float v = at_bytes<float>(colors, o + 4u * c); col[a][c] = cok ? v : 0.f; }
        }
      }
    }
    // ---- em / sm of the slots: from act / dsd, or (NOAD) re-derived from the records with the forward's own operations ----
    if (!NOAD) {
#pragma unroll
      for (int a = 0; a < NS; ++a)
        if (live[a]) { em[a] = FAST_EXP(-av[a]); sm[a] = FAST_SQRT(dv2[a] + 1e-10f); }
    }
    if (NOAD && ISO) {
      const float dn2f = (dx * dx + dy * dy) + dz * dz;      // the forward's association
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const PairOut o = pair_eval_iso_at(rc[a][0].x, rc[a][0].y, rc[a][0].z, rc[a][0].w, lm[a], dx, dy, dz, dn2f);
        em[a] = okv[a] ? FAST_EXP(-o.act) : em[a]; sm[a] = okv[a] ? FAST_SQRT(o.dsd + 1e-10f) : sm[a];
      }
    }
    if (NOAD && DIAG) {         // per-axis forms: the same from the compact records
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const float4 r0 = rc[a][0], r1 = rc[a][NRC - 1];
        const PairOut o = pair_eval_diag(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, dx, dy, dz);
        em[a] = okv[a] ? FAST_EXP(-o.act) : em[a]; sm[a] = okv[a] ? FAST_SQRT(o.dsd + 1e-10f) : sm[a];
      }
    }
    if (NOAD && !ISO && !DIAG) {         // general forms: the same from the packed (mu, A) records, with the forward's operations
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const float4 r0 = rc[a][0], r1 = rc[a][NRC == 3 ? 1 : 0], r2 = rc[a][NRC == 3 ? 2 : 0];
        const float A[9] = {r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        const PairOut o = pair_eval(r0.x, r0.y, r0.z, make_eval(r0.x, r0.y, r0.z, A), dx, dy, dz, dx * dx, dy * dy, dz * dz,
                                    dx * dy, dx * dz, dy * dz);
        em[a] = okv[a] ? FAST_EXP(-o.act) : em[a]; sm[a] = okv[a] ? FAST_SQRT(o.dsd + 1e-10f) : sm[a];
      }
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) live[a] = okv[a];
    if (SRC == 0 && on && bg == nullptr) {
      // merge_final alone (interpolate_attr): the image's gradient is the merged attributes' own, and `wsum` carries the
      // gradient of the per-pixel weight sum (what a get_silhouette on the same fragments hands back), or is NULL
#pragma unroll
      for (int c = 0; c < C; ++c) gr[c] = px_g[c];
      if (wsum != nullptr) g_sum_w = px_ws;
      // (get_silhouette = min(sum w, 1) behind the same fragments: its gradient passes like torch.minimum's -- all of it below 1,
      //  half at a tie, none above)
      if (rgb != nullptr) g_sum_w *= (px_rgb[0] < 1.0f ? 1.0f : (px_rgb[0] == 1.0f ? 0.5f : 0.0f));
    } else if (SRC == 0 && on) {
      const float ws = px_ws;
      float sil = fminf(ws, 1.0f);
      const float pass_s = (thr > 0.0f) ? 0.0f : (ws < 1.0f ? 1.0f : (ws == 1.0f ? 0.5f : 0.0f));
      if (thr > 0.0f) sil = sil > thr ? 1.0f : 0.0f;
      float g_mask = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float xc = fmaf(1.0f - sil, bg[c], px_rgb[c]);
        gr[c] = px_g[c] * (xc < 1.0f ? 1.0f : (xc == 1.0f ? 0.5f : 0.0f));     // min(x, 1) passes like torch.min
        g_mask = fmaf(-gr[c], bg[c], g_mask);
      }
      g_sum_w = g_mask * pass_s;
    }
    float dp_a = 0.0f, dp_b = 0.0f;      // (SRC == 2) the pixel's two scalars: g_w[k] = dp_a len_k + dp_b, g_len[k] += dp_a w_k
    if (SRC == 2) {
      const bool hit = px_ws > 0.0f;
      dp_a = thr > 0.0f ? (hit ? px_g[0] / px_ws : 0.0f) : px_g[0];
      dp_b = (thr > 0.0f && hit) ? -dp_a * px_rgb[0] : 0.0f;
      dp_b = fmaf(px_g[1], px_ws < 1.0f ? 1.0f : (px_ws == 1.0f ? 0.5f : 0.0f), dp_b);      // get_silhouette = min(S, 1) behind the same fragments
    }
    // ---- shade backward: g_w of the slots; u = g_w w ----
    float um[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      float gw;
      if (SRC == 0) gw = live[a] ? fmaf(gr[3], col[a][3], fmaf(gr[2], col[a][2], fmaf(gr[1], col[a][1], fmaf(gr[0], col[a][0], g_sum_w)))) : 0.0f;
      else if (SRC == 2) gw = live[a] ? fmaf(dp_a, lm[a], dp_b) : 0.0f;
      else gw = live[a] ? gwv[a] : 0.0f;
      um[a] = gw * wv[a];
    }
    // ---- composite backward (closed form, composite_core.h) ----
    FB_TICK(1);
    if (on) {
#pragma unroll
      for (int h2 = 0; h2 < NS / 2; ++h2) {
        const int a = 2 * h2;
        *reinterpret_cast<v2f *>(Llen + d0 + a) = (v2f){lm[a], lm[a + 1]};
        *reinterpret_cast<v2f *>(Lsp + d0 + a) = (v2f){sm[a] * kCs, sm[a + 1] * kCs};
        *reinterpret_cast<v2f *>(LE + d0 + a) = (v2f){em[a] * (sm[a] * kCs), em[a + 1] * (sm[a + 1] * kCs)};
        *reinterpret_cast<v2f *>(Lu + d0 + a) = splat(0.0f);
        *reinterpret_cast<v2f *>(LR + d0 + a) = splat(0.0f);
      }
      if (q < 2) {      // the sentinel pair in front of the pixel's row and the one behind it
        for (int t2 = q; t2 < 2; t2 += LP) {
          Llen[r0 + t2] = -kBig; Lsp[r0 + t2] = 1.0f; LE[r0 + t2] = 0.0f; Lu[r0 + t2] = 0.0f;
          const int eb = r0 + RS - 2 + t2;
          Llen[eb] = kBig; Lsp[eb] = 1.0f; LE[eb] = 0.0f; Lu[eb] = 0.0f;
          LR[r0 + t2] = 0.0f; LR[eb] = 0.0f;
        }
      }
    }
    wave_lds_sync();
    float ga[NS], gl[NS], gd[NS];
#if VOGE_FB_ABL & 2       // (timing experiment: no composite)
    for (int a = 0; a < NS; ++a) { ga[a] = um[a]; gl[a] = um[a] * sm[a]; gd[a] = um[a] * em[a]; }
#else
    compn_bwd_wave<NS>(lm, sm, em, um, Llen, Lsp, LE, Lu, d0, k0, NS * LP, q, LP, npm, on, on, true, occ, ga, gl, gd, LR);
#endif
    wave_lds_sync();      // the rows are rewritten by the next round
    FB_TICK(2);
    if (SRC == 1 && g_hitlen != nullptr) {      // vert_hit_length is the trace's len itself (Aggregation.py:107)
#pragma unroll
      for (int a = 0; a < NS; ++a)
        if (live[a]) gl[a] += at_bytes<float>(g_hitlen, fb + (OffT)(4 * a));
    }
    if (SRC == 2) {      // the depth's own gradient of len: a w_k
#pragma unroll
      for (int a = 0; a < NS; ++a)
        if (live[a]) gl[a] = fmaf(dp_a, wv[a], gl[a]);
    }
    // ---- trace backward terms (isotropic: trace_bwd.hip) + the colour term, one table entry per Gaussian.  (The
    // (mu, a) records are gathered only now: held across the composite they cost the kernel a wave per SIMD.) ----
    // (scalar sigmas without act / dsd: the records gathered above serve here too.  Otherwise they are gathered only now:
    //  held across the composite they cost the kernel a wave per SIMD -- 24 registers for the full forms)
    if (!NOAD || !ISO)
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      const uint32_t ro = (uint32_t)(live[a] ? id[a] : 0) * (16u * NRC);      // (P < 2^26: host)
#pragma unroll
      for (int r = 0; r < NRC; ++r)
        rc[a][r] = !(VOGE_FB_ABL & 8) ? at_bytes<float4>(rec, ro + 16u * r) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float dn2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float idn = __builtin_amdgcn_rcpf(dn2);
    // (two slots per lane: both slots' terms first, then ONE table pass for both -- wd_find2, wt_add2_by_group)
    constexpr bool PAIR = NS == 2;
    float4 valp[PAIR ? 2 : 1][NV4];
    bool gop[2] = {false, false};
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      float4 val[NV4];
#pragma unroll
      for (int r = 0; r < NV4; ++r) val[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      bool go = live[a];
      if (go) {
        if (ISO) {
          const float mx = rc[a][0].x, my = rc[a][0].y, mz = rc[a][0].z, aa = rc[a][0].w;
          const float t = fmaf(mz, dz, fmaf(my, dy, mx * dx)) * idn;
          float vx = fmaf(-t, dx, mx), vy = fmaf(-t, dy, my), vz = fmaf(-t, dz, mz);
          {   // (trace_bwd.hip: the component of v along d is t's rounding error; project it out before 2 a g_act scales it)
            const float rr = fmaf(vz, dz, fmaf(vy, dy, vx * dx)) * idn;
            vx = fmaf(-rr, dx, vx); vy = fmaf(-rr, dy, vy); vz = fmaf(-rr, dz, vz);
          }
          const float c1 = gl[a] * idn, c2 = 2.0f * aa * ga[a];
          val[0] = make_float4(fmaf(c1, dx, c2 * vx), fmaf(c1, dy, c2 * vy), fmaf(c1, dz, c2 * vz),
                               fmaf(ga[a], fmaf(vz, vz, fmaf(vy, vy, vx * vx)), gd[a] * dn2));
        } else if (DIAG) {
          // A = diag(a0, a1, a2): the general terms below with every product by a zero coefficient left out (they add +-0 there)
          const float4 r0 = rc[a][0], r1 = rc[a][NRC - 1];
          const float mx = r0.x, my = r0.y, mz = r0.z;
          const float adx = r0.w * dx, ady = r1.x * dy, adz = r1.y * dz;
          const float ksk = fmaf(dz, adz, fmaf(dy, ady, dx * adx)), msk = fmaf(mz, adz, fmaf(my, ady, mx * adx));
          const float ik = __builtin_amdgcn_rcpf(ksk);
          const float t = msk * ik;
          float vx = fmaf(-t, dx, mx), vy = fmaf(-t, dy, my), vz = fmaf(-t, dz, mz);
          {
            const float rr = fmaf(vz, adz, fmaf(vy, ady, vx * adx)) * ik;
            vx = fmaf(-rr, dx, vx); vy = fmaf(-rr, dy, vy); vz = fmaf(-rr, dz, vz);
          }
          const float avx = r0.w * vx, avy = r1.x * vy, avz = r1.y * vz;
          const float c1 = gl[a] * ik, g_a = ga[a], g_d = gd[a];
          const float o0 = fmaf(c1, adx, g_a * (avx + avx)), o1 = fmaf(c1, ady, g_a * (avy + avy)), o2 = fmaf(c1, adz, g_a * (avz + avz));
          const float o3 = fmaf(g_a, vx * vx, fmaf(g_d, dx * dx, c1 * (vx * dx)));
          const float o4 = fmaf(g_a, vy * vy, fmaf(g_d, dy * dy, c1 * (vy * dy)));
          const float o5 = fmaf(g_a, vz * vz, fmaf(g_d, dz * dz, c1 * (vz * dz)));
          val[0] = make_float4(o0, o1, o2, o3);
          if (SRC == 0) {
            val[NV4 >= 2 ? 1 : 0] = make_float4(o4, o5, wv[a] * gr[0], wv[a] * gr[1]);
            val[NV4 >= 3 ? 2 : 0] = make_float4(wv[a] * gr[2], wv[a] * gr[3], 0.f, 0.f);
          } else {
            val[NV4 >= 2 ? 1 : 0] = make_float4(o4, o5, 0.f, 0.f);
          }
        } else {
          // the merged per-target terms of trace_bwd.hip (header there): g_mu (3) and the unsymmetrised g_A (9)
          const float4 r0 = rc[a][0], r1 = rc[a][NRC == 3 ? 1 : 0], r2 = rc[a][NRC == 3 ? 2 : 0];
          const float mx = r0.x, my = r0.y, mz = r0.z;
          const float A[9] = {r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
          const float adx = fmaf(A[2], dz, fmaf(A[1], dy, A[0] * dx)), ady = fmaf(A[5], dz, fmaf(A[4], dy, A[3] * dx)),
                      adz = fmaf(A[8], dz, fmaf(A[7], dy, A[6] * dx));
          const float tdx = fmaf(A[6], dz, fmaf(A[3], dy, A[0] * dx)), tdy = fmaf(A[7], dz, fmaf(A[4], dy, A[1] * dx)),
                      tdz = fmaf(A[8], dz, fmaf(A[5], dy, A[2] * dx));
          const float ksk = fmaf(dz, adz, fmaf(dy, ady, dx * adx)), msk = fmaf(mz, adz, fmaf(my, ady, mx * adx));
          const float ik = __builtin_amdgcn_rcpf(ksk);
          const float t = msk * ik;
          float vx = fmaf(-t, dx, mx), vy = fmaf(-t, dy, my), vz = fmaf(-t, dz, mz);
          {   // (v^T A d = 0 by construction: what is left of it is t's rounding error; one projection along d removes it)
            const float rr = fmaf(vz, adz, fmaf(vy, ady, vx * adx)) * ik;
            vx = fmaf(-rr, dx, vx); vy = fmaf(-rr, dy, vy); vz = fmaf(-rr, dz, vz);
          }
          const float avx = fmaf(A[2], vz, fmaf(A[1], vy, A[0] * vx)), avy = fmaf(A[5], vz, fmaf(A[4], vy, A[3] * vx)),
                      avz = fmaf(A[8], vz, fmaf(A[7], vy, A[6] * vx));
          const float tvx = fmaf(A[6], vz, fmaf(A[3], vy, A[0] * vx)), tvy = fmaf(A[7], vz, fmaf(A[4], vy, A[1] * vx)),
                      tvz = fmaf(A[8], vz, fmaf(A[5], vy, A[2] * vx));
          const float c1 = gl[a] * ik, g_a = ga[a], g_d = gd[a];
          float o[12];
          o[0] = fmaf(c1, adx, g_a * (avx + tvx + t * (tdx - adx)));
          o[1] = fmaf(c1, ady, g_a * (avy + tvy + t * (tdy - ady)));
          o[2] = fmaf(c1, adz, g_a * (avz + tvz + t * (tdz - adz)));
          const float d[3] = {dx, dy, dz}, v[3] = {vx, vy, vz};
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c)
              o[3 + 3 * i + c] = fmaf(g_a, fmaf(v[i], v[c], t * (d[i] * v[c] - v[i] * d[c])), fmaf(g_d, d[i] * d[c], c1 * (v[i] * d[c])));
          val[0] = make_float4(o[0], o[1], o[2], o[3]);
          val[NV4 >= 3 ? 1 : 0] = make_float4(o[4], o[5], o[6], o[7]);
          val[NV4 >= 3 ? 2 : 0] = make_float4(o[8], o[9], o[10], o[11]);
        }
        if (SRC == 0 && !DIAG) val[NV4 - 1] = make_float4(wv[a] * gr[0], wv[a] * gr[1], wv[a] * gr[2], wv[a] * gr[3]);
        go = false;
#pragma unroll
        for (int r = 0; r < NV4; ++r) go = go || (val[r].x != 0.f || val[r].y != 0.f || val[r].z != 0.f || val[r].w != 0.f);
      }
      if (PAIR) {
#pragma unroll
        for (int r = 0; r < NV4; ++r) valp[PAIR ? a : 0][r] = val[r];
        gop[a] = go;
        continue;
      }
      if constexpr (!PAIR) {
      if (!__any(go)) continue;     // uniform
      FB_TICK(3);
#if VOGE_FB_ABL & 1       // (timing experiment: no table, nothing accumulated)
      if (go && val[0].x == 1.2345f && val[NV4 - 1].y == 3.21f) acc[id[a]] = val[0].w + val[NV4 - 1].x;
      continue;
#endif
      const int slot = wt_find(L.tab, id[a], go);
#ifdef VOGE_FB_TIMES      // (election rounds per accumulation: tools/fb_sections.py)
      {
        lds_vint *owner = lds_volatile(L.tab.owner);
        bool pending = go && slot >= 0;
        const unsigned long long m0 = __ballot(pending);
        unsigned rounds = 0;
        while (__any(pending)) {
          if (pending) owner[slot] = lane;
          if (pending && owner[slot] == lane) pending = false;
          ++rounds;
        }
        if (lane == 0 && blockIdx.x < kFbTimesWaves) {
          g_fb_tab[blockIdx.x][0] += 1; g_fb_tab[blockIdx.x][1] += rounds; g_fb_tab[blockIdx.x][2] += (unsigned)__popcll(m0);
        }
      }
#endif
      wt_add(L.tab, slot, val, go && slot >= 0, lane);
      if (go && slot < 0) {         // table full: rare, straight to memory
#pragma unroll
        for (int r = 0; r < NV4; ++r) {
          const float o[4] = {val[r].x, val[r].y, val[r].z, val[r].w};
#pragma unroll
          for (int c = 0; c < 4; ++c) sum_add(id[a], 4 * r + c, o[c]);
        }
      }
      FB_TICK(4);
      }
    }
    if constexpr (PAIR) if (__any(gop[0] | gop[1])) {
      FB_TICK(3);
#if VOGE_FB_ABL & 1       // (timing experiment: no table, nothing accumulated)
      if (gop[0] && gop[1] && valp[0][0].x == 1.2345f && valp[PAIR ? 1 : 0][NV4 - 1].y == 3.21f) acc[id[0]] = valp[0][NV4 - 1].w + valp[PAIR ? 1 : 0][0].x;
#else
      int slot0, slot1;
      wd_find2(L.tab, id[0], gop[0], id[NS - 1], gop[1], lane, slot0, slot1);
      wt_add2_by_group(L.tab, slot0, valp[0], gop[0] && slot0 >= 0, slot1, valp[PAIR ? 1 : 0], gop[1] && slot1 >= 0, pk.ord);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int sl = a == 0 ? slot0 : slot1;
        if (gop[a] && sl < 0) {         // table full: rare, straight to memory
#pragma unroll
          for (int r = 0; r < NV4; ++r) {
            const float o[4] = {valp[PAIR ? a : 0][r].x, valp[PAIR ? a : 0][r].y, valp[PAIR ? a : 0][r].z, valp[PAIR ? a : 0][r].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) sum_add(id[a == 0 ? 0 : NS - 1], 4 * r + c, o[c]);
          }
        }
      }
#endif
      FB_TICK(4);
    }
  }
  FB_TICK(0);
  {   // flush: NACC (4 | 8 | 12 | 16) adjacent lanes per entry -> the bytes of acc[p]: lane-coalesced atomics
    constexpr int EPI = 64 / NACC;      // entries per iteration (12 sums: five entries, four idle lanes)
    const int e = lane / NACC, c = lane - e * NACC;
    const float *vals = reinterpret_cast<const float *>(L.tab.vals);
    if constexpr (NS == 2) {      // the entries are dense: 0 .. n - 1, each with its key
      const int n = wd_count(L.tab);
      for (int i = e; i < n && e < EPI; i += EPI) sum_add(L.tab.ekey[i], c, vals[i * NACC + c]);
    } else {
      const int n = wt_compact(L.tab, lane);
      const lds_vint *list = lds_volatile(L.tab.owner);
      for (int i = e; i < n && e < EPI; i += EPI) {
        const int s = list[i];
        sum_add(L.tab.keys[s], c, vals[s * NACC + c]);
      }
    }
  }
  FB_TICK(5);
  FB_TOUT();
}

// acc [P][S] (S = 8: (g_mu, g_a | w g_rgb), S = 4: (g_mu, g_a)) -> the gradients of what the caller passed in: verts /
// sigmas through the view's chain rule (and the sum over the batch when one Gaussian set is shared by all views),
// colours [Nattr][C].
__global__ void __launch_bounds__(256)
fragment_bwd_finish_kernel(const float *__restrict__ acc, const int S, const float *__restrict__ a_in, const int P, const int N,
                           const int B, const IsoView view, const int C, const long Nattr, float *__restrict__ g_mus,
                           float *__restrict__ g_a, float *__restrict__ g_colors) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g_colors != nullptr && g < Nattr) {
    for (int c = 0; c < C; ++c) g_colors[(size_t)g * C + c] = (g < P) ? acc[S * (size_t)g + 4 + c] : 0.0f;
  }
  const int n_out = view.shared ? N : P;
  if (g >= n_out || g_mus == nullptr) return;
  float4 v = *reinterpret_cast<const float4 *>(acc + S * (size_t)g);
  if (view.shared)
    for (int b = 1; b < B; ++b) {
      const float4 w = *reinterpret_cast<const float4 *>(acc + S * ((size_t)b * N + g));
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
  g_mus[3 * (size_t)g] = v.x; g_mus[3 * (size_t)g + 1] = v.y; g_mus[3 * (size_t)g + 2] = v.z;
  float ga = v.w;
  if (view.mode == 1) ga = 2.0f * ga;
  else if (view.mode == 2) { const float s = a_in[g]; ga = -2.0f * ga / (s * s); }
  g_a[g] = ga;
}

// General 3x3 forms: mus [P,3] + isigmas [P,9] -> 3 x float4 per Gaussian (one gather stream), acc [P][16] zeroed
__global__ void __launch_bounds__(256)
fragment_bwd_pack_kernel(const float *__restrict__ mus, const float *__restrict__ isg, const int P, float4 *__restrict__ rec,
                         float4 *__restrict__ acc, const int S4 /* float4s of sums per Gaussian: 4 | 3 */) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P) return;
  for (int q = 0; q < S4; ++q) acc[S4 * (size_t)g + q] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float *m = mus + 3 * (size_t)g, *A = isg + 9 * (size_t)g;
  rec[3 * (size_t)g + 0] = make_float4(m[0], m[1], m[2], A[0]);
  rec[3 * (size_t)g + 1] = make_float4(A[1], A[2], A[3], A[4]);
  rec[3 * (size_t)g + 2] = make_float4(A[5], A[6], A[7], A[8]);
}
// acc [P][S] (S = 16 with the colour term, 12 without) -> g_mus [P,3], g_isigmas [P,9], g_colors [Nattr,C]
__global__ void __launch_bounds__(256)
fragment_bwd_finish_general_kernel(const float *__restrict__ acc, const int S, const int P, const int C, const long Nattr,
                                   float *__restrict__ g_mus, float *__restrict__ g_isg, float *__restrict__ g_colors) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long g = t >> 4;
  const int c = (int)(t & 15);
  if ((g >= P && g >= Nattr) || c >= S) return;
  const float v = (g < P) ? acc[g * S + c] : 0.0f;
  if (c < 3) { if (g < P && g_mus != nullptr) g_mus[3 * g + c] = v; }
  else if (c < 12) { if (g < P && g_isg != nullptr) g_isg[9 * g + (c - 3)] = v; }
  else if (c - 12 < C && g < Nattr && g_colors != nullptr) g_colors[g * C + (c - 12)] = v;
}

// act / dsd of fragments that were traced without them (A = a I): the sweep epilogue's own operations per live slot,
// the trace's sentinels elsewhere.  One thread per slot.
__global__ void __launch_bounds__(256)
fragment_act_dsd_iso_kernel(const float4 *__restrict__ rec, const float *__restrict__ rays, const int32_t *__restrict__ idx,
                            const float *__restrict__ len, const int32_t *__restrict__ cnt, const long npix, const int K,
                            const int P, float *__restrict__ act, float *__restrict__ dsd) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix * K) return;
  const long pix = t / K;
  const int k = (int)(t - pix * K);
  float a = VOGE_SENT_ACT, d = 0.0f;
  const int id = idx[t];
  if (k < cnt[pix] && id >= 0 && id < P) {
    const float4 r = rec[id];
    const float dx = rays[pix * 3], dy = rays[pix * 3 + 1], dz = rays[pix * 3 + 2];
    const PairOut o = pair_eval_iso_at(r.x, r.y, r.z, r.w, len[t], dx, dy, dz, (dx * dx + dy * dy) + dz * dz);
    a = o.act; d = o.dsd;
  }
  act[t] = a; dsd[t] = d;
}

}  // namespace voge

using namespace voge;

#ifdef VOGE_FB_TIMES
extern "C" int voge_debug_fb_times(unsigned long long *out, int reset) {      // out: [8] sums over the workgroups
  static unsigned long long host[voge::kFbTimesWaves][8];
  if (reset) {
    for (auto &row : host) for (auto &v : row) v = 0;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(voge::g_fb_times), host, sizeof(host));
  }
  const int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(voge::g_fb_times), sizeof(host));
  for (int i = 0; i < 8; ++i) out[i] = 0;
  for (int w = 0; w < voge::kFbTimesWaves; ++w)
    for (int i = 0; i < 8; ++i) out[i] += host[w][i];
  return rc;
}
extern "C" int voge_debug_fb_tab(unsigned long long *out /* [4] sums */, int reset) {
  static unsigned long long host[voge::kFbTimesWaves][4];
  if (reset) {
    for (auto &row : host) for (auto &v : row) v = 0;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(voge::g_fb_tab), host, sizeof(host));
  }
  const int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(voge::g_fb_tab), sizeof(host));
  for (int i = 0; i < 4; ++i) out[i] = 0;
  for (int w = 0; w < voge::kFbTimesWaves; ++w)
    for (int i = 0; i < 4; ++i) out[i] += host[w][i];
  return rc;
}
extern "C" int voge_debug_fb_wall(unsigned long long *out /* [n][2] */, int n, int reset) {
  static unsigned long long host[voge::kFbTimesWaves][2];
  if (reset) {
    for (auto &row : host) for (auto &v : row) v = 0;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(voge::g_fb_wall), host, sizeof(host));
  }
  const int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(voge::g_fb_wall), sizeof(host));
  for (int w = 0; w < n && w < voge::kFbTimesWaves; ++w) { out[2 * w] = host[w][0]; out[2 * w + 1] = host[w][1]; }
  return rc;
}
extern "C" int voge_debug_cw_stats(unsigned long long *out, int reset) {      // out: [4] sums (composite_core.h: CW_COUNT)
  static unsigned long long host[1 << 16][4];
  if (reset) {
    for (auto &row : host) for (auto &v : row) v = 0;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(voge::g_cw_stats), host, sizeof(host));
  }
  const int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(voge::g_cw_stats), sizeof(host));
  for (int i = 0; i < 4; ++i) out[i] = 0;
  for (int w = 0; w < (1 << 16); ++w)
    for (int i = 0; i < 4; ++i) out[i] += host[w][i];
  return rc;
}
#endif

extern "C" int voge_fragment_act_dsd_iso(const float *records, const float *rays, const int32_t *idx, const float *len,
                                         const int32_t *cnt, long npix, int K, int P, float *act, float *dsd,
                                         voge_stream_t stream) {
  if (npix < 0 || K <= 0 || P < 0) return VOGE_ERR_BAD_ARG;
  if (npix == 0) return 0;
  if ((!records && P > 0) || !rays || !idx || !len || !cnt || !act || !dsd) return VOGE_ERR_BAD_ARG;
  const long n = npix * K;
  hipLaunchKernelGGL(fragment_act_dsd_iso_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(records), rays, idx, len, cnt, npix, K, P, act, dsd);
  return launch_status();
}

// (the isotropic forms use the first 32 | 16 bytes per Gaussian; the general ones 48 of packed records + 64 | 48 of sums)
extern "C" size_t voge_fragment_bwd_workspace_bytes(int P) { return P <= 0 ? 0 : (size_t)P * 112; }
// The frame path's accumulators arrive zeroed (the frame's forward does that on its way: voge_frame_shade_fwd_iso's bwd_acc) and
// are good for ONE backward.
extern "C" size_t voge_frame_bwd_acc_bytes(int P) { return P <= 0 ? 0 : (size_t)P * 32; }
extern "C" size_t voge_frame_bwd_gen_acc_bytes(int P) { return P <= 0 ? 0 : (size_t)P * 64; }      // (kind 1 uses 48 | 32 of them)

// ---- the finishing passes of the general forms on the frame path (fragments made by voge_frame_trace_fwd_gen / _ori): the
// renderer's own chain rule (Renderer.py:130-137 backwards: the sum over the views of a shared set; d A / d sigma = 2 on the
// diagonal for per-axis sigmas, 2 everywhere for [3][3] ones) -- no general_preamble_bwd launch behind it.
// thread t of a finishing pass: the attributes' gradient (acc[..][attr_at ..]) and the vertices' (acc[..][0..2]; a shared set: its
// views in a fixed order)
__device__ __forceinline__ void finish_attr_verts(const float *__restrict__ acc, const int S, const int P, const int N, const int B,
                                                  const int shared_v, const int attr_at, const int C, const long Nattr,
                                                  float *__restrict__ g_verts, float *__restrict__ g_attr, const long t) {
  if (g_attr != nullptr && t < Nattr) {
    for (int c = 0; c < C; ++c) g_attr[t * C + c] = (t < P) ? acc[t * S + attr_at + c] : 0.0f;
  }
  if (g_verts != nullptr && t < (shared_v ? N : P)) {
    float v[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < (shared_v ? B : 1); ++b) {
      const float *a = acc + ((long)b * N + t) * S;
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2];
    }
    g_verts[3 * t] = v[0]; g_verts[3 * t + 1] = v[1]; g_verts[3 * t + 2] = v[2];
  }
}

__global__ void __launch_bounds__(256)
fragment_bwd_finish_view_kernel(const float *__restrict__ acc, const int S, const int P, const int N, const int B, const int shared_v,
                                const int shared_s, const int kind, const int C, const long Nattr, float *__restrict__ g_verts,
                                float *__restrict__ g_sigmas, float *__restrict__ g_attr) {
  // acc per Gaussian -- kind 2 (S = 16 | 12): g_mu [0..2], g_A [3..11], w g_rgb [12..15]; kind 1, the per-axis kernel's entries
  // (S = 12 | 8): g_mu [0..2], g_A00 [3], g_A11 [4], g_A22 [5], w g_rgb [6..9]
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  finish_attr_verts(acc, S, P, N, B, shared_v, kind == 1 ? 6 : 12, C, Nattr, g_verts, g_attr, t);
  if (g_sigmas != nullptr && kind == 1 && t < (shared_s ? N : P)) {
    float v[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < (shared_s ? B : 1); ++b) {
      const float *a = acc + ((long)b * N + t) * S + 3;
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2];
    }
    g_sigmas[3 * t] = 2.0f * v[0]; g_sigmas[3 * t + 1] = 2.0f * v[1]; g_sigmas[3 * t + 2] = 2.0f * v[2];
  } else if (g_sigmas != nullptr && t < (shared_s ? N : P)) {
    float v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = 0.f;
    for (int b = 0; b < (shared_s ? B : 1); ++b) {
      const float *a = acc + ((long)b * N + t) * S + 3;
#pragma unroll
      for (int i = 0; i < 9; ++i) v[i] += a[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) g_sigmas[9 * t + i] = 2.0f * v[i];
  }
}

// The oriented form's finishing pass (voge_frame_bwd_ori): kind 2's accumulator, G = the raw 3x3 sums acc[..][3..11] (a shared
// set: its views in a fixed order), through A = R diag(d) R^T backwards -- g_d[k] = r_k^T G r_k (r_k: column k of R), g_s = 2 g_d
// or -2 g_d / s^2, g_R = (G + G^T) R diag(d), g_qh by the derivative of quat_rotation's matrix, g_q = (g_qh - qh (qh . g_qh)) / |q|
// (zero for a quaternion without a usable norm: quat_usable, the record pass' decision).  One thread per Gaussian, R recomputed from
// q; P-sized work, done in fp64 from the fp32 sums (~150 DP operations, a square root and a few divisions per Gaussian: 5.3 us at
// 50 000 Gaussians, where the [3][3] form's finishing pass takes 5.2 -- profiles/r8_oriented_frame.txt; larger sets not measured).
__global__ void __launch_bounds__(256)
fragment_bwd_finish_ori_kernel(const float *__restrict__ acc, const int S, const int P, const int N, const int B, const int shared_v,
                               const int shared_s, const int sigma_mode, const float *__restrict__ scales,
                               const float *__restrict__ quats, const int C, const long Nattr, float *__restrict__ g_verts,
                               float *__restrict__ g_scales, float *__restrict__ g_quats, float *__restrict__ g_attr) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  finish_attr_verts(acc, S, P, N, B, shared_v, 12, C, Nattr, g_verts, g_attr, t);
  if (g_scales == nullptr || t >= (shared_s ? N : P)) return;
  double G[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) G[i] = 0.0;
  for (int b = 0; b < (shared_s ? B : 1); ++b) {
    const float *a = acc + ((long)b * N + t) * S + 3;
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] += (double)a[i];
  }
  const float4 q = reinterpret_cast<const float4 *>(quats)[t];
  double R[9], qh[4], inv;
  const bool ok = quat_usable(q.x, q.y, q.z, q.w);      // (the forward's own fp32 decision)
  quat_rotation<double>(ok, q.x, q.y, q.z, q.w, R, qh, inv);
  double d[3], gR[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = (double)scales[3 * t + k];
    d[k] = sigma_mode == 2 ? 2.0 / s : 2.0 * s;
    double gd = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      // (G + G^T) r_k, row i: g_R[i][k] = d_k * that; g_d[k] = r_k^T G r_k = half of r_k^T (G + G^T) r_k
      const double m = (G[3 * i] + G[i]) * R[k] + (G[3 * i + 1] + G[3 + i]) * R[3 + k] + (G[3 * i + 2] + G[6 + i]) * R[6 + k];
      gR[3 * i + k] = d[k] * m;
      gd += R[3 * i + k] * m;
    }
    gd *= 0.5;
    g_scales[3 * t + k] = (float)(sigma_mode == 2 ? -2.0 * gd / (s * s) : 2.0 * gd);
  }
  const double w = qh[0], x = qh[1], y = qh[2], z = qh[3];
  const double gw = 2.0 * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
  const double gx = 2.0 * (y * gR[1] + z * gR[2] + y * gR[3] - 2.0 * x * gR[4] - w * gR[5] + z * gR[6] + w * gR[7] - 2.0 * x * gR[8]);
  const double gy = 2.0 * (-2.0 * y * gR[0] + x * gR[1] + w * gR[2] + x * gR[3] + z * gR[5] - w * gR[6] + z * gR[7] - 2.0 * y * gR[8]);
  const double gz = 2.0 * (-2.0 * z * gR[0] - w * gR[1] + x * gR[2] + w * gR[3] - 2.0 * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
  const double along = w * gw + x * gx + y * gy + z * gz;
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) out = make_float4((float)((gw - w * along) * inv), (float)((gx - x * along) * inv), (float)((gy - y * along) * inv),
                            (float)((gz - z * along) * inv));
  reinterpret_cast<float4 *>(g_quats)[t] = out;
}

// ---- the host side: eleven entries, each a description (FbCall) handed to the ONE launcher, fb_run ----
namespace {
// What fragment_bwd_kernel is handed.  One kernel serves every form by reusing its operands:
//   shade (SRC 0; the image's gradient, to_colored_background): colors [Nattr,C]; rgb, wsum = the forward's image and weight sums;
//     bg, thr = the background stage; g = g_img with strides (pixel, channel).
//   merge (SRC 0; interpolate_attr): bg = NULL selects it inside the kernel, thr = -1; colors = the attributes; g = g_rgb with
//     strides; wsum = g_wsum | NULL and rgb = NULL -- or, with rgb = the forward's weight sums [pix], wsum = get_silhouette's gradient.
//   weights (SRC 1; their own gradient, any consumer): g = g_weight | NULL with strides (pixel, slot), g_hitlen | NULL; colors = rgb =
//     wsum = bg = NULL, thr = -1, Nattr = 0.
//   depth (SRC 2): rgb = the forward's depth, wsum = its weight sums, g = g_depth | NULL with gs_pix, bg = g_sil | NULL, thr = +1 | -1:
//     normalize on | off; no colors, Nattr = 0.
// act = dsd = NULL (NOAD): both are re-derived from the records.  fb_run sets P and acc, and for merge / weights the constants above.
struct FbArgs {
  const float4 *rec; const float *rays, *colors; const int32_t *idx, *cnt; const float *weight, *act, *len, *dsd, *rgb, *wsum, *bg;
  float thr; const float *g; long gs_pix, gs_c; const float *g_hitlen; float occ; int P; long nrows; int W, K; long Nattr; float *acc;
};
enum FbForm { FB_SHADE, FB_MERGE, FB_WEIGHTS, FB_DEPTH };      // K <= 128 (a lane owns a pair of slots; a pixel's lanes fit one wave);
                                                               // FB_WEIGHTS: K <= VOGE_MAX_K, four slots on a lane (NS = 4) above 128
// The finishing pass, and with it the records and the accumulator acc [P][S] (S floats of sums per Gaussian):
//   FIN_ISO      fragment_bwd_finish_kernel: 16-byte records (ISO), S = 8 | 4 without attributes; g1 = g_sigmas [.., 1], p1 = sigmas
//                (read for mode = sigma_mode 2), one `shared` flag for both gradients.
//   FIN_GENERAL  fragment_bwd_finish_general_kernel: the records are packed HERE from (mus, p1 = isigmas) into the workspace -- 48
//                bytes each at offset 0, acc behind them, zeroed by the same launch; S = 16 | 12; g1 = g_isigmas [P, 9].
//   FIN_VIEW     fragment_bwd_finish_view_kernel: the frame's packed records, mode = kind: 2 as FIN_GENERAL, 1 per-axis records (DIAG:
//                no act / dsd, S = 12 | 8, g1 [.., 3]).
//   FIN_ORI      fragment_bwd_finish_ori_kernel: kind 2's records and accumulator; p1 = scales, quats, mode = sigma_mode, g1 =
//                g_scales [.., 3], g_quats [.., 4].
enum FbFinish { FIN_ISO, FIN_GENERAL, FIN_VIEW, FIN_ORI };
struct FbCall {
  FbForm form; FbFinish fin; FbArgs k; int B, N, C;      // (the general forms: B = 1, N = P)
  void *ws; size_t ws_bytes;      // the workspace | the accumulator
  bool zero_here;                 // false: acc arrives zeroed (the frame entries, acc_is_zero)
  float *g0, *g1, *g_attr;        // the gradients of the means, of the second parameter, of the attributes [Nattr, C]
  const float *p1 = nullptr; int shared_v = 0, shared_s = 0, mode = 0; const float *mus = nullptr, *quats = nullptr; float *g_quats = nullptr;
};
const float4 *fb_rec(const float *records) { return reinterpret_cast<const float4 *>(records); }

template <int SRC, int C, int NS, bool ISO, bool NOAD, bool DIAG>
void fb_launch(const FbArgs &a, hipStream_t st) {
  const long blocks = (long)((a.W + kFbGW - 1) / kFbGW) * ((a.nrows + kFbGH - 1) / kFbGH);
  // (the kernel's gathers are unconditional at clamped ids: row 0 of the records (P >= 1 here) and of the colour table must be
  //  readable.  An empty colour table reads its dropped row out of the records instead.)
  const float *colors = (a.Nattr > 0 && a.colors != nullptr) ? a.colors : reinterpret_cast<const float *>(a.rec);
  auto launch = [&](auto off) {
    hipLaunchKernelGGL((fragment_bwd_kernel<SRC, C, NS, decltype(off), ISO, NOAD, DIAG>), dim3((unsigned)blocks), dim3(64), 0, st, a.rec,
                       a.rays, colors, a.idx, a.cnt, a.weight, a.act, a.len, a.dsd, a.rgb, a.wsum, a.bg, a.thr, a.g, a.gs_pix, a.gs_c,
                       a.g_hitlen, a.occ, a.P, a.nrows, a.W, a.K, a.Nattr, a.acc);
  };
  // The 32-bit form where every byte offset formed in OffT fits: per pixel the slot arrays take 4 K bytes, the ray 12, the shade
  // form's rgb 4 C (addressed through OffT only with a background), cnt / wsum / bg 4.  (4 K alone is not enough: with K <= 2 --
  // and K = 3 with C = 4 -- a launch under 2^30 slots has pixels whose ray or rgb offset is past 2^32.)
  long per_pix = a.K >= 3 ? 4l * a.K : 12l;
  if (SRC == 0 && a.bg != nullptr && 4l * C > per_pix) per_pix = 4l * C;
  if ((double)a.nrows * a.W * (double)per_pix < 4294967296.0) launch(uint32_t{}); else launch(size_t{});
}
// The instantiations are the ones listed here and no product of the parameters: depth has one form, DIAG one (ISO, NOAD) pair.
template <int SRC, int C, int NS>
void fb_launch_form(const FbArgs &a, const bool iso, const bool diag, hipStream_t st) {
  if constexpr (SRC == 2) fb_launch<2, 0, 2, true, true, false>(a, st);
  else if (diag) fb_launch<SRC, C, NS, false, true, true>(a, st);
  else if (iso) { if (a.act == nullptr) fb_launch<SRC, C, NS, true, true, false>(a, st); else fb_launch<SRC, C, NS, true, false, false>(a, st); }
  else { if (a.act == nullptr) fb_launch<SRC, C, NS, false, true, false>(a, st); else fb_launch<SRC, C, NS, false, false, false>(a, st); }
}
void fb_dispatch(const FbArgs &a, const FbForm form, const int C, const bool iso, const bool diag, hipStream_t st) {
  if (form == FB_DEPTH) fb_launch_form<2, 0, 2>(a, iso, diag, st);
  else if (form == FB_WEIGHTS) { if (a.K <= 128) fb_launch_form<1, 0, 2>(a, iso, diag, st); else fb_launch_form<1, 0, 4>(a, iso, diag, st); }
  else switch (C) {
    case 1: fb_launch_form<0, 1, 2>(a, iso, diag, st); break;
    case 2: fb_launch_form<0, 2, 2>(a, iso, diag, st); break;
    case 3: fb_launch_form<0, 3, 2>(a, iso, diag, st); break;
    default: fb_launch_form<0, 4, 2>(a, iso, diag, st); break;
  }
}

// validate -> empty case -> accumulator -> the fused kernel -> the finishing pass.  The order of the refusals is part of the ABI:
// sizes (-1), K (-3), the empty case (0), pointers (-1), the workspace (-2), the 32-bit offsets (-1).
int fb_run(FbCall c, voge_stream_t stream) {
  FbArgs &k = c.k;
  hipStream_t st = (hipStream_t)stream;
  const bool attr = c.form <= FB_MERGE, iso = c.fin == FIN_ISO, pack = c.fin == FIN_GENERAL, diag = c.fin == FIN_VIEW && c.mode == 1;
  if (c.B < 0 || c.N < 0 || k.nrows < 0 || k.W < 0 || k.K <= 0 || k.Nattr < 0 || (attr && (c.C <= 0 || c.C > 4)) ||
      (iso && (c.mode < 0 || c.mode > 2)))
    return VOGE_ERR_BAD_ARG;
  if (k.K > (c.form == FB_WEIGHTS ? VOGE_MAX_K : 128)) return VOGE_ERR_K_TOO_LARGE;
  const int P = k.P = c.B * c.N, C = attr ? c.C : 0;
  if (!attr) k.Nattr = 0;
  if (c.form != FB_WEIGHTS) k.g_hitlen = nullptr;
  if (c.form == FB_MERGE || c.form == FB_WEIGHTS) { k.bg = nullptr; k.thr = -1.0f; }
  if (c.form == FB_WEIGHTS) k.colors = k.rgb = k.wsum = nullptr;
  float *g_attr = attr ? c.g_attr : nullptr;
  // Three asymmetries between the entries, kept as they grew:
  //  (1) the weights' and the depth entries of their own (not voge_frame_bwd_gen's form 2) insist on both outputs -- unless there is
  //      no Gaussian to write to -- and zero them in the empty case; the others allow both to be NULL;
  const bool own = !attr && c.fin <= FIN_GENERAL;
  const long nv = c.shared_v ? c.N : P, ns = c.shared_s ? c.N : P;
  if (own && nv == 0) return 0;
  if (own && (!c.g0 || !c.g1)) return VOGE_ERR_BAD_ARG;
  if (P == 0 || k.nrows * k.W == 0) {      // nothing was traced: zero gradients
    hipError_t e = hipSuccess;
    auto zero = [&](float *p, const long n) { if (e == hipSuccess && p && n > 0) e = voge_fill_async(p, 0, sizeof(float) * (size_t)n, st); };
    //  (2) the attribute forms outside the frame's general entries zero only g_attr here and leave g0 / g1 unwritten;
    if (own || c.fin >= FIN_VIEW) { zero(c.g0, 3 * nv); zero(c.g1, ns * (iso ? 1 : (diag || c.fin == FIN_ORI) ? 3 : 9)); zero(c.g_quats, 4 * ns); }
    zero(g_attr, k.Nattr * C);
    return (int)e;
  }
  if (!(pack ? c.mus && c.p1 : k.rec != nullptr) || !k.rays || !k.idx || !k.cnt || !k.weight || !k.len || !c.ws) return VOGE_ERR_BAD_ARG;
  if (attr && (!k.colors || !k.g)) return VOGE_ERR_BAD_ARG;
  if (c.form == FB_SHADE && (!k.rgb || !k.wsum || !k.bg)) return VOGE_ERR_BAD_ARG;
  if (c.form == FB_DEPTH && (!k.rgb || !k.wsum || (!k.g && !k.bg))) return VOGE_ERR_BAD_ARG;
  if ((k.act == nullptr) != (k.dsd == nullptr) || (diag && k.act)) return VOGE_ERR_BAD_ARG;      // both or neither; per-axis records keep neither
  if ((c.g0 == nullptr) != (c.g1 == nullptr) || (iso && c.mode == 2 && c.g1 && !c.p1)) return VOGE_ERR_BAD_ARG;
  const int S = iso ? (attr ? 8 : 4) : (diag ? 8 : 12) + (attr ? 4 : 0);
  //  (3) the packing forms ask for the 112 bytes per Gaussian of voge_fragment_bwd_workspace_bytes, with and without attributes; the
  //      others for the accumulator they use.
  const size_t acc_bytes = (size_t)P * S * 4;
  if (c.ws_bytes < (pack ? voge_fragment_bwd_workspace_bytes(P) : acc_bytes)) return VOGE_ERR_WORKSPACE;
  if (P >= (1 << 26) || (attr && k.Nattr * C >= (1l << 30))) return VOGE_ERR_BAD_ARG;      // 32-bit byte offsets of the gathers
  k.acc = reinterpret_cast<float *>(c.ws);
  if (pack) {
    float4 *rec = reinterpret_cast<float4 *>(c.ws);
    k.rec = rec;
    k.acc += (size_t)P * 12;
    hipLaunchKernelGGL(fragment_bwd_pack_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, c.mus, c.p1, P, rec,
                       reinterpret_cast<float4 *>(k.acc), S / 4);
  } else if (c.zero_here) {
    const hipError_t e = voge_fill_async(k.acc, 0, acc_bytes, st);
    if (e != hipSuccess) return (int)e;
  }
  fb_dispatch(k, c.form, C, iso, diag, st);
  const long n_fin = (k.Nattr > P) ? k.Nattr : P;
  const dim3 grid((unsigned)(((pack ? 16 : 1) * n_fin + 255) / 256)), block(256);
  switch (c.fin) {
    case FIN_ISO:
      hipLaunchKernelGGL(fragment_bwd_finish_kernel, grid, block, 0, st, k.acc, S, c.p1, P, c.N, c.B, IsoView{nullptr, c.shared_v ? 1 : 0, c.mode},
                         C, k.Nattr, c.g0, c.g1, g_attr);
      break;
    case FIN_GENERAL:
      hipLaunchKernelGGL(fragment_bwd_finish_general_kernel, grid, block, 0, st, k.acc, S, P, C, k.Nattr, c.g0, c.g1, g_attr);
      break;
    case FIN_VIEW:
      hipLaunchKernelGGL(fragment_bwd_finish_view_kernel, grid, block, 0, st, k.acc, S, P, c.N, c.B, c.shared_v ? 1 : 0, c.shared_s ? 1 : 0,
                         c.mode, C, k.Nattr, c.g0, c.g1, g_attr);
      break;
    case FIN_ORI:
      hipLaunchKernelGGL(fragment_bwd_finish_ori_kernel, grid, block, 0, st, k.acc, S, P, c.N, c.B, c.shared_v ? 1 : 0, c.shared_s ? 1 : 0,
                         c.mode, c.p1, c.quats, C, k.Nattr, c.g0, c.g1, c.g_quats, g_attr);
      break;
  }
  return launch_status();
}
}  // namespace

// ---- the record (_iso) forms: the image's gradient; interpolate_attr's (+ get_silhouette's); the weights' own ----
extern "C" int voge_fragment_shade_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                           const float *rays, const float *colors, const int32_t *idx, const int32_t *cnt,
                                           const float *weight, const float *act, const float *len, const float *dsd,
                                           const float *rgb, const float *wsum, const float *bg, float thr,
                                           const float *g_img, long g_stride_pix, long g_stride_c, float occ, int B, int N,
                                           long nrows, int W, int K, int C, long Nattr, void *workspace, size_t workspace_bytes, float *g_verts,
                                           float *g_sigmas, float *g_colors, voge_stream_t stream) {
  return fb_run({FB_SHADE, FIN_ISO, {fb_rec(records), rays, colors, idx, cnt, weight, act, len, dsd, rgb, wsum, bg, thr, g_img, g_stride_pix,
                                     g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, workspace, workspace_bytes, true, g_verts, g_sigmas, g_colors, sigmas, shared, shared, sigma_mode}, stream);
}

extern "C" int voge_fragment_merge_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                           const float *rays, const float *attr, const int32_t *idx, const int32_t *cnt,
                                           const float *weight, const float *act, const float *len, const float *dsd,
                                           const float *g_rgb, long g_stride_pix, long g_stride_c, const float *g_wsum,
                                           float occ, int B, int N, long nrows, int W, int K, int C, long Nattr,
                                           void *workspace, size_t workspace_bytes, float *g_verts, float *g_sigmas,
                                           float *g_attr, voge_stream_t stream) {
  return fb_run({FB_MERGE, FIN_ISO, {fb_rec(records), rays, attr, idx, cnt, weight, act, len, dsd, nullptr, g_wsum, nullptr, -1.0f, g_rgb,
                                     g_stride_pix, g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, workspace, workspace_bytes, true, g_verts, g_sigmas, g_attr, sigmas, shared, shared, sigma_mode}, stream);
}

extern "C" int voge_fragment_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode, const float *rays,
                                     const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                                     const float *len, const float *dsd, const float *g_weight, long gw_stride_pix,
                                     long gw_stride_k, const float *g_hitlen, float occ, int B, int N, long nrows, int W, int K,
                                     void *workspace, size_t workspace_bytes, float *g_verts, float *g_sigmas,
                                     voge_stream_t stream) {
  return fb_run({FB_WEIGHTS, FIN_ISO, {fb_rec(records), rays, nullptr, idx, cnt, weight, act, len, dsd, nullptr, nullptr, nullptr, -1.0f,
                                       g_weight, gw_stride_pix, gw_stride_k, g_hitlen, occ, 0, nrows, W, K, 0, nullptr},
                 B, N, 0, workspace, workspace_bytes, true, g_verts, g_sigmas, nullptr, sigmas, shared, shared, sigma_mode}, stream);
}

// ---- the frame path: the record forms on the accumulator that the frame's forward zeroed (no fill launch, no act / dsd) ----
extern "C" int voge_frame_shade_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                        const float *rays, const float *colors, const int32_t *idx, const int32_t *cnt,
                                        const float *weight, const float *len, const float *rgb, const float *wsum,
                                        const float *bg, float thr, const float *g_img, long g_stride_pix, long g_stride_c,
                                        float occ, int B, int N, long nrows, int W, int K, int C, long Nattr, void *acc_zeroed,
                                        size_t acc_bytes, float *g_verts, float *g_sigmas, float *g_colors, voge_stream_t stream) {
  return fb_run({FB_SHADE, FIN_ISO, {fb_rec(records), rays, colors, idx, cnt, weight, nullptr, len, nullptr, rgb, wsum, bg, thr, g_img,
                                     g_stride_pix, g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, acc_zeroed, acc_bytes, false, g_verts, g_sigmas, g_colors, sigmas, shared, shared, sigma_mode}, stream);
}

extern "C" int voge_frame_merge_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode,
                                        const float *rays, const float *attr, const int32_t *idx, const int32_t *cnt,
                                        const float *weight, const float *len, const float *g_rgb, long g_stride_pix,
                                        long g_stride_c, const float *g_wsum, const float *wsum_fwd, float occ, int B, int N, long nrows,
                                        int W, int K, int C, long Nattr, void *acc_zeroed, size_t acc_bytes, float *g_verts,
                                        float *g_sigmas, float *g_attr, voge_stream_t stream) {
  return fb_run({FB_MERGE, FIN_ISO, {fb_rec(records), rays, attr, idx, cnt, weight, nullptr, len, nullptr, wsum_fwd, g_wsum, nullptr, -1.0f,
                                     g_rgb, g_stride_pix, g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, acc_zeroed, acc_bytes, false, g_verts, g_sigmas, g_attr, sigmas, shared, shared, sigma_mode}, stream);
}

// get_depth's backward (extension): the two per-pixel scalars are formed inside the kernel; four sums per Gaussian (g_mu, g_a).
extern "C" int voge_frame_depth_bwd_iso(const float *records, const float *sigmas, int shared, int sigma_mode, const float *rays,
                                        const int32_t *idx, const int32_t *cnt, const float *weight, const float *len,
                                        const float *depth, const float *wsum, const float *g_depth, long g_stride_pix,
                                        const float *g_sil, int normalize, float occ, int B, int N, long nrows, int W, int K,
                                        void *acc_zeroed, size_t acc_bytes, float *g_verts, float *g_sigmas, voge_stream_t stream) {
  if (g_stride_pix < 0) return VOGE_ERR_BAD_ARG;
  return fb_run({FB_DEPTH, FIN_ISO, {fb_rec(records), rays, nullptr, idx, cnt, weight, nullptr, len, nullptr, depth, wsum, g_sil,
                                     normalize ? 1.0f : -1.0f, g_depth, g_stride_pix, 0, nullptr, occ, 0, nrows, W, K, 0, nullptr},
                 B, N, 0, acc_zeroed, acc_bytes, false, g_verts, g_sigmas, nullptr, sigmas, shared, shared, sigma_mode}, stream);
}

// Every backward route of fragments made by voge_frame_trace_fwd_gen -- form 0: shade, 1: merge, 2: the weights' own (C, Nattr and
// g_attr unused) -- on the packed (mu, A) records of the forward (no pack launch); acc is zeroed here unless acc_is_zero (the
// frame's composite did it on its way).
extern "C" int voge_frame_bwd_gen(int form, const float *records, int shared_verts, int shared_sigmas, int kind, const float *rays,
                                  const float *attr, const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                                  const float *len, const float *dsd, const float *rgb, const float *wsum, const float *bg, float thr,
                                  const float *g, long g_stride0, long g_stride1, const float *g_hitlen, float occ, int B, int N,
                                  long nrows, int W, int K, int C, long Nattr, void *acc, size_t acc_bytes, int acc_is_zero,
                                  float *g_verts, float *g_sigmas, float *g_attr, voge_stream_t stream) {
  if (form < 0 || form > 2 || (kind != 1 && kind != 2)) return VOGE_ERR_BAD_ARG;
  return fb_run({(FbForm)form, FIN_VIEW, {fb_rec(records), rays, attr, idx, cnt, weight, act, len, dsd, rgb, wsum, bg, thr, g, g_stride0,
                                          g_stride1, g_hitlen, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, acc, acc_bytes, !acc_is_zero, g_verts, g_sigmas, g_attr, nullptr, shared_verts, shared_sigmas, kind}, stream);
}

// Every backward route of fragments made by voge_frame_trace_fwd_ori: voge_frame_bwd_gen(kind 2)'s fused kernel as it is, on the
// same records and accumulator (voge_frame_bwd_gen_acc_bytes), then the oriented finishing pass -- the gradients of verts, scales
// and quats as the user holds them, in place of the [3][3] gradient and autograd through R diag(s) R^T composed in torch.
extern "C" int voge_frame_bwd_ori(int form, const float *records, const float *scales, const float *quats, int shared_verts,
                                  int shared_sigmas, int sigma_mode, const float *rays, const float *attr, const int32_t *idx,
                                  const int32_t *cnt, const float *weight, const float *act, const float *len, const float *dsd,
                                  const float *rgb, const float *wsum, const float *bg, float thr, const float *g, long g_stride0,
                                  long g_stride1, const float *g_hitlen, float occ, int B, int N, long nrows, int W, int K, int C,
                                  long Nattr, void *acc, size_t acc_bytes, int acc_is_zero, float *g_verts, float *g_scales,
                                  float *g_quats, float *g_attr, voge_stream_t stream) {
  if (form < 0 || form > 2 || (sigma_mode != 1 && sigma_mode != 2) || (g_scales == nullptr) != (g_quats == nullptr)) return VOGE_ERR_BAD_ARG;
  if (g_scales != nullptr && (long)B * N > 0 &&      // (the finishing pass reads and writes the quaternions as float4)
      (!scales || !quats || ((reinterpret_cast<uintptr_t>(quats) | reinterpret_cast<uintptr_t>(g_quats)) & 15) != 0))
    return VOGE_ERR_BAD_ARG;
  return fb_run({(FbForm)form, FIN_ORI, {fb_rec(records), rays, attr, idx, cnt, weight, act, len, dsd, rgb, wsum, bg, thr, g, g_stride0,
                                         g_stride1, g_hitlen, occ, 0, nrows, W, K, Nattr, nullptr},
                 B, N, C, acc, acc_bytes, !acc_is_zero, g_verts, g_scales, g_attr, scales, shared_verts, shared_sigmas, sigma_mode, nullptr,
                 quats, g_quats}, stream);
}

// ---- the general 3x3 forms: the records are packed here from (mus, isigmas) ----
extern "C" int voge_fragment_shade_bwd(const float *mus, const float *isigmas, const float *rays, const float *colors,
                                       const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                                       const float *len, const float *dsd, const float *rgb, const float *wsum,
                                       const float *bg, float thr, const float *g_img, long g_stride_pix, long g_stride_c,
                                       float occ, int P, long nrows, int W, int K, int C, long Nattr, void *workspace,
                                       size_t workspace_bytes, float *g_mus, float *g_isigmas, float *g_colors,
                                       voge_stream_t stream) {
  return fb_run({FB_SHADE, FIN_GENERAL, {nullptr, rays, colors, idx, cnt, weight, act, len, dsd, rgb, wsum, bg, thr, g_img, g_stride_pix,
                                         g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 1, P, C, workspace, workspace_bytes, true, g_mus, g_isigmas, g_colors, isigmas, 0, 0, 0, mus}, stream);
}

extern "C" int voge_fragment_merge_bwd(const float *mus, const float *isigmas, const float *rays, const float *attr,
                                       const int32_t *idx, const int32_t *cnt, const float *weight, const float *act,
                                       const float *len, const float *dsd, const float *g_rgb, long g_stride_pix,
                                       long g_stride_c, const float *g_wsum, float occ, int P, long nrows, int W, int K, int C,
                                       long Nattr, void *workspace, size_t workspace_bytes, float *g_mus, float *g_isigmas,
                                       float *g_attr, voge_stream_t stream) {
  return fb_run({FB_MERGE, FIN_GENERAL, {nullptr, rays, attr, idx, cnt, weight, act, len, dsd, nullptr, g_wsum, nullptr, -1.0f, g_rgb,
                                         g_stride_pix, g_stride_c, nullptr, occ, 0, nrows, W, K, Nattr, nullptr},
                 1, P, C, workspace, workspace_bytes, true, g_mus, g_isigmas, g_attr, isigmas, 0, 0, 0, mus}, stream);
}

extern "C" int voge_fragment_bwd(const float *mus, const float *isigmas, const float *rays, const int32_t *idx,
                                 const int32_t *cnt, const float *weight, const float *act, const float *len,
                                 const float *dsd, const float *g_weight, long gw_stride_pix, long gw_stride_k,
                                 const float *g_hitlen, float occ, int P, long nrows, int W, int K, void *workspace,
                                 size_t workspace_bytes, float *g_mus, float *g_isigmas, voge_stream_t stream) {
  return fb_run({FB_WEIGHTS, FIN_GENERAL, {nullptr, rays, nullptr, idx, cnt, weight, act, len, dsd, nullptr, nullptr, nullptr, -1.0f,
                                           g_weight, gw_stride_pix, gw_stride_k, g_hitlen, occ, 0, nrows, W, K, 0, nullptr},
                 1, P, 0, workspace, workspace_bytes, true, g_mus, g_isigmas, nullptr, isigmas, 0, 0, 0, mus}, stream);
}

