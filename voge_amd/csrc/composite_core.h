// Shared pieces of the depth-ordered compositing (VoGE/Aggregation.py:30-107): constants, the erfc / Gaussian
// evaluators, the LDS row layout, and the forward row pass of the lane-owns-NS-slots form.  Used by composite.hip
// (voge_composite_fwd / _bwd) and fragment_bwd.hip; sweep_iso.h takes pk_fma and splat from here.  (Round 3's sweep once
// composited inside its epilogue through this header -- measured and not used, HISTORY.md §5; that epilogue is gone.)
#pragma once
#include "voge_common.h"

namespace voge {

typedef float v2f __attribute__((ext_vector_type(2)));

// hardware exp2 / sqrt: ~1-2 ulp, far inside the 1e-4 parity tolerance; the libm versions cost
// ~35 VALU instructions per lane in a VALU-bound kernel
#define FAST_EXP(x) __builtin_amdgcn_exp2f((x) * 1.4426950408889634f)
#define FAST_SQRT(x) __builtin_amdgcn_sqrtf(x)

#ifndef VOGE_COMP_MAXT
#define VOGE_COMP_MAXT 256
#endif
constexpr int kCompThreads = VOGE_COMP_MAXT;
constexpr float kInvNorm = 1.6487212707001282f;  // 1 / exp(-0.5), Aggregation.py:79
constexpr float kRsqrtPi = 0.5641895835477563f;
#ifndef VOGE_KSAT
#define VOGE_KSAT 3.5f
#endif
constexpr float kSat = VOGE_KSAT;                // erfc(3.5)/2 = 3.7e-7, below the fp32 rounding of S ~ O(1..K)
constexpr float kCs = 1.2011224087864498f;       // sqrt(log2 e): x' = x * kCs, exp(-x^2) = 2^(-x'^2)
constexpr float kBig = 3.0e38f;

// log2(erfc(x)/2) as a polynomial in x' = x sqrt(log2 e) on [0, 5 sqrt(log2 e)], weighted minimax
// on the absolute error of 2^Q (tools/fit_erfc.py).  Degree 5: |err| <= 6.0e-7 in the fp32 Horner
// evaluation (degree 6: 1.5e-7, degree 8: 5.2e-8; DESIGN.md §8 has the table).  The leading coefficient
// is NEGATIVE, so Q keeps falling past the fitted range: 2^Q is finite and non-increasing for every
// fp32 x' >= 5 sqrt(log2 e), at most 3.6e-13 there, and exactly 0 at +inf (kQ5 * inf = -inf, and
// -inf * x' + c stays -inf: no inf - inf can arise for x' >= 0).  So h_pair needs NO clamp of x' --
// the even degrees' positive leading coefficient made 2^Q diverge out there and cost two v_min_f32
// and a sixth packed FMA per pair.  Every caller of h_pair passes x' >= 0 and never a NaN: the
// sorted walks and diagonal blocks by sortedness (a NaN len marks the pixel unsorted), sentinel
// rows of +/-kBig give a huge finite x' or +inf, dead columns x' = 0 (tests/test_erfc_fit_cpu.py).
constexpr float kQ0 = -1.000001669e+00f, kQ1 = -1.355278134e+00f, kQ2 = -6.367735267e-01f,
                kQ3 = -8.563093096e-02f, kQ4 = 1.412141882e-02f, kQ5 = -1.158451778e-03f;

__device__ __forceinline__ v2f pk_fma(const v2f a, const v2f b, const v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f splat(const float x) { return (v2f){x, x}; }

// h(x') = erfc(x'/kCs)/2 for any x' in [0, +inf], two at a time: five packed FMAs and two exp2
__device__ __forceinline__ v2f h_pair(const v2f xp) {
  v2f q = pk_fma(splat(kQ5), xp, splat(kQ4));
  q = pk_fma(q, xp, splat(kQ3));
  q = pk_fma(q, xp, splat(kQ2));
  q = pk_fma(q, xp, splat(kQ1));
  q = pk_fma(q, xp, splat(kQ0));
  return (v2f){__builtin_amdgcn_exp2f(q.x), __builtin_amdgcn_exp2f(q.y)};
}
// The cold paths' evaluator (an unsorted list's full K x K scans): one value, and any input at all -- fminf
// turns a NaN into the cap, so a NaN len gives h(5) = 7.7e-13 as it always has.  These paths are not
// instruction bound; they keep the clamped degree-6 fit (|err| <= 1.5e-7, positive leading coefficient)
// they have had since the walks were written, bit for bit.
constexpr float kC0 = -9.999997020e-01f, kC1 = -1.355341077e+00f, kC2 = -6.364040971e-01f,
                kC3 = -8.642258495e-02f, kC4 = 1.487037074e-02f, kC5 = -1.475012978e-03f,
                kC6 = 4.851150516e-05f;
constexpr float kColdCap = 5.0f * kCs;           // that fit's range
__device__ __forceinline__ float h_one(const float xp) {
  const float x = fminf(xp, kColdCap);
  float q = fmaf(kC6, x, kC5);
  q = fmaf(q, x, kC4);
  q = fmaf(q, x, kC3);
  q = fmaf(q, x, kC2);
  q = fmaf(q, x, kC1);
  q = fmaf(q, x, kC0);
  return __builtin_amdgcn_exp2f(q);
}
// 2^(-x'^2) = exp(-x^2), two at a time
__device__ __forceinline__ v2f gauss_pair(const v2f xp) {
  const v2f q = -(xp * xp);
  return (v2f){__builtin_amdgcn_exp2f(q.x), __builtin_amdgcn_exp2f(q.y)};
}
// entries (e, e+1), e even: one 8-byte LDS read
__device__ __forceinline__ v2f ld2(const float *a, const int e) { return *reinterpret_cast<const v2f *>(a + e); }
__device__ __forceinline__ v2f abs2(const v2f v) { return (v2f){fabsf(v.x), fabsf(v.y)}; }

// Element at a BYTE offset from a base pointer.  With a 32-bit unsigned offset the compiler emits the scalar-base form
// (global_load v, voff, s[base:base+1]) and keeps the address arithmetic off the vector unit; kernels take the offset
// type as a template parameter and the host picks uint32_t when every byte offset of the launch fits.
template <typename T, typename OffT>
__device__ __forceinline__ const T &at_bytes(const void *base, const OffT byte_off) {
  return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}
template <typename T, typename OffT>
__device__ __forceinline__ T &at_bytes_w(void *base, const OffT byte_off) {
  return *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off);
}

// Row stride of the padded per-pixel arrays: two sentinels, K entries, two or three sentinels.
// PAD (two sentinel entries) and the stride are even: an entry's parity is its slot's parity and the
// pairs (2t, 2t+1) of a row are 8-byte aligned (ds_read_b64: 2 LDS cycles per wave; ds_read2_b32 of an odd pair costs 4).
__host__ __device__ constexpr int comp_pad(const int K) { return 2; }
__host__ __device__ constexpr int comp_row_stride(const int K) { return ((K + 1) & ~1) + 2 * comp_pad(K); }

__host__ __device__ inline int compn_lanes(const int K, const int NS) { return (K + NS - 1) / NS; }
__host__ __device__ inline int compn_stride(const int K, const int NS) { return compn_lanes(K, NS) * NS + 2 * comp_pad(K); }
// pixels a workgroup of `threads` lanes holds: workgroup form = threads / LP, wave form = (threads / 64) * (64 / LP)
__host__ __device__ inline int compn_pixels(const int K, const int NS, const int threads, const bool wave) {
  const int lp = compn_lanes(K, NS);
  return wave ? (threads / 64) * (64 / lp) : threads / lp;
}
__host__ __device__ inline int compn_rows(const int K, const int NS, const int threads, const bool wave) {
  return (compn_pixels(K, NS, threads, wave) * compn_stride(K, NS) + 3) & ~3;
}
// Forward row pass, wave form: the pixel's lanes (LP = ceil(K / NS) of them, lane q owns slots [NS q, NS q + NS))
// sit inside ONE wave, the pixel's padded (len, s', E) rows are in LDS (row origin of this lane's group: d0, an even
// index) and visible to the wave.  lm / sm / em: the lane's own len, s = sqrt(dsd + 1e-10), E = exp(-act) (E = 0 for
// an empty slot).  `sorted`: the pixel's list is depth ordered (the windowed walk); otherwise every column is visited.
// LP, q, seg_lo, d0, k0, K are PER-LANE values (pixels of different lane counts may share a wave: the packed kernels);
// LPmax is a wave-uniform upper bound of LP (the trip count of the scans).  LP and seg_lo are no longer read here (the
// column walks need no pixel-wide window radius); the callers, round 3's sweep among them, still pass them.
// Returns the weights of the lane's slots.  The association of the scans is a function of the lane's index in the
// pixel only, so a pixel's result does not depend on where it sits (row bands == whole frame, fused == stand-alone).
template <int NS>
__device__ __forceinline__ void compn_fwd_rows(const float (&lm)[NS], const float (&sm)[NS], const float (&em)[NS],
                                               const float *Llen, const float *Lsp, const float *LE, const int d0,
                                               const int k0, const int K, const int q, const int LP, const int LPmax,
                                               const bool in_wg, const bool active, const bool sorted, const int seg_lo,
                                               const float occ, float (&w)[NS]) {
  float sp[NS];
#pragma unroll
  for (int a = 0; a < NS; ++a) sp[a] = sm[a] * kCs;
  float esum = 0.0f;
#pragma unroll
  for (int a = 0; a < NS; ++a) esum += em[a];
  // Exclusive prefix (over the lanes of the pixel) of the per-lane sums of E, Hillis-Steele on wave shuffles (no pixel-wide
  // window radius rides along: a column walk goes as far as its own columns reach)
  float ex;
  {
    const float y = __shfl_up(esum, 1, 64);
    float x = (q > 0 && in_wg) ? y : 0.0f;
    for (int o = 1; o < LPmax; o <<= 1) {
      const float z = __shfl_up(x, o, 64);
      if (q >= o && in_wg) x += z;
    }
    ex = x;
  }
  bool any_e = false;
#pragma unroll
  for (int a = 0; a < NS; ++a) any_e = any_e || (em[a] != 0.0f);
  const float h0 = __builtin_amdgcn_exp2f(kQ0);      // h(0), exactly what h_pair(0) returns
  float S[NS];
#pragma unroll
  for (int a = 0; a < NS; ++a) S[a] = 0.0f;
  if (any_e && sorted) {
    v2f accF[NS], accB[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) { accF[a] = splat(0.0f); accB[a] = splat(0.0f); }
    // diagonal block (registers): for rows a < b, column b is behind row a and column a in front of row b
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      accF[a].x = em[a] * h0;         // self
#pragma unroll
      for (int b2 = a + 1; b2 < NS; ++b2) {
        const float gap = lm[b2] - lm[a];
        const v2f xp = (v2f){gap * sp[b2], gap * sp[a]};                 // (row a, col b), (row b, col a)
        const v2f h = h_pair(xp);
        accB[a].y = fmaf(em[b2], h.x, accB[a].y);
        accF[b2].y = fmaf(em[a], h.y, accF[b2].y);
      }
    }
    // Column walks (round 6): the lane walks the ROWS around its own columns, each as far as that column's own window
    // kSat / s_j reaches, and adds -E_j h (row behind: the column is in front of it) / +E_j h (row in front) to the row's cell
    // of LR -- the pixel's s' row, which a sorted pixel's walks no longer read: a lane's own s' and E are in its registers.
    // Row walks went as far as the pixel's WIDEST window for every column (HISTORY.md R6).  Read - add - write as in
    // compn_bwd_wave: in one iteration the lanes of a wave address different row pairs.
    float *const LR = const_cast<float *>(Lsp);
    float reachB = -kBig, reachF = kBig, lmS[NS], spS[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      const bool live = em[a] != 0.0f;
      const float r = kSat * __builtin_amdgcn_rcpf(sm[a]);
      reachB = live ? fmaxf(reachB, lm[a] + r) : reachB;
      reachF = live ? fminf(reachF, lm[a] - r) : reachF;
      lmS[a] = live ? lm[a] : 0.0f; spS[a] = live ? sp[a] : 0.0f;      // (an empty column: x = 0, E = 0 -- nothing, and nothing non-finite)
    }
#pragma unroll
    for (int a = 0; a < NS; a += 2) *reinterpret_cast<v2f *>(LR + d0 + a) = splat(0.0f);
    wave_lds_sync();
    for (int e = d0 + NS;; e += 2) {     // row pairs behind the own columns
      const v2f l2 = ld2(Llen, e);
      if (!(l2.x < reachB)) break;
      v2f racc = ld2(LR, e);
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const v2f xa = (l2 - splat(lmS[a])) * splat(spS[a]);
        racc = pk_fma(splat(-em[a]), h_pair(xa), racc);
      }
      *reinterpret_cast<v2f *>(LR + e) = racc;
      wave_lds_sync();
    }
    for (int e = d0 - 2;; e -= 2) {      // row pairs in front of the own columns
      const v2f l2 = ld2(Llen, e);
      if (!(l2.y > reachF)) break;
      v2f racc = ld2(LR, e);
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const v2f xa = (splat(lmS[a]) - l2) * splat(spS[a]);
        racc = pk_fma(splat(em[a]), h_pair(xa), racc);
      }
      *reinterpret_cast<v2f *>(LR + e) = racc;
      wave_lds_sync();
    }
    wave_lds_sync();      // (every column walk of the pixel has passed: its lanes share this wave)
    float pre = ex;
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      pre += em[a];                                                     // inclusive prefix sum of E
      S[a] = ((pre - (accF[a].x + accF[a].y)) + (accB[a].x + accB[a].y)) + *lds_volatile(LR + d0 + a);
    }
  } else if (any_e && active) {          // unsorted list: every column, signs from the data
    const int r0 = d0 - k0;
    for (int j = 0; j < K; ++j) {
      const float Ej = LE[r0 + j];
      if (Ej == 0.0f) continue;
      const float lj = Llen[r0 + j], sj = Lsp[r0 + j];
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const float xp = (lm[a] - lj) * sj;
        const float h = h_one(fabsf(xp));
        S[a] = fmaf(Ej, xp >= 0.0f ? 1.0f - h : h, S[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NS; ++a) w[a] = (em[a] != 0.0f) ? FAST_EXP(-occ * S[a]) * em[a] * kInvNorm : 0.0f;
}

// -DVOGE_FB_TIMES builds: lane utilisation of the window loops (tools/fb_sections.py).  Per workgroup (= wave) row:
// [0] row-loop iterations x 64, [1] lanes active in them, [2] column-loop iterations x 64, [3] lanes active in them.
#ifdef VOGE_FB_TIMES
__device__ unsigned long long g_cw_stats[1 << 16][4];
#define CW_COUNT(i) do { const unsigned long long m_ = __ballot(true); if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(m_) && blockIdx.x < (1 << 16)) { \
      g_cw_stats[blockIdx.x][i] += 64; g_cw_stats[blockIdx.x][(i) + 1] += (unsigned long long)__popcll(m_); } } while (0)
#else
#define CW_COUNT(i) do {} while (0)
#endif

// Backward, wave form, with the forward's weights given (u_m = g_m w_m comes from the caller): the closed-form
// gradients of the lane's own slots (header of composite.hip).  The pixel's padded rows len / s' / E s' are in LDS
// (the sentinel pads' u entries are zero); this routine stores u into Lu itself.  Same conventions as compn_fwd_rows.
// Round 5: the row sums r_m = sum_j E_j s_j phi(x_mj) are not walked for at all.  phi(x_mj), x_mj = (len_m - len_j) s_j,
// is a value the COLUMN walk of j's owner evaluates anyway (for u_m phi(x_mj)); that lane adds E_j s_j phi to row m's cell of
// LR (an LDS row array laid out like Lu, zeroed by the caller) and the row's owner reads the sum afterwards.  The add is a plain
// read - add - write: in one iteration of a walk the lanes of a wave address DIFFERENT row pairs (a pixel's lanes start NS rows
// apart and step by two together; other pixels have other rows), and a wave's LDS operations complete in order, so the next
// iteration's read sees this one's write -- the wave_barrier only keeps the compiler from moving the read above the write.
// (ds_add_f32 instead costs ~60 cycles per wave instruction: the kernel 129 -> 251 us.)  The column walk reaches every row inside column j's OWN window 3.5 / s_j -- where phi >= 4.8e-6 --
// while the row walk went as far as the pixel's widest window: the terms dropped are below that, like the column sums' own.
// One of the kernel's two window walks and its divergence are gone for one packed multiply and two LDS adds per column pair.
// (LR: a row array of the caller's LDS laid out like Lu, zeroed together with it.)
template <int NS>
__device__ __forceinline__ void compn_bwd_wave(const float (&lm)[NS], const float (&sm)[NS], const float (&em)[NS],
                                               const float (&um)[NS], const float *Llen, const float *Lsp, const float *LE,
                                               float *Lu, const int d0, const int k0, const int K, const int q, const int LP,
                                               const int LPmax, const bool in_wg, const bool active, const bool sorted,
                                               const float occ, float (&ga)[NS], float (&gl)[NS], float (&gd)[NS],
                                               float *LR) {
  constexpr int NP = NS / 2;
  float sp[NS], Es[NS];
#pragma unroll
  for (int a = 0; a < NS; ++a) { sp[a] = sm[a] * kCs; Es[a] = em[a] * sp[a]; }
  bool any_e = false;
#pragma unroll
  for (int a = 0; a < NS; ++a) any_e = any_e || (em[a] != 0.0f);
  const float h0 = __builtin_amdgcn_exp2f(kQ0);      // h(0), exactly what h_pair(0) returns
  // ---- rows = the lane's own slots: r_m = sum over the window of E_j s_j phi_mj ----
  float rterm[NS];
#pragma unroll
  for (int a = 0; a < NS; ++a) rterm[a] = 0.0f;
  if (any_e && sorted) {
    v2f accR[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) accR[a] = splat(0.0f);
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      accR[a].x = Es[a];         // self
#pragma unroll
      for (int b2 = a + 1; b2 < NS; ++b2) {
        const float gap = lm[b2] - lm[a];
        const v2f xp = (v2f){gap * sp[b2], gap * sp[a]};                 // (row a, col b), (row b, col a)
        const v2f g = gauss_pair(xp);
        accR[a].y = fmaf(Es[b2], g.x, accR[a].y);
        accR[b2].y = fmaf(Es[a], g.y, accR[b2].y);
      }
    }
    // (the own block only; the other lanes' columns arrive through LR during their column walks below)
#pragma unroll
    for (int a = 0; a < NS; ++a) rterm[a] = accR[a].x + accR[a].y;
  } else if (any_e && active) {          // unsorted list: every column
    const int r0 = d0 - k0;
    for (int j = 0; j < K; ++j) {
      const float Ej = LE[r0 + j];
      if (Ej == 0.0f) continue;
      const float lj = Llen[r0 + j], sj = Lsp[r0 + j];
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        const float xp = (lm[a] - lj) * sj;
        const float xc = fminf(fabsf(xp), 16.0f);
        rterm[a] = fmaf(Ej * (kRsqrtPi / kCs), __builtin_amdgcn_exp2f(-xc * xc), rterm[a]);
      }
    }
  }
  // ---- u, its suffix sums over the pixel, then the lane's own columns ----
  float usum = 0.0f;
#pragma unroll
  for (int a = 0; a < NS; ++a) usum += um[a];
  if (in_wg) {
#pragma unroll
    for (int h2 = 0; h2 < NP; ++h2) *reinterpret_cast<v2f *>(Lu + d0 + 2 * h2) = (v2f){um[2 * h2], um[2 * h2 + 1]};
  }
  float sx;   // sum of u over the slots behind this lane's group
  {
    // (Round 6 tried this ladder two other ways -- LDS cells: a store, then LPmax - 1 reads per lane, + 5 us; a linear scan on DPP
    //  wave_shl:1 shifts, LPmax - 1 dependent VALU operations and no LDS trip, + 0.7 us -- the 1 + log2(LP) shuffles stay.)
    const float y = __shfl_down(usum, 1, 64);
    float x = (q + 1 < LP && in_wg) ? y : 0.0f;
    for (int o = 1; o < LPmax; o <<= 1) {
      const float z = __shfl_down(x, o, 64);
      if (q + o < LP && in_wg) x += z;
    }
    sx = x;
    wave_lds_sync();
  }
#pragma unroll
  for (int a = 0; a < NS; ++a) { ga[a] = 0.0f; gl[a] = 0.0f; gd[a] = 0.0f; }
  if (any_e && active) {
    float cPhi[NS], cphi[NS], cphil[NS];
    if (sorted) {
      // ONE accumulator set per own column for the rows behind and the rows in front: with d = len_row - len_col in both
      // directions the column's three sums are  cPhi = suf - H,  cphi = P,  cphil = L  with
      //   H = sum_behind u h - sum_front u h,   P = sum u g,   L = sum u g d   (h, g at x' = |d| s' >= 0).
      // The front walk keeps |d| = len_col - len_row (what h and g are evaluated at) and accumulates -u h and (-u g) |d|:
      // a negation is exact, so each term has the bits it would have in a second set subtracted at the end.
      v2f H[NS], P[NS], L[NS];
      // One bound per walk, as in compn_fwd_rows: a row pair behind is walked while its first len lies inside the window
      // kSat / s_j of any LIVE own column, one in front while its second does.  An empty column (len = the empty slot's
      // sentinel) is not folded in: a lane with no live column keeps -kBig / +kBig and leaves at the first pair.  The
      // per-column test this replaces, len_row - len_col < r_j in fp32, holds only where len_row < len_col + r_j exactly
      // (fp32 subtraction is monotone and r_j is a float), and then len_row <= fl(len_col + r_j): with <= the bound never
      // drops a row that test walked; what it adds sits at the window's edge, where phi <= 4.8e-6.
      float reachB = -kBig, reachF = kBig;
#pragma unroll
      for (int b2 = 0; b2 < NS; ++b2) {
        const bool live = em[b2] != 0.0f;
        const float r = kSat * __builtin_amdgcn_rcpf(sm[b2]);
        reachB = live ? fmaxf(reachB, lm[b2] + r) : reachB;
        reachF = live ? fminf(reachF, lm[b2] - r) : reachF;
        H[b2] = (v2f){um[b2] * h0, 0.0f}; P[b2] = (v2f){um[b2], 0.0f}; L[b2] = splat(0.0f);   // self
      }
      // diagonal block: for own slots a < b, row b is behind column a and row a in front of column b
#pragma unroll
      for (int a = 0; a < NS; ++a) {
#pragma unroll
        for (int b2 = a + 1; b2 < NS; ++b2) {
          const float gap = lm[b2] - lm[a];
          const v2f xp = (v2f){gap * sp[a], gap * sp[b2]};      // (row b, col a), (row a, col b)
          const v2f g = gauss_pair(xp), h = h_pair(xp);
          H[a].y = fmaf(um[b2], h.x, H[a].y); P[a].y = fmaf(um[b2], g.x, P[a].y); L[a].y = fmaf(um[b2] * g.x, gap, L[a].y);
          H[b2].y = fmaf(-um[a], h.y, H[b2].y); P[b2].y = fmaf(um[a], g.y, P[b2].y); L[b2].y = fmaf(-(um[a] * g.y), gap, L[b2].y);
        }
      }
      for (int e = d0 + NS;; e += 2) {     // row pairs behind every own column
        const v2f l2 = ld2(Llen, e), u2 = ld2(Lu, e);
        v2f racc = ld2(LR, e);
        if (!(l2.x <= reachB)) break;
        CW_COUNT(2);
#pragma unroll
        for (int b2 = 0; b2 < NS; ++b2) {
          const v2f d = l2 - splat(lm[b2]);
          const v2f xp = d * splat(sp[b2]);
          const v2f g = gauss_pair(xp);
          const v2f y = u2 * g;
          H[b2] = pk_fma(u2, h_pair(xp), H[b2]); P[b2] = P[b2] + y; L[b2] = pk_fma(y, d, L[b2]);
          racc = pk_fma(splat(Es[b2]), g, racc);
        }
        *reinterpret_cast<v2f *>(LR + e) = racc;
        wave_lds_sync();
      }
      for (int e = d0 - 2;; e -= 2) {      // row pairs in front of every own column
        const v2f l2 = ld2(Llen, e), u2 = ld2(Lu, e);
        v2f racc = ld2(LR, e);
        if (!(l2.y >= reachF)) break;
        CW_COUNT(2);
#pragma unroll
        for (int b2 = 0; b2 < NS; ++b2) {
          const v2f d = splat(lm[b2]) - l2;
          const v2f xp = d * splat(sp[b2]);
          const v2f g = gauss_pair(xp);
          const v2f y = u2 * g;
          H[b2] = pk_fma(-u2, h_pair(xp), H[b2]); P[b2] = P[b2] + y; L[b2] = pk_fma(-y, d, L[b2]);
          racc = pk_fma(splat(Es[b2]), g, racc);
        }
        *reinterpret_cast<v2f *>(LR + e) = racc;
        wave_lds_sync();
      }
      // every column walk of the pixel has passed (its lanes share this wave): the row sums are complete
      wave_lds_sync();
#pragma unroll
      for (int a = 0; a < NS; ++a) rterm[a] = (rterm[a] + *lds_volatile(LR + d0 + a)) * (kRsqrtPi / kCs);
      float suf = sx;
#pragma unroll
      for (int b2 = NS - 1; b2 >= 0; --b2) {
        suf += um[b2];                                                   // inclusive suffix sum of u
        cPhi[b2] = suf - (H[b2].x + H[b2].y);
        cphi[b2] = (P[b2].x + P[b2].y) * kRsqrtPi;
        cphil[b2] = (L[b2].x + L[b2].y) * kRsqrtPi;
      }
    } else {
#pragma unroll
      for (int b2 = 0; b2 < NS; ++b2) { cPhi[b2] = 0.0f; cphi[b2] = 0.0f; cphil[b2] = 0.0f; }
      const int r0 = d0 - k0;
      for (int m = 0; m < K; ++m) {
        const float ur = Lu[r0 + m];
        if (ur == 0.0f) continue;
        const float lr = Llen[r0 + m];
#pragma unroll
        for (int b2 = 0; b2 < NS; ++b2) {
          const float dl = lr - lm[b2];
          const float xp = dl * sp[b2];
          const float h = h_one(fabsf(xp));
          const float xc = fminf(fabsf(xp), 16.0f);
          const float ph = ur * (__builtin_amdgcn_exp2f(-xc * xc) * kRsqrtPi);
          cPhi[b2] = fmaf(ur, xp >= 0.0f ? 1.0f - h : h, cPhi[b2]);
          cphi[b2] += ph;
          cphil[b2] = fmaf(ph, dl, cphil[b2]);
        }
      }
    }
#pragma unroll
    for (int b2 = 0; b2 < NS; ++b2) {
      if (em[b2] != 0.0f) {
        ga[b2] = fmaf(occ * em[b2], cPhi[b2], -um[b2]);
        gl[b2] = -occ * (um[b2] * rterm[b2] - em[b2] * sm[b2] * cphi[b2]);
        gd[b2] = -occ * em[b2] * (0.5f * __builtin_amdgcn_rcpf(sm[b2])) * cphil[b2];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Lane packing by hit count.  With the trace's per-pixel hit count at hand a pixel needs ceil(count / NS) lanes, not
// ceil(K / NS): at cfg3 the lit pixels hold 18 of K = 40 slots on average and 40 % of the pixels none, so a wave laid
// out for K idles more than half of its lanes through every scan, window walk and table update.  The packed kernels
// give a wave a GROUP of G <= 64 pixels (lane g < G holds pixel g's lane need) and walk it in rounds; a round takes
// the longest run of consecutive pixels whose lanes fit the wave.  A pixel's lanes stay adjacent and in slot order,
// so everything per pixel (scan association, window walks) is what the K-strided layout computes: bit-identical.
struct PackLane {
  int p;      // the lane's pixel inside the group (-1: idle lane)
  int s0;     // first lane of that pixel
  int np;     // its lanes
  int ord;    // its ordinal among the round's non-empty pixels (row origins in LDS)
};
// inclusive prefix sum over the wave
__device__ __forceinline__ int wave_incl_scan(int v, const int lane) {
  // DPP steps (VALU operands) instead of six dependent LDS-crossbar shuffles: shifts by 1, 2, 4, 8 inside every row of
  // 16 lanes (zeros shifted in), then lane 15 of rows 0 / 2 into rows 1 / 3, then lane 31 into rows 2 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);      // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);      // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);      // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);      // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 -> rows 2, 3
  (void)lane;
  return v;
}
// One round: pixels [pc, pe) of the group (pe returned; uniform), `off` = lanes consumed by earlier rounds.
// need / incl: lane g's pixel need and its inclusive prefix (lanes >= G: need 0).  np_max: the longest pixel of the round.
__device__ __forceinline__ int pack_round(const int need, const int incl, const int G, const int lane, const int pc,
                                          const int off, PackLane &pl, int &np_max) {
  const unsigned long long fit = __ballot(lane >= pc && lane < G && incl - off <= 64);
  const int pe = pc + __popcll(fit);      // (incl is monotone: the fitting pixels are a run; need <= 64: never empty)
  pl.p = -1; pl.s0 = 0; pl.np = 0; pl.ord = 0;
  int c = 0, nm = 0;
  const int excl = incl - need;
  for (int p = pc; p < pe; ++p) {         // uniform
    const int n = __builtin_amdgcn_readlane(need, p);
    if (n == 0) continue;
    const int s = __builtin_amdgcn_readlane(excl, p) - off;
    if (lane >= s) { pl.p = p; pl.s0 = s; pl.np = n; pl.ord = c; }
    ++c;
    nm = max(nm, n);
  }
  if (lane >= pl.s0 + pl.np) pl.p = -1;   // lanes behind the round's last pixel
  np_max = nm;
  return pe;
}

}  // namespace voge
