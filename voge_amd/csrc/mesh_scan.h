// The two-level integer scan that compacts a mesh (mesh_clean.hip's filter, mesh_simplify.hip's outputs): flags in blocks of
// kMcBlock, the exclusive prefix inside a block as a 16-bit number and the block's total; then ONE workgroup of kMcTop turns the
// tables of block totals into their exclusive scans in place, kMcTop entries a round with the total carried.  Item i lands in row
// blocks[i / kMcBlock] + loc[i].  Integer sums only: the same bits on every run.
#pragma once

#include "voge_common.h"

namespace voge {

constexpr int kMcBlock = 256;          // flags of a scan block (= threads of the local scan); ops.MESH_CLEAN_BLOCK
constexpr int kMcTop = 1024;           // block totals one round of the top level takes (= its threads); ops.MESH_CLEAN_TOP
constexpr long kMcMax = 268435455l;    // V, F <= 2^28 - 1

// One flag x (0 or 1) a thread of a kMcBlock workgroup; every thread of the workgroup calls (a barrier inside).  Writes loc (where
// `in`) and, by the last thread, the block's total.
__device__ __forceinline__ void mesh_scan_local(const uint32_t x, const bool in, uint16_t *__restrict__ loc_i, uint32_t *__restrict__ btot_b) {
  __shared__ uint32_t wtot[kMcBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint32_t base = 0u;
  for (int k = 0; k < wave; ++k) base += wtot[k];
  if (in) *loc_i = (uint16_t)(base + incl - x);
  if (tid == kMcBlock - 1) *btot_b = base + incl;
}

// ONE workgroup of kMcTop: the exclusive scan of tab[0, nb) in place -> the total (the same in every thread).  nb is the same in
// every thread: the barriers are uniform.
__device__ __forceinline__ uint32_t mesh_scan_top(uint32_t *__restrict__ tab, const long nb) {
  __shared__ uint32_t wtot[kMcTop / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0u;      // (at most 2^28 - 1 flags in all)
  for (long r0 = 0; r0 < nb; r0 += kMcTop) {
    const long i = r0 + tid;
    const uint32_t x = i < nb ? tab[i] : 0u;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += y;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0u, all = 0u;
    for (int k = 0; k < kMcTop / 64; ++k) {
      if (k < wave) base += wtot[k];
      all += wtot[k];
    }
    if (i < nb) tab[i] = carry + base + incl - x;
    carry += all;
    __syncthreads();      // (wtot is rewritten by the next round)
  }
  return carry;
}

}  // namespace voge
