// The two-level integer scan that compacts a mesh (mesh_clean.hip's filter, mesh_simplify.hip's outputs, meshing.hip's vertices and
// faces): counts in blocks of kMcBlock, the exclusive prefix inside a block as a 16-bit number and the block's total; then ONE
// workgroup of kMcTop turns the tables of block totals into their exclusive scans in place, kMcTop entries a round with the total
// carried.  Item i lands in row blocks[i / kMcBlock] + loc[i].  Integer sums only: the same bits on every run.
#pragma once

#include "voge_common.h"

namespace voge {

constexpr int kMcBlock = 256;          // items of a scan block (= threads of the local scan); ops.MESH_CLEAN_BLOCK, ops.MTET_BLOCK
constexpr int kMcTop = 1024;           // block totals one round of the top level takes (= its threads); ops.MESH_CLEAN_TOP, ops.MTET_TOP
constexpr long kMcMax = 268435455l;    // V, F <= 2^28 - 1

// One count x a thread of a kMcBlock workgroup; every thread of the workgroup calls (a barrier inside).  -> the thread's exclusive
// prefix; upto: its inclusive one, which in the LAST thread is the block's total.  (Two counts packed in one word scan together
// while neither half overflows into the other.)
__device__ __forceinline__ uint32_t mesh_scan_local(const uint32_t x, uint32_t &upto) {
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
  upto = base + incl;
  return base + incl - x;
}

// ONE workgroup of kMcTop: the exclusive scan of a table of nb block totals in place -> the total (the same in every thread).  nb
// is the same in every thread: the barriers are uniform.  W = uint32_t: the table is lo.  W = unsigned long long: entry i is
// lo[i] | hi[i] << 32, two tables scanned at once (no carry between the halves while the low total stays below 2^32).
template <class W>
__device__ __forceinline__ W mesh_scan_top(uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, const long nb) {
  __shared__ W wtot[kMcTop / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  W carry = 0;      // (the mesh filters: at most 2^28 - 1 flags in all)
  for (long r0 = 0; r0 < nb; r0 += kMcTop) {
    const long i = r0 + tid;
    W x = 0;
    if constexpr (sizeof(W) == 4) x = i < nb ? lo[i] : 0u;
    else x = i < nb ? ((unsigned long long)lo[i] | ((unsigned long long)hi[i] << 32)) : 0ull;
    W incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {      // (a 64-bit word travels as its two halves)
      W y = (uint32_t)__shfl_up((int)(uint32_t)incl, o, 64);
      if constexpr (sizeof(W) == 8) y |= (W)(uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o, 64) << 32;
      if (lane >= o) incl += y;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    W base = 0, all = 0;
    for (int k = 0; k < kMcTop / 64; ++k) {
      if (k < wave) base += wtot[k];
      all += wtot[k];
    }
    const W excl = carry + base + incl - x;
    if (i < nb) {
      lo[i] = (uint32_t)excl;
      if constexpr (sizeof(W) == 8) hi[i] = (uint32_t)(excl >> 32);
    }
    carry += all;
    __syncthreads();      // (wtot is rewritten by the next round)
  }
  return carry;
}
__device__ __forceinline__ uint32_t mesh_scan_top(uint32_t *__restrict__ tab, const long nb) { return mesh_scan_top<uint32_t>(tab, nullptr, nb); }

}  // namespace voge
