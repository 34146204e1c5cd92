// pob_sort.h -- the stable radix sort of (uint32 key, int32 value) pairs (DESIGN.md "Native stable
// radix sort"): the workspace layout as plain functions (host code; tests/host/sort_layout_host.cpp
// walks them under the sanitizers) and, for the device compiler, the wave and block primitives of
// pob_sort.hip's kernels.
//
// Least-significant-digit radix sort, POB_SORT_BITS = 8 bits a pass, four passes, keys in unsigned
// order.  A block of POB_SORT_LANES lanes owns one tile of POB_SORT_TILE consecutive elements; a pass
// is three launches (count, scan, scatter) and no block waits for another inside one.
#pragma once
#include <stdint.h>

#define POB_SORT_BITS 8
#define POB_SORT_RADIX 256        // digits of a pass: one lane of a block each
#define POB_SORT_LANES 256        // lanes of a block (four waves)
#define POB_SORT_WAVES 4
#define POB_SORT_ITEMS 8          // elements of a lane
#define POB_SORT_TILE (POB_SORT_LANES * POB_SORT_ITEMS)  // 2 048 elements of a block
#define POB_SORT_SCAN_CHUNK 256   // tiles k_sort_scan takes at a time: one lane each
#define POB_SORT_MAX_ROUNDS 3     // permutation_rounds(2^31 - 1)
#define POB_SORT_ALIGN 256        // every region of the workspace starts at a multiple of this

// The workspace, byte offsets from its base:
//   subs    (POB_SORT_MAX_ROUNDS, 2) uint32   the rounds' sort keys `sub` (pob_random_permutation only)
//   totals  (256,) uint32                     the pass's element count per digit
//   counts  (256, tiles) uint32               digit-major: the tiles' digit counts, then (in place) their
//                                             exclusive scan along the tiles of a digit
//   keys[2], vals[2]  (n,) each               the ping-pong pairs
struct pob_sort_layout {
  long long tiles, subs, totals, counts, keys[2], vals[2], bytes;
};

static inline long long pob_sort_round_up(long long b) { return (b + POB_SORT_ALIGN - 1) / POB_SORT_ALIGN * POB_SORT_ALIGN; }

// n in 1 .. 2^31 - 1 (the entry points check it): at most 2^20 tiles, below 36 GB in all
static inline pob_sort_layout pob_sort_layout_of(long long n) {
  pob_sort_layout L;
  L.tiles = (n + POB_SORT_TILE - 1) / POB_SORT_TILE;
  long long at = 0;
  L.subs = at;
  at += pob_sort_round_up(POB_SORT_MAX_ROUNDS * 2 * (long long)sizeof(uint32_t));
  L.totals = at;
  at += pob_sort_round_up(POB_SORT_RADIX * (long long)sizeof(uint32_t));
  L.counts = at;
  at += pob_sort_round_up(POB_SORT_RADIX * L.tiles * (long long)sizeof(uint32_t));
  for (int k = 0; k < 2; ++k) {
    L.keys[k] = at;
    at += pob_sort_round_up(n * (long long)sizeof(uint32_t));
  }
  for (int k = 0; k < 2; ++k) {
    L.vals[k] = at;
    at += pob_sort_round_up(n * (long long)sizeof(int32_t));
  }
  L.bytes = at;
  return L;
}

#ifdef __HIPCC__
#include "pob_math.h"

// lanes of the wave below this one whose bit is set in mask
POB_D uint32_t sort_below(const uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The lanes of the wave that hold this lane's digit, among the lanes of `valid`: eight ballot rounds,
// one per digit bit, each keeping the lanes that agree with this lane on that bit.  Every lane of the
// wave must be here.
POB_D uint64_t sort_match(const uint32_t digit, const uint64_t valid) {
  uint64_t mask = valid;
#pragma unroll
  for (int b = 0; b < POB_SORT_BITS; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t has = __ballot(bit);
    mask &= bit ? has : ~has;
  }
  return mask;
}

// Exclusive scan of one value per lane over the block's 256 lanes in lane order, the block's sum in
// total: a shuffle scan inside each wave, the four wave sums through part (LDS, POB_SORT_WAVES + 1
// words).  Every lane of the block must be here; part may be reused after the call returns.
POB_D uint32_t sort_block_scan(const uint32_t v, uint32_t *part, uint32_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  __syncthreads();  // the previous call's readers of part are done
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < POB_SORT_WAVES; ++w) {
    const uint32_t s = part[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  return before + inc - v;
}
#endif  // __HIPCC__
