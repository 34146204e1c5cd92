// pob_sort.hip -- stable LSD radix sort of (uint32 key, int32 value) pairs and, on top of it, the whole
// of jumpy.random_permutation (jax's _shuffle, [ext]) as one entry point (DESIGN.md "Native stable
// radix sort").  Of pob_mlp_tile.h it takes the error helpers only; the layout, the constants and the
// wave / block primitives are pob_sort.h's.
//
// A pass sorts by one 8-bit digit (shift = 0, 8, 16, 24) from one pair of buffers into another:
//   k_sort_count    one block per tile: the tile's digit histogram -> counts[digit][tile]
//   k_sort_scan     one block per digit: the exclusive scan of the digit's row of counts along the
//                   tiles, in place, POB_SORT_SCAN_CHUNK tiles at a time; the row's sum -> totals[digit]
//   k_sort_scatter  one block per tile: the stable rank of every element of the tile, the tile staged in
//                   LDS in digit order, each digit's run stored as consecutive-lane stores
// No block waits for another inside a launch: the digit's global base (the exclusive scan of totals,
// 256 words) is formed again by every scatter block.  The only atomics are k_sort_count's LDS adds
// into the tile's histogram, whose sums do not depend on their order; the ranks use none.
//
// Element order inside a tile: wave w owns elements [w 512, (w + 1) 512), item i of lane l is element
// w 512 + i 64 + l, so a wave's loads of an item are one coalesced segment and ascending (item, lane)
// is ascending element order.  GEN = true: the key of element j is tf_elem(sub, n, j) (the word
// random_bits(sub, (n,)) holds at j), formed in registers by count and scatter alike; `keys` then
// points at sub's two words.
//
// Matrix instructions have no use here: a pass moves 16 bytes an element and counts bits.
#include "pob_mlp_tile.h"
#include "pob_sort.h"

template <bool GEN>
__device__ __forceinline__ uint32_t sort_key(const uint32_t *keys, const uint32_t s0, const uint32_t s1,
                                             const uint32_t n, const uint32_t j) {
  return GEN ? tf_elem(s0, s1, n, j) : keys[j];
}

template <bool GEN>
__global__ __launch_bounds__(POB_SORT_LANES) void k_sort_count(const uint32_t *keys, const uint32_t n, const int shift,
                                                               const uint32_t tiles, uint32_t *counts) {
  __shared__ uint32_t hist[POB_SORT_RADIX];
  const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)POB_SORT_TILE;
  const uint32_t s0 = GEN ? keys[0] : 0u, s1 = GEN ? keys[1] : 0u;
  hist[tid] = 0u;
  __syncthreads();
  uint32_t k[POB_SORT_ITEMS];
#pragma unroll
  for (int i = 0; i < POB_SORT_ITEMS; ++i) {
    const uint32_t j = base + i * POB_SORT_LANES + tid;
    k[i] = j < n ? sort_key<GEN>(keys, s0, s1, n, j) : 0u;
  }
#pragma unroll
  for (int i = 0; i < POB_SORT_ITEMS; ++i)
    if (base + i * POB_SORT_LANES + tid < n) atomicAdd(&hist[(k[i] >> shift) & (POB_SORT_RADIX - 1)], 1u);
  __syncthreads();
  counts[(size_t)tid * tiles + blockIdx.x] = hist[tid];
}

__global__ __launch_bounds__(POB_SORT_LANES) void k_sort_scan(uint32_t *counts, const uint32_t tiles, uint32_t *totals) {
  __shared__ uint32_t part[POB_SORT_WAVES];
  uint32_t *row = counts + (size_t)blockIdx.x * tiles;
  uint32_t running = 0u;
  for (uint32_t c0 = 0; c0 < tiles; c0 += POB_SORT_SCAN_CHUNK) {
    const uint32_t t = c0 + threadIdx.x;
    const uint32_t v = t < tiles ? row[t] : 0u;
    uint32_t sum;
    const uint32_t before = sort_block_scan(v, part, sum);
    if (t < tiles) row[t] = running + before;
    running += sum;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = running;
}

template <bool GEN>
__global__ __launch_bounds__(POB_SORT_LANES) void k_sort_scatter(const uint32_t *keys, const int32_t *vals, const uint32_t n,
                                                                 const int shift, const uint32_t tiles,
                                                                 const uint32_t *counts, const uint32_t *totals,
                                                                 uint32_t *keys_out, int32_t *vals_out) {
  __shared__ uint32_t wcount[POB_SORT_WAVES][POB_SORT_RADIX];  // per wave and digit: the running count, then the run's start
  __shared__ uint32_t gbase[POB_SORT_RADIX];                   // output index of staging slot p of digit d: gbase[d] + p
  __shared__ uint32_t skey[POB_SORT_TILE];
  __shared__ int32_t sval[POB_SORT_TILE];
  __shared__ uint32_t part[POB_SORT_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)POB_SORT_TILE;
  const uint32_t valid = n - base < POB_SORT_TILE ? n - base : POB_SORT_TILE;
  // this lane's digit (tid) in the two tables, loaded ahead of their use
  const uint32_t digit_total = totals[tid], digit_before = counts[(size_t)tid * tiles + blockIdx.x];
  const uint32_t s0 = GEN ? keys[0] : 0u, s1 = GEN ? keys[1] : 0u;
  const uint32_t e0 = wave * (64 * POB_SORT_ITEMS) + lane;  // element of item 0
  uint32_t k[POB_SORT_ITEMS], rank[POB_SORT_ITEMS];
#pragma unroll
  for (int i = 0; i < POB_SORT_ITEMS; ++i) {
    const uint32_t e = e0 + 64 * i;
    k[i] = e < valid ? sort_key<GEN>(keys, s0, s1, n, base + e) : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int w = 0; w < POB_SORT_WAVES; ++w) wcount[w][tid] = 0u;
  __syncthreads();
  // the stable rank inside the wave: items ascending; per item the lanes of equal digit take the wave's
  // running count plus their place among themselves, and the lowest of them advances the count
  volatile uint32_t *mine = wcount[wave];
#pragma unroll
  for (int i = 0; i < POB_SORT_ITEMS; ++i) {
    const bool ok = e0 + 64 * i < valid;
    const uint32_t d = (k[i] >> shift) & (POB_SORT_RADIX - 1);
    const uint64_t same = sort_match(d, __ballot(ok));
    const uint32_t below = sort_below(same);
    const uint32_t c = ok ? mine[d] : 0u;
    rank[i] = c + below;
    __builtin_amdgcn_wave_barrier();
    if (ok && below == 0u) mine[d] = c + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // waves in wave order, digits in digit order: lane d turns the four counts of digit d into the starts
  // of the waves' runs in the staging area
  {
    uint32_t c[POB_SORT_WAVES], tile_total = 0u;
#pragma unroll
    for (int w = 0; w < POB_SORT_WAVES; ++w) {
      c[w] = wcount[w][tid];
      tile_total += c[w];
    }
    uint32_t sum;
    uint32_t start = sort_block_scan(tile_total, part, sum);      // the digit's run in the staging area
    const uint32_t digit_base = sort_block_scan(digit_total, part, sum);  // the digit's run in the output
    gbase[tid] = digit_base + digit_before - start;
#pragma unroll
    for (int w = 0; w < POB_SORT_WAVES; ++w) {
      wcount[w][tid] = start;
      start += c[w];
    }
  }
  __syncthreads();
  {
    int32_t v[POB_SORT_ITEMS];
#pragma unroll
    for (int i = 0; i < POB_SORT_ITEMS; ++i) {
      const uint32_t e = e0 + 64 * i;
      v[i] = e < valid ? (vals ? vals[base + e] : (int32_t)(base + e)) : 0;
    }
#pragma unroll
    for (int i = 0; i < POB_SORT_ITEMS; ++i)
      if (e0 + 64 * i < valid) {
        const uint32_t p = wcount[wave][(k[i] >> shift) & (POB_SORT_RADIX - 1)] + rank[i];
        skey[p] = k[i];
        sval[p] = v[i];
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < POB_SORT_ITEMS; ++i) {
    const uint32_t p = i * POB_SORT_LANES + tid;
    if (p < valid) {
      const uint32_t key = skey[p];
      const uint32_t o = gbase[(key >> shift) & (POB_SORT_RADIX - 1)] + p;
      if (keys_out) keys_out[o] = key;
      vals_out[o] = sval[p];
    }
  }
}

// subs[r] <- the second row of split(key_r), key_{r + 1} <- the first, from key_0 = key: the sort keys
// of the permutation's rounds.  One lane.
__global__ void k_perm_subs(const uint32_t *key, const int rounds, uint32_t *subs) {
  uint32_t k0 = key[0], k1 = key[1];
  for (int r = 0; r < rounds; ++r) {
    uint32_t n0, n1, s0, s1;
    tf_split(k0, k1, 2u, 0u, n0, n1);
    tf_split(k0, k1, 2u, 1u, s0, s1);
    subs[2 * r] = s0;
    subs[2 * r + 1] = s1;
    k0 = n0;
    k1 = n1;
  }
}

// n = 1: no round, the identity
__global__ void k_perm_one(int32_t *out) { out[0] = 0; }

struct sort_buffers {
  uint32_t tiles, *totals, *counts, *keys[2];
  int32_t *vals[2];
};

static int sort_check(const char *who, long long n, const void *workspace, long long ws_bytes, sort_buffers *b) {
  static thread_local char msg[160];
  if (n < 1 || n >= (1LL << 31)) {
    snprintf(msg, sizeof msg, "%s: n must be in 1 .. 2^31 - 1", who);
    return pob_fail_msg(POB_EINVAL, msg);
  }
  if (!workspace) {
    snprintf(msg, sizeof msg, "%s: workspace is NULL", who);
    return pob_fail_msg(POB_EINVAL, msg);
  }
  if ((uintptr_t)workspace & 3) {
    snprintf(msg, sizeof msg, "%s: workspace must be 4-byte aligned", who);
    return pob_fail_msg(POB_EINVAL, msg);
  }
  const pob_sort_layout L = pob_sort_layout_of(n);
  if (ws_bytes < L.bytes) {
    snprintf(msg, sizeof msg, "%s: workspace of %lld bytes, pob_sort_workspace_bytes(n) = %lld", who, ws_bytes, L.bytes);
    return pob_fail_msg(POB_EINVAL, msg);
  }
  char *ws = (char *)workspace;
  b->tiles = (uint32_t)L.tiles;
  b->totals = (uint32_t *)(ws + L.totals);
  b->counts = (uint32_t *)(ws + L.counts);
  for (int k = 0; k < 2; ++k) {
    b->keys[k] = (uint32_t *)(ws + L.keys[k]);
    b->vals[k] = (int32_t *)(ws + L.vals[k]);
  }
  return POB_OK;
}

// one pass: count, scan, scatter.  gen: keys points at the round's sub key
static void sort_pass(hipStream_t st, const sort_buffers &b, bool gen, const uint32_t *keys, const int32_t *vals, uint32_t n,
                      int shift, uint32_t *keys_out, int32_t *vals_out) {
  const dim3 tiles(b.tiles), lanes(POB_SORT_LANES);
  if (gen)
    hipLaunchKernelGGL(k_sort_count<true>, tiles, lanes, 0, st, keys, n, shift, b.tiles, b.counts);
  else
    hipLaunchKernelGGL(k_sort_count<false>, tiles, lanes, 0, st, keys, n, shift, b.tiles, b.counts);
  hipLaunchKernelGGL(k_sort_scan, dim3(POB_SORT_RADIX), lanes, 0, st, b.counts, b.tiles, b.totals);
  if (gen)
    hipLaunchKernelGGL(k_sort_scatter<true>, tiles, lanes, 0, st, keys, vals, n, shift, b.tiles, (const uint32_t *)b.counts,
                       (const uint32_t *)b.totals, keys_out, vals_out);
  else
    hipLaunchKernelGGL(k_sort_scatter<false>, tiles, lanes, 0, st, keys, vals, n, shift, b.tiles, (const uint32_t *)b.counts,
                       (const uint32_t *)b.totals, keys_out, vals_out);
}

extern "C" {

long long pob_sort_workspace_bytes(long long n) {
  if (n < 1 || n >= (1LL << 31)) return pob_fail_msg(POB_EINVAL, "sort: n must be in 1 .. 2^31 - 1");
  return pob_sort_layout_of(n).bytes;
}

int pob_sort_pairs_u32(const uint32_t *keys, const int32_t *vals, long long n, uint32_t *keys_out, int32_t *vals_out,
                       void *workspace, long long ws_bytes, void *stream) {
  if (!keys || !vals_out) return pob_fail_msg(POB_EINVAL, "sort_pairs: NULL argument (keys, vals_out)");
  if (((uintptr_t)keys | (uintptr_t)vals | (uintptr_t)keys_out | (uintptr_t)vals_out) & 3)
    return pob_fail_msg(POB_EINVAL, "sort_pairs: keys, vals and the outputs must be 4-byte aligned");
  sort_buffers b;
  const int rc = sort_check("sort_pairs", n, workspace, ws_bytes, &b);
  if (rc != POB_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t un = (uint32_t)n;
  sort_pass(st, b, false, keys, vals, un, 0, b.keys[0], b.vals[0]);
  sort_pass(st, b, false, b.keys[0], b.vals[0], un, 8, b.keys[1], b.vals[1]);
  sort_pass(st, b, false, b.keys[1], b.vals[1], un, 16, b.keys[0], b.vals[0]);
  sort_pass(st, b, false, b.keys[0], b.vals[0], un, 24, keys_out, vals_out);
  return mlp_hip_check(hipGetLastError(), "k_sort launch");
}

int pob_random_permutation(const uint32_t *key, long long n, int32_t *out, void *workspace, long long ws_bytes, void *stream) {
  if (!key || !out) return pob_fail_msg(POB_EINVAL, "random_permutation: NULL argument (key, out)");
  if (((uintptr_t)key | (uintptr_t)out) & 3) return pob_fail_msg(POB_EINVAL, "random_permutation: key and out must be 4-byte aligned");
  sort_buffers b;
  const int rc = sort_check("random_permutation", n, workspace, ws_bytes, &b);
  if (rc != POB_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t un = (uint32_t)n;
  // permutation_rounds(n) = ceil(3 ln n / ln(2^32 - 1)) without the logarithms: the least r with
  // n^3 <= (2^32 - 1)^r; n^3 < 2^93 is exact in __int128, and r = 3 holds for every n < 2^31
  const unsigned __int128 cube = (unsigned __int128)n * (unsigned __int128)n * (unsigned __int128)n;
  const unsigned __int128 m = 0xFFFFFFFFu;
  const int rounds = n == 1 ? 0 : cube <= m ? 1 : cube <= m * m ? 2 : 3;
  if (rounds == 0) {
    hipLaunchKernelGGL(k_perm_one, dim3(1), dim3(1), 0, st, out);
    return mlp_hip_check(hipGetLastError(), "k_perm_one launch");
  }
  uint32_t *subs = (uint32_t *)workspace;  // pob_sort_layout.subs = 0
  hipLaunchKernelGGL(k_perm_subs, dim3(1), dim3(1), 0, st, key, rounds, subs);
  for (int r = 0; r < rounds; ++r) {
    // the round's payload: iota, then the round before's order (vals[1]); the last pass of a round stores
    // no keys, the next round forms its own
    sort_pass(st, b, true, subs + 2 * r, r == 0 ? nullptr : b.vals[1], un, 0, b.keys[0], b.vals[0]);
    sort_pass(st, b, false, b.keys[0], b.vals[0], un, 8, b.keys[1], b.vals[1]);
    sort_pass(st, b, false, b.keys[1], b.vals[1], un, 16, b.keys[0], b.vals[0]);
    sort_pass(st, b, false, b.keys[0], b.vals[0], un, 24, nullptr, r == rounds - 1 ? out : b.vals[1]);
  }
  return mlp_hip_check(hipGetLastError(), "k_sort launch");
}

}  // extern "C"
