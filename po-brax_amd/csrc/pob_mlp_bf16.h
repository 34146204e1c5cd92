// pob_mlp_bf16.h -- the bf16 matrix-core forward of the MLP (pob_mlp_bf16.hip; DESIGN.md "Bf16
// forward"): the layouts, the weight pack and the layer of a four-wave block.
//
// The function (NOT the fmaf chain of pob_mlp.h: the first network kernel pinned to a float64
// reference within a tolerance, not to a C restatement): x^ = bf16(x) (after the normaliser's f32
// arithmetic in the _norm form), W^ = bf16(W), per layer a = b + h^ W^ with exact products and f32
// accumulation from the f32 bias in the order of v_mfma_f32_32x32x16_bf16, h = act(a) in f32 with
// pob_mlp.h's activations, h^ = bf16(h) for every hidden layer, the last layer's output f32 and
// unrounded.  bf16() is round-to-nearest-even (v_cvt_pk_bf16_f32).  No atomics and a fixed order:
// the same bits from run to run.
//
// Weights: k_mlp_pack_bf16 rewrites theta's matrices, on every call, into a caller-owned workspace
// in FRAGMENT ORDER: per layer [out tile of 32][k chunk of 16][lane 0 .. 63][8 bf16], `in` padded
// with zeros to a multiple of 16 and `out` to a multiple of 32.  Lane l's eight values are
// W[16 c + 8 (l >> 5) + e][32 t + (l & 31)], e = 0 .. 7: the instruction's A operand for the
// transposed product Y^T = W^T X^T.  A wave's fragment is one contiguous 1 KB block, one 16-byte
// load a lane, and the forward has neither a clamped address nor a tail test on a weight.
//
// Activations: a block of MLPB_WAVES = 4 waves owns MLPB_ROWS = 64 consecutive rows (two sub-tiles
// of 32).  Hidden activations live in LDS as bf16 [row][feature], TWO images (layer l reads one
// and writes the other: one block barrier a layer), 2 x 33 792 B: two blocks on a CU.  The B
// operand of lane l for k chunk c is the eight consecutive features 16 c + 8 (l >> 5) .. of row
// l & 31: one 16-byte LDS read.  The pitch is MLPB_PITCH = 264 bf16 = 132 dwords: consecutive rows
// start 4 banks apart, so the 16-byte reads of 8 consecutive rows (of 16, on 64 banks) tile all
// the banks exactly once; a wider read cannot do better.  In the accumulator a lane holds ONE row
// (l & 31) and four groups of four consecutive features (8 q + 4 (l >> 5) + 0 .. 3), so the
// epilogue packs four activations into one 8-byte store into [row][feature]; a wave's 64 such
// stores touch every bank exactly four times, the fewest passes 128 dwords can take.  Zero-padded
// weight columns and a zero bias give act(0) = 0 in the image's padded features: the next layer's
// k pad needs no clearing.
//
// The waves split a layer's output tiles as the f32 wide kernel does (wave w: tiles w and w + 4,
// each for both row sub-tiles; a layer of at most two tiles gives a wave one (tile, sub-tile)
// pair), so a weight fragment feeds every row of the block it is loaded for.  The next k chunk's
// fragments are loaded while the current chunk's MFMAs run.
#pragma once
#include "pob_mlp_tile.h"

#define MLPB_WAVES 4
#define MLPB_SUB 2
#define MLPB_ROWS (32 * MLPB_SUB)
#define MLPB_LANES (64 * MLPB_WAVES)
#define MLPB_PITCH (POB_MLP_MAX_WIDTH + 8)  // bf16 elements between two rows of an image
#define MLPB_KC 16                           // k of one v_mfma_f32_32x32x16_bf16
#define MLPB_GROUP 4                         // k chunks whose operands are loaded ahead of their MFMAs
#define MLPB_STAGE 8                         // observation elements a lane loads ahead of their LDS stores

typedef __bf16 mlpb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mlpb_bf16x4 __attribute__((ext_vector_type(4)));

static inline int mlpb_chunks(const int in) { return (in + MLPB_KC - 1) / MLPB_KC; }
static inline int mlpb_tiles(const int out) { return (out + 31) / 32; }
// 16-byte fragments (a lane's eight bf16) of one layer, and the workspace of a network in bytes
static inline long long mlpb_layer_frags(const int in, const int out) { return 64LL * mlpb_chunks(in) * mlpb_tiles(out); }
static inline long long mlpb_workspace_bytes(const MlpDesc &d) {
  long long n = 0;
  for (int l = 0; l < d.n_layers; ++l) n += mlpb_layer_frags(d.sizes[l], d.sizes[l + 1]);
  return n * 16;
}
static inline dim3 mlpb_grid(long long B) { return dim3((unsigned)((B + MLPB_ROWS - 1) / MLPB_ROWS)); }

// The operands of the MLPB_GROUP k chunks from c0: the A fragments of this wave's NT tiles (tile t
// lies 4 kc fragments of 64 lanes behind tile t - 1) and the B fragments of its NS row sub-tiles.  A
// chunk past the layer's repeats the last one (no branch between the loads; its MFMA is not issued).
template <int NT, int NS>
POB_MLP_D void mlpb_operands(mlpb_bf16x8 (&a)[2][MLPB_GROUP], mlpb_bf16x8 (&b)[MLPB_SUB][MLPB_GROUP], const __bf16 *src,
                             const mlpb_bf16x8 *wl, const int kc, const int c0) {
#pragma unroll
  for (int u = 0; u < MLPB_GROUP; ++u) {
    const int c = c0 + u < kc ? c0 + u : kc - 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t][u] = wl[(MLPB_WAVES * t * kc + c) * 64];
#pragma unroll
    for (int s = 0; s < NS; ++s) b[s][u] = *(const mlpb_bf16x8 *)(src + 32 * s * MLPB_PITCH + MLPB_KC * c);
  }
}

template <int NT, int NS>
POB_MLP_D void mlpb_mfmas(mlp_f32x16 (&acc)[2][MLPB_SUB], const mlpb_bf16x8 (&a)[2][MLPB_GROUP],
                          const mlpb_bf16x8 (&b)[MLPB_SUB][MLPB_GROUP], const int c0, const int kc) {
#pragma unroll
  for (int u = 0; u < MLPB_GROUP; ++u)
    if (c0 + u < kc) {  // uniform; chunks are summed in ascending order
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < NS; ++s)
          acc[t][s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t][u], b[s][u], acc[t][s], 0, 0, 0);
    }
}

// NT output tiles x NS row sub-tiles: acc[t][s] += W^T X^T over the kc chunks of the layer's input.
// wl: lane's fragment of this wave's first tile, chunk 0; src: lane's row and k half in the image.
// Two register images: a group's operands are loaded while the group before it is multiplied (the
// scheduling barriers keep the loads in front of those MFMAs).
template <int NT, int NS>
POB_MLP_D void mlpb_chain(mlp_f32x16 (&acc)[2][MLPB_SUB], const __bf16 *src, const mlpb_bf16x8 *wl, const int kc) {
  mlpb_bf16x8 a0[2][MLPB_GROUP], b0[MLPB_SUB][MLPB_GROUP], a1[2][MLPB_GROUP], b1[MLPB_SUB][MLPB_GROUP];
  mlpb_operands<NT, NS>(a0, b0, src, wl, kc, 0);
  for (int c0 = 0; c0 < kc; c0 += 2 * MLPB_GROUP) {
    mlpb_operands<NT, NS>(a1, b1, src, wl, kc, c0 + MLPB_GROUP);
    __builtin_amdgcn_sched_barrier(0);
    mlpb_mfmas<NT, NS>(acc, a0, b0, c0, kc);
    __builtin_amdgcn_sched_barrier(0);
    mlpb_operands<NT, NS>(a0, b0, src, wl, kc, c0 + 2 * MLPB_GROUP);
    __builtin_amdgcn_sched_barrier(0);
    mlpb_mfmas<NT, NS>(acc, a1, b1, c0 + MLPB_GROUP, kc);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One layer by the block's four waves: src image (in features) -> dst image (the out features and
// their zero pad up to the next multiple of 32), or, LAST, -> rows [b0, b0 + valid) of y (B, out) in f32.
template <bool LAST>
POB_MLP_D void mlpb_layer(const __bf16 *src, __bf16 *dst, const mlpb_bf16x8 *wp, const float *bias, const int in,
                          const int out, const bool activate, const int act, float *y, const int valid, const int lane,
                          const int wave) {
  const int j = lane & 31, h = lane >> 5;
  const int kc = (in + MLPB_KC - 1) / MLPB_KC, n_tiles = (out + 31) >> 5;
  const bool split = n_tiles * MLPB_SUB <= MLPB_WAVES;  // a wave per (tile, sub-tile) pair
  const int tile0 = split ? wave / MLPB_SUB : wave, sub0 = split ? wave % MLPB_SUB : 0;
  const int nt = tile0 >= n_tiles ? 0 : (!split && wave + MLPB_WAVES < n_tiles ? 2 : 1);  // tiles this wave holds
  const int ns = split ? 1 : MLPB_SUB;
  mlp_f32x16 acc[2][MLPB_SUB];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    mlp_acc_bias(acc[t][0], bias, 32 * (tile0 + MLPB_WAVES * t), out, h);
#pragma unroll
    for (int s = 1; s < MLPB_SUB; ++s) acc[t][s] = acc[t][0];
  }
  const __bf16 *s0 = src + (32 * sub0 + j) * MLPB_PITCH + 8 * h;
  const mlpb_bf16x8 *wl = wp + tile0 * kc * 64 + lane;
  if (nt == 2) mlpb_chain<2, MLPB_SUB>(acc, s0, wl, kc);
  else if (nt == 1 && !split) mlpb_chain<1, MLPB_SUB>(acc, s0, wl, kc);
  else if (nt == 1) mlpb_chain<1, 1>(acc, s0, wl, kc);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < MLPB_SUB; ++s)
      if (t < nt && s < ns) {
        const int row = 32 * (sub0 + s) + j, f0 = 32 * (tile0 + MLPB_WAVES * t) + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = activate ? mlp_activate(act, acc[t][s][4 * q + e]) : acc[t][s][4 * q + e];
          if (LAST) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (row < valid && f0 + 8 * q + e < out) y[(size_t)row * out + f0 + 8 * q + e] = v[e];
          } else {
            mlpb_bf16x4 p;
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = (__bf16)v[e];
            *(mlpb_bf16x4 *)(dst + row * MLPB_PITCH + f0 + 8 * q) = p;
          }
        }
      }
}

// The first image: rows [b0, b0 + 64) of x (B, D), f32, loaded coalesced (MLPB_STAGE in flight a
// lane), normalised if NORM (pob_obsnorm_apply in f32, mean and scale rows 0 and 1 of the (3, D)
// table), rounded to bf16; tail rows repeat the last valid one; features D .. roundup(D, 16) are 0.
template <bool NORM>
POB_MLP_D void mlpb_stage(__bf16 *img, const float *x, const int D, const int b0, const int valid, const float *norm,
                          const float clip, const int tid) {
  const int n = MLPB_ROWS * D;
  for (int e0 = tid; e0 < n; e0 += MLPB_LANES * MLPB_STAGE) {
    float v[MLPB_STAGE], mu[NORM ? MLPB_STAGE : 1], sc[NORM ? MLPB_STAGE : 1];
    int at[MLPB_STAGE];
#pragma unroll
    for (int u = 0; u < MLPB_STAGE; ++u) {
      const int e = e0 + MLPB_LANES * u;
      const bool ok = e < n;
      const int row = ok ? e / D : 0, col = ok ? e - row * D : 0;
      const int rr = row < valid ? row : valid - 1;
      v[u] = x[(size_t)(b0 + rr) * D + col];
      if (NORM) { mu[u] = norm[col]; sc[u] = norm[D + col]; }
      at[u] = ok ? row * MLPB_PITCH + col : -1;
    }
#pragma unroll
    for (int u = 0; u < MLPB_STAGE; ++u)
      if (at[u] >= 0) img[at[u]] = (__bf16)(NORM ? pob_obsnorm_apply(v[u], mu[u], sc[u], clip) : v[u]);
  }
  const int pad = ((D + MLPB_KC - 1) / MLPB_KC) * MLPB_KC - D;
  for (int e = tid; e < MLPB_ROWS * pad; e += MLPB_LANES) {
    const int row = e / pad;
    img[row * MLPB_PITCH + D + (e - row * pad)] = (__bf16)0.0f;
  }
}
