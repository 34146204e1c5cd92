// pob_mlp_wide.h -- the four-wave ("wide") layout of the MLP kernels, shared by the wide forward
// (pob_mlp.hip k_mlp_forward_wide) and the wide training pass (pob_mlp_train.hip).
//
// The same networks and the same bits as k_mlp_forward, laid out for wide layers over many rows
// (the critic's [obs -> 256 x 5 -> 1]; DESIGN.md "Wide forward").  A block of
// MLPW_WAVES = 4 waves owns MLPW_ROWS = 64 consecutive rows, i.e. MLPW_SUB = 2 row sub-tiles of 32.
// Their activations are ONE LDS image [feature][row] of 256 features at pitch 65 floats (odd: the
// row-major staging, where consecutive lanes walk features, and the operand reads, where they walk
// rows, both touch 32 different banks), 66 560 B: two blocks, eight waves, two per SIMD on a CU.
// The waves split a layer's OUTPUT tiles: wave w holds tiles w and w + 4 (32 (w + 4 i)), each for
// both row sub-tiles, so a k-step is two global loads of a weight fragment (still W[k][col] of the
// caller's theta, never copied) and two LDS reads feeding four MFMAs into four accumulators: per
// MFMA a quarter of the one-wave kernel's LDS reads and half its global loads, and theta is read
// from L2 once per 64 rows, not once per 32.  Operands are loaded one chunk of MLPW_KUNROLL k-steps
// ahead of the chunk whose MFMAs run (two register images).  A layer with so few output tiles
// that tiles x sub-tiles <= waves (the final 256 -> 1) gives each (tile, sub-tile) pair to a wave
// of its own.  The layer is rewritten in place: every wave has read every k of the image before
// it holds its outputs, so the block barriers once between the last read and the first write and
// once after the write.  Per output element the chain is mlp_chain's: bias, then the k-steps of
// mlp_kfeat in ascending order.
#pragma once
#include "pob_mlp_tile.h"

#define MLPW_WAVES 4
#define MLPW_SUB 2
#define MLPW_ROWS (MLP_ROWS * MLPW_SUB)
#define MLPW_LANES (64 * MLPW_WAVES)
#define MLPW_PITCH (MLPW_ROWS + 1)
#define MLPW_KUNROLL 8

// the four-wave kernels' grid: a block per 64 rows
static inline dim3 mlpw_grid(long long B) { return dim3((unsigned)((B + MLPW_ROWS - 1) / MLPW_ROWS)); }

// the operands of k-steps [s0, s0 + MLPW_KUNROLL): tile t's column is col0 + 32 MLPW_WAVES t of
// W (out columns), sub-tile s starts 32 s rows into src; a k-step past the layer's gives zeros
template <int NT, int NS>
POB_MLP_D void mlpw_operands(float (&a)[2][MLPW_KUNROLL], float (&b)[MLPW_SUB][MLPW_KUNROLL], const float *src,
                             const float *W, const int out, const int col0, const int in, const int s0, const int lane) {
  // every load is issued by every lane, from an address clamped into the layer, and a value from
  // past it replaced by 0 afterwards: no branch between the loads, so all of a chunk's are in flight
  // together (32-bit offsets from the uniform W and src: at most 256 x 256 floats)
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int u = 0; u < MLPW_KUNROLL; ++u) {
    const int k = mlp_kfeat(s0 + u, h);
    const bool kok = k < in;
    const unsigned kc = kok ? k : in - 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = col0 + 32 * MLPW_WAVES * t;
      const bool cok = col < out;
      const float w = W[kc * (unsigned)out + (unsigned)(cok ? col : out - 1)];
      a[t][u] = (kok && cok) ? w : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float v = src[kc * MLPW_PITCH + 32 * s + j];
      b[s][u] = kok ? v : 0.0f;
    }
  }
}

template <int NT, int NS>
POB_MLP_D void mlpw_mfmas(mlp_f32x16 (&acc)[2][MLPW_SUB], const float (&a)[2][MLPW_KUNROLL],
                          const float (&b)[MLPW_SUB][MLPW_KUNROLL], const int s0, const int ks) {
  if (s0 + MLPW_KUNROLL <= ks) {  // a whole chunk: no branch between its MFMAs
#pragma unroll
    for (int u = 0; u < MLPW_KUNROLL; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[t][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][u], b[s][u], acc[t][s], 0, 0, 0);
    return;
  }
#pragma unroll
  for (int u = 0; u < MLPW_KUNROLL; ++u)
    if (s0 + u < ks) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[t][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][u], b[s][u], acc[t][s], 0, 0, 0);
    }
}

// NT output tiles x NS row sub-tiles of one layer: acc[t][s] += the chain over the `in` features
template <int NT, int NS>
POB_MLP_D void mlpw_chain(mlp_f32x16 (&acc)[2][MLPW_SUB], const float *src, const float *W, const int out, const int col0,
                          const int in, const int lane) {
  const int ks = mlp_ksteps(in);
  float a0[2][MLPW_KUNROLL], b0[MLPW_SUB][MLPW_KUNROLL], a1[2][MLPW_KUNROLL], b1[MLPW_SUB][MLPW_KUNROLL];
  mlpw_operands<NT, NS>(a0, b0, src, W, out, col0, in, 0, lane);
  for (int s0 = 0; s0 < ks; s0 += 2 * MLPW_KUNROLL) {
    mlpw_operands<NT, NS>(a1, b1, src, W, out, col0, in, s0 + MLPW_KUNROLL, lane);
    mlpw_mfmas<NT, NS>(acc, a0, b0, s0, ks);
    mlpw_operands<NT, NS>(a0, b0, src, W, out, col0, in, s0 + 2 * MLPW_KUNROLL, lane);
    mlpw_mfmas<NT, NS>(acc, a1, b1, s0 + MLPW_KUNROLL, ks);
  }
}

// one layer, the image's first `in` features -> its first `out` features, by the block's four waves
POB_MLP_D void mlpw_layer(float *img, const float *W, const float *bias, const int in, const int out, const bool activate,
                          const int act, const int lane, const int wave) {
  const int j = lane & 31, h = lane >> 5;
  const int n_tiles = (out + 31) >> 5;
  const bool split = n_tiles * MLPW_SUB <= MLPW_WAVES;  // a wave per (tile, sub-tile) pair
  const int tile0 = split ? wave / MLPW_SUB : wave, sub0 = split ? wave % MLPW_SUB : 0;
  const int nt = tile0 >= n_tiles ? 0 : (!split && wave + MLPW_WAVES < n_tiles ? 2 : 1);  // tiles this wave holds
  const int ns = split ? 1 : MLPW_SUB;
  const int ot = 32 * tile0;
  mlp_f32x16 acc[2][MLPW_SUB];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    mlp_acc_bias(acc[t][0], bias, ot + 32 * MLPW_WAVES * t, out, h);
#pragma unroll
    for (int s = 1; s < MLPW_SUB; ++s) acc[t][s] = acc[t][0];
  }
  const float *src = img + 32 * sub0;
  if (nt == 2) mlpw_chain<2, MLPW_SUB>(acc, src, W, out, ot + j, in, lane);
  else if (nt == 1 && !split) mlpw_chain<1, MLPW_SUB>(acc, src, W, out, ot + j, in, lane);
  else if (nt == 1) mlpw_chain<1, 1>(acc, src, W, out, ot + j, in, lane);
  __syncthreads();  // every wave has read every k: the image may be rewritten
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < MLPW_SUB; ++s)
      if (t < nt && s < ns) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = ot + 32 * MLPW_WAVES * t + mlp_acc_row(r, h);
          if (i < out) img[i * MLPW_PITCH + 32 * (sub0 + s) + j] = activate ? mlp_activate(act, acc[t][s][r]) : acc[t][s][r];
        }
      }
  __syncthreads();
}
