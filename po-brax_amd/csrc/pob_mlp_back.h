// pob_mlp_back.h -- the one-wave tile code the training passes share (pob_mlp_train.hip,
// pob_gru_seq.hip): the saved pre-activations of a training forward, the transposed product of a
// backward walk, and the reduction that finishes a parameter gradient (DESIGN.md "MLP backward").
#pragma once
#include "pob_mlp_tile.h"

POB_MLP_D bool mlp_activated(const MlpDesc &d, const int l) { return l != d.n_layers - 1 || d.act_final; }

// element e of an image's first 32 * width floats as its place in the image
POB_MLP_D int mlp_img_at(const int e) { return (e >> 5) * MLP_PITCH + (e & 31); }

// dst image (in features) <- W (in, out) row-major times the src image (out features): per
// element acc = +0 and one fmaf(W[i][k], src[k], acc) per k in the order of mlp_kfeat
POB_MLP_D void mlp_layer_back(const float *src, float *dst, const float *W, const int in, const int out, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int ks = mlp_ksteps(out);
  for (int it = 0; it < in; it += 32) {
    const int row = it + j;
    const bool rok = row < in;
    mlp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int s0 = 0; s0 < ks; s0 += MLP_KUNROLL) {
      float a[MLP_KUNROLL], b[MLP_KUNROLL];
#pragma unroll
      for (int u = 0; u < MLP_KUNROLL; ++u) {
        const int k = mlp_kfeat(s0 + u, h);
        const bool kok = k < out;
        a[u] = (kok && rok) ? W[(size_t)row * out + k] : 0.0f;
        b[u] = kok ? src[k * MLP_PITCH + j] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < MLP_KUNROLL; ++u)
        if (s0 + u < ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = it + mlp_acc_row(r, h);
      if (i < in) dst[i * MLP_PITCH + j] = acc[r];
    }
  }
}

// One tile's chain of a transposed product: acc += sum over the `out` features of src of
// W[row][k] src[k][env] in the order of mlp_kfeat (W's rows are ldw floats apart; rok: this lane's
// row exists).  mlp_layer_back's inner loop, so that two matrices can share one accumulator.
POB_MLP_D void mlp_chain_back(mlp_f32x16 &acc, const float *src, const float *W, const int ldw, const int row,
                              const bool rok, const int out, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int ks = mlp_ksteps(out);
  for (int s0 = 0; s0 < ks; s0 += MLP_KUNROLL) {
    float a[MLP_KUNROLL], b[MLP_KUNROLL];
#pragma unroll
    for (int u = 0; u < MLP_KUNROLL; ++u) {
      const int k = mlp_kfeat(s0 + u, h);
      const bool kok = k < out;
      a[u] = (kok && rok) ? W[(size_t)row * ldw + k] : 0.0f;
      b[u] = kok ? src[k * MLP_PITCH + j] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < MLP_KUNROLL; ++u)
      if (s0 + u < ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
  }
}

// dtheta <- the (n_chunks, n_params) float64 chunk partials added per parameter in ascending chunk
// order and rounded once (the last launch of pob_mlp_train.hip's and pob_gru_seq.hip's backward)
#define MLP_BWD_RSTAGE 32  // chunk partials a lane loads ahead of their adds
static __global__ __launch_bounds__(256) void k_mlp_bwd_reduce(const double *partials, const long long n_chunks,
                                                               const long long n_params, float *dtheta) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_params) return;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += MLP_BWD_RSTAGE) {
    double v[MLP_BWD_RSTAGE];
#pragma unroll
    for (int u = 0; u < MLP_BWD_RSTAGE; ++u) v[u] = c0 + u < n_chunks ? partials[(size_t)(c0 + u) * n_params + p] : 0.0;
#pragma unroll
    for (int u = 0; u < MLP_BWD_RSTAGE; ++u)
      if (c0 + u < n_chunks) T = T + v[u];
  }
  dtheta[p] = (float)T;
}
