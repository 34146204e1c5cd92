// pob_lstm.hip -- the recurrent actor with an LSTM cell (DESIGN.md "LSTM cell"): obs -> pre-MLP ->
// LSTM cell -> post-MLP in one launch, the state [h ; c] carried by the caller.
//
//   k_lstm_forward      y, [h' ; c'] = LSTM network(x, [h ; c])
//   k_lstm_policy_act   the same forward, then the tanh-normal head of pob_policy_head.h
//
// The cell loop and the pool's layout are pob_lstm_tile.h's; the entry points are pob_gru.hip's
// (pob_gru_forward_norm, pob_gru_policy_act_norm), which hand an LSTM handle to the launchers here.
#include "pob_lstm_tile.h"
#include "pob_policy_head.h"

// The forward of one tile; [h' ; c'] is stored to h_io on the way.  Returns the image holding the
// post-MLP's output; `other` is the ping-pong image it is not in.
template <bool NORM>
POB_MLP_D float *lstm_tile_forward(const GruDesc &d, float *pool, const int B, const int b0, const float *x,
                                   const float *theta, const float *reset, float *h_io, float *obs_copy, float *h_in_copy,
                                   float *&other, const float *norm, const float clip, const int lane) {
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  const int I = d.pre[d.n_pre], H = d.hid;
  float *C = pool, *S = C + (I + H) * MLP_PITCH, *N = S + H * MLP_PITCH;
  float *P0 = N + H * MLP_PITCH, *P1 = P0 + d.p_rows[0] * MLP_PITCH;
  int pp = 0;
  mlp_tile_load<NORM>(d.n_pre ? P0 : C, x, d.pre[0], b0, valid, obs_copy, nullptr, norm, clip, lane);
  // the state row [h ; c]: h lands behind x, c in S; never normalised
  mlp_tile_load<false>(C + I * MLP_PITCH, h_io, 2 * H, b0, valid, h_in_copy, reset, nullptr, 0.0f, lane);
  __syncthreads();
  const float *W = theta;
  float *src = P0;
  if (d.n_pre) pp = 1;
  for (int l = 0; l < d.n_pre; ++l) {
    const int in = d.pre[l], out = d.pre[l + 1];
    const float *bias = W + (size_t)in * out;
    float *dst = l == d.n_pre - 1 ? C : (pp ? P1 : P0);
    mlp_layer(src, dst, W, bias, in, out, true, d.act, lane);
    __syncthreads();
    W = bias + out;
    src = dst;
    pp ^= 1;
  }
  lstm_cell(C, S, N, W, I, H, lane);
  __syncthreads();
  W += (size_t)4 * H * (I + H) + 4 * H;
  // h is spent: h' takes its rows, so that [h' ; c'] is one image of 2 H features like the one loaded
  for (int e = lane; e < MLP_ROWS * H; e += 64) {
    const int f = e >> 5, env = e & 31;
    C[(I + f) * MLP_PITCH + env] = N[f * MLP_PITCH + env];
  }
  __syncthreads();
  mlp_tile_store(h_io, C, I, 2 * H, b0, valid, lane);
  src = N;
  int in = H;
  for (int l = 0; l < d.n_post; ++l) {
    const int out = d.post[l];
    const float *bias = W + (size_t)in * out;
    float *dst = pp ? P1 : P0;
    mlp_layer(src, dst, W, bias, in, out, l != d.n_post - 1, d.act, lane);
    __syncthreads();
    W = bias + out;
    src = dst;
    in = out;
    pp ^= 1;
  }
  other = pp ? P1 : P0;
  return src;
}

template <int R, bool NORM>
__global__ __launch_bounds__(64) void k_lstm_forward(const GruDesc d, const int B, const float *x, const float *theta,
                                                     const float *reset, float *h_io, float *y, float *h_in_copy,
                                                     const float *norm, const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  float *other;
  const float *out = lstm_tile_forward<NORM>(d, pool, B, b0, x, theta, reset, h_io, nullptr, h_in_copy, other, norm, clip, lane);
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  mlp_tile_store(y, out, 0, d.post[d.n_post - 1], b0, valid, lane);
}

template <int R, bool NORM>
__global__ __launch_bounds__(64) void k_lstm_policy_act(const GruDesc d, const int B, const int total, const int first,
                                                        const float *obs, const float *theta, const uint32_t *key,
                                                        const int deterministic, const float *reset, float *h_io,
                                                        float *action, float *logp, float *raw, float *logits,
                                                        float *obs_copy, float *h_in_copy, const float *norm,
                                                        const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  float *T;  // the per-component log-probability terms
  float *L = lstm_tile_forward<NORM>(d, pool, B, b0, obs, theta, reset, h_io, obs_copy, h_in_copy, T, norm, clip, lane);
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  const int A = d.post[d.n_post - 1] >> 1;
  policy_tile_head(L, T, A, b0, valid, total, first, key, deterministic, action, logp, raw, logits, lane);
}

int lstm_forward_launch(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                        float *y, float *h_in_copy, const float *norm, float norm_clip, hipStream_t st) {
  GruDesc d = g->d;
  lstm_plan(d, false, d.p_rows);
  const dim3 grid = mlp_tile_grid(B);
  TILE_DISPATCH(k_lstm_forward, g->cls_forward, LSTM_HEIGHTS, d, B, x, theta, reset, h_io, y, h_in_copy)
  return mlp_hip_check(hipGetLastError(), "k_lstm_forward launch");
}

int lstm_policy_act_launch(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                           uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action,
                           float *logp, float *raw, float *logits, float *obs_copy, float *h_in_copy, const float *norm,
                           float norm_clip, hipStream_t st) {
  GruDesc d = g->d;
  lstm_plan(d, true, d.p_rows);
  const dim3 grid = mlp_tile_grid(B);
  const uint32_t *key = key_io;
  TILE_DISPATCH(k_lstm_policy_act, g->cls_actor, LSTM_HEIGHTS, d, B, total, first, obs, theta, key, deterministic, reset,
                h_io, action, logp, raw, logits, obs_copy, h_in_copy)
  if (!deterministic) hipLaunchKernelGGL(k_mlp_advance_key, dim3(1), dim3(1), 0, st, key_io);
  return mlp_hip_check(hipGetLastError(), "k_lstm_policy_act launch");
}
