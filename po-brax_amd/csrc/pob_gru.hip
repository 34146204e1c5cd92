// pob_gru.hip -- the recurrent actor (DESIGN.md "Recurrent actor"): obs -> pre-MLP -> GRU cell ->
// post-MLP in one launch, the hidden state carried by the caller.
//
//   k_gru_forward      y, h' = GRU network(x, h)
//   k_gru_policy_act   the same forward, then the tanh-normal head of pob_policy_head.h
//
// The cell and the pool's layout are pob_gru_tile.h's.
#include <new>

#include "pob_lstm_tile.h"
#include "pob_policy_head.h"

// The forward of one tile; h' is stored to h_io on the way.  Returns the image holding the post-
// MLP's output; `other` is the ping-pong image it is not in.
template <bool NORM>
POB_MLP_D float *gru_tile_forward(const GruDesc &d, float *pool, const int B, const int b0, const float *x,
                                  const float *theta, const float *reset, float *h_io, float *obs_copy, float *h_in_copy,
                                  float *&other, const float *norm, const float clip, const int lane) {
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  const int I = d.pre[d.n_pre], H = d.hid;
  float *C = pool, *N = C + (I + H) * MLP_PITCH;
  float *P0 = N + H * MLP_PITCH, *P1 = P0 + d.p_rows[0] * MLP_PITCH;
  int pp = 0;
  mlp_tile_load<NORM>(d.n_pre ? P0 : C, x, d.pre[0], b0, valid, obs_copy, nullptr, norm, clip, lane);
  mlp_tile_load<false>(C + I * MLP_PITCH, h_io, H, b0, valid, h_in_copy, reset, nullptr, 0.0f, lane);  // h: never normalised
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
  gru_cell(C, N, W, I, H, lane);
  __syncthreads();
  W += (size_t)3 * H * I + (size_t)3 * H * H + 4 * H;
  mlp_tile_store(h_io, N, 0, H, b0, valid, lane);
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
__global__ __launch_bounds__(64) void k_gru_forward(const GruDesc d, const int B, const float *x, const float *theta,
                                                    const float *reset, float *h_io, float *y, float *h_in_copy,
                                                    const float *norm, const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  float *other;
  const float *out = gru_tile_forward<NORM>(d, pool, B, b0, x, theta, reset, h_io, nullptr, h_in_copy, other, norm, clip, lane);
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  mlp_tile_store(y, out, 0, d.post[d.n_post - 1], b0, valid, lane);
}

template <int R, bool NORM>
__global__ __launch_bounds__(64) void k_gru_policy_act(const GruDesc d, const int B, const int total, const int first,
                                                       const float *obs, const float *theta, const uint32_t *key,
                                                       const int deterministic, const float *reset, float *h_io,
                                                       float *action, float *logp, float *raw, float *logits,
                                                       float *obs_copy, float *h_in_copy, const float *norm,
                                                       const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  float *T;  // the per-component log-probability terms
  float *L = gru_tile_forward<NORM>(d, pool, B, b0, obs, theta, reset, h_io, obs_copy, h_in_copy, T, norm, clip, lane);
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  const int A = d.post[d.n_post - 1] >> 1;
  policy_tile_head(L, T, A, b0, valid, total, first, key, deterministic, action, logp, raw, logits, lane);
}

// pob_gru_create and pob_lstm_create: the limits and the descriptor are the same, the cell's share
// of theta and the pool's plan are not.  The messages keep the "gru:" prefix for either cell: they
// name limits of the recurrent network, not of the cell.
static int recurrent_create(const int cell, int n_pre, const int *pre_sizes, int hidden, int n_post, const int *post_sizes,
                            int activation, pob_gru **out) {
  if (!out) return pob_fail_msg(POB_EINVAL, "gru: out is NULL");
  *out = nullptr;
  if (!pre_sizes || !post_sizes) return pob_fail_msg(POB_EINVAL, "gru: sizes is NULL");
  if (n_pre < 0 || n_pre > POB_GRU_MAX_PRE || n_post < 1 || n_post > POB_GRU_MAX_POST)
    return pob_fail_msg(POB_EINVAL, "gru: 0 to 3 pre-MLP and 1 to 4 post-MLP layers (at most 8 layers with the cell)");
  for (int l = 0; l <= n_pre; ++l)
    if (pre_sizes[l] < 1 || pre_sizes[l] > POB_MLP_MAX_WIDTH)
      return pob_fail_msg(POB_EINVAL, "gru: every width must be in 1 .. 256");
  for (int l = 0; l < n_post; ++l)
    if (post_sizes[l] < 1 || post_sizes[l] > POB_MLP_MAX_WIDTH)
      return pob_fail_msg(POB_EINVAL, "gru: every width must be in 1 .. 256");
  if (hidden < 1 || hidden > POB_GRU_MAX_HIDDEN) return pob_fail_msg(POB_EINVAL, "gru: the hidden width must be in 1 .. 128");
  if (pre_sizes[n_pre] + hidden > POB_MLP_MAX_WIDTH)
    return pob_fail_msg(POB_EINVAL, "gru: the cell's input and hidden widths together must be at most 256");
  if (activation != POB_ACT_RELU && activation != POB_ACT_SWISH && activation != POB_ACT_TANH)
    return pob_fail_msg(POB_EINVAL, "gru: unknown activation (0 relu, 1 swish, 2 tanh)");
  pob_gru *g = new (std::nothrow) pob_gru();
  if (!g) return pob_fail_msg(POB_ENOMEM, "gru: out of memory");
  GruDesc &d = g->d;
  d.n_pre = n_pre; d.n_post = n_post; d.hid = hidden; d.act = activation;
  for (int l = 0; l <= POB_GRU_MAX_PRE; ++l) d.pre[l] = l <= n_pre ? pre_sizes[l] : 0;
  for (int l = 0; l < POB_GRU_MAX_POST; ++l) d.post[l] = l < n_post ? post_sizes[l] : 0;
  long long n = 0;
  for (int l = 0; l < n_pre; ++l) n += ((long long)d.pre[l] + 1) * d.pre[l + 1];
  const long long I = d.pre[n_pre], H = hidden;
  n += cell == POB_CELL_LSTM ? 4 * H * (I + H) + 4 * H : 3 * H * I + 3 * H * H + 4 * H;
  long long in = H;
  for (int l = 0; l < n_post; ++l) { n += (in + 1) * d.post[l]; in = d.post[l]; }
  g->n_params = n;
  g->cell = cell;
  g->cls_forward = cell == POB_CELL_LSTM ? lstm_plan(d, false, nullptr) : gru_plan(d, false, nullptr);
  g->cls_actor = cell == POB_CELL_LSTM ? lstm_plan(d, true, nullptr) : gru_plan(d, true, nullptr);
  *out = g;
  return POB_OK;
}

extern "C" {

int pob_gru_create(int n_pre, const int *pre_sizes, int hidden, int n_post, const int *post_sizes, int activation,
                   pob_gru **out) {
  return recurrent_create(POB_CELL_GRU, n_pre, pre_sizes, hidden, n_post, post_sizes, activation, out);
}

int pob_lstm_create(int n_pre, const int *pre_sizes, int hidden, int n_post, const int *post_sizes, int activation,
                    pob_gru **out) {
  return recurrent_create(POB_CELL_LSTM, n_pre, pre_sizes, hidden, n_post, post_sizes, activation, out);
}

void pob_gru_destroy(pob_gru *g) { delete g; }

int pob_gru_param_count(const pob_gru *g, long long *n) {
  if (!g || !n) return pob_fail_msg(POB_EINVAL, "gru: NULL argument");
  *n = g->n_params;
  return POB_OK;
}

int pob_gru_forward_norm(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                         float *y, float *h_in_copy, const float *norm, float norm_clip, void *stream) {
  if (!g) return pob_fail_msg(POB_EINVAL, "gru is NULL");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "gru: batch size must be positive");
  if (!x || !theta || !y) return pob_fail_msg(POB_EINVAL, "gru: NULL argument");
  if (!h_io) return pob_fail_msg(POB_EINVAL, "gru: h_io is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (g->cell == POB_CELL_LSTM) return lstm_forward_launch(g, B, x, theta, reset, h_io, y, h_in_copy, norm, norm_clip, st);
  GruDesc d = g->d;
  gru_plan(d, false, d.p_rows);
  const dim3 grid = mlp_tile_grid(B);
  TILE_DISPATCH(k_gru_forward, g->cls_forward, GRU_HEIGHTS, d, B, x, theta, reset, h_io, y, h_in_copy)
  return mlp_hip_check(hipGetLastError(), "k_gru_forward launch");
}

int pob_gru_forward(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                    float *y, float *h_in_copy, void *stream) {
  return pob_gru_forward_norm(g, B, x, theta, reset, h_io, y, h_in_copy, nullptr, 0.0f, stream);
}

int pob_gru_policy_act_norm(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                            uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action,
                            float *logp, float *raw, float *logits, float *obs_copy, float *h_in_copy, const float *norm,
                            float norm_clip, void *stream) {
  if (!g) return pob_fail_msg(POB_EINVAL, "gru is NULL");
  const int out = g->d.post[g->d.n_post - 1];
  if (out & 1) return pob_fail_msg(POB_EINVAL, "policy: the last width must be even (loc and scale halves)");
  if (B < 1 || first < 0 || total < 1 || (long long)first + B > total)
    return pob_fail_msg(POB_EINVAL, "policy: bad shard (need first >= 0, B >= 1, first + B <= total)");
  if ((long long)total * (out >> 1) >= 4294967295LL) return pob_fail_msg(POB_EINVAL, "policy: too many action elements");
  if (!obs || !theta || !action) return pob_fail_msg(POB_EINVAL, "policy: NULL argument");
  if (!h_io) return pob_fail_msg(POB_EINVAL, "policy: h_io is NULL");
  if (!deterministic && !key_io) return pob_fail_msg(POB_EINVAL, "policy: key is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (g->cell == POB_CELL_LSTM)
    return lstm_policy_act_launch(g, B, total, first, obs, theta, key_io, deterministic, reset, h_io, action, logp, raw,
                                  logits, obs_copy, h_in_copy, norm, norm_clip, st);
  GruDesc d = g->d;
  gru_plan(d, true, d.p_rows);
  const dim3 grid = mlp_tile_grid(B);
  const uint32_t *key = key_io;
  TILE_DISPATCH(k_gru_policy_act, g->cls_actor, GRU_HEIGHTS, d, B, total, first, obs, theta, key, deterministic, reset, h_io,
                action, logp, raw, logits, obs_copy, h_in_copy)
  if (!deterministic) hipLaunchKernelGGL(k_mlp_advance_key, dim3(1), dim3(1), 0, st, key_io);
  return mlp_hip_check(hipGetLastError(), "k_gru_policy_act launch");
}

int pob_gru_policy_act(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                       uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action, float *logp,
                       float *raw, float *logits, float *obs_copy, float *h_in_copy, void *stream) {
  return pob_gru_policy_act_norm(g, B, total, first, obs, theta, key_io, deterministic, reset, h_io, action, logp, raw,
                                 logits, obs_copy, h_in_copy, nullptr, 0.0f, stream);
}

}  // extern "C"
