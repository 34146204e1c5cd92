// pob_mlp.hip -- policy networks on the matrix cores (gfx950): the fused MLP forward and the
// tanh-normal actor of DESIGN.md "Policy networks".
//
//   k_mlp_forward   y = MLP(x): every layer in one launch
//   k_mlp_forward_wide   the same, four waves on 64 rows: for wide layers over many rows (pob_mlp_wide.h)
//   k_policy_act   the same forward, then the tanh-normal head (brax NormalTanhDistribution [ext])
//
// The tile code and its layout are pob_mlp_tile.h's.  The other network kernels:
//   pob_mlp_bf16.hip   k_mlp_pack_bf16, k_mlp_forward_bf16: the opt-in bf16 matrix-core forward
//   pob_gru.hip        k_gru_forward, k_gru_policy_act: the recurrent actor
//   pob_mlp_train.hip  k_mlp_forward_train, k_mlp_bwd_* and their four-wave forms: the training passes
//   pob_gru_seq.hip    k_gru_seq_forward, k_gru_seq_backward, k_gru_bwd_weights, k_gru_seq_infer: the recurrent window
//   pob_learner.hip    observation normaliser, GAE, Adam, PPO loss
#include <new>

#include "pob_mlp_wide.h"
#include "pob_policy_head.h"

template <int H, bool NORM>
__global__ __launch_bounds__(64) void k_mlp_forward(const MlpDesc d, const int split, const int B, const float *x,
                                                    const float *theta, float *y, const float *norm, const float clip) {
  __shared__ float img[H * MLP_PITCH];
  float *imgA = img, *imgB = img + split * MLP_PITCH;
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  const float *out = mlp_tile_forward<NORM>(d, imgA, imgB, B, b0, x, theta, nullptr, norm, clip, lane);
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  mlp_tile_store(y, out, 0, d.sizes[d.n_layers], b0, valid, lane);
}

template <bool NORM>
__global__ __launch_bounds__(MLPW_LANES, 2) __attribute__((target("no-packed-fp32-ops"))) void k_mlp_forward_wide(const MlpDesc d, const int B, const float *x,
                                                                 const float *theta, float *y, const float *norm,
                                                                 const float clip) {
  __shared__ float img[POB_MLP_MAX_WIDTH * MLPW_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = blockIdx.x * MLPW_ROWS;
  const int valid = B - b0 < MLPW_ROWS ? B - b0 : MLPW_ROWS;
  mlp_tile_load<NORM, MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(img, x, d.sizes[0], b0, valid, nullptr, nullptr, norm, clip, tid);
  __syncthreads();
  const float *W = theta;
  for (int l = 0; l < d.n_layers; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    const float *bias = W + (size_t)in * out;
    mlpw_layer(img, W, bias, in, out, l != d.n_layers - 1 || d.act_final, d.act, lane, wave);
    W = bias + out;
  }
  mlp_tile_store<MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(y, img, 0, d.sizes[d.n_layers], b0, valid, tid);
}

template <int H, bool NORM>
__global__ __launch_bounds__(64) void k_policy_act(const MlpDesc d, const int split, const int B, const int total,
                                                   const int first, const float *obs, const float *theta,
                                                   const uint32_t *key, const int deterministic, float *action,
                                                   float *logp, float *raw, float *logits, float *obs_copy,
                                                   const float *norm, const float clip) {
  __shared__ float img[H * MLP_PITCH];
  float *imgA = img, *imgB = img + split * MLP_PITCH;
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  float *L = mlp_tile_forward<NORM>(d, imgA, imgB, B, b0, obs, theta, obs_copy, norm, clip, lane);
  float *T = L == imgA ? imgB : imgA;  // the per-component log-probability terms
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  const int A = d.sizes[d.n_layers] >> 1;
  policy_tile_head(L, T, A, b0, valid, total, first, key, deterministic, action, logp, raw, logits, lane);
}

// ============================================================================ C ABI
extern "C" {

int pob_mlp_create(int n_layers, const int *sizes, int activation, int activate_final, pob_mlp **out) {
  if (!out) return pob_fail_msg(POB_EINVAL, "mlp: out is NULL");
  *out = nullptr;
  if (!sizes) return pob_fail_msg(POB_EINVAL, "mlp: sizes is NULL");
  if (n_layers < 1 || n_layers > POB_MLP_MAX_LAYERS) return pob_fail_msg(POB_EINVAL, "mlp: 1 to 8 layers");
  for (int l = 0; l <= n_layers; ++l)
    if (sizes[l] < 1 || sizes[l] > POB_MLP_MAX_WIDTH) return pob_fail_msg(POB_EINVAL, "mlp: every width must be in 1 .. 256");
  if (activation != POB_ACT_RELU && activation != POB_ACT_SWISH && activation != POB_ACT_TANH)
    return pob_fail_msg(POB_EINVAL, "mlp: unknown activation (0 relu, 1 swish, 2 tanh)");
  pob_mlp *m = new (std::nothrow) pob_mlp();
  if (!m) return pob_fail_msg(POB_ENOMEM, "mlp: out of memory");
  m->d.n_layers = n_layers;
  m->n_params = 0;
  for (int l = 0; l <= POB_MLP_MAX_LAYERS; ++l) m->d.sizes[l] = l <= n_layers ? sizes[l] : 0;
  for (int l = 0; l < n_layers; ++l) m->n_params += ((long long)sizes[l] + 1) * sizes[l + 1];
  m->d.act = activation;
  m->d.act_final = activate_final ? 1 : 0;
  *out = m;
  return POB_OK;
}

void pob_mlp_destroy(pob_mlp *m) { delete m; }

int pob_mlp_param_count(const pob_mlp *m, long long *n) {
  if (!m || !n) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument");
  *n = m->n_params;
  return POB_OK;
}

int pob_mlp_forward_norm(const pob_mlp *m, int B, const float *x, const float *theta, float *y, const float *norm,
                         float norm_clip, void *stream) {
  if (!m) return pob_fail_msg(POB_EINVAL, "mlp is NULL");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "mlp: batch size must be positive");
  if (!x || !theta || !y) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument");
  int split;
  const int cls = image_rows(m->d, false, split);
  const dim3 grid = mlp_tile_grid(B);
  hipStream_t st = (hipStream_t)stream;
  TILE_DISPATCH(k_mlp_forward, cls, MLP_HEIGHTS, m->d, split, B, x, theta, y)
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward launch");
}

int pob_mlp_forward(const pob_mlp *m, int B, const float *x, const float *theta, float *y, void *stream) {
  return pob_mlp_forward_norm(m, B, x, theta, y, nullptr, 0.0f, stream);
}

int pob_mlp_forward_wide_norm(const pob_mlp *m, int B, const float *x, const float *theta, float *y, const float *norm,
                              float norm_clip, void *stream) {
  if (!m) return pob_fail_msg(POB_EINVAL, "mlp is NULL");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "mlp: batch size must be positive");
  if (!x || !theta || !y) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument");
  const dim3 grid = mlpw_grid(B);
  hipStream_t st = (hipStream_t)stream;
  if (norm) hipLaunchKernelGGL(k_mlp_forward_wide<true>, grid, dim3(MLPW_LANES), 0, st, m->d, B, x, theta, y, norm, norm_clip);
  else hipLaunchKernelGGL(k_mlp_forward_wide<false>, grid, dim3(MLPW_LANES), 0, st, m->d, B, x, theta, y, norm, norm_clip);
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward_wide launch");
}

int pob_mlp_forward_wide(const pob_mlp *m, int B, const float *x, const float *theta, float *y, void *stream) {
  return pob_mlp_forward_wide_norm(m, B, x, theta, y, nullptr, 0.0f, stream);
}

int pob_policy_act_norm(const pob_mlp *m, int B, int total, int first, const float *obs, const float *theta,
                        uint32_t *key_io, int deterministic, float *action, float *logp, float *raw, float *logits,
                        float *obs_copy, const float *norm, float norm_clip, void *stream) {
  if (!m) return pob_fail_msg(POB_EINVAL, "mlp is NULL");
  const int out = m->d.sizes[m->d.n_layers];
  if (out & 1) return pob_fail_msg(POB_EINVAL, "policy: the last width must be even (loc and scale halves)");
  if (B < 1 || first < 0 || total < 1 || (long long)first + B > total)
    return pob_fail_msg(POB_EINVAL, "policy: bad shard (need first >= 0, B >= 1, first + B <= total)");
  if ((long long)total * (out >> 1) >= 4294967295LL) return pob_fail_msg(POB_EINVAL, "policy: too many action elements");
  if (!obs || !theta || !action) return pob_fail_msg(POB_EINVAL, "policy: NULL argument");
  if (!deterministic && !key_io) return pob_fail_msg(POB_EINVAL, "policy: key is NULL");
  int split;
  const int cls = image_rows(m->d, true, split);
  const dim3 grid = mlp_tile_grid(B);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *key = key_io;
  TILE_DISPATCH(k_policy_act, cls, MLP_HEIGHTS, m->d, split, B, total, first, obs, theta, key, deterministic, action, logp,
                raw, logits, obs_copy)
  if (!deterministic) hipLaunchKernelGGL(k_mlp_advance_key, dim3(1), dim3(1), 0, st, key_io);
  return mlp_hip_check(hipGetLastError(), "k_policy_act launch");
}

int pob_policy_act(const pob_mlp *m, int B, int total, int first, const float *obs, const float *theta,
                   uint32_t *key_io, int deterministic, float *action, float *logp, float *raw, float *logits,
                   float *obs_copy, void *stream) {
  return pob_policy_act_norm(m, B, total, first, obs, theta, key_io, deterministic, action, logp, raw, logits, obs_copy,
                             nullptr, 0.0f, stream);
}

}  // extern "C"
