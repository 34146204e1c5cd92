// pob_mlp_bf16.hip -- the MLP forward with bf16 operands on the matrix cores (gfx950,
// v_mfma_f32_32x32x16_bf16) and f32 accumulation: the opt-in mixed-precision inference pass of the
// critic (DESIGN.md "Bf16 forward"; layouts and the layer in pob_mlp_bf16.h).
//
//   k_mlp_pack_bf16      theta's matrices -> bf16 in fragment order, into the caller's workspace
//   k_mlp_forward_bf16   y = MLP(x): every layer in one launch, four waves on 64 rows
//
// Both are launched by every call, the pack first on the same stream: theta is read at launch time,
// so an in-place optimiser step between two replays of a captured graph is seen.
#include "pob_mlp_bf16.h"

// One lane's fragment a thread: ws[(t kc + c) 64 + l] <- W[16 c + 8 (l >> 5) + e][32 t + (l & 31)], e = 0 .. 7,
// zero past the layer.  Consecutive lanes read consecutive columns of a row of W.
__global__ __launch_bounds__(256) void k_mlp_pack_bf16(const MlpDesc d, const float *theta, mlpb_bf16x8 *ws,
                                                        const int n_frags) {
  int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frags) return;
  mlpb_bf16x8 *dst = ws + f;
  const float *W = theta;
  int l = 0, in = d.sizes[0], out = d.sizes[1];
  for (;; ++l) {  // the layer of fragment f: f < n_frags, so l stays below n_layers
    in = d.sizes[l];
    out = d.sizes[l + 1];
    const int n = 64 * ((in + MLPB_KC - 1) / MLPB_KC) * ((out + 31) >> 5);
    if (f < n) break;
    f -= n;
    W += (size_t)(in + 1) * out;
  }
  const int kc = (in + MLPB_KC - 1) / MLPB_KC;
  const int lane = f & 63, c = (f >> 6) % kc, t = (f >> 6) / kc;
  const int col = 32 * t + (lane & 31), k0 = MLPB_KC * c + 8 * (lane >> 5);
  mlpb_bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bool ok = col < out && k0 + e < in;
    v[e] = (__bf16)(ok ? W[(k0 + e) * out + col] : 0.0f);
  }
  *dst = v;
}

template <bool NORM>
__global__ __launch_bounds__(MLPB_LANES, 2) void k_mlp_forward_bf16(const MlpDesc d, const int B, const float *x,
                                                                    const float *theta, const mlpb_bf16x8 *ws, float *y,
                                                                    const float *norm, const float clip) {
  __shared__ __attribute__((aligned(16))) __bf16 img[2][MLPB_ROWS * MLPB_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = blockIdx.x * MLPB_ROWS;
  const int valid = B - b0 < MLPB_ROWS ? B - b0 : MLPB_ROWS;
  mlpb_stage<NORM>(img[0], x, d.sizes[0], b0, valid, norm, clip, tid);
  __syncthreads();
  const float *W = theta;
  const int last = d.n_layers - 1;
  for (int l = 0; l < last; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    const float *bias = W + (size_t)in * out;
    mlpb_layer<false>(img[l & 1], img[(l + 1) & 1], ws, bias, in, out, true, d.act, nullptr, 0, lane, wave);
    __syncthreads();  // the one barrier of the layer: the other image is not written before the next one
    W = bias + out;
    ws += 64 * ((in + MLPB_KC - 1) / MLPB_KC) * ((out + 31) >> 5);
  }
  const int in = d.sizes[last], out = d.sizes[last + 1];
  mlpb_layer<true>(img[last & 1], nullptr, ws, W + (size_t)in * out, in, out, d.act_final != 0, d.act,
                   y + (size_t)b0 * out, valid, lane, wave);
}

// ============================================================================ C ABI
extern "C" {

int pob_mlp_bf16_workspace_bytes(const pob_mlp *m, long long *bytes) {
  if (!m || !bytes) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument");
  *bytes = mlpb_workspace_bytes(m->d);
  return POB_OK;
}

int pob_mlp_forward_bf16_norm(const pob_mlp *m, int B, const float *x, const float *theta, float *y, const float *norm,
                              float norm_clip, void *workspace, void *stream) {
  if (!m) return pob_fail_msg(POB_EINVAL, "mlp is NULL");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "mlp: batch size must be positive");
  if (!x || !theta || !y || !workspace) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  mlpb_bf16x8 *ws = (mlpb_bf16x8 *)workspace;
  const int n_frags = (int)(mlpb_workspace_bytes(m->d) / 16);  // at most 8 layers x 8 tiles x 16 chunks x 64
  hipLaunchKernelGGL(k_mlp_pack_bf16, dim3((n_frags + 255) / 256), dim3(256), 0, st, m->d, theta, ws, n_frags);
  const dim3 grid = mlpb_grid(B);
  if (norm) hipLaunchKernelGGL(k_mlp_forward_bf16<true>, grid, dim3(MLPB_LANES), 0, st, m->d, B, x, theta, ws, y, norm, norm_clip);
  else hipLaunchKernelGGL(k_mlp_forward_bf16<false>, grid, dim3(MLPB_LANES), 0, st, m->d, B, x, theta, ws, y, norm, norm_clip);
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward_bf16 launch");
}

int pob_mlp_forward_bf16(const pob_mlp *m, int B, const float *x, const float *theta, float *y, void *workspace,
                         void *stream) {
  return pob_mlp_forward_bf16_norm(m, B, x, theta, y, nullptr, 0.0f, workspace, stream);
}

}  // extern "C"
