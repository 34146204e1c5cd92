// pob_gru_seq_bf16.hip -- the recurrent window for inference with bf16 operands on the matrix cores
// (gfx950, v_mfma_f32_32x32x16_bf16) and f32 accumulation: the opt-in mixed-precision pass of the
// recurrent critic (DESIGN.md "Bf16 recurrent window"; layouts and layers in pob_gru_bf16.h).
//
//   k_gru_pack_bf16        theta's matrices -> bf16 in fragment order, the cell's fused, into the workspace
//   k_gru_seq_infer_bf16   S steps of obs -> pre-MLP -> GRU cell -> post-MLP in one launch, four waves
//                          on 64 sequences, the f32 h in registers, its bf16 image in LDS
//
// Both are launched by every call, the pack first on the same stream: theta is read at launch time,
// so an in-place optimiser step between two replays of a captured graph is seen.  Vector stores
// only, no atomics, no scratch, no allocation, no host synchronisation.
#include "pob_gru_bf16.h"

// One lane's fragment a thread, in the order the window kernel walks the workspace: the pre-MLP's
// layers, the fused cell, the post-MLP's layers.
__global__ __launch_bounds__(256) void k_gru_pack_bf16(const GruDesc d, const float *theta, grub_bf16x8 *ws,
                                                        const int n_frags) {
  int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frags) return;
  grub_bf16x8 *dst = ws + f;
  const float *W = theta;
  const int I = d.pre[d.n_pre], H = d.hid;
  for (int l = 0; l < d.n_pre; ++l) {
    const int in = d.pre[l], out = d.pre[l + 1], n = grub_dense_frags(in, out);
    if (f < n) { *dst = grub_pack_dense(W, in, out, f); return; }
    f -= n;
    W += (size_t)(in + 1) * out;
  }
  {
    const int n = grub_cell_frags(I, H);
    if (f < n) { *dst = grub_pack_cell(W, I, H, f); return; }
    f -= n;
    W += (size_t)3 * H * I + (size_t)3 * H * H + 4 * H;
  }
  int in = H;
  for (int l = 0; l < d.n_post; ++l) {
    const int out = d.post[l], n = grub_dense_frags(in, out);
    if (f < n) { *dst = grub_pack_dense(W, in, out, f); return; }
    f -= n;
    W += (size_t)(in + 1) * out;
    in = out;
  }
}

// POOL: the LDS pool's bytes (two classes: two blocks a CU, or the widest networks' one).
template <int POOL, bool NORM>
__global__ __launch_bounds__(GRUB_LANES, POOL <= 81920 ? 2 : 1) void k_gru_seq_infer_bf16(const GruDesc d, const GrubArgs a, const float *obs,
                                                                      const int32_t *idx, const float *h0,
                                                                      const float *reset, const float *theta,
                                                                      const grub_bf16x8 *ws, float *y, float *h_first,
                                                                      float *h_out, const float *norm) {
  __shared__ __attribute__((aligned(16))) unsigned char pool[POOL];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int m0 = blockIdx.x * GRUB_ROWS;
  const int valid = a.M - m0 < GRUB_ROWS ? a.M - m0 : GRUB_ROWS;
  const int D = d.pre[0], I = d.pre[d.n_pre], H = d.hid, out_w = d.post[d.n_post - 1];
  const int ph = grub_pitch(H), kcx = grub_chunks(I), kc = kcx + grub_chunks(H);
  int *envs = (int *)pool;
  __bf16 *Hb = (__bf16 *)(pool + GRUB_ENV_BYTES);
  __bf16 *P0 = Hb + GRUB_ROWS * ph, *P1 = P0 + GRUB_ROWS * a.pit0;
  if (tid < GRUB_ROWS) {
    const int rr = tid < valid ? tid : valid - 1;  // tail rows repeat the last valid one
    envs[tid] = idx ? idx[m0 + rr] : m0 + rr;
  }
  // The cell's units: H <= 64 gives each wave one (H tile, sub-tile) pair; wider, a wave takes a tile's
  // two sub-tiles in turn.  The unit's f32 h stays in hreg[.] of the lanes that compute it.
  const int ntH = grub_tiles(H);
  const bool split = 2 * ntH <= GRUB_WAVES;
  const int T0 = split ? wave >> 1 : wave, S0 = split ? wave & 1 : 0;
  const int nu = T0 < ntH ? (split ? 1 : 2) : 0;
  // hA / envA are the unit the loops below work on; after each unit a wave of two units swaps them
  // with hB / envB (a static register array cannot be indexed by the unit)
  float hA[16], hB[16];
  int envA, envB;
  {
    const int r0 = 32 * S0 + j, r1 = r0 + 32;
    envA = idx ? idx[m0 + (r0 < valid ? r0 : valid - 1)] : m0 + (r0 < valid ? r0 : valid - 1);
    envB = idx ? idx[m0 + (r1 < valid ? r1 : valid - 1)] : m0 + (r1 < valid ? r1 : valid - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * T0 + mlp_acc_row(r, hh);
      hA[r] = (nu > 0 && f < H) ? h0[(size_t)envA * H + f] : 0.0f;
      hB[r] = (nu > 1 && f < H) ? h0[(size_t)envB * H + f] : 0.0f;
    }
  }
#define GRUB_NEXT_UNIT()                                                  \
  if (nu == 2) {                                                          \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                      \
      const float t = hA[r]; hA[r] = hB[r]; hB[r] = t;                    \
    }                                                                     \
    const int t = envA; envA = envB; envB = t;                            \
  }
  for (int s = 0; s < a.S; ++s) {
    __syncthreads();  // the last step's readers of Hb, P0 and P1 are done (step 0: envs is written)
    // ---- the reset, h_first, and Hb where h changed behind the image's back
    for (int i = 0; i < nu; ++i) {
      const int row = 32 * (S0 + i) + j;
      const bool zero = reset && reset[(size_t)s * a.B + envA] != 0.0f;
      if (zero) {
#pragma unroll
        for (int r = 0; r < 16; ++r) hA[r] = 0.0f;
      }
      if (s == 0 && h_first && row < valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = 32 * T0 + mlp_acc_row(r, hh);
          if (f < H) h_first[(size_t)(m0 + row) * H + f] = hA[r];
        }
      }
      if (s == 0 || zero) grub_store_h(Hb, ph, row, T0, hh, hA);
      GRUB_NEXT_UNIT()
    }
    grub_stage<NORM>(P0, a.pit0, obs + (size_t)s * a.B * D, D, envs, norm, a.clip, tid);
    __syncthreads();
    // ---- the pre-MLP: x ends in P0 or P1 by cur
    const float *W = theta;
    const grub_bf16x8 *wp = ws;
    int cur = 0;
    for (int l = 0; l < d.n_pre; ++l) {
      const int in = d.pre[l], out = d.pre[l + 1];
      const float *bias = W + (size_t)in * out;
      grub_layer<false>(cur ? P1 : P0, cur ? a.pit1 : a.pit0, cur ? P0 : P1, cur ? a.pit0 : a.pit1, wp, bias, in, out, true,
                        d.act, nullptr, 0, lane, wave);
      __syncthreads();
      W = bias + out;
      wp += grub_dense_frags(in, out);
      cur ^= 1;
    }
    // ---- the cell: the products of every unit, gates and blend in registers
    {
      const float *b_rz = W + (size_t)(I + H) * 2 * H, *b_xn = b_rz + 2 * H + (size_t)I * H;
      const float *b_hn = b_xn + H + (size_t)H * H;
      const __bf16 *X = cur ? P1 : P0;
      const int px = cur ? a.pit1 : a.pit0;
      for (int i = 0; i < nu; ++i) {
        const int row = 32 * (S0 + i) + j;
        mlp_f32x16 ar, az, ax, ah;
        mlp_acc_bias(ar, b_rz, 32 * T0, H, hh);
        mlp_acc_bias(az, b_rz + H, 32 * T0, H, hh);
        mlp_acc_bias(ax, b_xn, 32 * T0, H, hh);
        mlp_acc_bias(ah, b_hn, 32 * T0, H, hh);
        grub_cell_chain(ar, az, ax, ah, X + row * px + 8 * hh, Hb + row * ph + 8 * hh, wp + T0 * kc * 3 * 64 + lane, kcx, kc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float rg = pob_sigmoidf(ar[r]), zg = pob_sigmoidf(az[r]);
          const float n = pob_tanhf(MLP_FMA(rg, ah[r], ax[r]));
          const float hn = MLP_FMA(zg, hA[r] - n, n);
          hA[r] = 32 * T0 + mlp_acc_row(r, hh) < H ? hn : 0.0f;
        }
        GRUB_NEXT_UNIT()
      }
      W += (size_t)3 * H * I + (size_t)3 * H * H + 4 * H;
      wp += grub_cell_frags(I, H);
    }
    __syncthreads();  // every wave has read Hb
    for (int i = 0; i < nu; ++i) {
      const int row = 32 * (S0 + i) + j;
      grub_store_h(Hb, ph, row, T0, hh, hA);
      if (h_out && s + 1 == a.h_out_step && row < valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = 32 * T0 + mlp_acc_row(r, hh);
          if (f < H) h_out[(size_t)(m0 + row) * H + f] = hA[r];
        }
      }
      GRUB_NEXT_UNIT()
    }
    __syncthreads();
    // ---- the post-MLP from Hb; the last layer goes to y
    const __bf16 *src = Hb;
    int ps = ph, in = H;
    for (int l = 0; l < d.n_post; ++l) {
      const int out = d.post[l];
      const float *bias = W + (size_t)in * out;
      if (l != d.n_post - 1) {
        cur ^= 1;
        __bf16 *dst = cur ? P1 : P0;
        const int pd = cur ? a.pit1 : a.pit0;
        grub_layer<false>(src, ps, dst, pd, wp, bias, in, out, true, d.act, nullptr, 0, lane, wave);
        __syncthreads();
        src = dst;
        ps = pd;
      } else {
        grub_layer<true>(src, ps, nullptr, 0, wp, bias, in, out, false, d.act, y + ((size_t)s * a.M + m0) * out_w, valid, lane,
                         wave);
      }
      W = bias + out;
      wp += grub_dense_frags(in, out);
      in = out;
    }
  }
}

#undef GRUB_NEXT_UNIT

// every limit of the entry points, before any HIP call (pob_gru_sequence_forward's)
static int grub_check(const pob_gru *g) {
  if (!g) return pob_fail_msg(POB_EINVAL, "gru is NULL");
  if (g->cell != POB_CELL_GRU)
    return pob_fail_msg(POB_EINVAL, "gru sequence bf16: the handle's cell is an lstm; the sequence kernels serve the gru cell only");
  return POB_OK;
}

#define GRUB_POOL_TWO 81408  // two blocks on a CU's 160 KiB
#define GRUB_POOL_ONE 86016  // the widest network: 256 + 64 (128 + 8 + 2 (256 + 8)) 2 = 85 248 B

#define GRUB_LAUNCH(POOL, N)                                                                                          \
  hipLaunchKernelGGL((k_gru_seq_infer_bf16<POOL, N>), grid, dim3(GRUB_LANES), 0, st, g->d, a, obs, idx, h0, reset, theta, \
                     (const grub_bf16x8 *)workspace, y, h_first, h_out, norm)

extern "C" {

int pob_gru_sequence_bf16_workspace_bytes(const pob_gru *g, long long *bytes) {
  const int rc = grub_check(g);
  if (rc != POB_OK) return rc;
  if (!bytes) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: bytes is NULL");
  *bytes = grub_plan(g->d, nullptr, nullptr) * 16;
  return POB_OK;
}

int pob_gru_sequence_forward_bf16(const pob_gru *g, int S, long long M, long long B, const float *obs, const int32_t *idx,
                                  const float *h0, const float *reset, const float *theta, float *y, float *h_first,
                                  float *h_out, int h_out_step, const float *norm, float norm_clip, void *workspace,
                                  void *stream) {
  const int rc = grub_check(g);
  if (rc != POB_OK) return rc;
  if (S < 1) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: the step count S must be positive");
  if (M < 1) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: the sequence count M must be positive");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: the env count B must be positive");
  if (!idx && M != B) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: without idx M must equal B");
  long long widest = 4 * g->d.hid;
  for (int l = 0; l <= g->d.n_pre; ++l) widest = g->d.pre[l] > widest ? g->d.pre[l] : widest;
  for (int l = 0; l < g->d.n_post; ++l) widest = g->d.post[l] > widest ? g->d.post[l] : widest;
  if (M > (1LL << 31) / widest || (long long)S * M + 1024 >= (1LL << 31) / widest)  // pob_gru_sequence_forward's limit
    return pob_fail_msg(POB_EINVAL, "gru sequence bf16: too many rows ((S M + 1024) times the widest array, 4 H included, must be below 2^31)");
  if (B >= (1LL << 31)) return pob_fail_msg(POB_EINVAL, "gru sequence bf16: at most 2^31 - 1 envs (idx is int32)");
  if (!obs || !h0 || !theta || !y || !workspace)
    return pob_fail_msg(POB_EINVAL, "gru sequence bf16: NULL argument (obs, h0, theta, y, workspace)");
  if (h_out_step < 1 || h_out_step > S)
    return pob_fail_msg(POB_EINVAL, "gru sequence bf16: h_out_step must be in 1 .. S");
  GrubArgs a;
  int pit[2], pool = 0;
  const int n_frags = (int)grub_plan(g->d, pit, &pool);
  a.S = S; a.M = (int)M; a.h_out_step = h_out_step; a.pit0 = pit[0]; a.pit1 = pit[1]; a.B = B; a.clip = norm_clip;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gru_pack_bf16, dim3((n_frags + 255) / 256), dim3(256), 0, st, g->d, theta, (grub_bf16x8 *)workspace,
                     n_frags);
  const dim3 grid((unsigned)((M + GRUB_ROWS - 1) / GRUB_ROWS));
  if (pool <= GRUB_POOL_TWO) {
    if (norm) GRUB_LAUNCH(GRUB_POOL_TWO, true);
    else GRUB_LAUNCH(GRUB_POOL_TWO, false);
  } else {
    if (norm) GRUB_LAUNCH(GRUB_POOL_ONE, true);
    else GRUB_LAUNCH(GRUB_POOL_ONE, false);
  }
  return mlp_hip_check(hipGetLastError(), "k_gru_seq_infer_bf16 launch");
}

}  // extern "C"
