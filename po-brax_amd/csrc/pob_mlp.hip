// pob_mlp.hip -- policy networks on the matrix cores (gfx950): the fused MLP forward and the
// tanh-normal actor of DESIGN.md "Policy networks".
//
//   k_mlp_forward   y = MLP(x): every layer in one launch
//   k_policy_act    the same forward, then the tanh-normal head (brax NormalTanhDistribution [ext])
//   k_gru_forward, k_gru_policy_act   the recurrent actor (pre-MLP, GRU cell, post-MLP; below)
//   k_mlp_forward_train, k_mlp_bwd_*  the training forward and the backward pass
//   k_gru_seq_forward, k_gru_seq_backward, k_gru_bwd_weights   the recurrent window's (at the end)
//   k_gru_seq_infer    the recurrent window for inference (the recurrent critic's pass)
//
// One 64-lane block (one wave) owns a tile of 32 batch rows.  It computes Y^T = W^T X^T with
// v_mfma_f32_32x32x2_f32: the env is the C column (lane & 31), the A operand of k-step s is row
// k = mlp_kfeat(s, lane >> 5) of W read from the caller's parameter buffer (coalesced, L2
// resident, never copied: an optimiser's in-place update is seen by a captured graph), the B
// operand is the activation of that feature from LDS.  The instruction is bit for bit
// fma(a_k1, b_k1, fma(a_k0, b_k0, C)), so with the accumulator started from the bias the layer
// is the fmaf chain of pob_mlp.h mlp_forward_ref, and the activations are that header's scalar
// functions: the kernels equal the restatement exactly.
//
// Activations live in two LDS images [feature][env] (pitch 33 floats: conflict-free both for the
// row-major global <-> LDS copies, where consecutive lanes walk features, and for the operand
// reads, where they walk envs), layer l reading image l & 1 and writing the other.  Both lie
// in one static pool whose height is a template parameter (64 / 152 / 288 / 512 features in
// all), chosen per network at launch, the second image starting behind the first one's widest
// layer: the reference's policy network takes 152 rows = 20 064 B, eight blocks per CU.  The
// first image is staged from 32 contiguous observation rows with coalesced loads, sixteen in
// flight per lane (tail rows clamped), outputs leave through the same images with coalesced
// stores (tail rows masked).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <new>

#include "../../include/pob.h"
#include "pob_mlp.h"

// sets pob_last_error's thread-local message (pob_kernels.hip)
int pob_fail_msg(int code, const char *msg);

#define MLP_ROWS 32    // batch rows of a tile
#define MLP_PITCH 33   // floats between two features of an LDS image
#define MLP_KUNROLL 16 // k-steps whose operands are loaded ahead of their MFMAs
#define MLP_STAGE 16   // observation elements a lane loads ahead of their LDS stores

typedef float mlp_f32x16 __attribute__((ext_vector_type(16)));

struct MlpDesc {
  int n_layers;
  int sizes[POB_MLP_MAX_LAYERS + 1];
  int act, act_final;
};

// register r of lane half h holds output feature (r & 3) + 8 (r >> 2) + 4 h of the 32-feature tile
POB_MLP_D int mlp_acc_row(const int r, const int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// One output tile's chain: acc += sum over the `in` features of src of W[k][col] src[k][env], in
// the order of mlp_kfeat (W's rows are ldw floats apart; cok: this lane's column exists).
POB_MLP_D void mlp_chain(mlp_f32x16 &acc, const float *src, const float *W, const int ldw, const int col, const bool cok,
                         const int in, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int ks = mlp_ksteps(in);
  for (int s0 = 0; s0 < ks; s0 += MLP_KUNROLL) {
    float a[MLP_KUNROLL], b[MLP_KUNROLL];
#pragma unroll
    for (int u = 0; u < MLP_KUNROLL; ++u) {
      const int k = mlp_kfeat(s0 + u, h);
      const bool kok = k < in;
      a[u] = (kok && cok) ? W[(size_t)k * ldw + col] : 0.0f;
      b[u] = kok ? src[k * MLP_PITCH + j] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < MLP_KUNROLL; ++u)
      if (s0 + u < ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
  }
}

// the accumulator of output tile ot started from the bias (0 past the layer's width)
POB_MLP_D void mlp_acc_bias(mlp_f32x16 &acc, const float *bias, const int ot, const int out, const int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = ot + mlp_acc_row(r, h);
    acc[r] = i < out ? bias[i] : 0.0f;
  }
}

// one layer: src image (in features) -> dst image (out features)
POB_MLP_D void mlp_layer(const float *src, float *dst, const float *W, const float *bias, const int in, const int out,
                         const bool activate, const int act, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  for (int ot = 0; ot < out; ot += 32) {
    mlp_f32x16 acc;
    mlp_acc_bias(acc, bias, ot, out, h);
    mlp_chain(acc, src, W, out, ot + j, ot + j < out, in, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ot + mlp_acc_row(r, h);
      if (i < out) dst[i * MLP_PITCH + j] = activate ? mlp_activate(act, acc[r]) : acc[r];
    }
  }
}

// rows [b0, b0 + valid) of a row-major (B, width) array <- features [f0, f0 + width) of an image
POB_MLP_D void mlp_tile_store(float *dst, const float *img, const int f0, const int width, const int b0, const int valid,
                              const int lane) {
  float *d = dst + (size_t)b0 * width;
  for (int e = lane; e < MLP_ROWS * width; e += 64) {
    const int row = e / width, col = e - row * width;
    if (row < valid) d[e] = img[(f0 + col) * MLP_PITCH + row];
  }
}

// features [0, D) of an image <- rows [b0, b0 + 32) of a row-major (B, D) array x: coalesced
// loads, MLP_STAGE in flight per lane, tail rows repeating the last valid one.  copy (may be
// NULL) receives the valid rows as loaded.  reset (may be NULL): a row whose reset[b] != 0 is
// staged as +0 in every feature.  NORM: the image takes pob_obsnorm_apply of the value, with the
// column's mean and scale (rows 0 and 1 of the (3, D) table `norm`) loaded along with it; copy
// keeps the raw row.
template <bool NORM>
POB_MLP_D void mlp_tile_load(float *img, const float *x, const int D, const int b0, const int valid, float *copy,
                             const float *reset, const float *norm, const float clip, const int lane) {
  // element e = row D + col of the tile's 32 contiguous rows; a lane's elements are 64 apart
  const int dq = 64 / D, dr = 64 - dq * D;
  int row = lane / D, col = lane - row * D;
  for (int e0 = lane; e0 < MLP_ROWS * D; e0 += 64 * MLP_STAGE) {
    float v[MLP_STAGE], mu[NORM ? MLP_STAGE : 1], sc[NORM ? MLP_STAGE : 1];
    int at[MLP_STAGE];  // the element's place in the image (-1: past the tile), bit 30: a row to copy out
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u) {
      const bool in_tile = e0 + 64 * u < MLP_ROWS * D;
      const int rr = row < valid ? row : valid - 1;  // tail rows repeat the last one
      v[u] = in_tile ? x[(size_t)(b0 + rr) * D + col] : 0.0f;
      if (reset) v[u] = (in_tile && reset[b0 + rr] != 0.0f) ? 0.0f : v[u];
      if (NORM) {
        mu[u] = in_tile ? norm[col] : 0.0f;
        sc[u] = in_tile ? norm[D + col] : 0.0f;
      }
      at[u] = in_tile ? (col * MLP_PITCH + row) | (row < valid ? 1 << 30 : 0) : -1;
      row += dq; col += dr;
      if (col >= D) { col -= D; ++row; }
    }
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u) {
      if (at[u] >= 0) {
        if (copy && (at[u] >> 30)) copy[(size_t)b0 * D + e0 + 64 * u] = v[u];
        img[at[u] & 0xFFFFF] = NORM ? pob_obsnorm_apply(v[u], mu[u], sc[u], clip) : v[u];
      }
    }
  }
}

// The forward of one tile.  Returns the image holding the last layer's output.
template <bool NORM>
POB_MLP_D float *mlp_tile_forward(const MlpDesc &d, float *imgA, float *imgB, const int B, const int b0, const float *x,
                                  const float *theta, float *obs_copy, const float *norm, const float clip,
                                  const int lane) {
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  mlp_tile_load<NORM>(imgA, x, d.sizes[0], b0, valid, obs_copy, nullptr, norm, clip, lane);
  __syncthreads();
  float *src = imgA, *dst = imgB;
  const float *W = theta;
  for (int l = 0; l < d.n_layers; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    const float *bias = W + (size_t)in * out;
    mlp_layer(src, dst, W, bias, in, out, l != d.n_layers - 1 || d.act_final, d.act, lane);
    __syncthreads();
    W = bias + out;
    float *t = src; src = dst; dst = t;
  }
  return src;
}

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

// The tanh-normal head of one tile: L holds the logits (2 A features), T (A features, another
// image) takes the per-component log-probability terms.  Env b of this launch is env first + b
// of a batch of `total`: its draw for action component a is element (first + b) A + a of
// uniform(split(key)[1], (total, A), -1, 1).  The key is only read here (k_mlp_advance_key,
// launched after, advances it).
POB_MLP_D void policy_tile_head(float *L, float *T, const int A, const int b0, const int valid, const int total,
                                const int first, const uint32_t *key, const int deterministic, float *action, float *logp,
                                float *raw, float *logits, const int lane) {
  if (logits) {
    mlp_tile_store(logits, L, 0, 2 * A, b0, valid, lane);
    __syncthreads();
  }
  uint32_t s0 = 0u, s1 = 0u;
  if (!deterministic) tf_split(key[0], key[1], 2u, 1u, s0, s1);
  for (int e = lane; e < MLP_ROWS * A; e += 64) {
    const int env = e & 31, a = e >> 5;
    if (env >= valid) continue;
    const float loc = L[a * MLP_PITCH + env], s = L[(A + a) * MLP_PITCH + env];
    float act, rw;
    if (deterministic) {
      act = pob_tanhf(loc);
      rw = loc;
    } else {
      const uint32_t i = (uint32_t)(first + b0 + env) * (uint32_t)A + (uint32_t)a;
      const float u = tf_uniform(s0, s1, (uint32_t)total * (uint32_t)A, i, -1.0f, 1.0f);
      float term;
      pob_tanh_normal(loc, s, u, act, rw, term);
      T[a * MLP_PITCH + env] = term;
    }
    L[a * MLP_PITCH + env] = act;
    L[(A + a) * MLP_PITCH + env] = rw;
  }
  __syncthreads();
  mlp_tile_store(action, L, 0, A, b0, valid, lane);
  if (raw) mlp_tile_store(raw, L, A, A, b0, valid, lane);
  if (!deterministic && logp && lane < valid) {
    float sum = 0.0f;
    for (int a = 0; a < A; ++a) sum = sum + T[a * MLP_PITCH + lane];
    logp[b0 + lane] = sum;
  }
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

__global__ void k_mlp_advance_key(uint32_t *key) {
  uint32_t o0, o1;
  tf_split(key[0], key[1], 2u, 0u, o0, o1);
  key[0] = o0; key[1] = o1;
}

// ============================================================================ recurrent actor
// obs -> pre-MLP -> GRU cell -> post-MLP (pob_mlp.h gru_forward_ref is the specification).  The
// pool holds four regions, in this order: C = [x ; h] (I + H features: the cell's input image,
// h staged directly behind x), N (H features: h'), and the ping-pong images P0, P1 of the dense
// layers' other activations (heights p_rows[0], p_rows[1], worked out by gru_plan on the host
// with the walk gru_tile_forward makes).
struct GruDesc {
  int n_pre, n_post, hid, act;
  int pre[POB_GRU_MAX_PRE + 1];  // pre[0] = obs width, pre[n_pre] = I
  int post[POB_GRU_MAX_POST];
  int p_rows[2];
};

// The cell on one tile: C (I + H features) -> N (H features).  g: the GRU block of theta.  Per
// 32-feature output tile four accumulators (r, z, cx, ch) take their chains, then n and h' are
// finished in registers, the old h read from C.
POB_MLP_D void gru_cell(const float *C, float *N, const float *g, const int I, const int H, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const float *W_rz = g, *b_rz = W_rz + (size_t)(I + H) * 2 * H;
  const float *W_xn = b_rz + 2 * H, *b_xn = W_xn + (size_t)I * H;
  const float *W_hn = b_xn + H, *b_hn = W_hn + (size_t)H * H;
  for (int ot = 0; ot < H; ot += 32) {
    const int col = ot + j;
    const bool cok = col < H;
    mlp_f32x16 ar, az, ax, ah;
    mlp_acc_bias(ar, b_rz, ot, H, h);
    mlp_chain(ar, C, W_rz, 2 * H, col, cok, I + H, lane);
    mlp_acc_bias(az, b_rz + H, ot, H, h);
    mlp_chain(az, C, W_rz, 2 * H, H + col, cok, I + H, lane);
    mlp_acc_bias(ax, b_xn, ot, H, h);
    mlp_chain(ax, C, W_xn, H, col, cok, I, lane);
    mlp_acc_bias(ah, b_hn, ot, H, h);
    mlp_chain(ah, C + I * MLP_PITCH, W_hn, H, col, cok, H, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ot + mlp_acc_row(r, h);
      if (i < H) {
        const float rg = pob_sigmoidf(ar[r]), zg = pob_sigmoidf(az[r]);
        const float n = pob_tanhf(MLP_FMA(rg, ah[r], ax[r]));
        const float hold = C[(I + i) * MLP_PITCH + j];
        N[i * MLP_PITCH + j] = MLP_FMA(zg, hold - n, n);
      }
    }
  }
}

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

// ============================================================================ C ABI
struct pob_mlp {
  MlpDesc d;
  long long n_params;
};

// The two images' heights: image l & 1 holds sizes[l]; the actor's terms (A features) go to the
// image the logits are not in.  Image B starts at row `split` of the pool; returns the pool's
// height class (0 .. 3: 64 / 152 / 288 / 512 rows).
static int image_rows(const MlpDesc &d, bool head, int &split) {
  int w[2] = {1, 1};
  for (int l = 0; l <= d.n_layers; ++l)
    if (d.sizes[l] > w[l & 1]) w[l & 1] = d.sizes[l];
  if (head) {
    const int A = d.sizes[d.n_layers] >> 1, o = (d.n_layers + 1) & 1;
    if (A > w[o]) w[o] = A;
  }
  split = w[0];
  const int rows = w[0] + w[1];
  return rows <= 64 ? 0 : (rows <= 152 ? 1 : (rows <= 288 ? 2 : 3));
}

// the normalising instantiation only where a table is given: the plain one is the code it was
// (TAIL: the template arguments after the pool height, each written MLP_TARG(x); may be empty)
#define MLP_TARG(x) , x
#define MLP_DISPATCH_T(KERNEL, TAIL, cls, ...)                                                    \
  switch (cls) {                                                                                  \
    case 0: hipLaunchKernelGGL((KERNEL<64 TAIL>), grid, dim3(64), 0, st, __VA_ARGS__); break;     \
    case 1: hipLaunchKernelGGL((KERNEL<152 TAIL>), grid, dim3(64), 0, st, __VA_ARGS__); break;    \
    case 2: hipLaunchKernelGGL((KERNEL<288 TAIL>), grid, dim3(64), 0, st, __VA_ARGS__); break;    \
    default: hipLaunchKernelGGL((KERNEL<512 TAIL>), grid, dim3(64), 0, st, __VA_ARGS__); break;   \
  }
#define MLP_DISPATCH_N(KERNEL, N, cls, ...) MLP_DISPATCH_T(KERNEL, MLP_TARG(N), cls, __VA_ARGS__)
#define MLP_DISPATCH(KERNEL, cls, ...)                                \
  if (norm) { MLP_DISPATCH_N(KERNEL, true, cls, __VA_ARGS__, norm, norm_clip) } \
  else { MLP_DISPATCH_N(KERNEL, false, cls, __VA_ARGS__, norm, norm_clip) }

static int mlp_hip_check(hipError_t e, const char *what) {
  if (e == hipSuccess) return POB_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
  return pob_fail_msg(POB_EHIP, msg);
}

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
  const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  MLP_DISPATCH(k_mlp_forward, cls, m->d, split, B, x, theta, y)
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward launch");
}

int pob_mlp_forward(const pob_mlp *m, int B, const float *x, const float *theta, float *y, void *stream) {
  return pob_mlp_forward_norm(m, B, x, theta, y, nullptr, 0.0f, stream);
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
  const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *key = key_io;
  MLP_DISPATCH(k_policy_act, cls, m->d, split, B, total, first, obs, theta, key, deterministic, action, logp, raw, logits,
               obs_copy)
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

struct pob_gru {
  GruDesc d;
  long long n_params;
  int cls_forward, cls_actor;  // pool height classes (GRU_DISPATCH)
};

// The heights of P0 and P1, by the walk of gru_tile_forward; with `head` the actor's terms (A
// features) go to the image the logits are not in.  Returns the pool's height class (0 .. 4:
// 96 / 192 / 288 / 512 / 896 rows; the widest legal network takes 256 + 128 + 256 + 256).
static int gru_plan(const GruDesc &d, bool head, int *p_rows) {
  int w[2] = {0, 0}, pp = 0;
  if (d.n_pre) { w[0] = d.pre[0]; pp = 1; }
  for (int l = 0; l < d.n_pre; ++l) {
    if (l != d.n_pre - 1 && d.pre[l + 1] > w[pp]) w[pp] = d.pre[l + 1];
    pp ^= 1;
  }
  for (int l = 0; l < d.n_post; ++l) {
    if (d.post[l] > w[pp]) w[pp] = d.post[l];
    pp ^= 1;
  }
  const int A = d.post[d.n_post - 1] >> 1;
  if (head && A > w[pp]) w[pp] = A;
  if (p_rows) { p_rows[0] = w[0]; p_rows[1] = w[1]; }
  const int rows = d.pre[d.n_pre] + 2 * d.hid + w[0] + w[1];
  return rows <= 96 ? 0 : (rows <= 192 ? 1 : (rows <= 288 ? 2 : (rows <= 512 ? 3 : 4)));
}

#define GRU_DISPATCH_N(KERNEL, N, cls, ...)                                                    \
  switch (cls) {                                                                               \
    case 0: hipLaunchKernelGGL((KERNEL<96, N>), grid, dim3(64), 0, st, __VA_ARGS__); break;    \
    case 1: hipLaunchKernelGGL((KERNEL<192, N>), grid, dim3(64), 0, st, __VA_ARGS__); break;   \
    case 2: hipLaunchKernelGGL((KERNEL<288, N>), grid, dim3(64), 0, st, __VA_ARGS__); break;   \
    case 3: hipLaunchKernelGGL((KERNEL<512, N>), grid, dim3(64), 0, st, __VA_ARGS__); break;   \
    default: hipLaunchKernelGGL((KERNEL<896, N>), grid, dim3(64), 0, st, __VA_ARGS__); break;  \
  }
#define GRU_DISPATCH(KERNEL, cls, ...)                                \
  if (norm) { GRU_DISPATCH_N(KERNEL, true, cls, __VA_ARGS__, norm, norm_clip) } \
  else { GRU_DISPATCH_N(KERNEL, false, cls, __VA_ARGS__, norm, norm_clip) }

extern "C" {

int pob_gru_create(int n_pre, const int *pre_sizes, int hidden, int n_post, const int *post_sizes, int activation,
                   pob_gru **out) {
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
  n += 3 * H * I + 3 * H * H + 4 * H;
  long long in = H;
  for (int l = 0; l < n_post; ++l) { n += (in + 1) * d.post[l]; in = d.post[l]; }
  g->n_params = n;
  g->cls_forward = gru_plan(d, false, nullptr);
  g->cls_actor = gru_plan(d, true, nullptr);
  *out = g;
  return POB_OK;
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
  GruDesc d = g->d;
  gru_plan(d, false, d.p_rows);
  const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  GRU_DISPATCH(k_gru_forward, g->cls_forward, d, B, x, theta, reset, h_io, y, h_in_copy)
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
  GruDesc d = g->d;
  gru_plan(d, true, d.p_rows);
  const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *key = key_io;
  GRU_DISPATCH(k_gru_policy_act, g->cls_actor, d, B, total, first, obs, theta, key, deterministic, reset, h_io, action,
               logp, raw, logits, obs_copy, h_in_copy)
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

// ============================================================================ observation normaliser
// The statistics of pob_mlp.h obsnorm_accumulate_ref / obsnorm_update_ref (the specification; DESIGN.md
// "Observation normaliser").  k_obsnorm_accumulate: one lane per (chunk, column), consecutive lanes
// on consecutive columns of a row (coalesced), the chunk's rows in ascending order into a float64
// pair in registers, OBSNORM_STAGE loads in flight per lane; the pair goes to the workspace
// (n_chunks, 2, D).  k_obsnorm_reduce: one lane per entry of (2, D) adds the chunk partials in
// ascending chunk order.  k_obsnorm_update: one block finishes the table in place.  No atomics:
// the order depends on N and D only.
#define OBSNORM_STAGE 16
#define OBSNORM_RSTAGE 32

__global__ __launch_bounds__(256) void k_obsnorm_accumulate(const float *x, const long long N, const int D,
                                                            const float *table, double *ws, const long long n_items) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_items) return;
  const long long c = g / D;
  const int f = (int)(g - c * D);
  const long long r0 = c * POB_OBSNORM_CHUNK;
  const int rows = N - r0 < POB_OBSNORM_CHUNK ? (int)(N - r0) : POB_OBSNORM_CHUNK;
  const float mean = table[f];
  const float *p = x + (size_t)r0 * D + f;
  double S1 = 0.0, S2 = 0.0;
  int r = 0;
  for (; r + OBSNORM_STAGE <= rows; r += OBSNORM_STAGE) {
    float v[OBSNORM_STAGE];
#pragma unroll
    for (int u = 0; u < OBSNORM_STAGE; ++u) v[u] = p[(size_t)(r + u) * D];
#pragma unroll
    for (int u = 0; u < OBSNORM_STAGE; ++u) pob_obsnorm_step(v[u], mean, S1, S2);
  }
  for (; r < rows; ++r) pob_obsnorm_step(p[(size_t)r * D], mean, S1, S2);
  ws[(size_t)(2 * c) * D + f] = S1;
  ws[(size_t)(2 * c + 1) * D + f] = S2;
}

__global__ __launch_bounds__(64) void k_obsnorm_reduce(const double *ws, const long long n_chunks, const int D,
                                                       double *sums) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= 2 * D) return;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += OBSNORM_RSTAGE) {
    double v[OBSNORM_RSTAGE];
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u) v[u] = c0 + u < n_chunks ? ws[(size_t)(c0 + u) * 2 * D + e] : 0.0;
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u)
      if (c0 + u < n_chunks) T = T + v[u];
  }
  sums[e] = T;
}

__global__ __launch_bounds__(POB_MLP_MAX_WIDTH) void k_obsnorm_update(double *count, float *table, const int D,
                                                                      const double *sums, const int R,
                                                                      const long long n_new) {
  const int f = threadIdx.x;
  const double cnt = count[0];
  __syncthreads();  // every lane holds the old count before lane 0 replaces it
  double total = cnt;
  if (f < D) {
    double S1 = 0.0, S2 = 0.0;
    for (int r = 0; r < R; ++r) {
      S1 = S1 + sums[(size_t)(2 * r) * D + f];
      S2 = S2 + sums[(size_t)(2 * r + 1) * D + f];
    }
    float mean = table[f], scale = table[D + f], m2 = table[2 * D + f];
    total = pob_obsnorm_finish(cnt, (double)n_new, S1, S2, mean, scale, m2);
    table[f] = mean;
    table[D + f] = scale;
    table[2 * D + f] = m2;
  }
  if (f == 0) count[0] = total;
}

static int obsnorm_chunks(long long N, int D, long long *n_chunks) {
  if (D < 1 || D > POB_MLP_MAX_WIDTH) return pob_fail_msg(POB_EINVAL, "obsnorm: the observation width must be in 1 .. 256");
  if (N < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the row count must be positive");
  if (N > (1LL << 40)) return pob_fail_msg(POB_EINVAL, "obsnorm: at most 2^40 rows");
  *n_chunks = (N + POB_OBSNORM_CHUNK - 1) / POB_OBSNORM_CHUNK;
  return POB_OK;
}

extern "C" {

int pob_obsnorm_workspace_bytes(long long N, int D, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "obsnorm: bytes is NULL");
  long long n_chunks;
  const int rc = obsnorm_chunks(N, D, &n_chunks);
  if (rc != POB_OK) return rc;
  *bytes = n_chunks * 2 * D * (long long)sizeof(double);
  return POB_OK;
}

int pob_obsnorm_accumulate(const float *obs, long long N, int D, const float *table, double *workspace, double *sums,
                           void *stream) {
  long long n_chunks;
  const int rc = obsnorm_chunks(N, D, &n_chunks);
  if (rc != POB_OK) return rc;
  if (!obs || !table || !workspace || !sums) return pob_fail_msg(POB_EINVAL, "obsnorm: NULL argument (obs, table, workspace, sums)");
  hipStream_t st = (hipStream_t)stream;
  const long long n_items = n_chunks * D;
  hipLaunchKernelGGL(k_obsnorm_accumulate, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, obs, N, D, table,
                     workspace, n_items);
  hipLaunchKernelGGL(k_obsnorm_reduce, dim3((unsigned)((2 * D + 63) / 64)), dim3(64), 0, st, workspace, n_chunks, D, sums);
  return mlp_hip_check(hipGetLastError(), "k_obsnorm_accumulate launch");
}

int pob_obsnorm_update(double *count_io, float *table_io, int D, const double *sums, int R, long long n_new, void *stream) {
  if (D < 1 || D > POB_MLP_MAX_WIDTH) return pob_fail_msg(POB_EINVAL, "obsnorm: the observation width must be in 1 .. 256");
  if (R < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the shard count R must be positive");
  if (n_new < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the row count must be positive");
  if (!count_io || !table_io || !sums) return pob_fail_msg(POB_EINVAL, "obsnorm: NULL argument (count, table, sums)");
  hipLaunchKernelGGL(k_obsnorm_update, dim3(1), dim3(POB_MLP_MAX_WIDTH), 0, (hipStream_t)stream, count_io, table_io, D, sums,
                     R, n_new);
  return mlp_hip_check(hipGetLastError(), "k_obsnorm_update launch");
}

}  // extern "C"

// ============================================================================ GAE
// gae_ref of pob_mlp.h (the specification; DESIGN.md "Critic pass and GAE").  One lane per env,
// consecutive lanes on consecutive b (every load and store a coalesced row segment), t
// descending.  The carried chain is pob_gae_step's fmaf and add; the loads do not depend on it,
// so the steps are taken in chunks of POB_GAE_CHUNK whose rows are all issued before the chunk
// before them is consumed (two register images: at one or two waves per CU the loop then waits
// for HBM once per chunk, not once per step).  The newest chunk takes the (T - 1) % POB_GAE_CHUNK
// + 1 steps that make every later chunk a full one.  TRUNC = false: truncation is NULL (m = 1 - 0).
// No LDS, no atomics, no scratch.
struct gae_rows { float tr[POB_GAE_CHUNK], se[POB_GAE_CHUNK], rw[POB_GAE_CHUNK], va[POB_GAE_CHUNK]; };

// rows t_hi, t_hi - 1, .., t_hi - POB_GAE_CHUNK + 1 of lane b; a row before the first (the newest
// chunk of a T that is no multiple of the chunk) is loaded as row 0 and never used
template <bool TRUNC>
__device__ __forceinline__ void gae_load(gae_rows &r, const int t_hi, const size_t B, const size_t b,
                                         const float *truncation, const float *second, const float *reward,
                                         const float *values) {
#pragma unroll
  for (int u = 0; u < POB_GAE_CHUNK; ++u) {
    const size_t i = (size_t)(t_hi - u > 0 ? t_hi - u : 0) * B + b;
    r.tr[u] = TRUNC ? truncation[i] : 0.0f;
    r.se[u] = second[i];
    r.rw[u] = reward[i];
    r.va[u] = values[i];
  }
}

template <bool TRUNC>
__global__ __launch_bounds__(64) void k_gae(const int T, const long long B, const float *truncation, const float *second,
                                            const int done_input, const float *reward, const float reward_scale,
                                            const float *values, const float *bootstrap, const float lambda,
                                            const float discount, float *vs, float *advantages) {
  const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
  if (lane >= B) return;
  const size_t b = (size_t)lane, Bs = (size_t)B;
  float acc = 0.0f, v_next = bootstrap[b], vs_next = v_next;
  int t = T - 1;                          // the chunk in `cur` is steps t, t - 1, .., t - n + 1
  int n = (T - 1) % POB_GAE_CHUNK + 1;
  gae_rows cur, nxt;
  gae_load<TRUNC>(cur, t, Bs, b, truncation, second, reward, values);
  for (;;) {
    const bool more = t - n >= 0;  // then t - n + 1 is a multiple of the chunk: a full chunk follows
    if (more) gae_load<TRUNC>(nxt, t - n, Bs, b, truncation, second, reward, values);
#pragma unroll
    for (int u = 0; u < POB_GAE_CHUNK; ++u)
      if (u < n) {
        float adv;
        pob_gae_step(cur.tr[u], cur.se[u], done_input, cur.rw[u], reward_scale, cur.va[u], lambda, discount, acc, v_next,
                     vs_next, adv);
        const size_t i = (size_t)(t - u) * Bs + b;
        if (advantages) advantages[i] = adv;
        if (vs) vs[i] = vs_next;
      }
    if (!more) break;
    t -= n;
    n = POB_GAE_CHUNK;
    cur = nxt;
  }
}

extern "C" {

int pob_gae(int T, long long B, const float *truncation, const float *second, int done_input, const float *reward,
            float reward_scale, const float *values, const float *bootstrap, float lambda, float discount, float *vs,
            float *advantages, void *stream) {
  if (T < 1) return pob_fail_msg(POB_EINVAL, "gae: the step count T must be positive");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "gae: the batch size B must be positive");
  if (B > (1LL << 36)) return pob_fail_msg(POB_EINVAL, "gae: at most 2^36 envs");
  if (!second || !reward || !values || !bootstrap)
    return pob_fail_msg(POB_EINVAL, "gae: NULL argument (second, reward, values, bootstrap)");
  if (!vs && !advantages) return pob_fail_msg(POB_EINVAL, "gae: vs and advantages are both NULL");
  const dim3 grid((unsigned)((B + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
  if (truncation)
    hipLaunchKernelGGL(k_gae<true>, grid, dim3(64), 0, st, T, B, truncation, second, done_input ? 1 : 0, reward,
                       reward_scale, values, bootstrap, lambda, discount, vs, advantages);
  else
    hipLaunchKernelGGL(k_gae<false>, grid, dim3(64), 0, st, T, B, truncation, second, done_input ? 1 : 0, reward,
                       reward_scale, values, bootstrap, lambda, discount, vs, advantages);
  return mlp_hip_check(hipGetLastError(), "k_gae launch");
}

}  // extern "C"

// ============================================================================ Adam
// adam_step_ref of pob_mlp.h (the specification; DESIGN.md "Learner on the device").  One launch
// steps every segment: the table travels BY VALUE as the kernel argument (a captured graph keeps the
// copy; no device pointer array that could go stale).  The work is streaming, 28 bytes an element: a
// lane owns ONE item, either a 16-byte group of four elements of the segment's aligned body (four
// 16-byte loads in flight, three 16-byte stores; consecutive lanes on consecutive groups) or one
// scalar element of its head or tail.  A segment's base is only 4-byte aligned: the host finds the
// head that brings theta, grad, m and v to a 16-byte boundary TOGETHER, and a segment whose four
// bases disagree modulo 16 is all head (scalar).  A block serves one segment (blk0: its first block),
// found by a select over the table, not by indexing it (no scratch).  Every lane forms the step's bias
// corrections from the state block itself (two uniform 8-byte loads, two float64 products); the
// block is advanced by k_adam_advance, one lane, after it on the same stream, so a replayed graph
// counts its own steps.  No LDS, no atomics, ordinary vector stores only.
#define ADAM_THREADS 256
struct AdamSeg {
  float *theta, *m, *v;
  const float *grad;
  long long head, nvec, nsc;  // scalar elements before the body, 16-byte groups, scalar elements in all
  unsigned blk0;
};
struct AdamTable {
  AdamSeg seg[POB_ADAM_MAX_SEG];
  int n_seg;
};

__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step(const AdamTable t, const double *state, const float lr,
                                                            const float beta1, const float beta2, const float eps) {
  AdamSeg s = t.seg[0];
#pragma unroll
  for (int k = 1; k < POB_ADAM_MAX_SEG; ++k)
    if (k < t.n_seg && blockIdx.x >= t.seg[k].blk0) s = t.seg[k];
  const long long item = (long long)(blockIdx.x - s.blk0) * ADAM_THREADS + threadIdx.x;
  if (item >= s.nvec + s.nsc) return;
  double p1, p2;
  float ic1, ic2;
  pob_adam_bias(state[0], state[1], beta1, beta2, p1, p2, ic1, ic2);
  if (item < s.nvec) {
    const size_t e = (size_t)s.head + 4 * (size_t)item;
    float4 th = *(const float4 *)(s.theta + e), m = *(const float4 *)(s.m + e), v = *(const float4 *)(s.v + e);
    const float4 g = *(const float4 *)(s.grad + e);
    pob_adam_elem(th.x, g.x, m.x, v.x, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.y, g.y, m.y, v.y, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.z, g.z, m.z, v.z, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.w, g.w, m.w, v.w, lr, beta1, beta2, eps, ic1, ic2);
    *(float4 *)(s.theta + e) = th;
    *(float4 *)(s.m + e) = m;
    *(float4 *)(s.v + e) = v;
  } else {
    const long long k = item - s.nvec;  // scalar element k: the head's, then the tail's behind the body
    const size_t e = (size_t)(k < s.head ? k : k + 4 * s.nvec);
    float th = s.theta[e], m = s.m[e], v = s.v[e];
    pob_adam_elem(th, s.grad[e], m, v, lr, beta1, beta2, eps, ic1, ic2);
    s.theta[e] = th;
    s.m[e] = m;
    s.v[e] = v;
  }
}

__global__ void k_adam_advance(double *state, const float beta1, const float beta2) {
  double p1, p2;
  float ic1, ic2;
  pob_adam_bias(state[0], state[1], beta1, beta2, p1, p2, ic1, ic2);
  state[0] = p1;
  state[1] = p2;
}

extern "C" {

int pob_adam_step(const pob_adam_seg *segs, int n_seg, double *state, float lr, float beta1, float beta2, float eps,
                  void *stream) {
  if (n_seg < 1 || n_seg > POB_ADAM_MAX_SEG) return pob_fail_msg(POB_EINVAL, "adam: 1 .. 4 segments a launch");
  if (!segs || !state) return pob_fail_msg(POB_EINVAL, "adam: NULL argument (segs, state)");
  if (((uintptr_t)state & 7) != 0) return pob_fail_msg(POB_EINVAL, "adam: the state block must be 8-byte aligned");
  AdamTable t;
  long long blocks = 0;
  for (int k = 0; k < POB_ADAM_MAX_SEG; ++k) {
    AdamSeg &s = t.seg[k];
    if (k >= n_seg) {
      s = AdamSeg{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0u};
      continue;
    }
    const pob_adam_seg &in = segs[k];
    if (!in.theta || !in.grad || !in.m || !in.v) return pob_fail_msg(POB_EINVAL, "adam: NULL segment pointer");
    if (in.n < 1 || in.n > (1LL << 36)) return pob_fail_msg(POB_EINVAL, "adam: a segment holds 1 .. 2^36 elements");
    const uintptr_t a[4] = {(uintptr_t)in.theta, (uintptr_t)in.grad, (uintptr_t)in.m, (uintptr_t)in.v};
    for (int q = 0; q < 4; ++q)
      if (a[q] & 3) return pob_fail_msg(POB_EINVAL, "adam: segment pointers must be 4-byte aligned");
    const bool together = (a[0] & 15) == (a[1] & 15) && (a[0] & 15) == (a[2] & 15) && (a[0] & 15) == (a[3] & 15);
    long long head = together ? (long long)(((16 - (a[0] & 15)) & 15) >> 2) : in.n;
    if (head > in.n) head = in.n;
    s.theta = in.theta; s.grad = in.grad; s.m = in.m; s.v = in.v;
    s.head = head;
    s.nvec = (in.n - head) / 4;
    s.nsc = in.n - 4 * s.nvec;
    s.blk0 = (unsigned)blocks;
    blocks += (s.nvec + s.nsc + ADAM_THREADS - 1) / ADAM_THREADS;
    if (blocks > INT_MAX) return pob_fail_msg(POB_EINVAL, "adam: too many elements for one launch");
  }
  t.n_seg = n_seg;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adam_step, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, st, t, (const double *)state, lr, beta1,
                     beta2, eps);
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, state, beta1, beta2);
  return mlp_hip_check(hipGetLastError(), "k_adam_step launch");
}

}  // extern "C"

// ============================================================================ PPO loss
// ppo_loss_ref of pob_mlp.h (the specification; DESIGN.md "PPO loss").  k_ppo_loss: a block of
// 256 lanes owns a tile of R consecutive minibatch rows, R = min(256, 1024 / A), so a lane has at
// most PPO_ITEMS (row, component) items.  The tile's logits arrive in LDS as the contiguous row
// segment they are in memory (coalesced, all of a lane's loads in flight), pitch 2 A + 1 per row;
// raw is gathered by idx in whole-row segments.  Consecutive lanes take consecutive components of
// a row: every item's pob_ppo_component runs once, its five gradient factors stay in the lane's
// registers, its two terms go back into the logits' own LDS slots.  One lane per row then sums the
// terms in a ascending (the pitch is odd: conflict-free), finishes pob_ppo_row, stores dvalues and
// the row's three summands and publishes g_lp; the items form pob_ppo_grad into the same slots,
// and dlogits leaves as the contiguous segment it is.  k_ppo_chunks: one block per chunk of
// POB_PPO_CHUNK rows loads the summands coalesced into LDS and three lanes add them in ascending
// row order (the fixed order admits no tree).  k_ppo_finish: one block stages the chunk partials
// through LDS, three lanes add them in ascending order, one forms the four scalars.  No atomics,
// no scratch.
#define PPO_THREADS 256
#define PPO_ITEMS 4      // (row, component) items of a lane
#define PPO_MAX_ROWS 256 // rows of a tile: one row-phase lane each
#define PPO_ELEMS (PPO_THREADS * PPO_ITEMS)  // a tile holds at most this many components
#define PPO_FSTAGE 512   // chunk partials k_ppo_finish stages through LDS at a time

// element e of a row-major (rows, W) tile as (row, col), advanced by the block's 256 lanes at a time
struct ppo_walk {
  int row, col, dq, dr, W;
  __device__ __forceinline__ ppo_walk(const int e, const int width) : W(width) {
    row = e / W; col = e - row * W;
    dq = PPO_THREADS / W; dr = PPO_THREADS - dq * W;
  }
  __device__ __forceinline__ void next() {
    row += dq; col += dr;
    if (col >= W) { col -= W; ++row; }
  }
};

__global__ __launch_bounds__(PPO_THREADS) void k_ppo_loss(const long long M, const int A, const int R, const float *logits,
                                                          const float *values, const int32_t *idx, const float *raw,
                                                          const float *old_logp, const float *advantages, const float *vs,
                                                          const uint32_t *key, const float entropy_cost,
                                                          const float ppo_epsilon, const float inv_m, float *dlogits,
                                                          float *dvalues, float *terms) {
  __shared__ float L[2 * PPO_ELEMS + PPO_MAX_ROWS];  // (R, 2 A) at pitch 2 A + 1: logits, then terms, then dlogits
  __shared__ float X[PPO_ELEMS];                     // (R, A): raw
  __shared__ long long J[PPO_MAX_ROWS];              // the rows' trajectory rows
  __shared__ float G[PPO_MAX_ROWS];                  // the rows' g_lp
  const int tid = threadIdx.x, W = 2 * A, P = W + 1;
  const long long b0 = (long long)blockIdx.x * R;
  const int valid = M - b0 < R ? (int)(M - b0) : R;
  // the row phase's operands, loaded ahead of their use
  float r_old = 0.0f, r_adv = 0.0f, r_vs = 0.0f, r_val = 0.0f;
  if (tid < valid) {
    const long long j = idx ? (long long)idx[b0 + tid] : b0 + tid;
    J[tid] = j;
    r_old = old_logp[j]; r_adv = advantages[j]; r_vs = vs[j];
    r_val = values[b0 + tid];
  }
  {
    const float *g = logits + (size_t)b0 * W;
    const int n = valid * W;
    ppo_walk w(tid, W);
    float v[2 * PPO_ITEMS];
    int at[2 * PPO_ITEMS];
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      const bool ok = e < n;
      v[k] = ok ? g[e] : 0.0f;
      at[k] = ok ? w.row * P + w.col : -1;
      w.next();
    }
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k)
      if (at[k] >= 0) L[at[k]] = v[k];
  }
  __syncthreads();
  const int n_items = valid * A;
  {
    ppo_walk w(tid, A);
    float v[PPO_ITEMS];
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      const bool ok = tid + PPO_THREADS * k < n_items;
      v[k] = ok ? raw[(size_t)J[w.row] * A + w.col] : 0.0f;
      w.next();
    }
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k)
      if (tid + PPO_THREADS * k < n_items) X[tid + PPO_THREADS * k] = v[k];
  }
  __syncthreads();
  uint32_t s0, s1;
  tf_split(key[0], key[1], 2u, 1u, s0, s1);
  const uint32_t n_draws = (uint32_t)M * (uint32_t)A;
  float f[PPO_ITEMS][5];
  {
    ppo_walk w(tid, A);
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      if (e < n_items) {
        const int lo = w.row * P + w.col;
        const uint32_t i = (uint32_t)(b0 + w.row) * (uint32_t)A + (uint32_t)w.col;
        const float u = tf_uniform(s0, s1, n_draws, i, -1.0f, 1.0f);
        float term, ent;
        pob_ppo_component(L[lo], L[lo + A], X[e], u, term, ent, f[k][0], f[k][1], f[k][2], f[k][3], f[k][4]);
        L[lo] = term;
        L[lo + A] = ent;
      }
      w.next();
    }
  }
  __syncthreads();
  if (tid < valid) {
    float logp = 0.0f, ent = 0.0f;
    for (int a = 0; a < A; ++a) {
      logp = logp + L[tid * P + a];
      ent = ent + L[tid * P + A + a];
    }
    float neg_surr, vl, g_lp, dvalue;
    pob_ppo_row(logp, r_old, r_adv, r_vs, r_val, ppo_epsilon, inv_m, neg_surr, vl, g_lp, dvalue);
    G[tid] = g_lp;
    if (dvalues) dvalues[b0 + tid] = dvalue;
    terms[(size_t)b0 + tid] = neg_surr;
    terms[(size_t)M + b0 + tid] = vl;
    terms[2 * (size_t)M + b0 + tid] = ent;
  }
  if (!dlogits) return;
  __syncthreads();
  {
    const float g_ent = -(entropy_cost * inv_m);
    ppo_walk w(tid, A);
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      if (tid + PPO_THREADS * k < n_items) {
        const int lo = w.row * P + w.col;
        float d_loc, d_p;
        pob_ppo_grad(G[w.row], g_ent, f[k][0], f[k][1], f[k][2], f[k][3], f[k][4], d_loc, d_p);
        L[lo] = d_loc;
        L[lo + A] = d_p;
      }
      w.next();
    }
  }
  __syncthreads();
  {
    float *g = dlogits + (size_t)b0 * W;
    const int n = valid * W;
    ppo_walk w(tid, W);
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      if (e < n) g[e] = L[w.row * P + w.col];
      w.next();
    }
  }
}

// partials (n_chunks, 3) <- the float64 sums of the chunk's rows of terms (3, M), rows ascending from +0.0
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_chunks(const long long M, const float *terms, double *partials) {
  __shared__ __attribute__((aligned(16))) float T[3][POB_PPO_CHUNK];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * POB_PPO_CHUNK;
  const int rows = M - r0 < POB_PPO_CHUNK ? (int)(M - r0) : POB_PPO_CHUNK;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < POB_PPO_CHUNK / PPO_THREADS; ++k) {
      const int r = tid + PPO_THREADS * k;
      T[q][r] = r < rows ? terms[(size_t)q * M + r0 + r] : 0.0f;
    }
  __syncthreads();
  if (tid < 3) {
    double S = 0.0;
    const float4 *t4 = (const float4 *)T[tid];  // four rows a read; the adds keep the rows' order
    int r = 0;
#pragma unroll 4
    for (; r + 4 <= rows; r += 4) {
      const float4 v = t4[r >> 2];
      S = S + (double)v.x;
      S = S + (double)v.y;
      S = S + (double)v.z;
      S = S + (double)v.w;
    }
    for (; r < rows; ++r) S = S + (double)T[tid][r];
    partials[(size_t)blockIdx.x * 3 + tid] = S;
  }
}

// losses <- the chunk partials (n_chunks, 3) added per column in ascending chunk order from +0.0:
// the block stages PPO_FSTAGE chunks at a time through LDS (coalesced), three lanes add them
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_finish(const long long M, const long long n_chunks,
                                                            const double *partials, const float entropy_cost,
                                                            float *losses) {
  __shared__ double P[3 * PPO_FSTAGE];
  __shared__ double S[3];
  const int tid = threadIdx.x;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += PPO_FSTAGE) {
    const int n = n_chunks - c0 < PPO_FSTAGE ? (int)(n_chunks - c0) : PPO_FSTAGE;
    for (int e = tid; e < 3 * n; e += PPO_THREADS) P[e] = partials[(size_t)c0 * 3 + e];
    __syncthreads();
    if (tid < 3) {
#pragma unroll 8
      for (int c = 0; c < n; ++c) T = T + P[3 * c + tid];
    }
    __syncthreads();
  }
  if (tid < 3) S[tid] = T;
  __syncthreads();
  if (tid == 0) pob_ppo_finish(S[0], S[1], S[2], M, entropy_cost, losses);
}

static int ppo_chunks(long long M, long long *n_chunks) {
  if (M < 1) return pob_fail_msg(POB_EINVAL, "ppo_loss: the row count M must be positive");
  if (M > 0xFFFFFFFELL) return pob_fail_msg(POB_EINVAL, "ppo_loss: too many rows (M A must be below 2^32 - 1)");
  *n_chunks = (M + POB_PPO_CHUNK - 1) / POB_PPO_CHUNK;
  return POB_OK;
}

extern "C" {

int pob_ppo_loss_workspace_bytes(long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "ppo_loss: bytes is NULL");
  long long n_chunks;
  const int rc = ppo_chunks(M, &n_chunks);
  if (rc != POB_OK) return rc;
  // the chunk partials (n_chunks, 3) float64, then the rows' summands (3, M) float32
  *bytes = n_chunks * 3 * (long long)sizeof(double) + ((3 * M * (long long)sizeof(float) + 7) & ~7LL);
  return POB_OK;
}

int pob_ppo_loss(long long M, int A, const float *logits, const float *values, const int32_t *idx, const float *raw,
                 const float *old_logp, const float *advantages, const float *vs, const uint32_t *key, float entropy_cost,
                 float ppo_epsilon, float *dlogits, float *dvalues, float *losses, double *workspace, void *stream) {
  long long n_chunks;
  const int rc = ppo_chunks(M, &n_chunks);
  if (rc != POB_OK) return rc;
  if (A < 1 || A > POB_PPO_MAX_A) return pob_fail_msg(POB_EINVAL, "ppo_loss: the action size A must be in 1 .. 128");
  if (M * A >= 4294967295LL) return pob_fail_msg(POB_EINVAL, "ppo_loss: too many action elements (M A must be below 2^32 - 1)");
  if (!logits || !values || !raw || !old_logp || !advantages || !vs)
    return pob_fail_msg(POB_EINVAL, "ppo_loss: NULL argument (logits, values, raw, old_logp, advantages, vs)");
  if (!key) return pob_fail_msg(POB_EINVAL, "ppo_loss: key is NULL");
  if (!losses || !workspace) return pob_fail_msg(POB_EINVAL, "ppo_loss: NULL argument (losses, workspace)");
  const int R = PPO_ELEMS / A < PPO_MAX_ROWS ? PPO_ELEMS / A : PPO_MAX_ROWS;
  const long long tiles = (M + R - 1) / R;
  hipStream_t st = (hipStream_t)stream;
  float *terms = (float *)(workspace + n_chunks * 3);
  const float inv_m = 1.0f / (float)M;
  hipLaunchKernelGGL(k_ppo_loss, dim3((unsigned)tiles), dim3(PPO_THREADS), 0, st, M, A, R, logits, values, idx, raw, old_logp,
                     advantages, vs, key, entropy_cost, ppo_epsilon, inv_m, dlogits, dvalues, terms);
  hipLaunchKernelGGL(k_ppo_chunks, dim3((unsigned)n_chunks), dim3(PPO_THREADS), 0, st, M, (const float *)terms, workspace);
  hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(PPO_THREADS), 0, st, M, n_chunks, (const double *)workspace, entropy_cost, losses);
  return mlp_hip_check(hipGetLastError(), "k_ppo_loss launch");
}

}  // extern "C"

// ============================================================================ MLP backward
// mlp_forward_train_ref / mlp_backward_ref of pob_mlp.h (the specification; DESIGN.md "MLP
// backward").  k_mlp_forward_train: k_mlp_forward with every activated layer's accumulator tile
// also stored to `saved` before the activation, through the LDS image (coalesced); the activation
// is then applied to the image in place.  k_mlp_bwd_delta: one wave per tile of 32 rows walks the
// layers downwards with the incoming gradient in one LDS image [feature][env] and delta in the
// other: z_l is staged like an observation tile, delta_l = mlp_activate_grad(z_l, g) is stored to
// the workspace (M, out) coalesced, and G^T = W_l Delta^T runs on the MFMA with accumulators from
// +0 (the A operand of k-step s is W_l[i][2 s + h], a column walk of the L2-resident row-major
// matrix); the last G is dx.  k_mlp_bwd_weights: one wave per (chunk of POB_MLP_BWD_CHUNK rows,
// 32 x 32 tile of a layer's (in + 1, out) block): per tile of 32 rows sixteen MFMAs with the row
// as k (A = the layer's input, mlp_activate(z_{l-1}) recomputed on load, 1 for the bias row; B =
// delta; both row-contiguous across lanes), the sixteen float32 accumulators then added into
// sixteen float64 registers and zeroed; the float64 chunk partial goes to the workspace.
// k_mlp_bwd_reduce: one lane per parameter adds the chunk partials in ascending order and rounds
// once.  Vector stores only, no atomics, no scratch, no allocation.
POB_MLP_D bool mlp_activated(const MlpDesc &d, const int l) { return l != d.n_layers - 1 || d.act_final; }

// element e of an image's first 32 * width floats as its place in the image
POB_MLP_D int mlp_img_at(const int e) { return (e >> 5) * MLP_PITCH + (e & 31); }

template <int H>
__global__ __launch_bounds__(64) void k_mlp_forward_train(const MlpDesc d, const int split, const int B, const float *x,
                                                          const float *theta, float *y, float *saved) {
  __shared__ float img[H * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  float *src = img, *dst = img + split * MLP_PITCH;
  mlp_tile_load<false>(src, x, d.sizes[0], b0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
  __syncthreads();
  const float *W = theta;
  float *sv = saved;
  for (int l = 0; l < d.n_layers; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    const float *bias = W + (size_t)in * out;
    mlp_layer(src, dst, W, bias, in, out, false, d.act, lane);
    __syncthreads();
    if (mlp_activated(d, l)) {
      mlp_tile_store(sv, dst, 0, out, b0, valid, lane);
      sv += (size_t)B * out;
      __syncthreads();
      for (int e = lane; e < MLP_ROWS * out; e += 64) dst[mlp_img_at(e)] = mlp_activate(d.act, dst[mlp_img_at(e)]);
      __syncthreads();
    }
    W = bias + out;
    float *t = src; src = dst; dst = t;
  }
  mlp_tile_store(y, src, 0, d.sizes[d.n_layers], b0, valid, lane);
}

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

template <int H>
__global__ __launch_bounds__(64) void k_mlp_bwd_delta(const MlpDesc d, const int split, const int B, const float *theta,
                                                      const float *saved, const float *dy, float *delta, float *dx) {
  __shared__ float img[H * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  float *cur = img, *oth = img + split * MLP_PITCH;  // cur holds the incoming gradient
  size_t woff = 0, soff = 0, doff = 0;
  for (int l = 0; l < d.n_layers; ++l) {
    woff += ((size_t)d.sizes[l] + 1) * d.sizes[l + 1];
    doff += (size_t)B * d.sizes[l + 1];
    if (mlp_activated(d, l)) soff += (size_t)B * d.sizes[l + 1];
  }
  mlp_tile_load<false>(cur, dy, d.sizes[d.n_layers], b0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
  __syncthreads();
  for (int l = d.n_layers - 1; l >= 0; --l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    woff -= ((size_t)in + 1) * out;
    doff -= (size_t)B * out;
    float *D = cur, *G = oth;
    if (mlp_activated(d, l)) {
      soff -= (size_t)B * out;
      mlp_tile_load<false>(oth, saved + soff, out, b0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
      __syncthreads();
      for (int e = lane; e < MLP_ROWS * out; e += 64)
        oth[mlp_img_at(e)] = mlp_activate_grad(d.act, oth[mlp_img_at(e)], cur[mlp_img_at(e)]);
      __syncthreads();
      D = oth; G = cur;
    }
    mlp_tile_store(delta + doff, D, 0, out, b0, valid, lane);
    if (l == 0 && !dx) break;
    mlp_layer_back(D, G, theta + woff, in, out, lane);
    __syncthreads();
    cur = G; oth = D;
  }
  if (dx) mlp_tile_store(dx, cur, 0, d.sizes[0], b0, valid, lane);
}

__global__ __launch_bounds__(64) void k_mlp_bwd_weights(const MlpDesc d, const int B, const long long n_params,
                                                        const float *x, const float *saved, const float *delta,
                                                        double *partials) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  // blockIdx.y counts the 32 x 32 tiles of the layers' (in + 1, out) blocks, layer by layer
  int t = blockIdx.y, l = 0, tj;
  size_t woff = 0, aoff = 0, doff = 0;  // layer l's block of theta, z_{l-1} in saved, delta_l
  for (;; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    tj = (out + 31) >> 5;
    const int n = ((in + 32) >> 5) * tj;
    if (t < n || l == d.n_layers - 1) break;
    t -= n;
    woff += ((size_t)in + 1) * out;
    doff += (size_t)B * out;
    if (l > 0) aoff += (size_t)B * in;
  }
  const int in = d.sizes[l], out = d.sizes[l + 1];
  const int ai = (t / tj) * 32 + j, bj = (t % tj) * 32 + j;
  const bool a_ok = ai < in, a_one = ai == in, b_ok = bj < out;
  const float *A = l ? saved + aoff : x, *D = delta + doff;
  const int r_begin = blockIdx.x * POB_MLP_BWD_CHUNK;
  const int r_end = B - r_begin < POB_MLP_BWD_CHUNK ? B : r_begin + POB_MLP_BWD_CHUNK;
  double sum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[r] = 0.0;
  for (int rt = r_begin; rt < r_end; rt += 32) {
    float a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = rt + mlp_kfeat(u, h);
      const bool rok = row < r_end;
      a[u] = (rok && a_ok) ? A[(size_t)row * in + ai] : 0.0f;
      b[u] = (rok && b_ok) ? D[(size_t)row * out + bj] : 0.0f;
    }
    if (l) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float v = mlp_activate(d.act, a[u]);
        a[u] = (rt + mlp_kfeat(u, h) < r_end && a_ok) ? v : 0.0f;
      }
    }
    if (a_one) {
#pragma unroll
      for (int u = 0; u < 16; ++u) a[u] = rt + mlp_kfeat(u, h) < r_end ? 1.0f : 0.0f;
    }
    mlp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = sum[r] + (double)acc[r];
  }
  double *P = partials + (size_t)blockIdx.x * (size_t)n_params + woff;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (t / tj) * 32 + mlp_acc_row(r, h);
    if (i <= in && b_ok) P[(size_t)i * out + bj] = sum[r];
  }
}

__global__ __launch_bounds__(256) void k_mlp_bwd_reduce(const double *partials, const long long n_chunks,
                                                        const long long n_params, float *dtheta) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_params) return;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += OBSNORM_RSTAGE) {
    double v[OBSNORM_RSTAGE];
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u) v[u] = c0 + u < n_chunks ? partials[(size_t)(c0 + u) * n_params + p] : 0.0;
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u)
      if (c0 + u < n_chunks) T = T + v[u];
  }
  dtheta[p] = (float)T;
}

static int mlp_widest(const MlpDesc &d) {
  int w = 1;
  for (int l = 0; l <= d.n_layers; ++l)
    if (d.sizes[l] > w) w = d.sizes[l];
  return w;
}

// the pool of the delta kernel, two images of the widest layer: the height class of MLP_DISPATCH_T
static int train_rows(const MlpDesc &d, int &split) {
  split = mlp_widest(d);
  const int rows = 2 * split;
  return rows <= 64 ? 0 : (rows <= 152 ? 1 : (rows <= 288 ? 2 : 3));
}

// the float counts of saved and of the workspace's delta arrays.  (M + a chunk) times the widest
// layer must stay below 2^31: the kernels count rows, and a chunk's end, in int
static int mlp_bwd_counts(const pob_mlp *m, long long M, long long *n_saved, long long *n_delta) {
  if (!m) return pob_fail_msg(POB_EINVAL, "mlp is NULL");
  if (M < 1) return pob_fail_msg(POB_EINVAL, "mlp: the row count M must be positive");
  if (M + POB_MLP_BWD_CHUNK >= (1LL << 31) / mlp_widest(m->d))
    return pob_fail_msg(POB_EINVAL, "mlp: too many rows ((M + 1024) times the widest layer must be below 2^31)");
  *n_saved = *n_delta = 0;
  for (int l = 0; l < m->d.n_layers; ++l) {
    *n_delta += M * m->d.sizes[l + 1];
    if (l != m->d.n_layers - 1 || m->d.act_final) *n_saved += M * m->d.sizes[l + 1];
  }
  return POB_OK;
}

extern "C" {

int pob_mlp_saved_bytes(const pob_mlp *m, long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "mlp: bytes is NULL");
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  *bytes = n_saved * (long long)sizeof(float);
  return POB_OK;
}

int pob_mlp_forward_train(const pob_mlp *m, long long M, const float *x, const float *theta, float *y, float *saved,
                          void *stream) {
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  if (!x || !theta || !y || (n_saved && !saved)) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument (x, theta, y, saved)");
  int split;
  const int cls = image_rows(m->d, false, split);
  const int B = (int)M;
  const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  MLP_DISPATCH_T(k_mlp_forward_train, , cls, m->d, split, B, x, theta, y, saved)
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward_train launch");
}

int pob_mlp_backward_workspace_bytes(const pob_mlp *m, long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "mlp: bytes is NULL");
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  const long long n_chunks = (M + POB_MLP_BWD_CHUNK - 1) / POB_MLP_BWD_CHUNK;
  // the delta arrays (M, sizes[l + 1]) float32 of every layer, then the chunk partials (n_chunks, n_params) float64
  *bytes = ((n_delta * (long long)sizeof(float) + 7) & ~7LL) + n_chunks * m->n_params * (long long)sizeof(double);
  return POB_OK;
}

int pob_mlp_backward(const pob_mlp *m, long long M, const float *x, const float *theta, const float *saved,
                     const float *dy, float *dtheta, float *dx, void *workspace, void *stream) {
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  if (!x || !theta || !dy || !dtheta || !workspace || (n_saved && !saved))
    return pob_fail_msg(POB_EINVAL, "mlp: NULL argument (x, theta, saved, dy, dtheta, workspace)");
  const int B = (int)M;
  const long long n_chunks = (M + POB_MLP_BWD_CHUNK - 1) / POB_MLP_BWD_CHUNK;
  float *delta = (float *)workspace;
  double *partials = (double *)((char *)workspace + ((n_delta * (long long)sizeof(float) + 7) & ~7LL));
  hipStream_t st = (hipStream_t)stream;
  {
    int split;
    const int cls = train_rows(m->d, split);
    const dim3 grid((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS));
    MLP_DISPATCH_T(k_mlp_bwd_delta, , cls, m->d, split, B, theta, saved, dy, delta, dx)
  }
  unsigned tiles = 0;
  for (int l = 0; l < m->d.n_layers; ++l) tiles += (unsigned)(((m->d.sizes[l] + 32) >> 5) * ((m->d.sizes[l + 1] + 31) >> 5));
  hipLaunchKernelGGL(k_mlp_bwd_weights, dim3((unsigned)n_chunks, tiles), dim3(64), 0, st, m->d, B, m->n_params, x, saved,
                     (const float *)delta, partials);
  hipLaunchKernelGGL(k_mlp_bwd_reduce, dim3((unsigned)((m->n_params + 255) / 256)), dim3(256), 0, st,
                     (const double *)partials, n_chunks, m->n_params, dtheta);
  return mlp_hip_check(hipGetLastError(), "k_mlp_bwd launch");
}

}  // extern "C"

// ============================================================================ recurrent backward
// gru_sequence_forward_train_ref / gru_sequence_backward_ref of pob_mlp.h (the specification;
// DESIGN.md "Recurrent backward").  k_gru_seq_forward: one wave per tile of 32 sequences loops
// over the window's T steps inside the launch, h staying in LDS between steps: each step is
// gru_tile_forward's walk (the same chains, so the same bits) with the observation rows gathered
// through idx, and every array the backward needs stored to `saved` through the LDS images
// (coalesced).  k_gru_seq_backward: the same tile with t descending, the carry in LDS: per step
// the post-MLP's delta walk (k_mlp_bwd_delta's), the cell's element-wise part in the rows' own
// order (coalesced loads of the gates, coalesced stores of the four deltas), the carry product
// and, under a pre-MLP, g_x on the MFMA with accumulators from +0, then the pre-MLP's delta walk.
// k_gru_bwd_weights: k_mlp_bwd_weights over a table of blocks (the dense layers, and W_rz in two
// row ranges, W_xn, W_hn reading xc / hin raw from saved); k_mlp_bwd_reduce finishes.  Vector
// stores only, no atomics, no scratch, no allocation, no host synchronisation.
struct GruSeqArgs {
  int T, M;            // steps, sequences
  long long B;         // envs of the trajectory arrays
  gru_seq_plan p;
};

// features [0, D) of an image <- rows of a row-major (B, D) array: tile row `row` reads array row
// idx[m0 + row] (idx NULL: m0 + row), tail rows repeating the last valid one.  NORM as in
// mlp_tile_load.
template <bool NORM>
POB_MLP_D void gru_seq_tile_gather(float *img, const float *x, const int D, const int32_t *idx, const int m0,
                                   const int valid, const float *norm, const float clip, const int lane) {
  const int dq = 64 / D, dr = 64 - dq * D;
  int row = lane / D, col = lane - row * D;
  for (int e0 = lane; e0 < MLP_ROWS * D; e0 += 64 * MLP_STAGE) {
    float v[MLP_STAGE], mu[NORM ? MLP_STAGE : 1], sc[NORM ? MLP_STAGE : 1];
    int at[MLP_STAGE];
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u) {
      const bool in_tile = e0 + 64 * u < MLP_ROWS * D;
      const int rr = row < valid ? row : valid - 1;
      const size_t src = in_tile ? (idx ? (size_t)idx[m0 + rr] : (size_t)(m0 + rr)) : 0;
      v[u] = in_tile ? x[src * D + col] : 0.0f;
      if (NORM) {
        mu[u] = in_tile ? norm[col] : 0.0f;
        sc[u] = in_tile ? norm[D + col] : 0.0f;
      }
      at[u] = in_tile ? col * MLP_PITCH + row : -1;
      row += dq; col += dr;
      if (col >= D) { col -= D; ++row; }
    }
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u)
      if (at[u] >= 0) img[at[u]] = NORM ? pob_obsnorm_apply(v[u], mu[u], sc[u], clip) : v[u];
  }
}

// gru_cell, with r, z, ch, n also written to the image GT (4 H features)
POB_MLP_D void gru_cell_train(const float *C, float *N, float *GT, const float *g, const int I, const int H,
                              const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const float *W_rz = g, *b_rz = W_rz + (size_t)(I + H) * 2 * H;
  const float *W_xn = b_rz + 2 * H, *b_xn = W_xn + (size_t)I * H;
  const float *W_hn = b_xn + H, *b_hn = W_hn + (size_t)H * H;
  for (int ot = 0; ot < H; ot += 32) {
    const int col = ot + j;
    const bool cok = col < H;
    mlp_f32x16 ar, az, ax, ah;
    mlp_acc_bias(ar, b_rz, ot, H, h);
    mlp_chain(ar, C, W_rz, 2 * H, col, cok, I + H, lane);
    mlp_acc_bias(az, b_rz + H, ot, H, h);
    mlp_chain(az, C, W_rz, 2 * H, H + col, cok, I + H, lane);
    mlp_acc_bias(ax, b_xn, ot, H, h);
    mlp_chain(ax, C, W_xn, H, col, cok, I, lane);
    mlp_acc_bias(ah, b_hn, ot, H, h);
    mlp_chain(ah, C + I * MLP_PITCH, W_hn, H, col, cok, H, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ot + mlp_acc_row(r, h);
      if (i < H) {
        const float rg = pob_sigmoidf(ar[r]), zg = pob_sigmoidf(az[r]);
        const float n = pob_tanhf(MLP_FMA(rg, ah[r], ax[r]));
        const float hold = C[(I + i) * MLP_PITCH + j];
        N[i * MLP_PITCH + j] = MLP_FMA(zg, hold - n, n);
        GT[i * MLP_PITCH + j] = rg;
        GT[(H + i) * MLP_PITCH + j] = zg;
        GT[(2 * H + i) * MLP_PITCH + j] = ah[r];
        GT[(3 * H + i) * MLP_PITCH + j] = n;
      }
    }
  }
}

template <int R, bool NORM>
__global__ __launch_bounds__(64) void k_gru_seq_forward(const GruDesc d, const GruSeqArgs a, const float *obs,
                                                        const int32_t *idx, const float *h0, const float *reset,
                                                        const float *theta, float *y, float *h_last, float *saved,
                                                        const float *norm, const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, m0 = blockIdx.x * MLP_ROWS;
  const int valid = a.M - m0 < MLP_ROWS ? a.M - m0 : MLP_ROWS;
  const int D = d.pre[0], I = d.pre[d.n_pre], H = d.hid, out_w = d.post[d.n_post - 1];
  const size_t Rows = (size_t)a.T * a.M;
  float *C = pool, *N = C + (I + H) * MLP_PITCH;
  float *P0 = N + H * MLP_PITCH, *P1 = P0 + d.p_rows[0] * MLP_PITCH, *GT = P0;  // GT lives between the dense walks
  float *Hc = C + I * MLP_PITCH;
  gru_seq_tile_gather<false>(Hc, h0, H, idx, m0, valid, nullptr, 0.0f, lane);
  for (int t = 0; t < a.T; ++t) {
    const size_t r0 = (size_t)t * a.M;  // the step's first row of the (R, .) arrays
    __syncthreads();
    gru_seq_tile_gather<NORM>(d.n_pre ? P0 : C, obs + (size_t)t * a.B * D, D, idx, m0, valid, norm, clip, lane);
    if (reset) {
      const int row = lane & 31, rr = row < valid ? row : valid - 1;
      const size_t env = idx ? (size_t)idx[m0 + rr] : (size_t)(m0 + rr);
      const bool zero = reset[(size_t)t * a.B + env] != 0.0f;
      if (zero)
        for (int f = lane >> 5; f < H; f += 2) Hc[f * MLP_PITCH + row] = 0.0f;
    }
    __syncthreads();
    const float *W = theta;
    float *src = P0;
    int pp = d.n_pre ? 1 : 0;
    if (d.n_pre) mlp_tile_store(saved + a.p.xin + r0 * D, P0, 0, D, m0, valid, lane);
    size_t so = (size_t)a.p.pre;
    for (int l = 0; l < d.n_pre; ++l) {
      const int in = d.pre[l], out = d.pre[l + 1];
      const float *bias = W + (size_t)in * out;
      float *dst = l == d.n_pre - 1 ? C : (pp ? P1 : P0);
      mlp_layer(src, dst, W, bias, in, out, false, d.act, lane);
      __syncthreads();
      mlp_tile_store(saved + so + r0 * out, dst, 0, out, m0, valid, lane);
      so += Rows * out;
      __syncthreads();
      for (int e = lane; e < MLP_ROWS * out; e += 64) dst[mlp_img_at(e)] = mlp_activate(d.act, dst[mlp_img_at(e)]);
      __syncthreads();
      W = bias + out;
      src = dst;
      pp ^= 1;
    }
    mlp_tile_store(saved + a.p.xc + r0 * I, C, 0, I, m0, valid, lane);
    mlp_tile_store(saved + a.p.hin + r0 * H, C, I, H, m0, valid, lane);
    gru_cell_train(C, N, GT, W, I, H, lane);
    __syncthreads();
    W += (size_t)3 * H * I + (size_t)3 * H * H + 4 * H;
    mlp_tile_store(saved + a.p.gate + r0 * 4 * H, GT, 0, 4 * H, m0, valid, lane);
    mlp_tile_store(saved + a.p.hn + r0 * H, N, 0, H, m0, valid, lane);
    if (h_last && t == a.T - 1) mlp_tile_store(h_last, N, 0, H, m0, valid, lane);
    __syncthreads();  // GT is read out before the post-MLP writes P0 / P1
    src = N;
    int in = H;
    so = (size_t)a.p.post;
    for (int l = 0; l < d.n_post; ++l) {
      const int out = d.post[l];
      const float *bias = W + (size_t)in * out;
      float *dst = pp ? P1 : P0;
      mlp_layer(src, dst, W, bias, in, out, false, d.act, lane);
      __syncthreads();
      if (l != d.n_post - 1) {
        mlp_tile_store(saved + so + r0 * out, dst, 0, out, m0, valid, lane);
        so += Rows * out;
        __syncthreads();
        for (int e = lane; e < MLP_ROWS * out; e += 64) dst[mlp_img_at(e)] = mlp_activate(d.act, dst[mlp_img_at(e)]);
        __syncthreads();
      }
      W = bias + out;
      src = dst;
      in = out;
      pp ^= 1;
    }
    mlp_tile_store(y + r0 * out_w, src, 0, out_w, m0, valid, lane);
    for (int e = lane; e < MLP_ROWS * H; e += 64) Hc[mlp_img_at(e)] = N[mlp_img_at(e)];  // h' is the next step's h
  }
}

// The window for inference (gru_sequence_forward_ref; DESIGN.md "Recurrent critic"): the tile and
// the step loop of k_gru_seq_forward with gru_tile_forward's own walk per step (activations fused
// into the layers, gru_cell), h staying in LDS, and no store but y, h_first and h_out.  The pool is
// gru_tile_forward's: C = [x ; h], N, P0, P1 -- no gate image.  h_out may be h0 when idx is NULL:
// the tile's rows of h0 are in LDS before the first barrier, its h_out store comes after it.
// The pool admits 12 / 7 / 5 / 3 / 2 / 1 blocks a CU; the cell's four accumulators and operand
// staging take more than 256 registers a lane, so one wave a SIMD (four blocks a CU) is resident.
// Asking for two waves a SIMD spills to scratch and measured 1.3 - 1.4 x slower.
template <int R, bool NORM>
__global__ __launch_bounds__(64) void k_gru_seq_infer(const GruDesc d, const int S, const int M, const long long B,
                                                      const float *obs, const int32_t *idx, const float *h0,
                                                      const float *reset, const float *theta, float *y, float *h_first,
                                                      float *h_out, const int h_out_step, const float *norm,
                                                      const float clip) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, m0 = blockIdx.x * MLP_ROWS;
  const int valid = M - m0 < MLP_ROWS ? M - m0 : MLP_ROWS;
  const int D = d.pre[0], I = d.pre[d.n_pre], H = d.hid, out_w = d.post[d.n_post - 1];
  float *C = pool, *N = C + (I + H) * MLP_PITCH;
  float *P0 = N + H * MLP_PITCH, *P1 = P0 + d.p_rows[0] * MLP_PITCH;
  float *Hc = C + I * MLP_PITCH;
  gru_seq_tile_gather<false>(Hc, h0, H, idx, m0, valid, nullptr, 0.0f, lane);
  for (int s = 0; s < S; ++s) {
    __syncthreads();
    gru_seq_tile_gather<NORM>(d.n_pre ? P0 : C, obs + (size_t)s * B * D, D, idx, m0, valid, norm, clip, lane);
    if (reset) {
      const int row = lane & 31, rr = row < valid ? row : valid - 1;
      const size_t env = idx ? (size_t)idx[m0 + rr] : (size_t)(m0 + rr);
      const bool zero = reset[(size_t)s * B + env] != 0.0f;
      if (zero)
        for (int f = lane >> 5; f < H; f += 2) Hc[f * MLP_PITCH + row] = 0.0f;
    }
    __syncthreads();
    if (h_first && s == 0) mlp_tile_store(h_first, C, I, H, m0, valid, lane);
    const float *W = theta;
    float *src = P0;
    int pp = d.n_pre ? 1 : 0;
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
    if (h_out && s + 1 == h_out_step) mlp_tile_store(h_out, N, 0, H, m0, valid, lane);
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
    mlp_tile_store(y + (size_t)s * M * out_w, src, 0, out_w, m0, valid, lane);
    for (int e = lane; e < MLP_ROWS * H; e += 64) Hc[mlp_img_at(e)] = N[mlp_img_at(e)];  // h' is the next step's h
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

template <int R>
__global__ __launch_bounds__(64) void k_gru_seq_backward(const GruDesc d, const GruSeqArgs a, const int wmax,
                                                         const int32_t *idx, const float *reset, const float *theta,
                                                         const float *saved, const float *dy, const float *dh_last,
                                                         float *delta, float *dh0) {
  __shared__ float pool[R * MLP_PITCH];
  const int lane = threadIdx.x, j = lane & 31, hh = lane >> 5, m0 = blockIdx.x * MLP_ROWS;
  const int valid = a.M - m0 < MLP_ROWS ? a.M - m0 : MLP_ROWS;
  const int I = d.pre[d.n_pre], H = d.hid, out_w = d.post[d.n_post - 1];
  const size_t Rows = (size_t)a.T * a.M;
  // CAR: the carry (during a step's products: z), DL: the cell's four deltas, GA / GB: the walks' images
  float *CAR = pool, *DL = CAR + H * MLP_PITCH, *GA = DL + 4 * H * MLP_PITCH, *GB = GA + wmax * MLP_PITCH;
  size_t w_cell = 0, w_end = 0, s_post_end = (size_t)a.p.post, d_post_end = (size_t)a.p.d_post;
  size_t s_pre_end = (size_t)a.p.pre, d_pre_end = (size_t)a.p.d_pre;
  for (int l = 0; l < d.n_pre; ++l) {
    w_cell += ((size_t)d.pre[l] + 1) * d.pre[l + 1];
    s_pre_end += Rows * d.pre[l + 1];
    d_pre_end += Rows * d.pre[l + 1];
  }
  w_end = w_cell + (size_t)3 * H * I + (size_t)3 * H * H + 4 * H;
  for (int l = 0; l < d.n_post; ++l) {
    w_end += ((size_t)(l ? d.post[l - 1] : H) + 1) * d.post[l];
    d_post_end += Rows * d.post[l];
    if (l != d.n_post - 1) s_post_end += Rows * d.post[l];
  }
  const float *W_rz = theta + w_cell, *W_xn = W_rz + (size_t)(I + H) * 2 * H + 2 * H;
  const float *W_hn = W_xn + (size_t)I * H + H;
  if (dh_last) {
    mlp_tile_load<false>(CAR, dh_last, H, m0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
  } else {
    for (int e = lane; e < MLP_ROWS * H; e += 64) CAR[mlp_img_at(e)] = 0.0f;
  }
  for (int t = a.T - 1; t >= 0; --t) {
    const size_t r0 = (size_t)t * a.M;
    float *cur = GA, *oth = GB;
    __syncthreads();
    mlp_tile_load<false>(cur, dy + r0 * out_w, out_w, m0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
    __syncthreads();
    // ---- the post-MLP's delta walk; cur ends as g_post (H features)
    size_t woff = w_end, soff = s_post_end, doff = d_post_end;
    for (int l = d.n_post - 1; l >= 0; --l) {
      const int in = l ? d.post[l - 1] : H, out = d.post[l];
      woff -= ((size_t)in + 1) * out;
      doff -= Rows * out;
      float *Dm = cur, *G = oth;
      if (l != d.n_post - 1) {
        soff -= Rows * out;
        mlp_tile_load<false>(oth, saved + soff + r0 * out, out, m0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
        __syncthreads();
        for (int e = lane; e < MLP_ROWS * out; e += 64)
          oth[mlp_img_at(e)] = mlp_activate_grad(d.act, oth[mlp_img_at(e)], cur[mlp_img_at(e)]);
        __syncthreads();
        Dm = oth; G = cur;
      }
      mlp_tile_store(delta + doff + r0 * out, Dm, 0, out, m0, valid, lane);
      __syncthreads();  // the store has read Dm's partner image before the product overwrites it
      mlp_layer_back(Dm, G, theta + woff, in, out, lane);
      __syncthreads();
      cur = G; oth = Dm;
    }
    // ---- the cell, element-wise, in the rows' own order: g_h stays in cur, z goes to CAR
    {
      const float *gt = saved + a.p.gate + (r0 + m0) * 4 * H, *hin = saved + a.p.hin + (r0 + m0) * H;
      float *dc = delta + a.p.d_cell + (r0 + m0) * 4 * H;
      for (int e = lane; e < valid * H; e += 64) {
        const int row = e / H, col = e - row * H;
        const float *g4 = gt + (size_t)row * 4 * H + col;
        const float rg = g4[0], zg = g4[H], ch = g4[2 * H], n = g4[3 * H], hi = hin[e];
        const int at = col * MLP_PITCH + row;
        const float g_h = cur[at] + CAR[at];
        float d_r, d_z, d_xn, d_hn;
        pob_gru_cell_grad(g_h, hi, rg, zg, ch, n, d_r, d_z, d_xn, d_hn);
        cur[at] = g_h;
        CAR[at] = zg;
        DL[at] = d_r; DL[H * MLP_PITCH + at] = d_z; DL[2 * H * MLP_PITCH + at] = d_xn; DL[3 * H * MLP_PITCH + at] = d_hn;
        float *o4 = dc + (size_t)row * 4 * H + col;
        o4[0] = d_r; o4[H] = d_z; o4[2 * H] = d_xn; o4[3 * H] = d_hn;
      }
      // tail rows of the images: finite values, never stored
      for (int e = lane; e < MLP_ROWS * H; e += 64) {
        const int col = e >> 5, row = e & 31;
        if (row >= valid) {
          const int at = col * MLP_PITCH + row;
          cur[at] = 0.0f; CAR[at] = 0.0f;
          DL[at] = 0.0f; DL[H * MLP_PITCH + at] = 0.0f; DL[2 * H * MLP_PITCH + at] = 0.0f; DL[3 * H * MLP_PITCH + at] = 0.0f;
        }
      }
    }
    __syncthreads();
    // ---- g_x (under a pre-MLP) into oth, then the carry into CAR
    if (d.n_pre) {
      for (int it = 0; it < I; it += 32) {
        const int row = it + j;
        const bool rok = row < I;
        mlp_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        mlp_chain_back(acc, DL, W_rz, 2 * H, row, rok, 2 * H, lane);
        mlp_chain_back(acc, DL + 2 * H * MLP_PITCH, W_xn, H, row, rok, H, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = it + mlp_acc_row(r, hh);
          if (i < I) oth[i * MLP_PITCH + j] = acc[r];
        }
      }
    }
    {
      bool zero = false;
      if (reset) {
        const int rr = j < valid ? j : valid - 1;
        const size_t env = idx ? (size_t)idx[m0 + rr] : (size_t)(m0 + rr);
        zero = reset[(size_t)t * a.B + env] != 0.0f;
      }
      for (int it = 0; it < H; it += 32) {
        const int row = it + j;
        const bool rok = row < H;
        mlp_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        mlp_chain_back(acc, DL, W_rz + (size_t)I * 2 * H, 2 * H, row, rok, 2 * H, lane);
        mlp_chain_back(acc, DL + 3 * H * MLP_PITCH, W_hn, H, row, rok, H, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = it + mlp_acc_row(r, hh);
          if (i < H) {
            const int at = i * MLP_PITCH + j;
            CAR[at] = zero ? 0.0f : MLP_FMA(cur[at], CAR[at], acc[r]);
          }
        }
      }
    }
    __syncthreads();
    // ---- the pre-MLP's delta walk from g_x (every layer activated, no dx)
    if (d.n_pre) {
      float *g = oth, *z = cur;
      size_t woff2 = w_cell, soff2 = s_pre_end, doff2 = d_pre_end;
      for (int l = d.n_pre - 1; l >= 0; --l) {
        const int in = d.pre[l], out = d.pre[l + 1];
        woff2 -= ((size_t)in + 1) * out;
        soff2 -= Rows * out;
        doff2 -= Rows * out;
        mlp_tile_load<false>(z, saved + soff2 + r0 * out, out, m0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
        __syncthreads();
        for (int e = lane; e < MLP_ROWS * out; e += 64)
          z[mlp_img_at(e)] = mlp_activate_grad(d.act, z[mlp_img_at(e)], g[mlp_img_at(e)]);
        __syncthreads();
        mlp_tile_store(delta + doff2 + r0 * out, z, 0, out, m0, valid, lane);
        if (l == 0) break;
        __syncthreads();
        mlp_layer_back(z, g, theta + woff2, in, out, lane);
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (dh0) mlp_tile_store(dh0, CAR, 0, H, m0, valid, lane);
}

// The blocks of the parameter gradient: block q is rows [0, in + bias) of an (., out) matrix at
// float offset woff of theta's packing, the sum over the rows of A[r][i] D[r][j]: A (R, in) at
// float offset a_off of saved (act: mlp_activate recomputed on load), the bias row the constant 1;
// D at float offset d_off of delta, its rows ldd floats apart.
#define GRU_BWD_MAX_BLOCKS (POB_GRU_MAX_PRE + 4 + POB_GRU_MAX_POST)
struct GruBwdBlocks {
  int n;
  int in[GRU_BWD_MAX_BLOCKS], out[GRU_BWD_MAX_BLOCKS], ldd[GRU_BWD_MAX_BLOCKS], bias[GRU_BWD_MAX_BLOCKS],
      act[GRU_BWD_MAX_BLOCKS];
  long long a_off[GRU_BWD_MAX_BLOCKS], d_off[GRU_BWD_MAX_BLOCKS], woff[GRU_BWD_MAX_BLOCKS];
};

__global__ __launch_bounds__(64) void k_gru_bwd_weights(const GruBwdBlocks q, const int act, const int B,
                                                        const long long n_params, const float *saved, const float *delta,
                                                        double *partials) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  int t = blockIdx.y, l = 0, tj;
  for (;; ++l) {
    tj = (q.out[l] + 31) >> 5;
    const int n = ((q.in[l] + q.bias[l] + 31) >> 5) * tj;
    if (t < n || l == q.n - 1) break;
    t -= n;
  }
  const int in = q.in[l], out = q.out[l], ldd = q.ldd[l];
  const bool recompute = q.act[l] != 0, has_bias = q.bias[l] != 0;
  const int ai = (t / tj) * 32 + j, bj = (t % tj) * 32 + j;
  const bool a_ok = ai < in, a_one = has_bias && ai == in, b_ok = bj < out;
  const float *A = saved + q.a_off[l], *D = delta + q.d_off[l];
  const int r_begin = blockIdx.x * POB_MLP_BWD_CHUNK;
  const int r_end = B - r_begin < POB_MLP_BWD_CHUNK ? B : r_begin + POB_MLP_BWD_CHUNK;
  double sum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[r] = 0.0;
  for (int rt = r_begin; rt < r_end; rt += 32) {
    float a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = rt + mlp_kfeat(u, h);
      const bool rok = row < r_end;
      a[u] = (rok && a_ok) ? A[(size_t)row * in + ai] : 0.0f;
      b[u] = (rok && b_ok) ? D[(size_t)row * ldd + bj] : 0.0f;
    }
    if (recompute) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float v = mlp_activate(act, a[u]);
        a[u] = (rt + mlp_kfeat(u, h) < r_end && a_ok) ? v : 0.0f;
      }
    }
    if (a_one) {
#pragma unroll
      for (int u = 0; u < 16; ++u) a[u] = rt + mlp_kfeat(u, h) < r_end ? 1.0f : 0.0f;
    }
    mlp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = sum[r] + (double)acc[r];
  }
  double *P = partials + (size_t)blockIdx.x * (size_t)n_params + q.woff[l];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (t / tj) * 32 + mlp_acc_row(r, h);
    if (i < in + (has_bias ? 1 : 0) && b_ok) P[(size_t)i * out + bj] = sum[r];
  }
}

// pool heights of the two sequential kernels (rows of MLP_PITCH floats) and their classes
// (with_obs: the observation width counts too; the backward's images never hold it)
static int gru_seq_widest(const GruDesc &d, bool with_obs) {
  int w = d.hid;
  for (int l = with_obs ? 0 : 1; l <= d.n_pre; ++l)
    if (d.pre[l] > w) w = d.pre[l];
  for (int l = 0; l < d.n_post; ++l)
    if (d.post[l] > w) w = d.post[l];
  return w;
}
static int gru_seq_forward_rows(const GruDesc &d) {
  const int p = d.p_rows[0] + d.p_rows[1];
  return d.pre[d.n_pre] + 2 * d.hid + (4 * d.hid > p ? 4 * d.hid : p);
}
static int gru_seq_backward_rows(const GruDesc &d) { return 5 * d.hid + 2 * gru_seq_widest(d, false); }

#define GRU_SEQ_FWD_N(N, rows, ...)                                                                              \
  if (rows <= 224) hipLaunchKernelGGL((k_gru_seq_forward<224, N>), grid, dim3(64), 0, st, __VA_ARGS__);          \
  else if (rows <= 512) hipLaunchKernelGGL((k_gru_seq_forward<512, N>), grid, dim3(64), 0, st, __VA_ARGS__);     \
  else hipLaunchKernelGGL((k_gru_seq_forward<896, N>), grid, dim3(64), 0, st, __VA_ARGS__);

// every limit of the sequence entry points, before any HIP call
static int gru_seq_check(const pob_gru *g, int T, long long M, long long B, bool have_idx, GruSeqArgs *a) {
  if (!g) return pob_fail_msg(POB_EINVAL, "gru is NULL");
  if (T < 1) return pob_fail_msg(POB_EINVAL, "gru sequence: the step count T must be positive");
  if (M < 1) return pob_fail_msg(POB_EINVAL, "gru sequence: the sequence count M must be positive");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "gru sequence: the env count B must be positive");
  if (!have_idx && M != B) return pob_fail_msg(POB_EINVAL, "gru sequence: without idx M must equal B");
  const long long widest = gru_seq_widest(g->d, true) > 4 * g->d.hid ? gru_seq_widest(g->d, true) : 4 * g->d.hid;
  if (M > (1LL << 31) / widest || (long long)T * M + POB_MLP_BWD_CHUNK >= (1LL << 31) / widest)
    return pob_fail_msg(POB_EINVAL, "gru sequence: too many rows ((T M + 1024) times the widest array, 4 H included, must be below 2^31)");
  if (B >= (1LL << 31)) return pob_fail_msg(POB_EINVAL, "gru sequence: at most 2^31 - 1 envs (idx is int32)");
  if (a) {
    a->T = T; a->M = (int)M; a->B = B;
    a->p = gru_seq_layout(g->d.n_pre, g->d.pre, g->d.hid, g->d.n_post, g->d.post, (long long)T * M);
  }
  return POB_OK;
}

extern "C" {

int pob_gru_sequence_saved_bytes(const pob_gru *g, int T, long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "gru sequence: bytes is NULL");
  GruSeqArgs a;
  const int rc = gru_seq_check(g, T, M, M, false, &a);
  if (rc != POB_OK) return rc;
  *bytes = a.p.n_saved * (long long)sizeof(float);
  return POB_OK;
}

int pob_gru_sequence_forward_train(const pob_gru *g, int T, long long M, long long B, const float *obs, const int32_t *idx,
                                   const float *h0, const float *reset, const float *theta, float *y, float *h_last,
                                   float *saved, const float *norm, float norm_clip, void *stream) {
  GruSeqArgs a;
  const int rc = gru_seq_check(g, T, M, B, idx != nullptr, &a);
  if (rc != POB_OK) return rc;
  if (!obs || !h0 || !theta || !y || !saved)
    return pob_fail_msg(POB_EINVAL, "gru sequence: NULL argument (obs, h0, theta, y, saved)");
  GruDesc d = g->d;
  gru_plan(d, false, d.p_rows);
  const int rows = gru_seq_forward_rows(d);
  const dim3 grid((unsigned)((M + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  if (norm) { GRU_SEQ_FWD_N(true, rows, d, a, obs, idx, h0, reset, theta, y, h_last, saved, norm, norm_clip) }
  else { GRU_SEQ_FWD_N(false, rows, d, a, obs, idx, h0, reset, theta, y, h_last, saved, norm, norm_clip) }
  return mlp_hip_check(hipGetLastError(), "k_gru_seq_forward launch");
}

int pob_gru_sequence_backward_workspace_bytes(const pob_gru *g, int T, long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "gru sequence: bytes is NULL");
  GruSeqArgs a;
  const int rc = gru_seq_check(g, T, M, M, false, &a);
  if (rc != POB_OK) return rc;
  const long long n_chunks = ((long long)T * M + POB_MLP_BWD_CHUNK - 1) / POB_MLP_BWD_CHUNK;
  *bytes = ((a.p.n_delta * (long long)sizeof(float) + 7) & ~7LL) + n_chunks * g->n_params * (long long)sizeof(double);
  return POB_OK;
}

int pob_gru_sequence_backward(const pob_gru *g, int T, long long M, long long B, const int32_t *idx, const float *reset,
                              const float *theta, const float *saved, const float *dy, const float *dh_last,
                              float *dtheta, float *dh0, void *workspace, void *stream) {
  GruSeqArgs a;
  const int rc = gru_seq_check(g, T, M, B, idx != nullptr, &a);
  if (rc != POB_OK) return rc;
  if (!theta || !saved || !dy || !dtheta || !workspace)
    return pob_fail_msg(POB_EINVAL, "gru sequence: NULL argument (theta, saved, dy, dtheta, workspace)");
  const GruDesc &d = g->d;
  const int I = d.pre[d.n_pre], H = d.hid;
  const long long R = (long long)T * M, n_chunks = (R + POB_MLP_BWD_CHUNK - 1) / POB_MLP_BWD_CHUNK;
  float *delta = (float *)workspace;
  double *partials = (double *)((char *)workspace + ((a.p.n_delta * (long long)sizeof(float) + 7) & ~7LL));
  hipStream_t st = (hipStream_t)stream;
  {
    const int wmax = gru_seq_widest(d, false), rows = gru_seq_backward_rows(d);
    const dim3 grid((unsigned)((M + MLP_ROWS - 1) / MLP_ROWS));
    if (rows <= 224)
      hipLaunchKernelGGL((k_gru_seq_backward<224>), grid, dim3(64), 0, st, d, a, wmax, idx, reset, theta, saved, dy, dh_last, delta, dh0);
    else if (rows <= 448)
      hipLaunchKernelGGL((k_gru_seq_backward<448>), grid, dim3(64), 0, st, d, a, wmax, idx, reset, theta, saved, dy, dh_last, delta, dh0);
    else
      hipLaunchKernelGGL((k_gru_seq_backward<1152>), grid, dim3(64), 0, st, d, a, wmax, idx, reset, theta, saved, dy, dh_last, delta, dh0);
  }
  GruBwdBlocks q;
  int n = 0;
  long long woff = 0, so = a.p.pre, dof = a.p.d_pre;
  auto add = [&](int in, int out, int ldd, int bias, int act, long long a_off, long long d_off, long long w) {
    q.in[n] = in; q.out[n] = out; q.ldd[n] = ldd; q.bias[n] = bias; q.act[n] = act;
    q.a_off[n] = a_off; q.d_off[n] = d_off; q.woff[n] = w;
    ++n;
  };
  for (int l = 0; l < d.n_pre; ++l) {
    const int in = d.pre[l], out = d.pre[l + 1];
    add(in, out, out, 1, l != 0, l ? so - R * in : a.p.xin, dof, woff);
    woff += ((long long)in + 1) * out; so += R * out; dof += R * out;
  }
  add(I, 2 * H, 4 * H, 0, 0, a.p.xc, a.p.d_cell, woff);
  add(H, 2 * H, 4 * H, 1, 0, a.p.hin, a.p.d_cell, woff + (long long)I * 2 * H);
  woff += (long long)(I + H + 1) * 2 * H;
  add(I, H, 4 * H, 1, 0, a.p.xc, a.p.d_cell + 2 * H, woff);
  woff += (long long)(I + 1) * H;
  add(H, H, 4 * H, 1, 0, a.p.hin, a.p.d_cell + 3 * H, woff);
  woff += (long long)(H + 1) * H;
  so = a.p.post; dof = a.p.d_post;
  for (int l = 0; l < d.n_post; ++l) {
    const int in = l ? d.post[l - 1] : H, out = d.post[l];
    add(in, out, out, 1, l != 0, l ? so - R * in : a.p.hn, dof, woff);
    woff += ((long long)in + 1) * out; dof += R * out;
    if (l != d.n_post - 1) so += R * out;
  }
  q.n = n;
  unsigned tiles = 0;
  for (int l = 0; l < n; ++l) tiles += (unsigned)(((q.in[l] + q.bias[l] + 31) >> 5) * ((q.out[l] + 31) >> 5));
  while (n < GRU_BWD_MAX_BLOCKS) add(1, 1, 1, 0, 0, 0, 0, 0);  // the unused entries: defined values
  hipLaunchKernelGGL(k_gru_bwd_weights, dim3((unsigned)n_chunks, tiles), dim3(64), 0, st, q, d.act, (int)R, g->n_params, saved,
                     (const float *)delta, partials);
  hipLaunchKernelGGL(k_mlp_bwd_reduce, dim3((unsigned)((g->n_params + 255) / 256)), dim3(256), 0, st,
                     (const double *)partials, n_chunks, g->n_params, dtheta);
  return mlp_hip_check(hipGetLastError(), "k_gru_seq_backward launch");
}

// k_gru_seq_infer's pool heights, each the tallest that keeps its count of blocks on a CU's 160 KiB
// of LDS at 132 B a row (12 / 7 / 5 / 3 / 2 / 1 blocks; DESIGN.md "Recurrent critic" has the table)
#define GRU_SEQ_INFER_N(N, rows, ...)                                                                         \
  if (rows <= 96) hipLaunchKernelGGL((k_gru_seq_infer<96, N>), grid, dim3(64), 0, st, __VA_ARGS__);           \
  else if (rows <= 160) hipLaunchKernelGGL((k_gru_seq_infer<160, N>), grid, dim3(64), 0, st, __VA_ARGS__);    \
  else if (rows <= 248) hipLaunchKernelGGL((k_gru_seq_infer<248, N>), grid, dim3(64), 0, st, __VA_ARGS__);    \
  else if (rows <= 408) hipLaunchKernelGGL((k_gru_seq_infer<408, N>), grid, dim3(64), 0, st, __VA_ARGS__);    \
  else if (rows <= 616) hipLaunchKernelGGL((k_gru_seq_infer<616, N>), grid, dim3(64), 0, st, __VA_ARGS__);    \
  else hipLaunchKernelGGL((k_gru_seq_infer<896, N>), grid, dim3(64), 0, st, __VA_ARGS__);

int pob_gru_sequence_forward(const pob_gru *g, int S, long long M, long long B, const float *obs, const int32_t *idx,
                             const float *h0, const float *reset, const float *theta, float *y, float *h_first,
                             float *h_out, int h_out_step, const float *norm, float norm_clip, void *stream) {
  const int rc = gru_seq_check(g, S, M, B, idx != nullptr, nullptr);
  if (rc != POB_OK) return rc;
  if (!obs || !h0 || !theta || !y) return pob_fail_msg(POB_EINVAL, "gru sequence: NULL argument (obs, h0, theta, y)");
  if (h_out_step < 1 || h_out_step > S)
    return pob_fail_msg(POB_EINVAL, "gru sequence: h_out_step must be in 1 .. S");
  GruDesc d = g->d;
  gru_plan(d, false, d.p_rows);
  const int rows = d.pre[d.n_pre] + 2 * d.hid + d.p_rows[0] + d.p_rows[1];
  const dim3 grid((unsigned)((M + MLP_ROWS - 1) / MLP_ROWS));
  hipStream_t st = (hipStream_t)stream;
  if (norm) { GRU_SEQ_INFER_N(true, rows, d, S, (int)M, B, obs, idx, h0, reset, theta, y, h_first, h_out, h_out_step, norm, norm_clip) }
  else { GRU_SEQ_INFER_N(false, rows, d, S, (int)M, B, obs, idx, h0, reset, theta, y, h_first, h_out, h_out_step, norm, norm_clip) }
  return mlp_hip_check(hipGetLastError(), "k_gru_seq_infer launch");
}

}  // extern "C"
