// pob_mlp_tile.h -- the one-wave tile code of the policy networks on the matrix cores (gfx950),
// shared by the network sources (DESIGN.md "Policy networks"): pob_mlp.hip, pob_gru.hip,
// pob_mlp_train.hip, pob_gru_seq.hip; pob_learner.hip takes only the host helpers at the end.
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
//
// The library is built without relocatable device code: a kernel is launched from the source that
// defines it, so the two small kernels more than one source launches are defined with internal
// linkage in the headers of their users: k_mlp_advance_key in pob_policy_head.h, k_mlp_bwd_reduce
// in pob_mlp_back.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

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
// (ROWS rows at PITCH floats a feature, copied by a block of LANES lanes: the one-wave tile's by default)
template <int ROWS = MLP_ROWS, int LANES = 64, int PITCH = MLP_PITCH>
POB_MLP_D void mlp_tile_store(float *dst, const float *img, const int f0, const int width, const int b0, const int valid,
                              const int lane) {
  float *d = dst + (size_t)b0 * width;
  for (int e = lane; e < ROWS * width; e += LANES) {
    const int row = e / width, col = e - row * width;
    if (row < valid) d[e] = img[(f0 + col) * PITCH + row];
  }
}

// features [0, D) of an image <- rows [b0, b0 + ROWS) of a row-major (B, D) array x: coalesced
// loads, MLP_STAGE in flight per lane, tail rows repeating the last valid one.  copy (may be
// NULL) receives the valid rows as loaded.  reset (may be NULL): a row whose reset[b] != 0 is
// staged as +0 in every feature.  NORM: the image takes pob_obsnorm_apply of the value, with the
// column's mean and scale (rows 0 and 1 of the (3, D) table `norm`) loaded along with it; copy
// keeps the raw row.  ROWS, LANES, PITCH: as mlp_tile_store's.
template <bool NORM, int ROWS = MLP_ROWS, int LANES = 64, int PITCH = MLP_PITCH>
POB_MLP_D void mlp_tile_load(float *img, const float *x, const int D, const int b0, const int valid, float *copy,
                             const float *reset, const float *norm, const float clip, const int lane) {
  // element e = row D + col of the tile's ROWS contiguous rows; a lane's elements are LANES apart
  const int dq = LANES / D, dr = LANES - dq * D;
  int row = lane / D, col = lane - row * D;
  for (int e0 = lane; e0 < ROWS * D; e0 += LANES * MLP_STAGE) {
    float v[MLP_STAGE], mu[NORM ? MLP_STAGE : 1], sc[NORM ? MLP_STAGE : 1];
    int at[MLP_STAGE];  // the element's place in the image (-1: past the tile), bit 30: a row to copy out
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u) {
      const bool in_tile = e0 + LANES * u < ROWS * D;
      const int rr = row < valid ? row : valid - 1;  // tail rows repeat the last one
      v[u] = in_tile ? x[(size_t)(b0 + rr) * D + col] : 0.0f;
      if (reset) v[u] = (in_tile && reset[b0 + rr] != 0.0f) ? 0.0f : v[u];
      if (NORM) {
        mu[u] = in_tile ? norm[col] : 0.0f;
        sc[u] = in_tile ? norm[D + col] : 0.0f;
      }
      at[u] = in_tile ? (col * PITCH + row) | (row < valid ? 1 << 30 : 0) : -1;
      row += dq; col += dr;
      if (col >= D) { col -= D; ++row; }
    }
#pragma unroll
    for (int u = 0; u < MLP_STAGE; ++u) {
      if (at[u] >= 0) {
        if (copy && (at[u] >> 30)) copy[(size_t)b0 * D + e0 + LANES * u] = v[u];
        img[at[u] & 0xFFFFF] = NORM ? pob_obsnorm_apply(v[u], mu[u], sc[u], clip) : v[u];
      }
    }
  }
}

// ---- the gathering load (DESIGN.md "Row-indexed training pass"): tile row r is row idx[b0 + r] of
// an (N, D) array read in place.  Rows are not neighbours in memory, so the lanes are dealt by row,
// not by flat element: a GROUP of G consecutive lanes (G = 64 for D > 32, else the power of two that
// covers D, at least LANES / ROWS) owns one row at a time and walks its columns, lane c of the group
// taking columns c, c + G, .. (CH = ceil(D / G) <= 4 of them): every load instruction of a group is
// one contiguous piece of one row, and a lane's column set never changes, so its mean and scale are
// loaded once, not per element.  The block's LANES / G groups take rows g, g + LANES / G, ..
// The tile's ROWS indices are loaded once, lane r of every wave holding idx[b0 + min(r, valid - 1)]
// (tail rows repeat the last valid index); a group reads its row's index from that register by a
// wave shuffle.  MLP_STAGE loads are in flight per lane: MLP_STAGE / CH rows times CH columns.
// idx values are the caller's to keep inside [0, N): with them every element load is inside x.
template <bool NORM, int CH, int ROWS, int LANES, int PITCH>
POB_MLP_D void mlp_tile_gather_ch(float *img, const float *x, const int D, const int g_shift, const int my_row,
                                  const float *norm, const float clip, const int tid) {
  constexpr int RS = MLP_STAGE / CH;  // rows of one stage
  const int G = 1 << g_shift, c = tid & (G - 1), g = tid >> g_shift, ng = LANES >> g_shift;
  float mu[CH], sc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const bool cok = c + G * k < D;
    mu[k] = (NORM && cok) ? norm[c + G * k] : 0.0f;
    sc[k] = (NORM && cok) ? norm[D + c + G * k] : 0.0f;
  }
  for (int base = 0; base < ROWS; base += ng * RS) {  // the same trip count in every lane: the shuffle's sources are live
    const int r0 = base + g;
    float v[RS][CH];
#pragma unroll
    for (int u = 0; u < RS; ++u) {
      const int row = r0 + ng * u;
      const int src = __shfl(my_row, row < ROWS ? row : 0);  // every lane, before any branch
#pragma unroll
      for (int k = 0; k < CH; ++k)
        v[u][k] = (row < ROWS && c + G * k < D) ? x[(size_t)src * D + (c + G * k)] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < RS; ++u) {
      const int row = r0 + ng * u;
#pragma unroll
      for (int k = 0; k < CH; ++k)
        if (row < ROWS && c + G * k < D)
          img[(c + G * k) * PITCH + row] = NORM ? pob_obsnorm_apply(v[u][k], mu[k], sc[k], clip) : v[u][k];
    }
  }
}

// features [0, D) of an image <- rows idx[b0 .. b0 + ROWS) of x (N, D); NORM as mlp_tile_load's
template <bool NORM, int ROWS = MLP_ROWS, int LANES = 64, int PITCH = MLP_PITCH>
POB_MLP_D void mlp_tile_gather(float *img, const float *x, const int D, const int32_t *idx, const int b0, const int valid,
                               const float *norm, const float clip, const int tid) {
  const int r = tid & 63;
  const int my_row = idx[b0 + (r < valid ? r : valid - 1)];
  int g_shift = 6;
  if (D <= 32) {
    g_shift = 0;
    while ((1 << g_shift) < D) ++g_shift;
    const int least = __builtin_ctz(LANES / ROWS);
    g_shift = g_shift < least ? least : g_shift;
  }
  const int ch = (D + (1 << g_shift) - 1) >> g_shift;
  if (ch == 1) mlp_tile_gather_ch<NORM, 1, ROWS, LANES, PITCH>(img, x, D, g_shift, my_row, norm, clip, tid);
  else if (ch == 2) mlp_tile_gather_ch<NORM, 2, ROWS, LANES, PITCH>(img, x, D, g_shift, my_row, norm, clip, tid);
  else if (ch == 3) mlp_tile_gather_ch<NORM, 3, ROWS, LANES, PITCH>(img, x, D, g_shift, my_row, norm, clip, tid);
  else mlp_tile_gather_ch<NORM, 4, ROWS, LANES, PITCH>(img, x, D, g_shift, my_row, norm, clip, tid);
}

// the first image of a training forward: the contiguous load, or the gathering one where idx is given
template <bool NORM, int ROWS = MLP_ROWS, int LANES = 64, int PITCH = MLP_PITCH>
POB_MLP_D void mlp_tile_load_rows(float *img, const float *x, const int D, const int32_t *idx, const int b0,
                                  const int valid, const float *norm, const float clip, const int tid) {
  if (idx) mlp_tile_gather<NORM, ROWS, LANES, PITCH>(img, x, D, idx, b0, valid, norm, clip, tid);
  else mlp_tile_load<NORM, ROWS, LANES, PITCH>(img, x, D, b0, valid, nullptr, nullptr, norm, clip, tid);
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

// ---------------------------------------------------------------------------- host side
struct pob_mlp {
  MlpDesc d;
  long long n_params;
};

// The two images' heights: image l & 1 holds sizes[l]; the actor's terms (A features) go to the
// image the logits are not in.  Image B starts at row `split` of the pool; returns the pool's
// height class (0 .. 3: 64 / 152 / 288 / 512 rows).
static inline int image_rows(const MlpDesc &d, bool head, int &split) {
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

// the one-wave kernels' grid: a block per tile of 32 rows
static inline dim3 mlp_tile_grid(long long B) { return dim3((unsigned)((B + MLP_ROWS - 1) / MLP_ROWS)); }

// The launch of KERNEL<height, N> (N: true, false, or empty for a kernel with no further template
// argument) at the pool height class cls of HEIGHTS, a list of five (a list of four classes
// repeats its last): MLP_HEIGHTS is image_rows' and train_rows', GRU_HEIGHTS gru_plan's.  Needs
// `grid` and `st` in scope.  TILE_DISPATCH takes the normalising instantiation only where a table
// is given (the plain one is the code it was) and appends `norm, norm_clip` to the arguments.
#define MLP_HEIGHTS 64, 152, 288, 512, 512
#define GRU_HEIGHTS 96, 192, 288, 512, 896
#define TILE_TARG_
#define TILE_TARG_true , true
#define TILE_TARG_false , false
#define TILE_DISPATCH_H(KERNEL, N, cls, H0, H1, H2, H3, H4, ...)                                      \
  switch (cls) {                                                                                      \
    case 0: hipLaunchKernelGGL((KERNEL<H0 TILE_TARG_##N>), grid, dim3(64), 0, st, __VA_ARGS__); break; \
    case 1: hipLaunchKernelGGL((KERNEL<H1 TILE_TARG_##N>), grid, dim3(64), 0, st, __VA_ARGS__); break; \
    case 2: hipLaunchKernelGGL((KERNEL<H2 TILE_TARG_##N>), grid, dim3(64), 0, st, __VA_ARGS__); break; \
    case 3: hipLaunchKernelGGL((KERNEL<H3 TILE_TARG_##N>), grid, dim3(64), 0, st, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL((KERNEL<H4 TILE_TARG_##N>), grid, dim3(64), 0, st, __VA_ARGS__); break; \
  }
#define TILE_DISPATCH_T(KERNEL, N, cls, HEIGHTS, ...) TILE_DISPATCH_H(KERNEL, N, cls, HEIGHTS, __VA_ARGS__)
#define TILE_DISPATCH(KERNEL, cls, HEIGHTS, ...)                                             \
  if (norm) { TILE_DISPATCH_T(KERNEL, true, cls, HEIGHTS, __VA_ARGS__, norm, norm_clip) }    \
  else { TILE_DISPATCH_T(KERNEL, false, cls, HEIGHTS, __VA_ARGS__, norm, norm_clip) }

static inline int mlp_hip_check(hipError_t e, const char *what) {
  if (e == hipSuccess) return POB_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
  return pob_fail_msg(POB_EHIP, msg);
}
