// pob_gru_bf16.h -- the bf16 matrix-core recurrent window (pob_gru_seq_bf16.hip; DESIGN.md "Bf16
// recurrent window"): the layouts, the weight fragments and the layers of a four-wave block.
//
// The function is gru_sequence_forward_ref's network and step loop (pob_mlp.h) with the rounding
// rule of the bf16 MLP forward (pob_mlp_bf16.h): every operand of a matrix product is rounded to
// bf16 (nearest even) where it enters the product -- the normalised observation row, every weight
// matrix, the dense layers' hidden activations, h where it enters the r, z and candidate products
// -- and everything else is f32: accumulators from the f32 bias, the activations, pob_sigmoidf /
// pob_tanhf, n = tanh(cx + r ch) and the blend h' = n + z (h - n) on the UNROUNDED f32 h, which is
// also what is carried from step to step and stored.  The sums are in the order of
// v_mfma_f32_32x32x16_bf16: deterministic, not an fmaf chain.
//
// A block of GRUB_WAVES = 4 waves owns GRUB_ROWS = 64 sequences (two sub-tiles of 32) for the whole
// window.  It computes transposed products Y^T = W^T X^T: a weight fragment is the instruction's A
// operand, eight consecutive features of one row of a bf16 [row][feature] LDS image its B operand
// (one 16-byte read), and in the accumulator a lane holds ONE row (lane & 31) and the features
// 8 q + 4 (lane >> 5) + 0 .. 3 of a 32-feature tile.
//
// LDS: the env numbers of the 64 rows; Hb, the bf16 image of h (roundup(H, 32) features); P0 and P1,
// the dense layers' ping-pong images (the observation is staged into P0; the cell reads its x from
// whichever image the pre-MLP ended in).  A row of an image of width w is roundup(w, 32) + 8 bf16
// = 16 k + 4 dwords: 16 consecutive rows start in 16 distinct 4-bank groups, so the 16-byte operand
// reads are conflict-free.  The f32 h never touches LDS: (row, feature) of the cell's output is
// held by the same lane at every step, so h lives in that lane's registers (16 a (tile, sub-tile)
// unit) next to the accumulators it is blended with.
//
// Weights (k_gru_pack_bf16, every call): the dense layers in pob_mlp_bf16.h's fragment order
// [out tile of 32][k chunk of 16][lane][8 bf16]; the cell fused as
// [H tile of 32][k chunk][3][lane][8 bf16] over the chunks of x (I padded to 16) followed by the
// chunks of h (H padded to 16): fragment 0 is W_rz's r column, 1 its z column, 2 the candidate's
// (W_xn in an x chunk, W_hn in an h chunk), so one B fragment of [x ; h] feeds the r and z
// accumulators and cx or ch.  Zero padded: no clamped address and no tail test on a weight.
#pragma once
#include "pob_gru_tile.h"

#define GRUB_WAVES 4
#define GRUB_ROWS 64
#define GRUB_LANES (64 * GRUB_WAVES)
#define GRUB_KC 16     // k of one v_mfma_f32_32x32x16_bf16
#define GRUB_GROUP 2   // the cell: k chunks (3 weight fragments + 1 row fragment each) loaded ahead of their MFMAs
#define GRUB_DGROUP 4  // a dense layer: k chunks (1 + 1 fragments) loaded ahead
#define GRUB_STAGE 8   // observation elements a lane loads ahead of their LDS stores
#define GRUB_ENV_BYTES (GRUB_ROWS * 4)

typedef __bf16 grub_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 grub_bf16x4 __attribute__((ext_vector_type(4)));

static inline __host__ __device__ int grub_chunks(const int in) { return (in + GRUB_KC - 1) / GRUB_KC; }
static inline __host__ __device__ int grub_tiles(const int out) { return (out + 31) >> 5; }
static inline __host__ __device__ int grub_pitch(const int w) { return w ? 32 * grub_tiles(w) + 8 : 0; }
// 16-byte fragments of a dense layer and of the fused cell
static inline __host__ __device__ int grub_dense_frags(const int in, const int out) { return 64 * grub_chunks(in) * grub_tiles(out); }
static inline __host__ __device__ int grub_cell_frags(const int I, const int H) {
  return 64 * 3 * (grub_chunks(I) + grub_chunks(H)) * grub_tiles(H);
}

// what the window kernel needs beyond GruDesc: small, by value
struct GrubArgs {
  int S, M, h_out_step;
  int pit0, pit1;  // bf16 elements between two rows of P0, P1
  long long B;
  float clip;
};

// The pitches of P0 and P1 by the walk of k_gru_seq_infer_bf16 (the observation in P0, every dense
// layer but the last writing the image it does not read; the post-MLP's first layer reads Hb),
// the workspace's fragments, and the pool's bytes.
static inline long long grub_plan(const GruDesc &d, int *pit, int *pool_bytes) {
  int w[2] = {d.pre[0], 0}, cur = 0;
  long long frags = 0;
  for (int l = 0; l < d.n_pre; ++l) {
    cur ^= 1;
    if (d.pre[l + 1] > w[cur]) w[cur] = d.pre[l + 1];
    frags += grub_dense_frags(d.pre[l], d.pre[l + 1]);
  }
  frags += grub_cell_frags(d.pre[d.n_pre], d.hid);
  for (int l = 0; l < d.n_post; ++l) {
    cur ^= 1;
    if (l != d.n_post - 1 && d.post[l] > w[cur]) w[cur] = d.post[l];
    frags += grub_dense_frags(l ? d.post[l - 1] : d.hid, d.post[l]);
  }
  if (pit) { pit[0] = grub_pitch(w[0]); pit[1] = grub_pitch(w[1]); }
  if (pool_bytes) *pool_bytes = GRUB_ENV_BYTES + GRUB_ROWS * 2 * (grub_pitch(d.hid) + grub_pitch(w[0]) + grub_pitch(w[1]));
  return frags;
}

#ifdef __HIPCC__
// lane's fragment f of a dense (in, out) matrix W: W[16 c + 8 (l >> 5) + e][32 t + (l & 31)], zero past the layer
POB_MLP_D grub_bf16x8 grub_pack_dense(const float *W, const int in, const int out, const int f) {
  const int kc = grub_chunks(in);
  const int lane = f & 63, c = (f >> 6) % kc, t = (f >> 6) / kc;
  const int col = 32 * t + (lane & 31), k0 = GRUB_KC * c + 8 * (lane >> 5);
  grub_bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (__bf16)((col < out && k0 + e < in) ? W[(size_t)(k0 + e) * out + col] : 0.0f);
  return v;
}

// lane's fragment f of the fused cell; g: the GRU block of theta
POB_MLP_D grub_bf16x8 grub_pack_cell(const float *g, const int I, const int H, const int f) {
  const int kcx = grub_chunks(I), kc = kcx + grub_chunks(H);
  const int lane = f & 63, q = f >> 6, gate = q % 3, c = (q / 3) % kc, t = q / (3 * kc);
  const bool xpart = c < kcx;
  const int col = 32 * t + (lane & 31), k0 = GRUB_KC * (xpart ? c : c - kcx) + 8 * (lane >> 5), kin = xpart ? I : H;
  const float *W_rz = g, *W_xn = W_rz + (size_t)(I + H) * 2 * H + 2 * H, *W_hn = W_xn + (size_t)I * H + H;
  grub_bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float w = 0.0f;
    if (col < H && k < kin) {
      if (gate < 2) w = W_rz[(size_t)((xpart ? 0 : I) + k) * 2 * H + gate * H + col];
      else w = xpart ? W_xn[(size_t)k * H + col] : W_hn[(size_t)k * H + col];
    }
    v[e] = (__bf16)w;
  }
  return v;
}

// ---- a dense layer: one accumulator a (tile, sub-tile) unit, the block's waves taking units in turn
POB_MLP_D void grub_operands(grub_bf16x8 (&a)[GRUB_DGROUP], grub_bf16x8 (&b)[GRUB_DGROUP], const __bf16 *src,
                             const grub_bf16x8 *wl, const int kc, const int c0) {
#pragma unroll
  for (int u = 0; u < GRUB_DGROUP; ++u) {
    const int c = c0 + u < kc ? c0 + u : kc - 1;  // a chunk past the layer repeats the last one; its MFMA is not issued
    a[u] = wl[c * 64];
    b[u] = *(const grub_bf16x8 *)(src + GRUB_KC * c);
  }
}
POB_MLP_D void grub_mfmas(mlp_f32x16 &acc, const grub_bf16x8 (&a)[GRUB_DGROUP], const grub_bf16x8 (&b)[GRUB_DGROUP],
                          const int c0, const int kc) {
#pragma unroll
  for (int u = 0; u < GRUB_DGROUP; ++u)
    if (c0 + u < kc) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u], acc, 0, 0, 0);
}
// acc += W^T X^T over the kc chunks; src: lane's row and k half in the image, wl: lane's fragment of chunk 0
POB_MLP_D void grub_chain(mlp_f32x16 &acc, const __bf16 *src, const grub_bf16x8 *wl, const int kc) {
  grub_bf16x8 a0[GRUB_DGROUP], b0[GRUB_DGROUP], a1[GRUB_DGROUP], b1[GRUB_DGROUP];
  grub_operands(a0, b0, src, wl, kc, 0);
  for (int c0 = 0; c0 < kc; c0 += 2 * GRUB_DGROUP) {
    grub_operands(a1, b1, src, wl, kc, c0 + GRUB_DGROUP);
    __builtin_amdgcn_sched_barrier(0);
    grub_mfmas(acc, a0, b0, c0, kc);
    __builtin_amdgcn_sched_barrier(0);
    grub_operands(a0, b0, src, wl, kc, c0 + 2 * GRUB_DGROUP);
    __builtin_amdgcn_sched_barrier(0);
    grub_mfmas(acc, a1, b1, c0 + GRUB_DGROUP, kc);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// src image (pitch ps, `in` features, zero to the next multiple of 16) -> dst image (pitch pd: the
// out features and zeros to the next multiple of 32), or, LAST, -> rows [0, valid) of y (., out) in f32
template <bool LAST>
POB_MLP_D void grub_layer(const __bf16 *src, const int ps, __bf16 *dst, const int pd, const grub_bf16x8 *wp,
                          const float *bias, const int in, const int out, const bool activate, const int act, float *y,
                          const int valid, const int lane, const int wave) {
  const int j = lane & 31, h = lane >> 5, kc = grub_chunks(in), nu = 2 * grub_tiles(out);
  for (int u = wave; u < nu; u += GRUB_WAVES) {
    const int tile = u >> 1, row = 32 * (u & 1) + j, f0 = 32 * tile + 4 * h;
    mlp_f32x16 acc;
    mlp_acc_bias(acc, bias, 32 * tile, out, h);
    grub_chain(acc, src + row * ps + 8 * h, wp + tile * kc * 64 + lane, kc);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = activate ? mlp_activate(act, acc[4 * q + e]) : acc[4 * q + e];
      if (LAST) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (row < valid && f0 + 8 * q + e < out) y[(size_t)row * out + f0 + 8 * q + e] = v[e];
      } else {
        grub_bf16x4 p;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = (__bf16)v[e];  // a padded column: zero weights, zero bias, act(0) = 0
        *(grub_bf16x4 *)(dst + row * pd + f0 + 8 * q) = p;
      }
    }
  }
}

// ---- the cell's products for one (H tile, sub-tile) unit: r, z over every chunk, cx over x's, ch over h's
struct grub_cell_ops {
  grub_bf16x8 a[GRUB_GROUP][3], b[GRUB_GROUP];
};
POB_MLP_D void grub_cell_operands(grub_cell_ops &o, const __bf16 *xs, const __bf16 *hs, const grub_bf16x8 *wl, const int kcx,
                                  const int kc, const int c0) {
#pragma unroll
  for (int u = 0; u < GRUB_GROUP; ++u) {
    const int c = c0 + u < kc ? c0 + u : kc - 1;
#pragma unroll
    for (int g = 0; g < 3; ++g) o.a[u][g] = wl[(3 * c + g) * 64];
    o.b[u] = *(const grub_bf16x8 *)(c < kcx ? xs + GRUB_KC * c : hs + GRUB_KC * (c - kcx));
  }
}
POB_MLP_D void grub_cell_mfmas(mlp_f32x16 &ar, mlp_f32x16 &az, mlp_f32x16 &ax, mlp_f32x16 &ah, const grub_cell_ops &o,
                               const int kcx, const int kc, const int c0) {
#pragma unroll
  for (int u = 0; u < GRUB_GROUP; ++u)
    if (c0 + u < kc) {  // uniform
      ar = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.a[u][0], o.b[u], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.a[u][1], o.b[u], az, 0, 0, 0);
      if (c0 + u < kcx) ax = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.a[u][2], o.b[u], ax, 0, 0, 0);
      else ah = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.a[u][2], o.b[u], ah, 0, 0, 0);
    }
}
// xs, hs: lane's row and k half in the x image and in Hb; wl: lane's first fragment of the unit's H tile
POB_MLP_D void grub_cell_chain(mlp_f32x16 &ar, mlp_f32x16 &az, mlp_f32x16 &ax, mlp_f32x16 &ah, const __bf16 *xs,
                               const __bf16 *hs, const grub_bf16x8 *wl, const int kcx, const int kc) {
  grub_cell_ops o0, o1;
  grub_cell_operands(o0, xs, hs, wl, kcx, kc, 0);
  for (int c0 = 0; c0 < kc; c0 += 2 * GRUB_GROUP) {
    grub_cell_operands(o1, xs, hs, wl, kcx, kc, c0 + GRUB_GROUP);
    __builtin_amdgcn_sched_barrier(0);
    grub_cell_mfmas(ar, az, ax, ah, o0, kcx, kc, c0);
    __builtin_amdgcn_sched_barrier(0);
    grub_cell_operands(o0, xs, hs, wl, kcx, kc, c0 + 2 * GRUB_GROUP);
    __builtin_amdgcn_sched_barrier(0);
    grub_cell_mfmas(ar, az, ax, ah, o1, kcx, kc, c0 + GRUB_GROUP);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// lane's 16 features of tile `tile`, row `row`, rounded into Hb (pitch ph)
POB_MLP_D void grub_store_h(__bf16 *Hb, const int ph, const int row, const int tile, const int h, const float (&v)[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    grub_bf16x4 p;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = (__bf16)v[4 * q + e];
    *(grub_bf16x4 *)(Hb + row * ph + 32 * tile + 4 * h + 8 * q) = p;
  }
}

// The observation image: row r of the block <- row envs[r] of x (B, D), f32, loaded coalesced
// (GRUB_STAGE in flight a lane), normalised if NORM (pob_obsnorm_apply in f32), rounded to bf16;
// features D .. roundup(D, 16) are 0.  envs already repeats the last valid row in the tail rows.
template <bool NORM>
POB_MLP_D void grub_stage(__bf16 *img, const int pitch, const float *x, const int D, const int *envs, const float *norm,
                          const float clip, const int tid) {
  const int n = GRUB_ROWS * D;
  for (int e0 = tid; e0 < n; e0 += GRUB_LANES * GRUB_STAGE) {
    float v[GRUB_STAGE], mu[NORM ? GRUB_STAGE : 1], sc[NORM ? GRUB_STAGE : 1];
    int at[GRUB_STAGE];
#pragma unroll
    for (int u = 0; u < GRUB_STAGE; ++u) {
      const int e = e0 + GRUB_LANES * u;
      const bool ok = e < n;
      const int row = ok ? e / D : 0, col = ok ? e - row * D : 0;
      v[u] = x[(size_t)envs[row] * D + col];
      if (NORM) { mu[u] = norm[col]; sc[u] = norm[D + col]; }
      at[u] = ok ? row * pitch + col : -1;
    }
#pragma unroll
    for (int u = 0; u < GRUB_STAGE; ++u)
      if (at[u] >= 0) img[at[u]] = (__bf16)(NORM ? pob_obsnorm_apply(v[u], mu[u], sc[u], clip) : v[u]);
  }
  const int pad = grub_chunks(D) * GRUB_KC - D;
  for (int e = tid; e < GRUB_ROWS * pad; e += GRUB_LANES) {
    const int row = e / pad;
    img[row * pitch + D + (e - row * pad)] = (__bf16)0.0f;
  }
}
#endif
