// pob_gru_seq.hip -- the recurrent window: a whole window of T steps in one launch, for training
// (forward and backward) and for inference (the recurrent critic's pass).
//
// gru_sequence_forward_train_ref / gru_sequence_backward_ref of pob_mlp.h (the specification;
// DESIGN.md "Recurrent backward").  k_gru_seq_forward: one wave per tile of 32 sequences loops
// over the window's T steps inside the launch, h staying in LDS between steps: each step is
// gru_tile_forward's walk (pob_gru.hip; the same chains, so the same bits) with the observation
// rows gathered through idx, and every array the backward needs stored to `saved` through the LDS
// images (coalesced).  k_gru_seq_backward: the same tile with t descending, the carry in LDS: per step
// the post-MLP's delta walk (k_mlp_bwd_delta's), the cell's element-wise part in the rows' own
// order (coalesced loads of the gates, coalesced stores of the four deltas), the carry product
// and, under a pre-MLP, g_x on the MFMA with accumulators from +0, then the pre-MLP's delta walk.
// k_gru_bwd_weights: k_mlp_bwd_weights over a table of blocks (the dense layers, and W_rz in two
// row ranges, W_xn, W_hn reading xc / hin raw from saved); k_mlp_bwd_reduce finishes.  Vector
// stores only, no atomics, no scratch, no allocation, no host synchronisation.
#include "pob_gru_tile.h"
#include "pob_mlp_back.h"

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
  if (g->cell != POB_CELL_GRU)
    return pob_fail_msg(POB_EINVAL, "gru sequence: the handle's cell is an lstm; the sequence kernels serve the gru cell only");
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
  const dim3 grid = mlp_tile_grid(M);
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
    const dim3 grid = mlp_tile_grid(M);
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
  const dim3 grid = mlp_tile_grid(M);
  hipStream_t st = (hipStream_t)stream;
  if (norm) { GRU_SEQ_INFER_N(true, rows, d, S, (int)M, B, obs, idx, h0, reset, theta, y, h_first, h_out, h_out_step, norm, norm_clip) }
  else { GRU_SEQ_INFER_N(false, rows, d, S, (int)M, B, obs, idx, h0, reset, theta, y, h_first, h_out, h_out_step, norm, norm_clip) }
  return mlp_hip_check(hipGetLastError(), "k_gru_seq_infer launch");
}

}  // extern "C"
