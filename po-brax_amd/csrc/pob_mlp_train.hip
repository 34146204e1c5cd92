// pob_mlp_train.hip -- the MLP's training passes: the forward that keeps what the backward needs,
// and the backward pass, each in the one-wave and in the four-wave layout.
//
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
// k_mlp_bwd_reduce (pob_mlp_back.h): one lane per parameter adds the chunk partials in ascending
// order and rounds once.  Vector stores only, no atomics, no scratch, no allocation.
// The row-indexed pass (pob_mlp_*_rows; DESIGN.md "Row-indexed training pass") is the same kernels with
// the first image, and the weight gradient's layer-0 operand, read as norm.apply(x[idx]) in place.
#include "pob_mlp_back.h"
#include "pob_mlp_wide.h"

// ROWS: the first image is row idx[b0 + r] of x (idx NULL: row b0 + r), normalised when NORM (the
// row-indexed pass: DESIGN.md "Row-indexed training pass"); neither: the contiguous rows of x as they are
template <int H, bool ROWS, bool NORM>
__global__ __launch_bounds__(64) void k_mlp_forward_train(const MlpDesc d, const int split, const int B, const float *x,
                                                          const int32_t *idx, const float *theta, float *y, float *saved,
                                                          const float *norm, const float norm_clip) {
  __shared__ float img[H * MLP_PITCH];
  const int lane = threadIdx.x, b0 = blockIdx.x * MLP_ROWS;
  const int valid = B - b0 < MLP_ROWS ? B - b0 : MLP_ROWS;
  float *src = img, *dst = img + split * MLP_PITCH;
  if (ROWS) mlp_tile_load_rows<NORM>(src, x, d.sizes[0], idx, b0, valid, norm, norm_clip, lane);
  else mlp_tile_load<false>(src, x, d.sizes[0], b0, valid, nullptr, nullptr, nullptr, 0.0f, lane);
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

// ROWS: layer 0's left operand is row idx[r] of x (idx NULL: row r) under the normaliser (norm NULL:
// as it is), recomputed from the raw row with the forward's pob_obsnorm_apply: the same bits.  A
// lane's column ai is fixed, so its mean and scale are loaded once.  A tile's 32 row indices sit in ONE
// register, lane i (and i + 32) holding the index of row rt + i: the NEXT tile's are loaded while this
// tile's operands are in flight, and a lane half takes its sixteen by wave shuffles.
template <bool ROWS>
POB_MLP_D void mlp_bwd_weights_block(const MlpDesc &d, const int B, const long long n_params, const float *x,
                                     const int32_t *idx, const float *saved, const float *delta, double *partials,
                                     const float *norm, const float norm_clip) {
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
  const bool gather = ROWS && l == 0;
  float mu = 0.0f, sc = 0.0f;
  int src = 0;  // the row of x behind row rt + j of the tile at hand (a row past the chunk: its last row's)
  if (gather) {
    if (norm && a_ok) { mu = norm[ai]; sc = norm[in + ai]; }
    const int row = r_begin + j < r_end ? r_begin + j : r_end - 1;
    src = idx ? idx[row] : row;
  }
  for (int rt = r_begin; rt < r_end; rt += 32) {
    float a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = rt + mlp_kfeat(u, h);
      const bool rok = row < r_end;
      if (gather) {
        const int s = __shfl(src, mlp_kfeat(u, h));  // every lane, before the branch
        a[u] = (rok && a_ok) ? A[(size_t)s * in + ai] : 0.0f;
      } else {
        a[u] = (rok && a_ok) ? A[(size_t)row * in + ai] : 0.0f;
      }
      b[u] = (rok && b_ok) ? D[(size_t)row * out + bj] : 0.0f;
    }
    if (gather) {
      const int row = rt + 32 + j < r_end ? rt + 32 + j : r_end - 1;  // the next tile's indices, under this tile's loads
      src = idx ? idx[row] : row;
      if (norm) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const float v = pob_obsnorm_apply(a[u], mu, sc, norm_clip);
          a[u] = (rt + mlp_kfeat(u, h) < r_end && a_ok) ? v : 0.0f;
        }
      }
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

__global__ __launch_bounds__(64) void k_mlp_bwd_weights(const MlpDesc d, const int B, const long long n_params,
                                                        const float *x, const float *saved, const float *delta,
                                                        double *partials) {
  mlp_bwd_weights_block<false>(d, B, n_params, x, nullptr, saved, delta, partials, nullptr, 0.0f);
}

// held to the plain kernel's four waves a SIMD
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_mlp_bwd_weights_rows(
    const MlpDesc d, const int B, const long long n_params, const float *x, const int32_t *idx, const float *saved,
    const float *delta, double *partials, const float *norm, const float norm_clip) {
  mlp_bwd_weights_block<true>(d, B, n_params, x, idx, saved, delta, partials, norm, norm_clip);
}

// ============================================================================ wide training pass
// k_mlp_forward_train_wide / k_mlp_bwd_delta_wide: k_mlp_forward_train's and k_mlp_bwd_delta's
// bits in k_mlp_forward_wide's layout (pob_mlp_wide.h; DESIGN.md "Wide training pass"): four waves
// on 64 rows, ONE image [feature][row] at pitch 65 (66 560 B, two blocks a CU), a weight fragment
// feeding both row sub-tiles.  Every pass over the image that touches global memory walks it in
// mlp_tile_store's pattern: element e = row width + col of the block's 64 contiguous rows goes to
// lane e mod 256, so the global side is coalesced and the LDS side (stride 65) conflict-free, and
// an element is read, changed and written by the one lane that owns it: no barrier inside a pass.
#define MLPW_ZSTAGE 8  // pre-activations a lane loads ahead of their activation gradients

// mlpw_barrier(), spelled out: these kernels are compiled without the packed float32 operations, a
// target feature the header's function does not share, so that one stays a call (and every value
// live across it a saved register); the builtins inline
POB_MLP_D void mlpw_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// mlpw_layer with the accumulators written back as they are (z_l, no activation)
POB_MLP_D void mlpw_layer_raw(float *img, const float *W, const float *bias, const int in, const int out, const int lane,
                              const int wave) {
  const int j = lane & 31, h = lane >> 5;
  const int n_tiles = (out + 31) >> 5;
  const bool split = n_tiles * MLPW_SUB <= MLPW_WAVES;
  const int tile0 = split ? wave / MLPW_SUB : wave, sub0 = split ? wave % MLPW_SUB : 0;
  const int nt = tile0 >= n_tiles ? 0 : (!split && wave + MLPW_WAVES < n_tiles ? 2 : 1);
  const int ns = split ? 1 : MLPW_SUB;
  const int ot = 32 * tile0;
  mlp_f32x16 acc[2][MLPW_SUB];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    mlp_acc_bias(acc[t][0], bias, ot + 32 * MLPW_WAVES * t, out, h);
#pragma unroll
    for (int s = 1; s < MLPW_SUB; ++s) acc[t][s] = acc[t][0];
  }
  const float *src = img + 32 * sub0;
  if (nt == 2) mlpw_chain<2, MLPW_SUB>(acc, src, W, out, ot + j, in, lane);
  else if (nt == 1 && !split) mlpw_chain<1, MLPW_SUB>(acc, src, W, out, ot + j, in, lane);
  else if (nt == 1) mlpw_chain<1, 1>(acc, src, W, out, ot + j, in, lane);
  mlpw_barrier();  // every wave has read every k: the image may be rewritten
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < MLPW_SUB; ++s)
      if (t < nt && s < ns) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = ot + 32 * MLPW_WAVES * t + mlp_acc_row(r, h);
          if (i < out) img[i * MLPW_PITCH + 32 * (sub0 + s) + j] = acc[t][s][r];
        }
      }
  mlpw_barrier();
}

// (row, col) of a lane's next element of the walk above: LANES further on in a row-major (., width)
struct mlpw_walk {
  int row, col, dq, dr;
  POB_MLP_D mlpw_walk(const int width, const int tid)
      : row(tid / width), col(tid - (tid / width) * width), dq(MLPW_LANES / width), dr(MLPW_LANES - (MLPW_LANES / width) * width) {}
  POB_MLP_D void next(const int width) {
    row += dq; col += dr;
    if (col >= width) { col -= width; ++row; }
  }
};

// idx, norm: the row-indexed pass (k_mlp_forward_train<H, true, NORM>'s first image in this layout), chosen
// at run time, uniformly, before the layers: ONE kernel, since the layers' functions are calls here and a
// second kernel calling them costs this one, at 256 VGPRs, four spilled registers
__global__ __launch_bounds__(MLPW_LANES, 2) __attribute__((target("no-packed-fp32-ops"))) void k_mlp_forward_train_wide(
    const MlpDesc d, const int B, const float *x, const int32_t *idx, const float *theta, float *y, float *saved,
    const float *norm, const float norm_clip) {
  __shared__ float img[POB_MLP_MAX_WIDTH * MLPW_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = blockIdx.x * MLPW_ROWS;
  const int valid = B - b0 < MLPW_ROWS ? B - b0 : MLPW_ROWS;
  if (norm) mlp_tile_load_rows<true, MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(img, x, d.sizes[0], idx, b0, valid, norm, norm_clip, tid);
  else if (idx) mlp_tile_gather<false, MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(img, x, d.sizes[0], idx, b0, valid, nullptr, 0.0f, tid);
  else mlp_tile_load<false, MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(img, x, d.sizes[0], b0, valid, nullptr, nullptr, nullptr, 0.0f, tid);
  mlpw_barrier();
  const float *W = theta;
  float *sv = saved;
  for (int l = 0; l < d.n_layers; ++l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    const float *bias = W + (size_t)in * out;
    mlpw_layer_raw(img, W, bias, in, out, lane, wave);  // z_l; ends with a barrier
    if (mlp_activated(d, l)) {
      // one pass: z to saved, mlp_activate(z) back to the element (the lane's own)
      float *s = sv + (size_t)b0 * out;
      mlpw_walk w(out, tid);
      for (int e = tid; e < MLPW_ROWS * out; e += MLPW_LANES) {
        const int at = w.col * MLPW_PITCH + w.row;
        const float z = img[at];
        if (w.row < valid) s[e] = z;
        img[at] = mlp_activate(d.act, z);
        w.next(out);
      }
      sv += (size_t)B * out;
      mlpw_barrier();
    }
    W = bias + out;
  }
  mlp_tile_store<MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(y, img, 0, d.sizes[d.n_layers], b0, valid, tid);
}

// the operands of k-steps [s0, s0 + MLPW_KUNROLL) of G^T = W Delta^T: k runs over the layer's `out`
// features, tile t's row of W (in, out) is row0 + 32 MLPW_WAVES t (lane j walks a column of the
// row-major matrix: the two lane halves read neighbouring floats of 32 rows), sub-tile s starts
// 32 s rows into src.  As mlpw_operands: every load from a clamped address, zeroed afterwards.
template <int NT, int NS>
POB_MLP_D void mlpwb_operands(float (&a)[2][MLPW_KUNROLL], float (&b)[MLPW_SUB][MLPW_KUNROLL], const float *src,
                              const float *W, const int in, const int row0, const int out, const int s0, const int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int u = 0; u < MLPW_KUNROLL; ++u) {
    const int k = mlp_kfeat(s0 + u, h);
    const bool kok = k < out;
    const unsigned kc = kok ? k : out - 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int row = row0 + 32 * MLPW_WAVES * t;
      const bool rok = row < in;
      const float w = W[(unsigned)(rok ? row : in - 1) * (unsigned)out + kc];
      a[t][u] = (kok && rok) ? w : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float v = src[kc * MLPW_PITCH + 32 * s + j];
      b[s][u] = kok ? v : 0.0f;
    }
  }
}

// NT input tiles x NS row sub-tiles of one layer's G^T: acc[t][s] += the chain over the `out` features
template <int NT, int NS>
POB_MLP_D void mlpwb_chain(mlp_f32x16 (&acc)[2][MLPW_SUB], const float *src, const float *W, const int in, const int row0,
                           const int out, const int lane) {
  const int ks = mlp_ksteps(out);
  float a0[2][MLPW_KUNROLL], b0[MLPW_SUB][MLPW_KUNROLL], a1[2][MLPW_KUNROLL], b1[MLPW_SUB][MLPW_KUNROLL];
  mlpwb_operands<NT, NS>(a0, b0, src, W, in, row0, out, 0, lane);
  for (int s0 = 0; s0 < ks; s0 += 2 * MLPW_KUNROLL) {
    mlpwb_operands<NT, NS>(a1, b1, src, W, in, row0, out, s0 + MLPW_KUNROLL, lane);
    mlpw_mfmas<NT, NS>(acc, a0, b0, s0, ks);
    mlpwb_operands<NT, NS>(a0, b0, src, W, in, row0, out, s0 + 2 * MLPW_KUNROLL, lane);
    mlpw_mfmas<NT, NS>(acc, a1, b1, s0 + MLPW_KUNROLL, ks);
  }
}

// the image's first `out` features (delta_l) -> its first `in` features (the gradient to layer
// l - 1's output), in place: the waves split the INPUT tiles as mlpw_layer splits the output ones
POB_MLP_D void mlpwb_layer(float *img, const float *W, const int in, const int out, const int lane, const int wave) {
  const int j = lane & 31, h = lane >> 5;
  const int n_tiles = (in + 31) >> 5;
  const bool split = n_tiles * MLPW_SUB <= MLPW_WAVES;  // a wave per (tile, sub-tile) pair
  const int tile0 = split ? wave / MLPW_SUB : wave, sub0 = split ? wave % MLPW_SUB : 0;
  const int nt = tile0 >= n_tiles ? 0 : (!split && wave + MLPW_WAVES < n_tiles ? 2 : 1);
  const int ns = split ? 1 : MLPW_SUB;
  const int it = 32 * tile0;
  mlp_f32x16 acc[2][MLPW_SUB];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < MLPW_SUB; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][s][r] = 0.0f;
  const float *src = img + 32 * sub0;
  if (nt == 2) mlpwb_chain<2, MLPW_SUB>(acc, src, W, in, it + j, out, lane);
  else if (nt == 1 && !split) mlpwb_chain<1, MLPW_SUB>(acc, src, W, in, it + j, out, lane);
  else if (nt == 1) mlpwb_chain<1, 1>(acc, src, W, in, it + j, out, lane);
  mlpw_barrier();  // every wave has read every k: the image may be rewritten
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < MLPW_SUB; ++s)
      if (t < nt && s < ns) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = it + 32 * MLPW_WAVES * t + mlp_acc_row(r, h);
          if (i < in) img[i * MLPW_PITCH + 32 * (sub0 + s) + j] = acc[t][s][r];
        }
      }
  mlpw_barrier();
}

__global__ __launch_bounds__(MLPW_LANES, 2) __attribute__((target("no-packed-fp32-ops"))) void k_mlp_bwd_delta_wide(
    const MlpDesc d, const int B, const float *theta, const float *saved, const float *dy, float *delta, float *dx) {
  __shared__ float img[POB_MLP_MAX_WIDTH * MLPW_PITCH];  // the incoming gradient, then delta_l, of the layer's out features
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = blockIdx.x * MLPW_ROWS;
  const int valid = B - b0 < MLPW_ROWS ? B - b0 : MLPW_ROWS;
  size_t woff = 0, soff = 0, doff = 0;
  for (int l = 0; l < d.n_layers; ++l) {
    woff += ((size_t)d.sizes[l] + 1) * d.sizes[l + 1];
    doff += (size_t)B * d.sizes[l + 1];
    if (mlp_activated(d, l)) soff += (size_t)B * d.sizes[l + 1];
  }
  mlp_tile_load<false, MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(img, dy, d.sizes[d.n_layers], b0, valid, nullptr, nullptr, nullptr, 0.0f,
                                                         tid);
  mlpw_barrier();
  for (int l = d.n_layers - 1; l >= 0; --l) {
    const int in = d.sizes[l], out = d.sizes[l + 1];
    woff -= ((size_t)in + 1) * out;
    doff -= (size_t)B * out;
    if (mlp_activated(d, l)) {
      // delta = mlp_activate_grad(z, g) in place: z straight from saved (coalesced, MLPW_ZSTAGE in
      // flight a lane, tail rows repeating the last valid one), g from the lane's own element
      soff -= (size_t)B * out;
      const float *z = saved + soff;
      float *dl = delta + doff + (size_t)b0 * out;
      mlpw_walk w(out, tid);
      for (int e0 = tid; e0 < MLPW_ROWS * out; e0 += MLPW_LANES * MLPW_ZSTAGE) {
        float zv[MLPW_ZSTAGE];
        int at[MLPW_ZSTAGE];  // the element's place in the image (-1: past the tile), bit 30: a row to store
#pragma unroll
        for (int u = 0; u < MLPW_ZSTAGE; ++u) {
          const bool in_tile = e0 + MLPW_LANES * u < MLPW_ROWS * out;
          const int rr = w.row < valid ? w.row : valid - 1;
          zv[u] = in_tile ? z[(size_t)(b0 + rr) * out + w.col] : 0.0f;
          at[u] = in_tile ? (w.col * MLPW_PITCH + w.row) | (w.row < valid ? 1 << 30 : 0) : -1;
          w.next(out);
        }
#pragma unroll
        for (int u = 0; u < MLPW_ZSTAGE; ++u) {
          if (at[u] >= 0) {
            const int p = at[u] & 0xFFFFF;
            const float dv = mlp_activate_grad(d.act, zv[u], img[p]);
            img[p] = dv;
            if (at[u] >> 30) dl[e0 + MLPW_LANES * u] = dv;
          }
        }
      }
    } else {
      mlp_tile_store<MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(delta + doff, img, 0, out, b0, valid, tid);
    }
    if (l == 0 && !dx) return;
    mlpw_barrier();  // delta_l is whole before any wave reads its k
    mlpwb_layer(img, theta + woff, in, out, lane, wave);
  }
  mlp_tile_store<MLPW_ROWS, MLPW_LANES, MLPW_PITCH>(dx, img, 0, d.sizes[0], b0, valid, tid);
}

static int mlp_widest(const MlpDesc &d) {
  int w = 1;
  for (int l = 0; l <= d.n_layers; ++l)
    if (d.sizes[l] > w) w = d.sizes[l];
  return w;
}

// the pool of the delta kernel, two images of the widest layer: the height class of MLP_HEIGHTS
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

// the 32 x 32 tiles of the layers' (in + 1, out) blocks: k_mlp_bwd_weights' blockIdx.y
static unsigned mlp_weight_tiles(const MlpDesc &d) {
  unsigned tiles = 0;
  for (int l = 0; l < d.n_layers; ++l) tiles += (unsigned)(((d.sizes[l] + 32) >> 5) * ((d.sizes[l + 1] + 31) >> 5));
  return tiles;
}

// the template arguments after the pool height of k_mlp_forward_train (TILE_DISPATCH_T's N)
#define TILE_TARG_plain , false, false
#define TILE_TARG_rows , true, false
#define TILE_TARG_rows_norm , true, true

// the row-indexed entries' own checks: x is (N, D); without idx the M rows are its first ones
static int mlp_rows_check(long long M, long long N, const int32_t *idx) {
  if (N < 1) return pob_fail_msg(POB_EINVAL, "mlp: the row count N of x must be positive");
  if (!idx && M > N) return pob_fail_msg(POB_EINVAL, "mlp: without idx the M rows are x's first: M must not exceed N");
  return POB_OK;
}

// pob_mlp_forward_train and its four-wave form; idx, norm: the row-indexed pass (both NULL: the plain one)
static int mlp_forward_train(const pob_mlp *m, long long M, const float *x, const int32_t *idx, const float *theta, float *y,
                             float *saved, const float *norm, float norm_clip, bool wide, void *stream) {
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  if (!x || !theta || !y || (n_saved && !saved)) return pob_fail_msg(POB_EINVAL, "mlp: NULL argument (x, theta, y, saved)");
  const int B = (int)M;
  hipStream_t st = (hipStream_t)stream;
  if (wide) {
    hipLaunchKernelGGL(k_mlp_forward_train_wide, mlpw_grid(M), dim3(MLPW_LANES), 0, st, m->d, B, x, idx, theta, y, saved, norm,
                       norm_clip);
    return mlp_hip_check(hipGetLastError(), "k_mlp_forward_train_wide launch");
  }
  int split;
  const int cls = image_rows(m->d, false, split);
  const dim3 grid = mlp_tile_grid(M);
  if (norm) { TILE_DISPATCH_T(k_mlp_forward_train, rows_norm, cls, MLP_HEIGHTS, m->d, split, B, x, idx, theta, y, saved, norm, norm_clip) }
  else if (idx) { TILE_DISPATCH_T(k_mlp_forward_train, rows, cls, MLP_HEIGHTS, m->d, split, B, x, idx, theta, y, saved, norm, norm_clip) }
  else { TILE_DISPATCH_T(k_mlp_forward_train, plain, cls, MLP_HEIGHTS, m->d, split, B, x, idx, theta, y, saved, norm, norm_clip) }
  return mlp_hip_check(hipGetLastError(), "k_mlp_forward_train launch");
}

// pob_mlp_backward and its four-wave form: the delta kernel of the layout asked for, then the
// parameter gradient from the same delta arrays by the same two kernels; idx, norm: layer 0's
// left operand gathered and normalised as the forward's was (then there is no dx)
static int mlp_backward(const pob_mlp *m, long long M, const float *x, const int32_t *idx, const float *theta,
                        const float *saved, const float *dy, float *dtheta, float *dx, const float *norm, float norm_clip,
                        void *workspace, bool wide, void *stream) {
  long long n_saved, n_delta;
  const int rc = mlp_bwd_counts(m, M, &n_saved, &n_delta);
  if (rc != POB_OK) return rc;
  if (!x || !theta || !dy || !dtheta || !workspace || (n_saved && !saved))
    return pob_fail_msg(POB_EINVAL, "mlp: NULL argument (x, theta, saved, dy, dtheta, workspace)");
  if (dx && (idx || norm)) return pob_fail_msg(POB_EINVAL, "mlp: no dx through idx or norm (pass dx = NULL)");
  const int B = (int)M;
  const long long n_chunks = (M + POB_MLP_BWD_CHUNK - 1) / POB_MLP_BWD_CHUNK;
  float *delta = (float *)workspace;
  double *partials = (double *)((char *)workspace + ((n_delta * (long long)sizeof(float) + 7) & ~7LL));
  hipStream_t st = (hipStream_t)stream;
  if (wide) {
    hipLaunchKernelGGL(k_mlp_bwd_delta_wide, mlpw_grid(M), dim3(MLPW_LANES), 0, st, m->d, B, theta, saved, dy, delta, dx);
  } else {
    int split;
    const int cls = train_rows(m->d, split);
    const dim3 grid = mlp_tile_grid(M);
    TILE_DISPATCH_T(k_mlp_bwd_delta, , cls, MLP_HEIGHTS, m->d, split, B, theta, saved, dy, delta, dx)
  }
  const dim3 wgrid((unsigned)n_chunks, mlp_weight_tiles(m->d));
  if (idx || norm)
    hipLaunchKernelGGL(k_mlp_bwd_weights_rows, wgrid, dim3(64), 0, st, m->d, B, m->n_params, x, idx, saved, (const float *)delta,
                       partials, norm, norm_clip);
  else
    hipLaunchKernelGGL(k_mlp_bwd_weights, wgrid, dim3(64), 0, st, m->d, B, m->n_params, x, saved, (const float *)delta, partials);
  hipLaunchKernelGGL(k_mlp_bwd_reduce, dim3((unsigned)((m->n_params + 255) / 256)), dim3(256), 0, st,
                     (const double *)partials, n_chunks, m->n_params, dtheta);
  return mlp_hip_check(hipGetLastError(), wide ? "k_mlp_bwd_wide launch" : "k_mlp_bwd launch");
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
  return mlp_forward_train(m, M, x, nullptr, theta, y, saved, nullptr, 0.0f, false, stream);
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
  return mlp_backward(m, M, x, nullptr, theta, saved, dy, dtheta, dx, nullptr, 0.0f, workspace, false, stream);
}

int pob_mlp_forward_train_wide(const pob_mlp *m, long long M, const float *x, const float *theta, float *y, float *saved,
                               void *stream) {
  return mlp_forward_train(m, M, x, nullptr, theta, y, saved, nullptr, 0.0f, true, stream);
}

int pob_mlp_backward_wide(const pob_mlp *m, long long M, const float *x, const float *theta, const float *saved,
                          const float *dy, float *dtheta, float *dx, void *workspace, void *stream) {
  return mlp_backward(m, M, x, nullptr, theta, saved, dy, dtheta, dx, nullptr, 0.0f, workspace, true, stream);
}

// ---- the row-indexed pass (DESIGN.md "Row-indexed training pass")
int pob_mlp_forward_train_rows(const pob_mlp *m, long long M, long long N, const float *x, const int32_t *idx,
                               const float *theta, float *y, float *saved, const float *norm, float norm_clip, void *stream) {
  const int rc = mlp_rows_check(M, N, idx);
  return rc != POB_OK ? rc : mlp_forward_train(m, M, x, idx, theta, y, saved, norm, norm_clip, false, stream);
}

int pob_mlp_backward_rows(const pob_mlp *m, long long M, long long N, const float *x, const int32_t *idx, const float *theta,
                          const float *saved, const float *dy, float *dtheta, float *dx, const float *norm, float norm_clip,
                          void *workspace, void *stream) {
  const int rc = mlp_rows_check(M, N, idx);
  return rc != POB_OK ? rc : mlp_backward(m, M, x, idx, theta, saved, dy, dtheta, dx, norm, norm_clip, workspace, false, stream);
}

int pob_mlp_forward_train_wide_rows(const pob_mlp *m, long long M, long long N, const float *x, const int32_t *idx,
                                    const float *theta, float *y, float *saved, const float *norm, float norm_clip,
                                    void *stream) {
  const int rc = mlp_rows_check(M, N, idx);
  return rc != POB_OK ? rc : mlp_forward_train(m, M, x, idx, theta, y, saved, norm, norm_clip, true, stream);
}

int pob_mlp_backward_wide_rows(const pob_mlp *m, long long M, long long N, const float *x, const int32_t *idx,
                               const float *theta, const float *saved, const float *dy, float *dtheta, float *dx,
                               const float *norm, float norm_clip, void *workspace, void *stream) {
  const int rc = mlp_rows_check(M, N, idx);
  return rc != POB_OK ? rc : mlp_backward(m, M, x, idx, theta, saved, dy, dtheta, dx, norm, norm_clip, workspace, true, stream);
}

}  // extern "C"
