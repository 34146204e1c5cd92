// pob_gru_tile.h -- the recurrent network's tile code, shared by the recurrent actor (pob_gru.hip)
// and the recurrent window (pob_gru_seq.hip).
//
// obs -> pre-MLP -> GRU cell -> post-MLP (pob_mlp.h gru_forward_ref is the specification).  The
// pool holds four regions, in this order: C = [x ; h] (I + H features: the cell's input image,
// h staged directly behind x), N (H features: h'), and the ping-pong images P0, P1 of the dense
// layers' other activations (heights p_rows[0], p_rows[1], worked out by gru_plan on the host
// with the walk gru_tile_forward makes: pob_gru.hip, and again in pob_gru_seq.hip's kernels).
#pragma once
#include "pob_mlp_tile.h"

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

struct pob_gru {
  GruDesc d;
  long long n_params;
  int cls_forward, cls_actor;  // pool height classes (GRU_HEIGHTS; an LSTM handle's: LSTM_HEIGHTS)
  int cell;                    // POB_CELL_GRU, or POB_CELL_LSTM (pob_lstm_create: pob_lstm_tile.h)
};
#define POB_CELL_GRU 0
#define POB_CELL_LSTM 1

// The heights of P0 and P1, by the walk of gru_tile_forward; with `head` the actor's terms (A features) go to
// the image the logits are not in.  Returns the pool's height class (0 .. 4:
// 96 / 192 / 288 / 512 / 896 rows; the widest legal network takes 256 + 128 + 256 + 256).
static inline int gru_plan(const GruDesc &d, bool head, int *p_rows) {
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
