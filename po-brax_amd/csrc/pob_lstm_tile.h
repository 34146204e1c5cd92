// pob_lstm_tile.h -- the LSTM cell of the recurrent network on one tile (DESIGN.md "LSTM cell";
// pob_mlp.h lstm_cell_ref / lstm_forward_ref are the specification), its pool plan, and the
// launchers pob_lstm.hip defines for the pob_gru_* entry points of pob_gru.hip.
//
// The pool holds five regions, in this order: C = [x ; h] (I + H features, h directly behind x:
// the concatenation is one operand), S (H features: c, so the state row [h ; c] is staged as ONE
// image of 2 H features behind x), N (H features: h'), and the ping-pong images P0, P1 of
// pob_gru_tile.h (the same walk, so gru_plan's heights).
//
// The cell loop: per 32-feature output tile the wave keeps FOUR accumulators (i, f, g, o), each
// started from its bias, and advances them in one k-loop over C: per k-step one B fragment from
// LDS shared by four MFMAs, and four A fragments from columns j, H + j, 2 H + j, 3 H + j of W (row
// stride 4 H).  The operands of chunk n + 1 (LSTM_KCHUNK k-steps) are loaded while chunk n's
// MFMAs run, every load from a clamped address and zeroed afterwards, so no load waits on a
// branch.  The four chains are independent: each one's order is mlp_chain_ref's.
#pragma once
#include "pob_gru_tile.h"

#define LSTM_KCHUNK 8  // k-steps of one operand chunk; two chunks are live (the one in the MFMAs, the one in flight)
#define LSTM_HEIGHTS 128, 256, 384, 608, 1024

struct LstmFrag {
  float a[4][LSTM_KCHUNK], b[LSTM_KCHUNK];
};

// the operands of k-steps [s0, s0 + LSTM_KCHUNK): W's row k at the four gates' columns, C's feature k
POB_MLP_D void lstm_operands(LstmFrag &f, const float *C, const float *W, const int H, const unsigned colc, const bool cok,
                             const int in, const int s0, const int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int u = 0; u < LSTM_KCHUNK; ++u) {
    const int k = mlp_kfeat(s0 + u, h);
    const bool kok = k < in;
    const unsigned kc = kok ? k : in - 1;
    const float *row = W + (size_t)kc * (4 * H) + colc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float w = row[q * H];
      f.a[q][u] = (kok && cok) ? w : 0.0f;
    }
    const float v = C[kc * MLP_PITCH + j];
    f.b[u] = kok ? v : 0.0f;
  }
}

POB_MLP_D void lstm_mfmas(mlp_f32x16 (&acc)[4], const LstmFrag &f, const int s0, const int ks) {
#pragma unroll
  for (int u = 0; u < LSTM_KCHUNK; ++u)
    if (s0 + u < ks) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[q][u], f.b[u], acc[q], 0, 0, 0);
    }
}

// The cell on one tile: C (I + H features), S (H features: c, overwritten with c') -> N (H
// features: h').  g: the LSTM block of theta.  The gate pre-activations stay in registers.
POB_MLP_D void lstm_cell(const float *C, float *S, float *N, const float *g, const int I, const int H, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int in = I + H, ks = mlp_ksteps(in);
  const float *W = g, *b = W + (size_t)in * 4 * H;
  for (int ot = 0; ot < H; ot += 32) {
    const int col = ot + j;
    const bool cok = col < H;
    const unsigned colc = cok ? col : H - 1;
    mlp_f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) mlp_acc_bias(acc[q], b + q * H, ot, H, h);
    LstmFrag f0, f1;
    lstm_operands(f0, C, W, H, colc, cok, in, 0, lane);
    for (int s0 = 0; s0 < ks; s0 += 2 * LSTM_KCHUNK) {
      lstm_operands(f1, C, W, H, colc, cok, in, s0 + LSTM_KCHUNK, lane);
      lstm_mfmas(acc, f0, s0, ks);
      lstm_operands(f0, C, W, H, colc, cok, in, s0 + 2 * LSTM_KCHUNK, lane);
      lstm_mfmas(acc, f1, s0 + LSTM_KCHUNK, ks);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ot + mlp_acc_row(r, h);
      if (i < H) {
        const float ig = pob_sigmoidf(acc[0][r]), fg = pob_sigmoidf(acc[1][r]);
        const float gg = pob_tanhf(acc[2][r]), og = pob_sigmoidf(acc[3][r]);
        const float cn = MLP_FMA(fg, S[i * MLP_PITCH + j], ig * gg);
        S[i * MLP_PITCH + j] = cn;
        N[i * MLP_PITCH + j] = og * pob_tanhf(cn);
      }
    }
  }
}

// gru_plan for an LSTM handle: P0's and P1's heights are the GRU's (the same walk); the pool holds
// I + 3 H rows before them.  Returns the height class of LSTM_HEIGHTS (the widest legal network
// takes 256 + 128 + 128 + 256 + 256 rows).
static inline int lstm_plan(const GruDesc &d, bool head, int *p_rows) {
  int w[2];
  gru_plan(d, head, w);
  if (p_rows) { p_rows[0] = w[0]; p_rows[1] = w[1]; }
  const int rows = d.pre[d.n_pre] + 3 * d.hid + w[0] + w[1];
  return rows <= 128 ? 0 : (rows <= 256 ? 1 : (rows <= 384 ? 2 : (rows <= 608 ? 3 : 4)));
}

// pob_lstm.hip: the launches behind pob_gru_forward_norm / pob_gru_policy_act_norm for a handle whose
// cell is POB_CELL_LSTM (arguments already checked there; h_io and h_in_copy are (B, 2 H))
int lstm_forward_launch(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                        float *y, float *h_in_copy, const float *norm, float norm_clip, hipStream_t st);
int lstm_policy_act_launch(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                           uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action,
                           float *logp, float *raw, float *logits, float *obs_copy, float *h_in_copy, const float *norm,
                           float norm_clip, hipStream_t st);
