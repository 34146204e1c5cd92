// Host build of the recurrent-actor restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST):
// gru_param_count / gru_forward_ref / gru_policy_ref for ctypes, the cell's r, z, cx, ch of one
// batch (the layout tests), and pob_sigmoidf.  -DGRU_MAIN adds a stand-alone program (run under
// -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

static int gru_shape_ok(int n_pre, const int *pre, int H, int n_post, const int *post) {
  if (n_pre < 0 || n_pre > POB_GRU_MAX_PRE || n_post < 1 || n_post > POB_GRU_MAX_POST) return 0;
  for (int l = 0; l <= n_pre; ++l)
    if (pre[l] < 1 || pre[l] > POB_MLP_MAX_WIDTH) return 0;
  for (int l = 0; l < n_post; ++l)
    if (post[l] < 1 || post[l] > POB_MLP_MAX_WIDTH) return 0;
  return H >= 1 && H <= POB_GRU_MAX_HIDDEN && pre[n_pre] + H <= POB_MLP_MAX_WIDTH;
}

extern "C" {
long long gru_ref_param_count(int n_pre, const int *pre, int H, int n_post, const int *post) {
  return gru_param_count(n_pre, pre, H, n_post, post);
}
int gru_ref_forward(int n_pre, const int *pre, int H, int n_post, const int *post, int activation, int B, const float *x,
                    const float *theta, const float *reset, const float *h_in, float *y, float *h_out, float *h_in_copy) {
  if (!gru_shape_ok(n_pre, pre, H, n_post, post)) return -1;
  gru_forward_ref(n_pre, pre, H, n_post, post, activation, B, x, theta, reset, h_in, y, h_out, h_in_copy);
  return 0;
}
int gru_ref_policy(int n_pre, const int *pre, int H, int n_post, const int *post, int activation, int B, const float *obs,
                   const float *theta, const float *reset, const float *h_in, const float *u, int deterministic,
                   float *logits, float *h_out, float *h_in_copy, float *action, float *logp, float *raw) {
  if (!gru_shape_ok(n_pre, pre, H, n_post, post) || (post[n_post - 1] & 1)) return -1;
  gru_policy_ref(n_pre, pre, H, n_post, post, activation, B, obs, theta, reset, h_in, u, deterministic, logits, h_out,
                 h_in_copy, action, logp, raw);
  return 0;
}
// the cell alone on B rows: x (B, I), h (B, H), g = the GRU block -> r, z, cx, ch, hn (B, H each)
int gru_ref_cell(int I, int H, int B, const float *x, const float *h, const float *g, float *r, float *z, float *cx,
                 float *ch, float *hn) {
  if (I < 1 || H < 1 || H > POB_GRU_MAX_HIDDEN || I + H > POB_MLP_MAX_WIDTH) return -1;
  float c[POB_MLP_MAX_WIDTH];
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < I; ++k) c[k] = x[(long long)b * I + k];
    for (int k = 0; k < H; ++k) c[I + k] = h[(long long)b * H + k];
    const long long o = (long long)b * H;
    gru_cell_ref(I, H, c, g, r + o, z + o, cx + o, ch + o, hn + o);
  }
  return 0;
}
float gru_ref_sigmoid(float x) { return pob_sigmoidf(x); }
}

#ifdef GRU_MAIN
int main() {
  int cases = 0;
  if (pob_sigmoidf(0.0f) != 0.5f) return 1;
  // the limits: 3 pre layers, I + H = 256 with H = 128, 4 post layers, widths 1 and 256, odd widths
  const int pre[4] = {255, 256, 1, 128}, post[4] = {256, 7, 33, 16};
  const int H = 128, B = 5;
  const long long n = gru_param_count(3, pre, H, 4, post);
  float *theta = (float *)malloc(sizeof(float) * n), *x = (float *)malloc(sizeof(float) * B * 255);
  float *h = (float *)malloc(sizeof(float) * B * H), *hc = (float *)malloc(sizeof(float) * B * H);
  float *y = (float *)malloc(sizeof(float) * B * 16), *reset = (float *)malloc(sizeof(float) * B);
  uint32_t st = 4321u;
  for (long long i = 0; i < n; ++i) { st = st * 1664525u + 1013904223u; theta[i] = ((float)(st >> 8) * 0x1p-24f - 0.5f) * 0.2f; }
  for (int i = 0; i < B * 255; ++i) { st = st * 1664525u + 1013904223u; x[i] = (float)(st >> 8) * 0x1p-24f * 6.0f - 3.0f; }
  for (int i = 0; i < B * H; ++i) { st = st * 1664525u + 1013904223u; h[i] = (float)(st >> 8) * 0x1p-23f - 1.0f; }
  for (int i = 0; i < B; ++i) reset[i] = i == 1 ? 1.0f : (i == 2 ? NAN : (i == 3 ? -0.0f : 0.0f));
  for (int act = 0; act < 3; ++act) {
    for (int step = 0; step < 3; ++step) {  // in place: h_out = h_in
      gru_forward_ref(3, pre, H, 4, post, act, B, x, theta, step == 1 ? reset : NULL, h, y, h, hc);
      for (int i = 0; i < B * 16; ++i) if (!isfinite(y[i])) return 2;
      for (int i = 0; i < B * H; ++i) if (!(fabsf(h[i]) <= 1.0f)) return 3;
      if (step == 1)
        for (int k = 0; k < H; ++k) {
          if (mlp_f2u(hc[1 * H + k]) != 0u || mlp_f2u(hc[2 * H + k]) != 0u) return 4;  // reset rows start from +0
        }
      ++cases;
    }
  }
  // a small odd net (the pad of every chain), no pre-MLP, the actor
  const int pre1[1] = {5}, post1[1] = {6};
  const long long n1 = gru_param_count(0, pre1, 3, 1, post1);
  if (n1 != 3 * 3 * 5 + 3 * 3 * 3 + 4 * 3 + 4 * 6 || n1 > n) return 5;
  float logits[B * 6], action[B * 3], logp[B], raw[B * 3], u[B * 3], h3[B * 3] = {0};
  for (int i = 0; i < B * 3; ++i) u[i] = i == 0 ? -1.0f : -1.0f + 0.1f * (float)i;
  gru_policy_ref(0, pre1, 3, 1, post1, 1, B, x, theta, reset, h3, u, 0, logits, h3, NULL, action, logp, raw);
  for (int i = 0; i < B; ++i) if (!isfinite(logp[i])) return 6;
  gru_policy_ref(0, pre1, 3, 1, post1, 1, B, x, theta, NULL, h3, u, 1, logits, h3, NULL, action, logp, raw);
  for (int i = 0; i < B * 3; ++i) if (!(fabsf(action[i]) <= 1.0f)) return 7;
  cases += 2;
  free(theta); free(x); free(h); free(hc); free(y); free(reset);
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
