// Host build of the recurrent training forward / backward restatement of po-brax_amd/csrc/pob_mlp.h
// (POB_MLP_HOST): gru_sequence_forward_train_ref and gru_sequence_backward_ref for ctypes, next to
// the single-step gru_forward_ref and mlp_backward_ref they are checked against.  -DGRU_BWD_MAIN
// adds a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
long long gru_bwd_ref_param_count(int n_pre, const int *pre, int H, int n_post, const int *post) {
  return gru_param_count(n_pre, pre, H, n_post, post);
}
// out[12]: gru_seq_layout's fields in their order
void gru_bwd_ref_layout(int n_pre, const int *pre, int H, int n_post, const int *post, long long R, long long *out) {
  const gru_seq_plan p = gru_seq_layout(n_pre, pre, H, n_post, post, R);
  const long long v[12] = {p.xin, p.pre, p.xc, p.hin, p.gate, p.hn, p.post, p.n_saved, p.d_pre, p.d_cell, p.d_post, p.n_delta};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
}
void gru_bwd_ref_step(int n_pre, const int *pre, int H, int n_post, const int *post, int act, int B, const float *x,
                      const float *theta, const float *reset, const float *h_in, float *y, float *h_out, float *h_in_copy) {
  gru_forward_ref(n_pre, pre, H, n_post, post, act, B, x, theta, reset, h_in, y, h_out, h_in_copy);
}
void gru_bwd_ref_forward(int n_pre, const int *pre, int H, int n_post, const int *post, int act, int T, long long M,
                         long long B, const float *obs, const int32_t *idx, const float *h0, const float *reset,
                         const float *norm, float norm_clip, const float *theta, float *y, float *h_last, float *saved) {
  gru_sequence_forward_train_ref(n_pre, pre, H, n_post, post, act, T, M, B, obs, idx, h0, reset, norm, norm_clip, theta, y,
                                 h_last, saved);
}
int gru_bwd_ref_backward(int n_pre, const int *pre, int H, int n_post, const int *post, int act, int T, long long M,
                         long long B, const int32_t *idx, const float *reset, const float *theta, const float *saved,
                         const float *dy, const float *dh_last, float *dtheta, float *dh0, float *delta) {
  return gru_sequence_backward_ref(n_pre, pre, H, n_post, post, act, T, M, B, idx, reset, theta, saved, dy, dh_last, dtheta,
                                   dh0, delta);
}
int gru_bwd_ref_mlp_backward(int n_layers, const int *sizes, int activation, int activate_final, long long M, const float *x,
                             const float *theta, const float *saved, const float *dy, float *dtheta, float *dx) {
  return mlp_backward_ref(n_layers, sizes, activation, activate_final, M, x, theta, saved, dy, dtheta, dx, NULL);
}
float gru_bwd_ref_sum(long long M, const float *a, long long lda, const float *d, long long ldd) {
  return mlp_bwd_sum(M, a, lda, d, ldd, NULL);
}
void gru_bwd_ref_cell_grad(float g, float hin, float r, float z, float ch, float n, float *out4) {
  pob_gru_cell_grad(g, hin, r, z, ch, n, out4[0], out4[1], out4[2], out4[3]);
}
void gru_bwd_ref_obsnorm(float *x, long long B, int D, const float *table, float clip) { obsnorm_apply_ref(x, B, D, table, clip); }
}

#ifdef GRU_BWD_MAIN
static uint32_t st = 13u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  // n_pre, pre sizes (n_pre + 1), H, n_post, post sizes
  struct net { int n_pre, pre[4], H, n_post, post[4]; };
  const net nets[3] = {{0, {7}, 5, 1, {4}}, {1, {9, 6}, 33, 2, {5, 2}}, {3, {4, 3, 5, 2}, 1, 4, {3, 3, 3, 2}}};
  const int Ts[3] = {1, 2, 5};
  const long long Ms[3] = {1, 33, 300};
  for (int ni = 0; ni < 3; ++ni)
    for (int ti = 0; ti < 3; ++ti)
      for (int mi = 0; mi < 3; ++mi)
        for (int act = 0; act < 3; ++act)
          for (int variant = 0; variant < 2; ++variant) {  // everything given; every optional argument NULL
            const net &n = nets[ni];
            const int T = Ts[ti], D = n.pre[0], H = n.H, out = n.post[n.n_post - 1];
            const long long M = Ms[mi], B = variant ? M : M + 3, R = (long long)T * M;
            const long long P = gru_param_count(n.n_pre, n.pre, H, n.n_post, n.post);
            const gru_seq_plan p = gru_seq_layout(n.n_pre, n.pre, H, n.n_post, n.post, R);
            float *obs = (float *)malloc(sizeof(float) * T * B * D), *h0 = (float *)malloc(sizeof(float) * B * H);
            float *rs = (float *)malloc(sizeof(float) * T * B), *th = (float *)malloc(sizeof(float) * P);
            float *nm = (float *)malloc(sizeof(float) * 3 * D), *y = (float *)malloc(sizeof(float) * R * out);
            float *hl = (float *)malloc(sizeof(float) * M * H), *sv = (float *)malloc(sizeof(float) * p.n_saved);
            float *dy = (float *)malloc(sizeof(float) * R * out), *dt = (float *)malloc(sizeof(float) * P);
            float *dh = (float *)malloc(sizeof(float) * M * H), *de = (float *)malloc(sizeof(float) * p.n_delta);
            int32_t *idx = (int32_t *)malloc(sizeof(int32_t) * M);
            for (long long i = 0; i < T * B * D; ++i) obs[i] = 6.0f * uni() - 3.0f;
            for (long long i = 0; i < B * H; ++i) h0[i] = 2.0f * uni() - 1.0f;
            for (long long i = 0; i < T * B; ++i) rs[i] = uni() < 0.2f ? 1.0f : 0.0f;
            for (long long i = 0; i < P; ++i) th[i] = uni() - 0.5f;
            for (int i = 0; i < 3 * D; ++i) nm[i] = 0.5f + uni();
            for (long long i = 0; i < R * out; ++i) dy[i] = (2.0f * uni() - 1.0f) / (float)R;
            for (long long i = 0; i < M * H; ++i) dh[i] = 2.0f * uni() - 1.0f;
            for (long long i = 0; i < M; ++i) idx[i] = (int32_t)(B - 1 - i);
            gru_sequence_forward_train_ref(n.n_pre, n.pre, H, n.n_post, n.post, act, T, M, B, obs, variant ? NULL : idx, h0,
                                           variant ? NULL : rs, variant ? NULL : nm, 5.0f, th, y, variant ? NULL : hl, sv);
            for (long long i = 0; i < R * out; ++i)
              if (!isfinite(y[i])) return 1;
            if (gru_sequence_backward_ref(n.n_pre, n.pre, H, n.n_post, n.post, act, T, M, B, variant ? NULL : idx,
                                          variant ? NULL : rs, th, sv, dy, variant ? NULL : dh, dt, variant ? NULL : hl,
                                          variant ? NULL : de))
              return 2;
            for (long long i = 0; i < P; ++i)
              if (!isfinite(dt[i])) return 3;
            free(obs); free(h0); free(rs); free(th); free(nm); free(y); free(hl); free(sv); free(dy); free(dt); free(dh);
            free(de); free(idx);
            ++cases;
          }
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
