// Host build of the inference window's restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST):
// gru_sequence_forward_ref for ctypes (the chained single step and the training forward it is checked
// against come from gru_bwd_host.cpp).  -DGRU_SEQ_INFER_MAIN adds a stand-alone program (run under
// -fsanitize=address,undefined): every output sits in a block of exactly its size, so a write past
// row M is an error there.
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
int gru_seq_infer_ref(int n_pre, const int *pre, int H, int n_post, const int *post, int act, int S, long long M, long long B,
                      const float *obs, const int32_t *idx, const float *h0, const float *reset, const float *norm,
                      float norm_clip, const float *theta, float *y, float *h_first, float *h_out, int h_out_step) {
  return gru_sequence_forward_ref(n_pre, pre, H, n_post, post, act, S, M, B, obs, idx, h0, reset, norm, norm_clip, theta, y,
                                  h_first, h_out, h_out_step);
}
}

#ifdef GRU_SEQ_INFER_MAIN
static uint32_t st = 17u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  struct net { int n_pre, pre[4], H, n_post, post[4]; };
  const net nets[3] = {{0, {7}, 5, 1, {1}}, {0, {30}, 64, 1, {1}}, {1, {114, 32}, 33, 2, {16, 1}}};
  const int Ss[3] = {1, 3, 9};
  const long long Ms[3] = {1, 31, 33};
  for (int ni = 0; ni < 3; ++ni)
    for (int si = 0; si < 3; ++si)
      for (int mi = 0; mi < 3; ++mi)
        for (int variant = 0; variant < 3; ++variant) {  // everything given; every optional argument NULL; h_out = h0
          const net &n = nets[ni];
          const int S = Ss[si], D = n.pre[0], H = n.H, act = (ni + si + mi) % 3;
          const long long M = Ms[mi], B = variant ? M : M + 3, R = (long long)S * M;
          const long long P = gru_param_count(n.n_pre, n.pre, H, n.n_post, n.post);
          float *obs = (float *)malloc(sizeof(float) * S * B * D), *h0 = (float *)malloc(sizeof(float) * B * H);
          float *rs = (float *)malloc(sizeof(float) * S * B), *th = (float *)malloc(sizeof(float) * P);
          float *nm = (float *)malloc(sizeof(float) * 3 * D), *y = (float *)malloc(sizeof(float) * R);
          float *y2 = (float *)malloc(sizeof(float) * R), *hf = (float *)malloc(sizeof(float) * M * H);
          float *ho = (float *)malloc(sizeof(float) * M * H), *hl = (float *)malloc(sizeof(float) * M * H);
          float *sv = (float *)malloc(sizeof(float) * gru_seq_layout(n.n_pre, n.pre, H, n.n_post, n.post, R).n_saved);
          int32_t *idx = (int32_t *)malloc(sizeof(int32_t) * M);
          for (long long i = 0; i < S * B * D; ++i) obs[i] = 6.0f * uni() - 3.0f;
          for (long long i = 0; i < B * H; ++i) h0[i] = 2.0f * uni() - 1.0f;
          for (long long i = 0; i < S * B; ++i) rs[i] = uni() < 0.2f ? 1.0f : 0.0f;
          for (long long i = 0; i < P; ++i) th[i] = uni() - 0.5f;
          for (int i = 0; i < 3 * D; ++i) nm[i] = 0.5f + uni();
          for (long long i = 0; i < M; ++i) idx[i] = (int32_t)(B - 1 - i);
          const int32_t *ix = variant ? NULL : idx;
          const float *r = variant == 1 ? NULL : rs, *tab = variant == 1 ? NULL : nm;
          // the training forward first: it reads h0 before the aliased run overwrites it
          gru_sequence_forward_train_ref(n.n_pre, n.pre, H, n.n_post, n.post, act, S, M, B, obs, ix, h0, r, tab, 5.0f, th, y2,
                                         hl, sv);
          if (gru_sequence_forward_ref(n.n_pre, n.pre, H, n.n_post, n.post, act, S, M, B, obs, ix, h0, r, tab, 5.0f, th, y,
                                       variant == 1 ? NULL : hf, variant == 1 ? NULL : (variant == 2 ? h0 : ho), S))
            return 1;
          for (long long i = 0; i < R; ++i)
            if (!isfinite(y[i]) || mlp_f2u(y[i]) != mlp_f2u(y2[i])) return 2;
          if (variant != 1) {
            const float *got = variant == 2 ? h0 : ho;
            for (long long i = 0; i < M * H; ++i)
              if (mlp_f2u(got[i]) != mlp_f2u(hl[i])) return 3;
          }
          free(obs); free(h0); free(rs); free(th); free(nm); free(y); free(y2); free(hf); free(ho); free(hl); free(sv);
          free(idx);
          ++cases;
        }
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
