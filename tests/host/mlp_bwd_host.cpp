// Host build of the MLP training forward / backward restatement of po-brax_amd/csrc/pob_mlp.h
// (POB_MLP_HOST): mlp_forward_train_ref and mlp_backward_ref for ctypes.  -DMLP_BWD_MAIN adds a
// stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
int mlp_bwd_ref_chunk(void) { return POB_MLP_BWD_CHUNK; }
long long mlp_bwd_ref_param_count(int n_layers, const int *sizes) { return mlp_param_count(n_layers, sizes); }
long long mlp_bwd_ref_saved_count(int n_layers, const int *sizes, int activate_final, long long M) {
  return mlp_saved_count(n_layers, sizes, activate_final, M);
}
void mlp_bwd_ref_forward(int n_layers, const int *sizes, int activation, int activate_final, int B, const float *x,
                         const float *theta, float *y) {
  mlp_forward_ref(n_layers, sizes, activation, activate_final, B, x, theta, y);
}
void mlp_bwd_ref_forward_train(int n_layers, const int *sizes, int activation, int activate_final, long long M,
                               const float *x, const float *theta, float *y, float *saved) {
  mlp_forward_train_ref(n_layers, sizes, activation, activate_final, M, x, theta, y, saved);
}
// dx and delta (every layer's delta (M, sizes[l + 1]), ascending l) may be NULL
int mlp_bwd_ref_backward(int n_layers, const int *sizes, int activation, int activate_final, long long M, const float *x,
                         const float *theta, const float *saved, const float *dy, float *dtheta, float *dx, float *delta) {
  return mlp_backward_ref(n_layers, sizes, activation, activate_final, M, x, theta, saved, dy, dtheta, dx, delta);
}
// one element's sum in the tile / chunk order; a may be NULL (the constant 1); partials may be NULL
float mlp_bwd_ref_sum(long long M, const float *a, long long lda, const float *d, long long ldd, double *partials) {
  return mlp_bwd_sum(M, a, lda, d, ldd, partials);
}
float mlp_bwd_ref_activate(int act, float z) { return mlp_activate(act, z); }
float mlp_bwd_ref_activate_grad(int act, float z, float g) { return mlp_activate_grad(act, z, g); }
}

#ifdef MLP_BWD_MAIN
static uint32_t st = 11u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  const int nets[4][POB_MLP_MAX_LAYERS + 2] = {{1, 3, 1}, {2, 5, 7, 4}, {3, 27, 33, 16, 1}, {8, 4, 3, 3, 3, 3, 3, 3, 3, 2}};
  const long long Ms[4] = {1, 33, POB_MLP_BWD_CHUNK, POB_MLP_BWD_CHUNK + 1};
  for (int ni = 0; ni < 4; ++ni)
    for (int mi = 0; mi < 4; ++mi)
      for (int act = 0; act < 3; ++act)
        for (int variant = 0; variant < 3; ++variant) {  // all outputs; no dx, no delta; activate_final
          const int L = nets[ni][0], *sizes = nets[ni] + 1, fin = variant == 2;
          const long long M = Ms[mi], P = mlp_param_count(L, sizes), S = mlp_saved_count(L, sizes, fin, M);
          long long nd = 0;
          for (int l = 0; l < L; ++l) nd += M * sizes[l + 1];
          float *x = (float *)malloc(sizeof(float) * M * sizes[0]), *th = (float *)malloc(sizeof(float) * P);
          float *y = (float *)malloc(sizeof(float) * M * sizes[L]), *y2 = (float *)malloc(sizeof(float) * M * sizes[L]);
          float *sv = (float *)malloc(sizeof(float) * (S ? S : 1)), *dy = (float *)malloc(sizeof(float) * M * sizes[L]);
          float *dt = (float *)malloc(sizeof(float) * P), *dx = (float *)malloc(sizeof(float) * M * sizes[0]);
          float *de = (float *)malloc(sizeof(float) * nd);
          for (long long i = 0; i < M * sizes[0]; ++i) x[i] = 6.0f * uni() - 3.0f;
          for (long long i = 0; i < P; ++i) th[i] = uni() - 0.5f;
          for (long long i = 0; i < M * sizes[L]; ++i) dy[i] = (2.0f * uni() - 1.0f) / (float)M;
          mlp_forward_train_ref(L, sizes, act, fin, M, x, th, y, sv);
          mlp_forward_ref(L, sizes, act, fin, (int)M, x, th, y2);
          for (long long i = 0; i < M * sizes[L]; ++i)
            if (mlp_f2u(y[i]) != mlp_f2u(y2[i])) return 1;
          if (mlp_backward_ref(L, sizes, act, fin, M, x, th, sv, dy, dt, variant == 1 ? NULL : dx, variant == 1 ? NULL : de))
            return 2;
          for (long long i = 0; i < P; ++i)
            if (!isfinite(dt[i])) return 3;
          if (variant != 1)
            for (long long i = 0; i < M * sizes[0]; ++i)
              if (!isfinite(dx[i])) return 4;
          free(x); free(th); free(y); free(y2); free(sv); free(dy); free(dt); free(dx); free(de);
          ++cases;
        }
  // one layer by hand: y = x W + b without activation, two rows
  {
    const int sizes[2] = {2, 1};
    const float x[4] = {1.0f, 2.0f, 3.0f, 5.0f}, th[3] = {7.0f, -2.0f, 0.5f}, dy[2] = {1.0f, -4.0f};
    float y[2], dt[3], dx[4];
    mlp_forward_train_ref(1, sizes, POB_ACT_SWISH, 0, 2, x, th, y, NULL);
    if (y[0] != 3.5f || y[1] != 11.5f) return 5;
    if (mlp_backward_ref(1, sizes, POB_ACT_SWISH, 0, 2, x, th, NULL, dy, dt, dx, NULL)) return 6;
    if (dt[0] != -11.0f || dt[1] != -18.0f || dt[2] != -3.0f) return 7;
    if (dx[0] != 7.0f || dx[1] != -2.0f || dx[2] != -28.0f || dx[3] != 8.0f) return 8;
    ++cases;
  }
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
