// Host build of the Adam restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST): adam_step_ref for ctypes.
// -DADAM_MAIN adds a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {
int adam_ref_max_seg(void) { return POB_ADAM_MAX_SEG; }
int adam_ref_run(int n_seg, float **theta, const float **grad, float **m, float **v, const long long *n, double *state,
                 float lr, float beta1, float beta2, float eps) {
  if (n_seg < 1 || n_seg > POB_ADAM_MAX_SEG || !theta || !grad || !m || !v || !n || !state) return -1;
  for (int s = 0; s < n_seg; ++s)
    if (n[s] < 1 || !theta[s] || !grad[s] || !m[s] || !v[s]) return -1;
  adam_step_ref(n_seg, theta, grad, m, v, n, state, lr, beta1, beta2, eps);
  return 0;
}
}

#ifdef ADAM_MAIN
static uint32_t st = 11u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  const long long ns[7] = {1, 3, 63, 64, 65, 255, 1027};
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b < 7; b += 3) {
      // two segments of exactly n floats each (the sanitizer guards both ends), three carried steps
      const long long n[2] = {ns[a], ns[b]};
      float *th[2], *g[2], *m[2], *v[2], *th0[2];
      for (int s = 0; s < 2; ++s) {
        th[s] = (float *)malloc(sizeof(float) * n[s]);
        th0[s] = (float *)malloc(sizeof(float) * n[s]);
        g[s] = (float *)malloc(sizeof(float) * n[s]);
        m[s] = (float *)calloc(n[s], sizeof(float));
        v[s] = (float *)calloc(n[s], sizeof(float));
        for (long long i = 0; i < n[s]; ++i) th[s][i] = th0[s][i] = 2.0f * uni() - 1.0f;
      }
      double state[2] = {1.0, 1.0};
      double p1 = 1.0, p2 = 1.0;
      for (int step = 0; step < 3; ++step) {
        for (int s = 0; s < 2; ++s)
          for (long long i = 0; i < n[s]; ++i) g[s][i] = 0.02f * uni() - 0.01f;
        const float *gc[2] = {g[0], g[1]};
        adam_step_ref(2, th, gc, m, v, n, state, 3e-4f, 0.9f, 0.999f, 1e-8f);
        p1 *= (double)0.9f;
        p2 *= (double)0.999f;
        if (state[0] != p1 || state[1] != p2) return 1;
      }
      for (int s = 0; s < 2; ++s) {
        for (long long i = 0; i < n[s]; ++i) {
          if (!isfinite(th[s][i]) || !isfinite(m[s][i]) || !(v[s][i] >= 0.0f)) return 2;
          // three steps of at most about lr each
          if (fabsf(th[s][i] - th0[s][i]) > 4.0f * 3e-4f) return 3;
        }
        free(th[s]); free(th0[s]); free(g[s]); free(m[s]); free(v[s]);
      }
      ++cases;
    }
  // one element by hand: g = 1 from m = v = 0: m_hat = v_hat = 1 up to the roundings, theta moves by about -lr
  float th = 1.0f, g1 = 1.0f, m1 = 0.0f, v1 = 0.0f;
  float *tp = &th, *mp = &m1, *vp = &v1;
  const float *gp = &g1;
  const long long one = 1;
  double state[2] = {1.0, 1.0};
  adam_step_ref(1, &tp, &gp, &mp, &vp, &one, state, 0.5f, 0.9f, 0.999f, 1e-8f);
  if (fabsf(th - 0.5f) > 1e-6f || m1 != 1.0f - 0.9f || v1 != 1.0f - 0.999f) return 4;
  // g = 0, m = 0: theta keeps its bits
  float th2 = -0.0f, g2 = 0.0f, m2 = 0.0f, v2 = 0.25f;
  tp = &th2; gp = &g2; mp = &m2; vp = &v2;
  adam_step_ref(1, &tp, &gp, &mp, &vp, &one, state, 0.5f, 0.9f, 0.999f, 1e-8f);
  uint32_t bits;
  memcpy(&bits, &th2, 4);
  if (bits != 0x80000000u) return 5;
  cases += 2;
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
