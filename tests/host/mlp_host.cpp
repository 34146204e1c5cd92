// Host build of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST): the scalar functions over arrays,
// glibc's float32 functions over the same arrays (the yardstick of their error bounds), and the
// restatements mlp_forward_ref / policy_head_ref that the GPU tests compare the kernels with.
// -DMLP_MAIN adds a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
// which: 0 exp, 1 log, 2 tanh, 3 softplus, 4 sigmoid, 5 swish, 6 erfinv
int mlp_scalar(int which, long long n, const float *x, float *y) {
  for (long long i = 0; i < n; ++i) {
    switch (which) {
      case 0: y[i] = pob_expf(x[i]); break;
      case 1: y[i] = pob_logf(x[i]); break;
      case 2: y[i] = pob_tanhf(x[i]); break;
      case 3: y[i] = pob_softplusf(x[i]); break;
      case 4: y[i] = pob_sigmoidf(x[i]); break;
      case 5: y[i] = pob_swishf(x[i]); break;
      case 6: y[i] = pob_erfinvf(x[i]); break;
      default: return -1;
    }
  }
  return 0;
}
// the same functions spelled with glibc's float32 libm (no erfinv there)
int mlp_scalar_libm(int which, long long n, const float *x, float *y) {
  for (long long i = 0; i < n; ++i) {
    const float v = x[i];
    switch (which) {
      case 0: y[i] = expf(v); break;
      case 1: y[i] = logf(v); break;
      case 2: y[i] = tanhf(v); break;
      case 3: y[i] = fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))); break;
      case 4: y[i] = 1.0f / (1.0f + expf(-v)); break;
      case 5: y[i] = v / (1.0f + expf(-v)); break;
      default: return -1;
    }
  }
  return 0;
}
long long mlp_ref_param_count(int n_layers, const int *sizes) { return mlp_param_count(n_layers, sizes); }
int mlp_ref_forward(int n_layers, const int *sizes, int activation, int activate_final, int B, const float *x,
                    const float *theta, float *y) {
  if (n_layers < 1 || n_layers > POB_MLP_MAX_LAYERS) return -1;
  for (int l = 0; l <= n_layers; ++l)
    if (sizes[l] < 1 || sizes[l] > POB_MLP_MAX_WIDTH) return -1;
  mlp_forward_ref(n_layers, sizes, activation, activate_final, B, x, theta, y);
  return 0;
}
int mlp_ref_head(int B, int A, const float *logits, const float *u, int deterministic, float *action, float *logp,
                 float *raw) {
  policy_head_ref(B, A, logits, u, deterministic, action, logp, raw);
  return 0;
}
int mlp_ref_kfeat(int s, int h) { return mlp_kfeat(s, h); }
}

#ifdef MLP_MAIN
static int near(float a, double b, double rel) { return fabs((double)a - b) <= rel * fabs(b) + 1e-30; }
int main() {
  int cases = 0;
  for (int i = -880; i <= 880; ++i) {
    const float x = 0.1f * (float)i;
    if (!near(pob_expf(x), exp((double)x), 4e-7)) { printf("exp %g\n", x); return 1; }
    if (!near(pob_tanhf(x), tanh((double)x), 6e-7)) { printf("tanh %g\n", x); return 1; }
    if (!near(pob_softplusf(x), log1p(exp(-fabs((double)x))) + (x > 0 ? x : 0), 6e-7)) { printf("softplus %g\n", x); return 1; }
    cases += 3;
  }
  for (int e = -149; e <= 127; ++e) {
    const float x = ldexpf(1.3f, e);
    if (!near(pob_logf(x), log((double)x), 4e-7)) { printf("log %g\n", x); return 1; }
    ++cases;
  }
  if (pob_expf(-200.0f) != 0.0f || !isinf(pob_expf(100.0f)) || !isnan(pob_expf(NAN))) return 2;
  if (!isinf(pob_logf(0.0f)) || !isnan(pob_logf(-1.0f)) || !isinf(pob_logf(INFINITY))) return 3;
  if (pob_tanhf(50.0f) != 1.0f || pob_tanhf(-50.0f) != -1.0f) return 4;
  for (int i = -999; i <= 999; ++i) {
    const float y = pob_erfinvf(0.001f * (float)i);
    if (!near((float)erf((double)y), 0.001 * i, 2e-6) && i != 0) { printf("erfinv %d\n", i); return 5; }
    ++cases;
  }
  if (!isfinite(pob_erfinvf(POB_U_MIN)) || !isfinite(pob_erfinvf(0x1.fffffep-1f))) return 6;
  // networks at the limits: 8 layers, widths 1 and 256, an odd input width
  const int sizes[9] = {255, 256, 1, 33, 256, 7, 2, 256, 16};
  const long long n = mlp_param_count(8, sizes);
  float *theta = (float *)malloc(sizeof(float) * n), *x = (float *)malloc(sizeof(float) * 5 * 255);
  float *y = (float *)malloc(sizeof(float) * 5 * 16);
  uint32_t st = 12345u;
  for (long long i = 0; i < n; ++i) { st = st * 1664525u + 1013904223u; theta[i] = ((float)(st >> 8) * 0x1p-24f - 0.5f) * 0.2f; }
  for (int i = 0; i < 5 * 255; ++i) { st = st * 1664525u + 1013904223u; x[i] = (float)(st >> 8) * 0x1p-24f * 6.0f - 3.0f; }
  for (int act = 0; act < 3; ++act) {
    mlp_forward_ref(8, sizes, act, act == 1, 5, x, theta, y);
    for (int i = 0; i < 5 * 16; ++i) if (!isfinite(y[i])) return 7;
    ++cases;
  }
  float action[5 * 8], logp[5], raw[5 * 8], u[5 * 8];
  for (int i = 0; i < 40; ++i) u[i] = i == 0 ? -1.0f : -1.0f + 0.05f * (float)i;
  policy_head_ref(5, 8, y, u, 0, action, logp, raw);
  for (int i = 0; i < 5; ++i) if (!isfinite(logp[i])) return 8;
  policy_head_ref(5, 8, y, u, 1, action, logp, raw);
  for (int i = 0; i < 40; ++i) if (!(fabsf(action[i]) <= 1.0f)) return 9;
  cases += 2;
  free(theta); free(x); free(y);
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
