// Host build of the observation-normaliser restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST):
// obsnorm_accumulate_ref / obsnorm_update_ref / obsnorm_apply_ref for ctypes.  -DOBSNORM_MAIN adds
// a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
int obsnorm_ref_chunk(void) { return POB_OBSNORM_CHUNK; }
int obsnorm_ref_accumulate(const float *x, long long N, int D, const float *table, double *sums) {
  if (N < 1 || D < 1 || D > POB_MLP_MAX_WIDTH) return -1;
  obsnorm_accumulate_ref(x, N, D, table, sums);
  return 0;
}
int obsnorm_ref_update(double *count, float *table, int D, const double *sums, int R, long long n_new) {
  if (R < 1 || n_new < 1 || D < 1 || D > POB_MLP_MAX_WIDTH) return -1;
  obsnorm_update_ref(count, table, D, sums, R, n_new);
  return 0;
}
// x (B, D) normalised in place
int obsnorm_ref_apply(float *x, long long B, int D, const float *table, float clip) {
  if (D < 1 || D > POB_MLP_MAX_WIDTH) return -1;
  obsnorm_apply_ref(x, B, D, table, clip);
  return 0;
}
float obsnorm_ref_apply1(float x, float mean, float scale, float clip) { return pob_obsnorm_apply(x, mean, scale, clip); }
}

#ifdef OBSNORM_MAIN
int main() {
  int cases = 0;
  const int Ds[3] = {1, 114, 256};
  const long long Ns[5] = {1, 1023, 1024, 1025, 2 * POB_OBSNORM_CHUNK + 7};
  uint32_t st = 99u;
  for (int di = 0; di < 3; ++di)
    for (int ni = 0; ni < 5; ++ni) {
      const int D = Ds[di];
      const long long N = Ns[ni];
      float *x = (float *)malloc(sizeof(float) * N * D), *table = (float *)malloc(sizeof(float) * 3 * D);
      double *sums = (double *)malloc(sizeof(double) * 2 * 2 * D), count = 0.0;
      for (int f = 0; f < D; ++f) { table[f] = 0.0f; table[D + f] = 1.0f; table[2 * D + f] = 1.0f; }
      for (int step = 0; step < 3; ++step) {
        for (long long i = 0; i < N * D; ++i) {
          st = st * 1664525u + 1013904223u;
          x[i] = (i % D) == 0 ? 2.5f : (float)(st >> 8) * 0x1p-24f * 40.0f - 20.0f + (float)(i % D);
        }
        // two shards: the halves of the rows (the first may be empty of rows only when N = 1)
        const long long n0 = N / 2;
        int R = 0;
        if (n0 > 0) { obsnorm_accumulate_ref(x, n0, D, table, sums); ++R; }
        obsnorm_accumulate_ref(x + n0 * D, N - n0, D, table, sums + (long long)R * 2 * D);
        ++R;
        obsnorm_update_ref(&count, table, D, sums, R, N);
        if (count != (double)(N * (step + 1))) return 1;
        for (int f = 0; f < 3 * D; ++f) if (!isfinite(table[f])) return 2;
        for (int f = 0; f < D; ++f) if (!(table[D + f] > 0.0f && table[D + f] <= 1000.0f)) return 3;
      }
      if (fabsf(table[0] - 2.5f) > 1e-6f) return 4;  // the constant column's mean
      obsnorm_apply_ref(x, N, D, table, 5.0f);
      for (long long i = 0; i < N * D; ++i) if (!(fabsf(x[i]) <= 5.0f)) return 5;
      obsnorm_apply_ref(x, N, D, NULL, 5.0f);
      free(x); free(table); free(sums);
      ++cases;
    }
  if (pob_obsnorm_apply(NAN, 0.0f, 1.0f, 5.0f) == pob_obsnorm_apply(NAN, 0.0f, 1.0f, 5.0f)) return 6;  // NaN stays NaN
  if (pob_obsnorm_apply(100.0f, 0.0f, 1.0f, 0.0f) != 100.0f) return 7;
  ++cases;
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
