// Host build of the GAE restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST): gae_ref for ctypes.
// -DGAE_MAIN adds a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
int gae_ref_chunk(void) { return POB_GAE_CHUNK; }
int gae_ref_run(int T, long long B, const float *truncation, const float *second, int done_input, const float *reward,
                float reward_scale, const float *values, const float *bootstrap, float lambda, float discount, float *vs,
                float *advantages) {
  if (T < 1 || B < 1 || !second || !reward || !values || !bootstrap) return -1;
  gae_ref(T, B, truncation, second, done_input, reward, reward_scale, values, bootstrap, lambda, discount, vs, advantages);
  return 0;
}
}

#ifdef GAE_MAIN
static uint32_t st = 7u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  const int Ts[5] = {1, 2, POB_GAE_CHUNK, POB_GAE_CHUNK + 1, 2 * POB_GAE_CHUNK + 3};
  const long long Bs[3] = {1, 65, 257};
  for (int ti = 0; ti < 5; ++ti)
    for (int bi = 0; bi < 3; ++bi)
      for (int variant = 0; variant < 4; ++variant) {
        const int T = Ts[ti];
        const long long B = Bs[bi], n = T * B;
        float *tr = (float *)malloc(sizeof(float) * n), *dn = (float *)malloc(sizeof(float) * n);
        float *rw = (float *)malloc(sizeof(float) * n), *va = (float *)malloc(sizeof(float) * n);
        float *vs = (float *)malloc(sizeof(float) * n), *ad = (float *)malloc(sizeof(float) * n);
        float *bo = (float *)malloc(sizeof(float) * B);
        for (long long i = 0; i < n; ++i) {
          dn[i] = uni() < 0.1f ? 1.0f : 0.0f;
          tr[i] = dn[i] != 0.0f && uni() < 0.5f ? 1.0f : 0.0f;
          rw[i] = 6.0f * uni() - 3.0f;
          va[i] = 60.0f * uni() - 30.0f;
        }
        for (long long b = 0; b < B; ++b) bo[b] = 60.0f * uni() - 30.0f;
        // variants: all outputs; no truncation; vs only; advantages only
        gae_ref(T, B, variant == 1 ? NULL : tr, dn, 1, rw, 0.5f, va, bo, 0.95f, 0.99f, variant == 3 ? NULL : vs,
                variant == 2 ? NULL : ad);
        for (long long i = 0; i < n; ++i) {
          if (variant != 3 && !isfinite(vs[i])) return 1;
          if (variant != 2 && !isfinite(ad[i])) return 2;
          // a truncated step: advantage 0 and vs == values
          if (variant == 0 && tr[i] != 0.0f && (ad[i] != 0.0f || vs[i] != va[i])) return 3;
        }
        free(tr); free(dn); free(rw); free(va); free(vs); free(ad); free(bo);
        ++cases;
      }
  // one step by hand: m = 1, term = 0, g = 0.5; delta = adv = fmaf(0.5, 4, 2) - 1 = 3; vs = 4
  const float z = 0.0f, r = 2.0f, v = 1.0f, b = 4.0f;
  float vs1, ad1;
  gae_ref(1, 1, &z, &z, 0, &r, 1.0f, &v, &b, 0.95f, 0.5f, &vs1, &ad1);
  if (vs1 != 4.0f || ad1 != 3.0f) return 4;
  ++cases;
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
