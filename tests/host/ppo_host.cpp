// Host build of the PPO-loss restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST): ppo_loss_ref
// for ctypes.  -DPPO_MAIN adds a stand-alone program (run under -fsanitize=address,undefined).
#define POB_MLP_HOST
#include "pob_mlp.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {
int ppo_ref_chunk(void) { return POB_PPO_CHUNK; }
int ppo_ref_max_a(void) { return POB_PPO_MAX_A; }
// partials: (ceil(M / chunk), 3) float64, may be NULL
int ppo_ref_run(long long M, int A, const float *logits, const float *values, const int32_t *idx, const float *raw,
                const float *old_logp, const float *advantages, const float *vs, const float *u, float entropy_cost,
                float ppo_epsilon, float *dlogits, float *dvalues, float *losses, double *partials) {
  if (M < 1 || A < 1 || A > POB_PPO_MAX_A || !logits || !values || !raw || !old_logp || !advantages || !vs || !u || !losses)
    return -1;
  ppo_loss_ref(M, A, logits, values, idx, raw, old_logp, advantages, vs, u, entropy_cost, ppo_epsilon, dlogits, dvalues,
               losses, partials);
  return 0;
}
// The pieces, for the tests that spell a property out: factors (7, M, A) = term, ent, dlp_loc, dlp_sc,
// den_loc, den_sc, sig of every component; rows (6, M) = logp, ent, neg_surr, vl, g_lp, dvalue.
void ppo_ref_pieces(long long M, int A, const float *logits, const float *values, const int32_t *idx, const float *raw,
                    const float *old_logp, const float *advantages, const float *vs, const float *u, float ppo_epsilon,
                    float *factors, float *rows) {
  const float inv_m = 1.0f / (float)M;
  for (long long i = 0; i < M; ++i) {
    const long long j = idx ? idx[i] : i;
    float logp = 0.0f, ent = 0.0f;
    for (int a = 0; a < A; ++a) {
      float f[7];
      pob_ppo_component(logits[i * 2 * A + a], logits[i * 2 * A + A + a], raw[j * A + a], u[i * A + a], f[0], f[1], f[2],
                        f[3], f[4], f[5], f[6]);
      for (int q = 0; q < 7; ++q) factors[(q * M + i) * A + a] = f[q];
      logp = logp + f[0];
      ent = ent + f[1];
    }
    float r[4];
    pob_ppo_row(logp, old_logp[j], advantages[j], vs[j], values[i], ppo_epsilon, inv_m, r[0], r[1], r[2], r[3]);
    rows[i] = logp;
    rows[M + i] = ent;
    for (int q = 0; q < 4; ++q) rows[(2 + q) * M + i] = r[q];
  }
}
float ppo_ref_expf(float x) { return pob_expf(x); }
}

#ifdef PPO_MAIN
static uint32_t st = 7u;
static float uni() {
  st = st * 1664525u + 1013904223u;
  return (float)(st >> 8) * 0x1p-24f;
}

int main() {
  int cases = 0;
  const long long Ms[4] = {1, 65, POB_PPO_CHUNK, POB_PPO_CHUNK + 1};
  const int As[4] = {1, 3, 8, POB_PPO_MAX_A};
  for (int mi = 0; mi < 4; ++mi)
    for (int ai = 0; ai < 4; ++ai)
      for (int variant = 0; variant < 4; ++variant) {
        const long long M = Ms[mi], N = variant == 1 ? M + 7 : M;
        const int A = As[ai];
        const long long chunks = (M + POB_PPO_CHUNK - 1) / POB_PPO_CHUNK;
        float *lg = (float *)malloc(sizeof(float) * M * 2 * A), *va = (float *)malloc(sizeof(float) * M);
        float *u = (float *)malloc(sizeof(float) * M * A), *rw = (float *)malloc(sizeof(float) * N * A);
        float *ol = (float *)malloc(sizeof(float) * N), *ad = (float *)malloc(sizeof(float) * N);
        float *vs = (float *)malloc(sizeof(float) * N);
        float *dl = (float *)malloc(sizeof(float) * M * 2 * A), *dv = (float *)malloc(sizeof(float) * M);
        double *pa = (double *)malloc(sizeof(double) * chunks * 3);
        int32_t *ix = (int32_t *)malloc(sizeof(int32_t) * M);
        for (long long i = 0; i < M * 2 * A; ++i) lg[i] = 4.0f * uni() - 2.0f;
        for (long long i = 0; i < M * A; ++i) u[i] = 2.0f * uni() - 1.0f;
        u[0] = -1.0f;  // the clamp
        for (long long i = 0; i < N * A; ++i) rw[i] = 6.0f * uni() - 3.0f;
        for (long long i = 0; i < N; ++i) {
          ol[i] = -3.0f * A * uni();
          ad[i] = 4.0f * uni() - 2.0f;
          vs[i] = 60.0f * uni() - 30.0f;
        }
        for (long long i = 0; i < M; ++i) {
          va[i] = 60.0f * uni() - 30.0f;
          ix[i] = (int32_t)((N - 1 - i % N + (long long)(uni() * 3.0f)) % N);  // repeats, every entry in [0, N)
        }
        // variants: all outputs; idx into a longer trajectory; no dlogits; no dvalues and no partials
        float losses[4];
        ppo_loss_ref(M, A, lg, va, variant == 1 ? ix : NULL, rw, ol, ad, vs, u, 1e-4f, 0.3f, variant == 2 ? NULL : dl,
                     variant == 3 ? NULL : dv, losses, variant == 3 ? NULL : pa);
        for (int k = 0; k < 4; ++k)
          if (!isfinite(losses[k])) return 1;
        if (losses[0] != (losses[1] + losses[2]) + losses[3]) return 2;
        if (variant != 2)
          for (long long i = 0; i < M * 2 * A; ++i)
            if (!isfinite(dl[i])) return 3;
        if (variant != 3)
          for (long long i = 0; i < M; ++i)
            if (!isfinite(dv[i])) return 4;
        free(lg); free(va); free(u); free(rw); free(ol); free(ad); free(vs); free(dl); free(dv); free(pa); free(ix);
        ++cases;
      }
  // one row by hand: logp == old_logp gives rho = 1, so g_lp = -adv / M and dvalue = -(vs - v) / 2 / M
  {
    const float lg[2] = {0.25f, -0.5f}, x = 0.75f, u = 0.125f, adv = 2.0f, vs = 3.0f, v = 1.0f;
    float term, en, f[5], dl[2], dv, losses[4];
    pob_ppo_component(lg[0], lg[1], x, u, term, en, f[0], f[1], f[2], f[3], f[4]);
    const float old = 0.0f + term;
    ppo_loss_ref(1, 1, lg, &v, NULL, &x, &old, &adv, &vs, &u, 0.0f, 0.3f, dl, &dv, losses, NULL);
    if (dv != -1.0f || losses[2] != 1.0f || losses[1] != -2.0f || losses[3] != 0.0f) return 5;
    if (dl[0] != -2.0f * f[0] || dl[1] != (-2.0f * f[1]) * f[4]) return 6;
    ++cases;
  }
  printf("%d cases OK\n", cases);
  return 0;
}
#endif
