// pob_policy_head.h -- the tanh-normal head of the two actor kernels (pob_mlp.hip k_policy_act,
// pob_gru.hip k_gru_policy_act; DESIGN.md "Policy networks") and the kernel that advances their key.
#pragma once
#include "pob_mlp_tile.h"

// The tanh-normal head of one tile: L holds the logits (2 A features), T (A features, another
// image) takes the per-component log-probability terms.  Env b of this launch is env first + b
// of a batch of `total`: its draw for action component a is element (first + b) A + a of
// uniform(split(key)[1], (total, A), -1, 1).  The key is only read here (k_mlp_advance_key,
// launched after, advances it).
POB_MLP_D void policy_tile_head(float *L, float *T, const int A, const int b0, const int valid, const int total,
                                const int first, const uint32_t *key, const int deterministic, float *action, float *logp,
                                float *raw, float *logits, const int lane) {
  if (logits) {
    mlp_tile_store(logits, L, 0, 2 * A, b0, valid, lane);
    __syncthreads();
  }
  uint32_t s0 = 0u, s1 = 0u;
  if (!deterministic) tf_split(key[0], key[1], 2u, 1u, s0, s1);
  for (int e = lane; e < MLP_ROWS * A; e += 64) {
    const int env = e & 31, a = e >> 5;
    if (env >= valid) continue;
    const float loc = L[a * MLP_PITCH + env], s = L[(A + a) * MLP_PITCH + env];
    float act, rw;
    if (deterministic) {
      act = pob_tanhf(loc);
      rw = loc;
    } else {
      const uint32_t i = (uint32_t)(first + b0 + env) * (uint32_t)A + (uint32_t)a;
      const float u = tf_uniform(s0, s1, (uint32_t)total * (uint32_t)A, i, -1.0f, 1.0f);
      float term;
      pob_tanh_normal(loc, s, u, act, rw, term);
      T[a * MLP_PITCH + env] = term;
    }
    L[a * MLP_PITCH + env] = act;
    L[(A + a) * MLP_PITCH + env] = rw;
  }
  __syncthreads();
  mlp_tile_store(action, L, 0, A, b0, valid, lane);
  if (raw) mlp_tile_store(raw, L, A, A, b0, valid, lane);
  if (!deterministic && logp && lane < valid) {
    float sum = 0.0f;
    for (int a = 0; a < A; ++a) sum = sum + T[a * MLP_PITCH + lane];
    logp[b0 + lane] = sum;
  }
}

// launched after either actor kernel (pob_mlp.hip, pob_gru.hip)
static __global__ void k_mlp_advance_key(uint32_t *key) {
  uint32_t o0, o1;
  tf_split(key[0], key[1], 2u, 0u, o0, o1);
  key[0] = o0; key[1] = o1;
}
