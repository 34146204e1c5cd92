// pob_mlp.h -- the scalar math and the plain-C restatement of the policy-network kernels
// (pob_mlp.hip: k_mlp_forward, k_policy_act, the recurrent k_gru_forward, k_gru_policy_act, the
// observation normaliser's k_obsnorm_*, k_gae, k_ppo_* and the training forward / backward pass
// k_mlp_forward_train, k_mlp_bwd_*, and the recurrent window's k_gru_seq_forward, k_gru_seq_backward,
// k_gru_bwd_weights, k_gru_seq_infer, and the optimiser's k_adam_step).
// Compiled for the device by hipcc and, with POB_MLP_HOST, for the host by g++
// (tests/host/mlp_host.cpp, gru_host.cpp, obsnorm_host.cpp, gae_host.cpp, ppo_host.cpp,
// mlp_bwd_host.cpp, gru_bwd_host.cpp, gru_seq_infer_host.cpp, adam_host.cpp); both with -ffp-contract=off.
//
// Every function is a fixed sequence of float32 +, *, fmaf, integer bit operations, and the
// correctly rounded reciprocal and square root (pob_rcp / pob_sqrt of pob_math.h on the device,
// 1.0f / x and sqrtf on the host: the same values).  No ocml, no libm, no tables in memory, so
// host and device give the same bits and mlp_forward_ref / policy_act_ref below ARE the
// specification of the kernels (DESIGN.md "Policy networks").
//
// Layer: y[j] = act(b[j] + sum_k x[k] W[k][j]), W row-major (in, out).  The accumulator starts
// from the bias and takes one fmaf per input feature in the order mlp_kfeat gives: k-step s
// (one v_mfma_f32_32x32x2_f32) adds lane half 0's feature, then lane half 1's, i.e. natural
// order 0, 1, 2, ..  An odd input width is padded with one zero feature (x = 0, w = 0), whose
// fmaf(0, 0, acc) the restatement spells too (it turns an accumulator of -0 into +0).
#pragma once
#include <stdint.h>
#ifdef POB_MLP_HOST
#include <math.h>
#include <stdlib.h>
#define POB_MLP_D static inline
POB_MLP_D float mlp_rcp(float x) { return 1.0f / x; }
POB_MLP_D float mlp_sqrt(float x) { return sqrtf(x); }
POB_MLP_D uint32_t mlp_f2u(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
POB_MLP_D float mlp_u2f(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
#else
#include "pob_math.h"
#define POB_MLP_D __device__ __forceinline__
POB_MLP_D float mlp_rcp(float x) { return pob_rcp(x); }
POB_MLP_D float mlp_sqrt(float x) { return pob_sqrt(x); }
POB_MLP_D uint32_t mlp_f2u(float x) { return __float_as_uint(x); }
POB_MLP_D float mlp_u2f(uint32_t u) { return __uint_as_float(u); }
#endif
#define MLP_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

#define POB_MLP_MAX_LAYERS 8
#define POB_MLP_MAX_WIDTH 256
#define POB_GRU_MAX_HIDDEN 128  // the recurrent actor: hidden width, pre- and post-MLP depths
#define POB_GRU_MAX_PRE 3
#define POB_GRU_MAX_POST 4
enum { POB_ACT_RELU = 0, POB_ACT_SWISH = 1, POB_ACT_TANH = 2 };

// input feature of k-step s, lane half h (the summation order: s ascending, h = 0 then 1)
POB_MLP_D constexpr int mlp_kfeat(const int s, const int h) { return 2 * s + h; }
POB_MLP_D constexpr int mlp_ksteps(const int in) { return (in + 1) >> 1; }

// exp(x): n = rint(x log2 e) by the 1.5 * 2^23 shift, r = x - n ln 2 in two fused steps
// (Cody-Waite), the degree-7 Taylor polynomial in Horner form, and the scale 2^n applied as
// two exact powers of two, so results in the subnormal range round once.  x <= -104 gives 0,
// x >= 89 gives inf, NaN gives NaN.
POB_MLP_D float pob_expf(float x) {
  x = x < -104.0f ? -104.0f : x;
  x = x > 89.0f ? 89.0f : x;
  const float t = MLP_FMA(x, 1.44269504f, 12582912.0f);
  const float fn = t - 12582912.0f;
  const int n = (int)(mlp_f2u(t) - 0x4B400000u);
  float r = MLP_FMA(fn, -0.693145751953125f, x);
  r = MLP_FMA(fn, -1.42860677e-6f, r);
  float p = 1.98412698e-4f;
  p = MLP_FMA(p, r, 1.38888889e-3f);
  p = MLP_FMA(p, r, 8.33333333e-3f);
  p = MLP_FMA(p, r, 4.16666667e-2f);
  p = MLP_FMA(p, r, 1.66666667e-1f);
  p = MLP_FMA(p, r, 0.5f);
  p = MLP_FMA(p, r, 1.0f);
  p = MLP_FMA(p, r, 1.0f);
  const int n1 = n >> 1, n2 = n - n1;
  const float s1 = mlp_u2f((uint32_t)(n1 + 127) << 23), s2 = mlp_u2f((uint32_t)(n2 + 127) << 23);
  return (p * s1) * s2;
}

// log(x): x = 2^k m with m in [sqrt(1/2), sqrt(2)), f = m - 1 (exact), s = f / (2 + f),
// log m = f - (f^2/2 - s (f^2/2 + R(s^2))) with the four-term even polynomial of the fdlibm
// family [ext], then k ln 2 in two parts.  Subnormal x is scaled by 2^25 first.  log(0) =
// -inf, x < 0 and NaN give NaN, inf gives inf.
POB_MLP_D float pob_logf(float x) {
  const bool sub = x < 0x1p-126f;
  const float xs = sub ? x * 0x1p25f : x;
  uint32_t ix = mlp_f2u(xs) + (0x3F800000u - 0x3F3504F3u);
  const int k = (int)(ix >> 23) - 127 - (sub ? 25 : 0);
  ix = (ix & 0x007FFFFFu) + 0x3F3504F3u;
  const float f = mlp_u2f(ix) - 1.0f;
  const float s = f * mlp_rcp(2.0f + f);
  const float z = s * s, w = z * z;
  const float t1 = w * MLP_FMA(w, 0.24279078841f, 0.40000972152f);
  const float t2 = z * MLP_FMA(w, 0.28498786688f, 0.66666662693f);
  const float R = t2 + t1;
  const float hfsq = (0.5f * f) * f;
  const float dk = (float)k;
  float r = MLP_FMA(s, hfsq + R, dk * 9.0580006145e-06f);
  r = ((r - hfsq) + f) + dk * 6.9313812256e-01f;
  r = x == 0.0f ? mlp_u2f(0xFF800000u) : r;
  r = x < 0.0f ? mlp_u2f(0x7FC00000u) : r;
  r = mlp_f2u(x) == 0x7F800000u ? x : r;
  r = x != x ? x : r;
  return r;
}

// tanh(x): |x| < 0.625 the odd polynomial x + x z P(z), z = x^2 (Cephes form [ext]); else
// 1 - 2 / (exp(2 |x|) + 1) with the sign of x; |x| >= 10 gives +-1.
POB_MLP_D float pob_tanhf(float x) {
  const float a = x < 0.0f ? -x : x;
  const float z = x * x;
  float p = -5.70498872745e-3f;
  p = MLP_FMA(p, z, 2.06390887954e-2f);
  p = MLP_FMA(p, z, -5.37397155531e-2f);
  p = MLP_FMA(p, z, 1.33314422036e-1f);
  p = MLP_FMA(p, z, -3.33332819422e-1f);
  const float small = MLP_FMA(p * z, x, x);
  const float e = pob_expf(2.0f * (a > 10.0f ? 10.0f : a));
  float big = 1.0f - 2.0f * mlp_rcp(e + 1.0f);
  big = x < 0.0f ? -big : big;
  float r = a < 0.625f ? small : big;
  r = x != x ? x : r;
  return r;
}

// log1p(t) for t in [0, 1]: u = fl(1 + t), log u + (t - (u - 1)) / u (the rounding of 1 + t
// given back to first order; t below 2^-24 returns t)
POB_MLP_D float pob_log1p_unit(float t) {
  const float u = 1.0f + t;
  const float c = t - (u - 1.0f);
  return MLP_FMA(c, mlp_rcp(u), pob_logf(u));
}
// softplus(x) = max(x, 0) + log1p(exp(-|x|)): no cancellation on either side
POB_MLP_D float pob_softplusf(float x) {
  const float a = x < 0.0f ? -x : x;
  const float m = x > 0.0f ? x : 0.0f;
  const float r = m + pob_log1p_unit(pob_expf(-a));
  return x != x ? x : r;
}
// sigmoid(x) = 1 / (1 + exp(-x)); swish(x) = x sigmoid(x)
POB_MLP_D float pob_sigmoidf(float x) { return mlp_rcp(1.0f + pob_expf(-x)); }
POB_MLP_D float pob_swishf(float x) { return x * pob_sigmoidf(x); }

// erfinv(x) on (-1, 1): w = -log((1 - x)(1 + x)); two polynomials, in w - 2.5 for w < 5 and in
// sqrt(w) - 3 beyond (M. Giles, "Approximating the erfinv function", 2010 [ext]), times x.
POB_MLP_D float pob_erfinvf(float x) {
  const float w = -pob_logf((1.0f - x) * (1.0f + x));
  const float wc = w - 2.5f;
  float p = 2.81022636e-08f;
  p = MLP_FMA(p, wc, 3.43273939e-07f);
  p = MLP_FMA(p, wc, -3.5233877e-06f);
  p = MLP_FMA(p, wc, -4.39150654e-06f);
  p = MLP_FMA(p, wc, 0.00021858087f);
  p = MLP_FMA(p, wc, -0.00125372503f);
  p = MLP_FMA(p, wc, -0.00417768164f);
  p = MLP_FMA(p, wc, 0.246640727f);
  p = MLP_FMA(p, wc, 1.50140941f);
  const float wt = mlp_sqrt(w < 5.0f ? 5.0f : w) - 3.0f;
  float q = -0.000200214257f;
  q = MLP_FMA(q, wt, 0.000100950558f);
  q = MLP_FMA(q, wt, 0.00134934322f);
  q = MLP_FMA(q, wt, -0.00367342844f);
  q = MLP_FMA(q, wt, 0.00573950773f);
  q = MLP_FMA(q, wt, -0.0076224613f);
  q = MLP_FMA(q, wt, 0.00943887047f);
  q = MLP_FMA(q, wt, 1.00167406f);
  q = MLP_FMA(q, wt, 2.83297682f);
  return (w < 5.0f ? p : q) * x;
}

POB_MLP_D float mlp_activate(const int act, const float x) {
  if (act == POB_ACT_RELU) return x > 0.0f ? x : 0.0f;
  if (act == POB_ACT_SWISH) return pob_swishf(x);
  return pob_tanhf(x);
}

// The backward pass of the activation: delta = g act'(z) from the saved pre-activation z and the
// incoming gradient g (DESIGN.md "MLP backward").  relu gives +0 wherever z <= 0 (a NaN z too).
#define POB_MLP_BWD_CHUNK 1024  // rows of one chunk of the parameter gradient's summation order
POB_MLP_D float mlp_activate_grad(const int act, const float z, const float g) {
  if (act == POB_ACT_RELU) return z > 0.0f ? g : 0.0f;
  if (act == POB_ACT_SWISH) {
    const float s = pob_sigmoidf(z);
    return g * MLP_FMA(z * s, 1.0f - s, s);
  }
  const float t = pob_tanhf(z);
  return g * MLP_FMA(-t, t, 1.0f);
}

// The tanh-normal head of one action component (brax NormalTanhDistribution [ext]): scale =
// softplus(s) + 0.001, eps = sqrt(2) erfinv(u) with u clamped to -1 + 2^-24 from below (the
// uniform draw can return -1), raw = loc + scale eps, action = tanh(raw), and the component's
// log-probability term -eps^2/2 - log scale - log(2 pi)/2 - 2 (log 2 - raw - softplus(-2 raw)).
#define POB_U_MIN (-0x1.fffffep-1f)
POB_MLP_D void pob_tanh_normal(const float loc, const float s, float u, float &action, float &raw, float &term) {
  const float scale = pob_softplusf(s) + 0.001f;
  u = u > POB_U_MIN ? u : POB_U_MIN;
  const float eps = 1.41421354f * pob_erfinvf(u);
  raw = MLP_FMA(scale, eps, loc);
  action = pob_tanhf(raw);
  const float t0 = (-0.5f * eps) * eps;
  const float t1 = (t0 - pob_logf(scale)) - 0.918938533f;
  const float ld = 2.0f * ((0.693147181f - raw) - pob_softplusf(-2.0f * raw));
  term = t1 - ld;
}

// ---------------------------------------------------------------------------- observation normaliser
// The running normaliser of brax <= 0.0.12 training/normalization.py [ext] (DESIGN.md "Observation
// normaliser").  State: count (float64), table (3, D) float32 = mean, scale, m2.  What an actor
// kernel does to a staged observation element of column f: one float32 subtract, one float32
// multiply (no contraction), then the clamp; clip <= 0 turns the clamp off.  A NaN stays NaN.
#define POB_OBSNORM_CHUNK 1024  // rows of one chunk of the statistics' summation order
POB_MLP_D float pob_obsnorm_apply(const float x, const float mean, const float scale, const float clip) {
  float t = (x - mean) * scale;
  if (clip > 0.0f) { t = t < -clip ? -clip : t; t = t > clip ? clip : t; }
  return t;
}
// One row into a chunk's accumulator pair of a column: d is centred on the OLD mean.
POB_MLP_D void pob_obsnorm_step(const float x, const float mean, double &S1, double &S2) {
  const double d = (double)x - (double)mean;
  S1 = S1 + d;
  S2 = __builtin_fma(d, d, S2);
}
// The update of one column from its sums S1 = sum d, S2 = sum d^2 over n_new new rows (Welford in
// one pass: m2 grows by sum (x - mean')(x - mean) = S2 - S1^2 / total).  Returns the new count.
POB_MLP_D double pob_obsnorm_finish(const double count, const double n_new, const double S1, const double S2, float &mean,
                                    float &scale, float &m2) {
  const double total = count + n_new;
  const double t = S1 / total;
  mean = (float)((double)mean + t);
  m2 = (float)((double)m2 + __builtin_fma(-S1, t, S2));
  double v = (double)m2 / (total + 1.0);
  v = v < 1e-6 ? 1e-6 : v;
  v = v > 1e6 ? 1e6 : v;
  scale = mlp_rcp(mlp_sqrt((float)v));
  return total;
}

// ---------------------------------------------------------------------------- GAE
// One step of brax v1 PPO's compute_gae [ext] for one env, t descending (DESIGN.md "Critic pass
// and GAE"): deltas = (r + g v_{t+1} - v) m, acc = delta + g m lambda acc, vs = acc + v, adv =
// (r + g vs_{t+1} - v) m with g = discount (1 - term), m = 1 - truncation, in ONE reverse pass.
// Carried per env: acc (from +0), v_next and vs_next (both from the bootstrap value).  second is
// termination, or done when done_input (then term = done m).  No special cases: a NaN stays NaN.
#define POB_GAE_CHUNK 8  // steps whose rows k_gae loads ahead of their use
POB_MLP_D void pob_gae_step(const float trunc, const float second, const int done_input, const float reward,
                            const float reward_scale, const float v, const float lambda, const float discount, float &acc,
                            float &v_next, float &vs_next, float &adv) {
  const float m = 1.0f - trunc;
  const float term = done_input ? second * m : second;
  const float g = discount * (1.0f - term);
  const float r = reward * reward_scale;
  const float delta = (MLP_FMA(g, v_next, r) - v) * m;
  adv = (MLP_FMA(g, vs_next, r) - v) * m;
  acc = MLP_FMA((g * m) * lambda, acc, delta);
  vs_next = acc + v;
  v_next = v;
}

// ---------------------------------------------------------------------------- PPO loss
// brax v1 ppo.compute_ppo_loss [ext] on the tanh-normal head, with its gradient to the logits and
// the values (DESIGN.md "PPO loss").  One action component: the log-probability term of the STORED
// pre-tanh action x (the noise e re-derived from it; constants and term spelling of
// pob_tanh_normal), the sampled-entropy term from the draw u (clamped like the head's), and the
// factors of both terms' derivatives: d term / d loc = dlp_loc, d term / d scale = dlp_sc, d ent /
// d loc = den_loc, d ent / d scale = den_sc, d scale / d p = sig.
#define POB_PPO_MAX_A 128             // action components: the logits' width 2 A is a legal network width
#define POB_PPO_CHUNK POB_OBSNORM_CHUNK  // rows of one chunk of the scalars' summation order
POB_MLP_D void pob_ppo_component(const float loc, const float p, const float x, float u, float &term, float &ent,
                                 float &dlp_loc, float &dlp_sc, float &den_loc, float &den_sc, float &sig) {
  const float scale = pob_softplusf(p) + 0.001f;
  const float inv = mlp_rcp(scale), ls = pob_logf(scale);
  const float e = (x - loc) * inv;
  const float t1 = (((-0.5f * e) * e) - ls) - 0.918938533f;
  const float ldx = 2.0f * ((0.693147181f - x) - pob_softplusf(-2.0f * x));
  term = t1 - ldx;
  u = u > POB_U_MIN ? u : POB_U_MIN;
  const float eps = 1.41421354f * pob_erfinvf(u);
  const float y = MLP_FMA(scale, eps, loc);
  const float ldy = 2.0f * ((0.693147181f - y) - pob_softplusf(-2.0f * y));
  ent = (1.418938533f + ls) + ldy;
  dlp_loc = e * inv;
  dlp_sc = MLP_FMA(e, e, -1.0f) * inv;
  den_loc = -2.0f * pob_tanhf(y);
  den_sc = MLP_FMA(eps, den_loc, inv);
  sig = pob_sigmoidf(p);
}
// One row after its components: logp, ent = the sums of the terms (a ascending from +0).  neg_surr
// = -min(rho adv, clip(rho) adv) and vl = (vs - value)^2 / 4 are the row's parts of the policy and
// value losses; g_lp = d total / d logp (0 on the clipped branch; a tie takes the unclipped one),
// dvalue = d total / d value.  No special cases: a NaN compares false and takes the clipped branch.
POB_MLP_D void pob_ppo_row(const float logp, const float old_logp, const float adv, const float vs, const float value,
                           const float ppo_epsilon, const float inv_m, float &neg_surr, float &vl, float &g_lp,
                           float &dvalue) {
  const float rho = pob_expf(logp - old_logp);
  const float lo = 1.0f - ppo_epsilon, hi = 1.0f + ppo_epsilon;
  float c = rho < lo ? lo : rho;
  c = c > hi ? hi : c;
  const float s1 = rho * adv, s2 = c * adv;
  const bool unclipped = s1 <= s2;
  neg_surr = -(unclipped ? s1 : s2);
  g_lp = unclipped ? -(s1 * inv_m) : 0.0f;
  const float verr = vs - value;
  vl = (verr * verr) * 0.25f;
  dvalue = (-0.5f * verr) * inv_m;
}
// The gradient of one component from the row's g_lp and g_ent = -(entropy_cost inv_m)
POB_MLP_D void pob_ppo_grad(const float g_lp, const float g_ent, const float dlp_loc, const float dlp_sc,
                            const float den_loc, const float den_sc, const float sig, float &d_loc, float &d_p) {
  d_loc = MLP_FMA(g_lp, dlp_loc, g_ent * den_loc);
  d_p = MLP_FMA(g_lp, dlp_sc, g_ent * den_sc) * sig;
}
// losses[4] = total, policy, value, entropy from the float64 sums of neg_surr, vl, ent over M rows
POB_MLP_D void pob_ppo_finish(const double S_p, const double S_v, const double S_e, const long long M,
                              const float entropy_cost, float *losses) {
  const double m = (double)M;
  const float policy = (float)(S_p / m), value = (float)(S_v / m);
  const float entropy = (float)(-(double)entropy_cost * (S_e / m));
  losses[0] = (policy + value) + entropy;
  losses[1] = policy;
  losses[2] = value;
  losses[3] = entropy;
}

// ---------------------------------------------------------------------------- Adam
// optax's adam [ext] (brax v1 PPO's optimiser; no weight decay, no amsgrad) in a fixed float32
// order (DESIGN.md "Learner on the device").  The step count lives in the state block as the two
// running float64 products P1 = beta1^t, P2 = beta2^t (from 1.0; P <- P (double)beta, one float64
// product a step), so there is no counter and no pow.  Per step, once: the new products, c = (float)
// (1.0 - P) rounded once from float64, and the bias corrections as reciprocals ic = 1 / c.  Per
// element: m = fmaf(beta1, m, (1 - beta1) g), v = fmaf(beta2, v, ((1 - beta2) g) g), m_hat = m ic1,
// v_hat = v ic2, theta = fmaf(-lr, m_hat (1 / (sqrt(v_hat) + eps)), theta): every quotient is a
// product with a correctly rounded reciprocal, and 1 - beta is one float32 subtraction.
#define POB_ADAM_MAX_SEG 4  // (theta, grad, m, v, n) segments of one launch
POB_MLP_D void pob_adam_bias(const double p1, const double p2, const float beta1, const float beta2, double &p1_new,
                             double &p2_new, float &ic1, float &ic2) {
  p1_new = p1 * (double)beta1;
  p2_new = p2 * (double)beta2;
  ic1 = mlp_rcp((float)(1.0 - p1_new));
  ic2 = mlp_rcp((float)(1.0 - p2_new));
}
POB_MLP_D void pob_adam_elem(float &theta, const float g, float &m, float &v, const float lr, const float beta1,
                             const float beta2, const float eps, const float ic1, const float ic2) {
  m = MLP_FMA(beta1, m, (1.0f - beta1) * g);
  v = MLP_FMA(beta2, v, ((1.0f - beta2) * g) * g);
  const float m_hat = m * ic1, v_hat = v * ic2;
  const float den = mlp_sqrt(v_hat) + eps;
  theta = MLP_FMA(-lr, m_hat * mlp_rcp(den), theta);
}

#ifdef POB_MLP_HOST
// One Adam step of n_seg <= POB_ADAM_MAX_SEG segments: theta, m, v (n[s] floats each) updated in
// place from grad, all under the bias corrections of ONE advance of state[2] = {beta1^t, beta2^t},
// which is stored back.  Segments share nothing else.
static inline void adam_step_ref(const int n_seg, float *const *theta, const float *const *grad, float *const *m,
                                 float *const *v, const long long *n, double *state, const float lr, const float beta1,
                                 const float beta2, const float eps) {
  double p1, p2;
  float ic1, ic2;
  pob_adam_bias(state[0], state[1], beta1, beta2, p1, p2, ic1, ic2);
  for (int s = 0; s < n_seg; ++s)
    for (long long i = 0; i < n[s]; ++i) pob_adam_elem(theta[s][i], grad[s][i], m[s][i], v[s][i], lr, beta1, beta2, eps, ic1, ic2);
  state[0] = p1;
  state[1] = p2;
}

// The PPO loss of M minibatch rows: logits (M, 2 A), values (M), u (M, A) the entropy draws
// (uniform(split(key)[1], (M, A), -1, 1) on the device); raw (N, A), old_logp, advantages, vs (N)
// in trajectory order, row i reading trajectory row idx[i] (NULL: i).  dlogits (M, 2 A), dvalues
// (M), partials (n_chunks, 3) may be NULL.  The three sums: rows cut into chunks of POB_PPO_CHUNK,
// a chunk's triple from +0.0 in ascending row order (partials), the chunk partials added in
// ascending chunk order from +0.0 (the order of obsnorm_accumulate_ref).
static inline void ppo_loss_ref(const long long M, const int A, const float *logits, const float *values,
                                const int32_t *idx, const float *raw, const float *old_logp, const float *advantages,
                                const float *vs, const float *u, const float entropy_cost, const float ppo_epsilon,
                                float *dlogits, float *dvalues, float *losses, double *partials) {
  const float inv_m = 1.0f / (float)M;
  const float g_ent = -(entropy_cost * inv_m);
  float f[5 * POB_PPO_MAX_A];
  double T[3] = {0.0, 0.0, 0.0};
  for (long long r0 = 0; r0 < M; r0 += POB_PPO_CHUNK) {
    const long long r1 = r0 + POB_PPO_CHUNK < M ? r0 + POB_PPO_CHUNK : M;
    double S[3] = {0.0, 0.0, 0.0};
    for (long long i = r0; i < r1; ++i) {
      const long long j = idx ? idx[i] : i;
      float logp = 0.0f, ent = 0.0f;
      for (int a = 0; a < A; ++a) {
        float term, en;
        pob_ppo_component(logits[i * 2 * A + a], logits[i * 2 * A + A + a], raw[j * A + a], u[i * A + a], term, en,
                          f[5 * a], f[5 * a + 1], f[5 * a + 2], f[5 * a + 3], f[5 * a + 4]);
        logp = logp + term;
        ent = ent + en;
      }
      float neg_surr, vl, g_lp, dvalue;
      pob_ppo_row(logp, old_logp[j], advantages[j], vs[j], values[i], ppo_epsilon, inv_m, neg_surr, vl, g_lp, dvalue);
      if (dvalues) dvalues[i] = dvalue;
      if (dlogits)
        for (int a = 0; a < A; ++a)
          pob_ppo_grad(g_lp, g_ent, f[5 * a], f[5 * a + 1], f[5 * a + 2], f[5 * a + 3], f[5 * a + 4],
                       dlogits[i * 2 * A + a], dlogits[i * 2 * A + A + a]);
      S[0] = S[0] + (double)neg_surr;
      S[1] = S[1] + (double)vl;
      S[2] = S[2] + (double)ent;
    }
    for (int q = 0; q < 3; ++q) {
      if (partials) partials[(r0 / POB_PPO_CHUNK) * 3 + q] = S[q];
      T[q] = T[q] + S[q];
    }
  }
  pob_ppo_finish(T[0], T[1], T[2], M, entropy_cost, losses);
}

// vs, advantages (T, B) of truncation (NULL: zeros), second, reward, values (T, B) row-major and
// bootstrap (B); either output may be NULL.  Each env on its own, t descending from T - 1.
static inline void gae_ref(const int T, const long long B, const float *truncation, const float *second,
                           const int done_input, const float *reward, const float reward_scale, const float *values,
                           const float *bootstrap, const float lambda, const float discount, float *vs, float *advantages) {
  for (long long b = 0; b < B; ++b) {
    float acc = 0.0f, v_next = bootstrap[b], vs_next = bootstrap[b];
    for (int t = T - 1; t >= 0; --t) {
      const long long i = (long long)t * B + b;
      float adv;
      pob_gae_step(truncation ? truncation[i] : 0.0f, second[i], done_input, reward[i], reward_scale, values[i], lambda,
                   discount, acc, v_next, vs_next, adv);
      if (advantages) advantages[i] = adv;
      if (vs) vs[i] = vs_next;
    }
  }
}

// sums (2, D) float64 of x (N, D) against table row 0 (mean): rows cut into chunks of
// POB_OBSNORM_CHUNK, a chunk's pair per column from +0.0 in ascending row order, the chunk
// partials added per column in ascending chunk order from +0.0.  The order depends on N and D only.
static inline void obsnorm_accumulate_ref(const float *x, const long long N, const int D, const float *table, double *sums) {
  for (int f = 0; f < D; ++f) {
    double T1 = 0.0, T2 = 0.0;
    for (long long r0 = 0; r0 < N; r0 += POB_OBSNORM_CHUNK) {
      const long long r1 = r0 + POB_OBSNORM_CHUNK < N ? r0 + POB_OBSNORM_CHUNK : N;
      double S1 = 0.0, S2 = 0.0;
      for (long long r = r0; r < r1; ++r) pob_obsnorm_step(x[r * D + f], table[f], S1, S2);
      T1 = T1 + S1;
      T2 = T2 + S2;
    }
    sums[f] = T1;
    sums[D + f] = T2;
  }
}
// count, table (3, D) updated in place from sums (R, 2, D), one pair per shard in rank order
// (added per column in ascending r from +0.0), n_new = the row count over all shards.
static inline void obsnorm_update_ref(double *count, float *table, const int D, const double *sums, const int R,
                                      const long long n_new) {
  double total = *count;
  for (int f = 0; f < D; ++f) {
    double S1 = 0.0, S2 = 0.0;
    for (int r = 0; r < R; ++r) {
      S1 = S1 + sums[((long long)r * 2) * D + f];
      S2 = S2 + sums[((long long)r * 2 + 1) * D + f];
    }
    total = pob_obsnorm_finish(*count, (double)n_new, S1, S2, table[f], table[D + f], table[2 * D + f]);
  }
  *count = total;
}
// x (B, D) normalised in place by table rows 0, 1 (NULL: left as it is)
static inline void obsnorm_apply_ref(float *x, const long long B, const int D, const float *table, const float clip) {
  if (!table) return;
  for (long long b = 0; b < B; ++b)
    for (int f = 0; f < D; ++f) x[b * D + f] = pob_obsnorm_apply(x[b * D + f], table[f], table[D + f], clip);
}

// ---------------------------------------------------------------------------- restatement
// theta packing: W_0 (in_0, out_0) row-major, b_0 (out_0), W_1, b_1, ..  (sizes[0] = input)
static inline long long mlp_param_count(const int n_layers, const int *sizes) {
  long long n = 0;
  for (int l = 0; l < n_layers; ++l) n += ((long long)sizes[l] + 1) * sizes[l + 1];
  return n;
}
// y (B, sizes[n_layers]) = the network on x (B, sizes[0])
static inline void mlp_forward_ref(const int n_layers, const int *sizes, const int activation, const int activate_final,
                                   const int B, const float *x, const float *theta, float *y) {
  float a[POB_MLP_MAX_WIDTH + 1], o[POB_MLP_MAX_WIDTH + 1];
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < sizes[0]; ++k) a[k] = x[(long long)b * sizes[0] + k];
    const float *W = theta;
    for (int l = 0; l < n_layers; ++l) {
      const int in = sizes[l], out = sizes[l + 1];
      const float *bias = W + (long long)in * out;
      for (int j = 0; j < out; ++j) {
        float acc = bias[j];
        for (int s = 0; s < mlp_ksteps(in); ++s)
          for (int h = 0; h < 2; ++h) {
            const int k = mlp_kfeat(s, h);
            acc = k < in ? MLP_FMA(W[(long long)k * out + j], a[k], acc) : MLP_FMA(0.0f, 0.0f, acc);
          }
        o[j] = (l != n_layers - 1 || activate_final) ? mlp_activate(activation, acc) : acc;
      }
      for (int j = 0; j < out; ++j) a[j] = o[j];
      W = bias + out;
    }
    for (int j = 0; j < sizes[n_layers]; ++j) y[(long long)b * sizes[n_layers] + j] = a[j];
  }
}
// ---- the training forward and the backward pass (DESIGN.md "MLP backward"; k_mlp_forward_train,
// k_mlp_bwd_delta, k_mlp_bwd_weights, k_mlp_bwd_reduce).  Layer l is ACTIVATED when l != n_layers
// - 1 || activate_final.  saved holds the pre-activation z_l (M, sizes[l + 1]) row-major of every
// activated layer, the layers one after the other in ascending l.
static inline bool mlp_layer_activated(const int n_layers, const int activate_final, const int l) {
  return l != n_layers - 1 || activate_final;
}
static inline long long mlp_saved_count(const int n_layers, const int *sizes, const int activate_final, const long long M) {
  long long n = 0;
  for (int l = 0; l < n_layers; ++l)
    if (mlp_layer_activated(n_layers, activate_final, l)) n += M * sizes[l + 1];
  return n;
}
// y = mlp_forward_ref's (the same chain), saved = the pre-activations
static inline void mlp_forward_train_ref(const int n_layers, const int *sizes, const int activation,
                                         const int activate_final, const long long M, const float *x, const float *theta,
                                         float *y, float *saved) {
  float a[POB_MLP_MAX_WIDTH + 1], o[POB_MLP_MAX_WIDTH + 1];
  for (long long b = 0; b < M; ++b) {
    for (int k = 0; k < sizes[0]; ++k) a[k] = x[b * sizes[0] + k];
    const float *W = theta;
    float *sv = saved;
    for (int l = 0; l < n_layers; ++l) {
      const int in = sizes[l], out = sizes[l + 1];
      const float *bias = W + (long long)in * out;
      const bool activate = mlp_layer_activated(n_layers, activate_final, l);
      for (int j = 0; j < out; ++j) {
        float acc = bias[j];
        for (int s = 0; s < mlp_ksteps(in); ++s)
          for (int h = 0; h < 2; ++h) {
            const int k = mlp_kfeat(s, h);
            acc = k < in ? MLP_FMA(W[(long long)k * out + j], a[k], acc) : MLP_FMA(0.0f, 0.0f, acc);
          }
        if (activate) sv[b * out + j] = acc;
        o[j] = activate ? mlp_activate(activation, acc) : acc;
      }
      for (int j = 0; j < out; ++j) a[j] = o[j];
      if (activate) sv += M * out;
      W = bias + out;
    }
    for (int j = 0; j < sizes[n_layers]; ++j) y[b * sizes[n_layers] + j] = a[j];
  }
}
// One element of a parameter gradient: sum over the M rows of a[r] d[r] (a: stride lda, NULL = the
// constant 1.0f of the bias row; d: stride ldd).  Rows are cut into tiles of 32, a tile's partial
// is the float32 chain acc = +0, acc = fmaf(a[r], d[r], acc) in ascending r (sixteen k-steps of the
// 32x32x2 instruction with the row as k, the order of mlp_kfeat); tile partials are added in
// float64 in ascending order from +0.0 inside chunks of POB_MLP_BWD_CHUNK rows, the chunk partials
// in float64 in ascending order from +0.0, and the total is rounded to float32 once.  Rows past M
// add nothing: an accumulator started at +0 is not -0 (but for one corner, below), so the
// instruction's fmaf(0, 0, acc) of a padded row (or of an odd width's pad in the propagated
// gradient) changes no bit and is not spelled.  The corner: a product that underflows can round
// +0 to -0.  Here the float64 addition from +0.0 removes it again; in the propagated gradient of
// an odd out whose last product so underflows (a delta far below 2^-100) the kernel's pad gives +0
// where mlp_backward_ref keeps -0.  partials (may be NULL) receives the chunk partials.
static inline float mlp_bwd_sum(const long long M, const float *a, const long long lda, const float *d, const long long ldd,
                                double *partials) {
  double total = 0.0;
  for (long long c0 = 0; c0 < M; c0 += POB_MLP_BWD_CHUNK) {
    const long long c1 = c0 + POB_MLP_BWD_CHUNK < M ? c0 + POB_MLP_BWD_CHUNK : M;
    double chunk = 0.0;
    for (long long t0 = c0; t0 < c1; t0 += 32) {
      const long long t1 = t0 + 32 < c1 ? t0 + 32 : c1;
      float acc = 0.0f;
      for (long long r = t0; r < t1; ++r) acc = MLP_FMA(a ? a[r * lda] : 1.0f, d[r * ldd], acc);
      chunk = chunk + (double)acc;
    }
    if (partials) partials[c0 / POB_MLP_BWD_CHUNK] = chunk;
    total = total + chunk;
  }
  return (float)total;
}
// dtheta (mlp_param_count floats, theta's packing: layer l's block is an (in + 1, out) matrix whose
// last row is the bias) and dx (M, sizes[0]; may be NULL) from dy (M, sizes[n_layers]), x, theta and
// the training forward's saved.  l descending from n_layers - 1 with g = dy above the last layer:
//   delta[r][j] = mlp_activate_grad(z_l[r][j], g[r][j]) if layer l is activated, else g[r][j]
//   dtheta_l[i][j] = mlp_bwd_sum over r of a[r][i] delta[r][j]; a = layer l's input: x for l = 0,
//     else mlp_activate(z_{l-1}[r][i]) recomputed (the forward's bits); row i = in: the constant 1
//   g[r][i] = sum_j W_l[i][j] delta[r][j]: acc = +0, one fmaf(W_l[i][j], delta[r][j], acc) per j in
//     natural order (the k order of mlp_kfeat over the output features); dx = g of layer 0
// delta_out (may be NULL) receives every layer's delta (M, sizes[l + 1]), ascending l.  Returns
// 0, or -1 when its buffers cannot be allocated.
static inline int mlp_backward_ref(const int n_layers, const int *sizes, const int activation, const int activate_final,
                                   const long long M, const float *x, const float *theta, const float *saved,
                                   const float *dy, float *dtheta, float *dx, float *delta_out) {
  float *delta = (float *)malloc(sizeof(float) * M * POB_MLP_MAX_WIDTH);
  float *g = (float *)malloc(sizeof(float) * M * POB_MLP_MAX_WIDTH);
  float *a = (float *)malloc(sizeof(float) * M * POB_MLP_MAX_WIDTH);
  if (!delta || !g || !a) { free(delta); free(g); free(a); return -1; }
  long long woff = mlp_param_count(n_layers, sizes), soff = mlp_saved_count(n_layers, sizes, activate_final, M), doff = 0;
  for (int l = 0; l < n_layers; ++l) doff += M * sizes[l + 1];
  for (long long e = 0; e < M * sizes[n_layers]; ++e) g[e] = dy[e];
  for (int l = n_layers - 1; l >= 0; --l) {
    const int in = sizes[l], out = sizes[l + 1];
    woff -= ((long long)in + 1) * out;
    doff -= M * out;
    const float *W = theta + woff;
    if (mlp_layer_activated(n_layers, activate_final, l)) {
      soff -= M * out;
      for (long long e = 0; e < M * out; ++e) delta[e] = mlp_activate_grad(activation, saved[soff + e], g[e]);
    } else {
      for (long long e = 0; e < M * out; ++e) delta[e] = g[e];
    }
    if (delta_out)
      for (long long e = 0; e < M * out; ++e) delta_out[doff + e] = delta[e];
    if (l == 0) {
      for (long long e = 0; e < M * in; ++e) a[e] = x[e];
    } else {  // z_{l-1} lies right below z_l in saved
      const float *zp = saved + (soff - M * in);
      for (long long e = 0; e < M * in; ++e) a[e] = mlp_activate(activation, zp[e]);
    }
    for (int i = 0; i <= in; ++i)
      for (int j = 0; j < out; ++j)
        dtheta[woff + (long long)i * out + j] = mlp_bwd_sum(M, i < in ? a + i : NULL, in, delta + j, out, NULL);
    if (l > 0 || dx) {
      float *dst = l > 0 ? g : dx;
      for (long long r = 0; r < M; ++r)
        for (int i = 0; i < in; ++i) {
          float acc = 0.0f;
          for (int j = 0; j < out; ++j) acc = MLP_FMA(W[(long long)i * out + j], delta[r * out + j], acc);
          dst[r * in + i] = acc;
        }
    }
  }
  free(delta); free(g); free(a);
  return 0;
}

// The actor on rows of logits (B, 2 A) and the uniform draws u (B, A); logp sums the terms in
// natural order a = 0 .. A - 1 from +0.  Deterministic: action = tanh(loc), raw = loc, logp
// is not written.
static inline void policy_head_ref(const int B, const int A, const float *logits, const float *u, const int deterministic,
                                   float *action, float *logp, float *raw) {
  for (int b = 0; b < B; ++b) {
    float sum = 0.0f;
    for (int a = 0; a < A; ++a) {
      const float loc = logits[(long long)b * 2 * A + a], s = logits[(long long)b * 2 * A + A + a];
      float act, rw, term;
      if (deterministic) {
        act = pob_tanhf(loc); rw = loc;
      } else {
        pob_tanh_normal(loc, s, u[(long long)b * A + a], act, rw, term);
        sum = sum + term;
      }
      action[(long long)b * A + a] = act;
      raw[(long long)b * A + a] = rw;
    }
    if (!deterministic) logp[b] = sum;
  }
}

// ---------------------------------------------------------------------------- recurrent actor
// obs -> pre-MLP (n_pre layers, pre_sizes[0] = obs width, activation after every one) -> GRU
// cell (hidden width H, input x of width I = pre_sizes[n_pre]) -> post-MLP (n_post layers of
// widths post_sizes[0 .. n_post), activation after all but the last).  theta: the pre-MLP's W, b
// pairs, W_rz (I + H, 2 H), b_rz (2 H), W_xn (I, H), b_xn (H), W_hn (H, H), b_hn (H), the
// post-MLP's pairs; every matrix row-major (in, out).  The cell, with c = [x ; h]:
//   r[j]  = sigmoid(b_rz[j]     + sum_k c[k] W_rz[k][j])
//   z[j]  = sigmoid(b_rz[H + j] + sum_k c[k] W_rz[k][H + j])
//   cx[j] = b_xn[j] + sum_k x[k] W_xn[k][j],   ch[j] = b_hn[j] + sum_k h[k] W_hn[k][j]
//   n[j]  = tanh(fmaf(r[j], ch[j], cx[j])),    h'[j] = fmaf(z[j], h[j] - n[j], n[j])
// every sum the chain of mlp_chain_ref (DESIGN.md "Recurrent actor").
static inline long long gru_param_count(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                        const int *post_sizes) {
  long long n = 0;
  for (int l = 0; l < n_pre; ++l) n += ((long long)pre_sizes[l] + 1) * pre_sizes[l + 1];
  const long long I = pre_sizes[n_pre];
  n += 3 * H * I + 3LL * H * H + 4 * H;
  int in = H;
  for (int l = 0; l < n_post; ++l) { n += ((long long)in + 1) * post_sizes[l]; in = post_sizes[l]; }
  return n;
}
// the chain of mlp_forward_ref: bias, then one fmaf per feature of `a` (width in) in natural
// order, column j of W (row stride ldw), an odd length padded with fmaf(0, 0, acc)
static inline float mlp_chain_ref(const float bias, const float *W, const int ldw, const int j, const float *a, const int in) {
  float acc = bias;
  for (int s = 0; s < mlp_ksteps(in); ++s)
    for (int h = 0; h < 2; ++h) {
      const int k = mlp_kfeat(s, h);
      acc = k < in ? MLP_FMA(W[(long long)k * ldw + j], a[k], acc) : MLP_FMA(0.0f, 0.0f, acc);
    }
  return acc;
}
// One env's cell: c = [x ; h] (I + H contiguous floats), g = the GRU block of theta.  Writes
// r, z, cx, ch, hn (H each).
static inline void gru_cell_ref(const int I, const int H, const float *c, const float *g, float *r, float *z, float *cx,
                                float *ch, float *hn) {
  const float *W_rz = g, *b_rz = W_rz + (long long)(I + H) * 2 * H;
  const float *W_xn = b_rz + 2 * H, *b_xn = W_xn + (long long)I * H;
  const float *W_hn = b_xn + H, *b_hn = W_hn + (long long)H * H;
  for (int j = 0; j < H; ++j) {
    r[j] = pob_sigmoidf(mlp_chain_ref(b_rz[j], W_rz, 2 * H, j, c, I + H));
    z[j] = pob_sigmoidf(mlp_chain_ref(b_rz[H + j], W_rz, 2 * H, H + j, c, I + H));
    cx[j] = mlp_chain_ref(b_xn[j], W_xn, H, j, c, I);
    ch[j] = mlp_chain_ref(b_hn[j], W_hn, H, j, c + I, H);
    const float n = pob_tanhf(MLP_FMA(r[j], ch[j], cx[j]));
    hn[j] = MLP_FMA(z[j], c[I + j] - n, n);
  }
}
// y (B, post_sizes[n_post - 1]), h_out (B, H) = the network on x (B, pre_sizes[0]) and h_in (B, H);
// reset (B) may be NULL: where reset[b] != 0 (a NaN too) env b starts from h = +0.  h_in_copy
// (B, H, may be NULL) receives the h the step started from, after the reset.  h_out may be h_in.
static inline void gru_forward_ref(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                   const int *post_sizes, const int activation, const int B, const float *x,
                                   const float *theta, const float *reset, const float *h_in, float *y, float *h_out,
                                   float *h_in_copy) {
  float a[POB_MLP_MAX_WIDTH + 1], o[POB_MLP_MAX_WIDTH + 1], c[POB_MLP_MAX_WIDTH + 1];
  float r[POB_GRU_MAX_HIDDEN], z[POB_GRU_MAX_HIDDEN], cx[POB_GRU_MAX_HIDDEN], ch[POB_GRU_MAX_HIDDEN], hn[POB_GRU_MAX_HIDDEN];
  const int D = pre_sizes[0], I = pre_sizes[n_pre], out_w = post_sizes[n_post - 1];
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < D; ++k) a[k] = x[(long long)b * D + k];
    const float *W = theta;
    for (int l = 0; l < n_pre; ++l) {
      const int in = pre_sizes[l], out = pre_sizes[l + 1];
      const float *bias = W + (long long)in * out;
      for (int j = 0; j < out; ++j) o[j] = mlp_activate(activation, mlp_chain_ref(bias[j], W, out, j, a, in));
      for (int j = 0; j < out; ++j) a[j] = o[j];
      W = bias + out;
    }
    for (int k = 0; k < I; ++k) c[k] = a[k];
    const bool zero = reset && reset[b] != 0.0f;
    for (int k = 0; k < H; ++k) {
      c[I + k] = zero ? 0.0f : h_in[(long long)b * H + k];
      if (h_in_copy) h_in_copy[(long long)b * H + k] = c[I + k];
    }
    gru_cell_ref(I, H, c, W, r, z, cx, ch, hn);
    W += 3LL * H * I + 3LL * H * H + 4 * H;
    for (int k = 0; k < H; ++k) { h_out[(long long)b * H + k] = hn[k]; a[k] = hn[k]; }
    int in = H;
    for (int l = 0; l < n_post; ++l) {
      const int out = post_sizes[l];
      const float *bias = W + (long long)in * out;
      for (int j = 0; j < out; ++j) {
        const float acc = mlp_chain_ref(bias[j], W, out, j, a, in);
        o[j] = l != n_post - 1 ? mlp_activate(activation, acc) : acc;
      }
      for (int j = 0; j < out; ++j) a[j] = o[j];
      W = bias + out;
      in = out;
    }
    for (int j = 0; j < out_w; ++j) y[(long long)b * out_w + j] = a[j];
  }
}
// The recurrent actor: gru_forward_ref's y is the logits (B, 2 A), then policy_head_ref on the
// uniform draws u (B, A).
static inline void gru_policy_ref(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                  const int *post_sizes, const int activation, const int B, const float *obs,
                                  const float *theta, const float *reset, const float *h_in, const float *u,
                                  const int deterministic, float *logits, float *h_out, float *h_in_copy, float *action,
                                  float *logp, float *raw) {
  gru_forward_ref(n_pre, pre_sizes, H, n_post, post_sizes, activation, B, obs, theta, reset, h_in, logits, h_out, h_in_copy);
  policy_head_ref(B, post_sizes[n_post - 1] >> 1, logits, u, deterministic, action, logp, raw);
}
#endif

// ---------------------------------------------------------------------------- recurrent backward
// The training forward of the recurrent network over a window of T steps and its truncated
// backward pass through time (DESIGN.md "Recurrent backward"; k_gru_seq_forward,
// k_gru_seq_backward, k_gru_bwd_weights).  R = T M rows in the flat order r = t M + m.  What the
// forward keeps, as float offsets into `saved`, every array (R, width) row-major:
//   xin   the normalised observation rows (R, D), only under a pre-MLP
//   pre   the pre-MLP's pre-activations, mlp_forward_train_ref's layout (every layer activated)
//   xc    the cell's input x (R, I): the pre-MLP's output, or the normalised observation
//   hin   the h each step started from, after the reset (R, H)
//   gate  r, z, ch, n (R, 4 H): four runs of H per row
//   hn    h' (R, H)
//   post  the post-MLP's pre-activations (its last layer is not activated)
// and the backward's delta arrays, as float offsets into its workspace: the pre-MLP's layers
// (R, pre[l + 1]) ascending, the cell's (R, 4 H) = delta_r, delta_z, delta_xn, delta_hn, the
// post-MLP's layers (R, post[l]) ascending; `n_delta` floats in all, the float64 chunk partials
// (n_chunks, n_params) behind them at the next multiple of 8 bytes.
struct gru_seq_plan {
  long long xin, pre, xc, hin, gate, hn, post, n_saved;
  long long d_pre, d_cell, d_post, n_delta;
};
static inline gru_seq_plan gru_seq_layout(const int n_pre, const int *pre, const int H, const int n_post, const int *post,
                                          const long long R) {
  gru_seq_plan p;
  const long long D = pre[0], I = pre[n_pre];
  long long o = 0, e = 0;
  p.xin = o; if (n_pre) o += R * D;
  p.pre = o; p.d_pre = e;
  for (int l = 0; l < n_pre; ++l) { o += R * pre[l + 1]; e += R * pre[l + 1]; }
  p.xc = o; o += R * I;
  p.hin = o; o += R * H;
  p.gate = o; o += R * 4 * H;
  p.hn = o; o += R * H;
  p.post = o; p.d_cell = e; e += R * 4 * H;
  p.d_post = e;
  for (int l = 0; l < n_post; ++l) { if (l != n_post - 1) o += R * post[l]; e += R * post[l]; }
  p.n_saved = o; p.n_delta = e;
  return p;
}
// The element-wise part of the cell's backward pass for one feature: g = the gradient arriving at
// h', hin the h the step started from.  One rounding per spelled operation; r, z, n are the
// forward's values, never another spelling of sigmoid or tanh.
POB_MLP_D void pob_gru_cell_grad(const float g, const float hin, const float r, const float z, const float ch, const float n,
                                 float &d_r, float &d_z, float &d_xn, float &d_hn) {
  const float omz = 1.0f - z;
  const float dz = g * (hin - n);
  const float dn = g * omz;
  const float ds = dn * MLP_FMA(-n, n, 1.0f);
  d_xn = ds;
  d_hn = ds * r;
  d_r = ((ds * ch) * r) * (1.0f - r);
  d_z = (dz * z) * omz;
}

#ifdef POB_MLP_HOST
// y (T, M, out), h_last (M, H; may be NULL) and saved (gru_seq_layout's n_saved floats) of the
// window: obs (T, B, D) and reset (T, B; may be NULL) are read in place, sequence m being env
// idx[m] (NULL: m, M == B); h0 (B, H); norm (3, D) may be NULL.  Step t is gru_forward_ref on the
// gathered, normalised rows from the h' of step t - 1 (h0 at t = 0): the same chains.
static inline void gru_sequence_forward_train_ref(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                                  const int *post_sizes, const int activation, const int T, const long long M,
                                                  const long long B, const float *obs, const int32_t *idx, const float *h0,
                                                  const float *reset, const float *norm, const float norm_clip,
                                                  const float *theta, float *y, float *h_last, float *saved) {
  float a[POB_MLP_MAX_WIDTH + 1], o[POB_MLP_MAX_WIDTH + 1], c[POB_MLP_MAX_WIDTH + 1];
  float r[POB_GRU_MAX_HIDDEN], z[POB_GRU_MAX_HIDDEN], cx[POB_GRU_MAX_HIDDEN], ch[POB_GRU_MAX_HIDDEN], hn[POB_GRU_MAX_HIDDEN];
  float h[POB_GRU_MAX_HIDDEN];
  const int D = pre_sizes[0], I = pre_sizes[n_pre], out_w = post_sizes[n_post - 1];
  const long long R = (long long)T * M;
  const gru_seq_plan p = gru_seq_layout(n_pre, pre_sizes, H, n_post, post_sizes, R);
  for (long long m = 0; m < M; ++m) {
    const long long b = idx ? idx[m] : m;
    for (int k = 0; k < H; ++k) h[k] = h0[b * H + k];
    for (int t = 0; t < T; ++t) {
      const long long row = (long long)t * M + m;
      for (int k = 0; k < D; ++k) {
        const float v = obs[((long long)t * B + b) * D + k];
        a[k] = norm ? pob_obsnorm_apply(v, norm[k], norm[D + k], norm_clip) : v;
        if (n_pre) saved[p.xin + row * D + k] = a[k];
      }
      const float *W = theta;
      long long so = p.pre;
      for (int l = 0; l < n_pre; ++l) {
        const int in = pre_sizes[l], out = pre_sizes[l + 1];
        const float *bias = W + (long long)in * out;
        for (int j = 0; j < out; ++j) {
          const float acc = mlp_chain_ref(bias[j], W, out, j, a, in);
          saved[so + row * out + j] = acc;
          o[j] = mlp_activate(activation, acc);
        }
        for (int j = 0; j < out; ++j) a[j] = o[j];
        so += R * out;
        W = bias + out;
      }
      const bool zero = reset && reset[(long long)t * B + b] != 0.0f;
      for (int k = 0; k < I; ++k) { c[k] = a[k]; saved[p.xc + row * I + k] = a[k]; }
      for (int k = 0; k < H; ++k) { c[I + k] = zero ? 0.0f : h[k]; saved[p.hin + row * H + k] = c[I + k]; }
      gru_cell_ref(I, H, c, W, r, z, cx, ch, hn);
      W += 3LL * H * I + 3LL * H * H + 4 * H;
      for (int k = 0; k < H; ++k) {
        float *gt = saved + p.gate + row * 4 * H;
        gt[k] = r[k]; gt[H + k] = z[k]; gt[2 * H + k] = ch[k];
        // n is not among gru_cell_ref's outputs: the same expression, hence the same bits
        gt[3 * H + k] = pob_tanhf(MLP_FMA(r[k], ch[k], cx[k]));
        saved[p.hn + row * H + k] = hn[k];
        h[k] = hn[k]; a[k] = hn[k];
      }
      int in = H;
      so = p.post;
      for (int l = 0; l < n_post; ++l) {
        const int out = post_sizes[l];
        const float *bias = W + (long long)in * out;
        for (int j = 0; j < out; ++j) {
          const float acc = mlp_chain_ref(bias[j], W, out, j, a, in);
          if (l != n_post - 1) saved[so + row * out + j] = acc;
          o[j] = l != n_post - 1 ? mlp_activate(activation, acc) : acc;
        }
        for (int j = 0; j < out; ++j) a[j] = o[j];
        if (l != n_post - 1) so += R * out;
        W = bias + out;
        in = out;
      }
      for (int j = 0; j < out_w; ++j) y[row * out_w + j] = a[j];
    }
    if (h_last)
      for (int k = 0; k < H; ++k) h_last[m * H + k] = h[k];
  }
}

// The window without the training arrays (k_gru_seq_infer; DESIGN.md "Recurrent critic"): S chained
// gru_forward_ref steps on the gathered, normalised rows.  obs (S, B, D), reset (S, B; may be
// NULL), idx, h0 (B, H), norm as above; y (S, M, out).  h_first (M, H; may be NULL): the state step 0
// started from, after step 0's reset (the step's h_in_copy).  h_out (M, H; may be NULL): the state
// after h_out_step steps (1 .. S), before step h_out_step's reset; without idx it may be h0 itself
// (h0 is read out before anything is written).  Returns 0, or -1 when its buffers cannot be allocated.
static inline int gru_sequence_forward_ref(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                           const int *post_sizes, const int activation, const int S, const long long M,
                                           const long long B, const float *obs, const int32_t *idx, const float *h0,
                                           const float *reset, const float *norm, const float norm_clip,
                                           const float *theta, float *y, float *h_first, float *h_out,
                                           const int h_out_step) {
  const int D = pre_sizes[0], out_w = post_sizes[n_post - 1];
  float *x = (float *)malloc(sizeof(float) * M * D), *rs = (float *)malloc(sizeof(float) * M);
  float *h = (float *)malloc(sizeof(float) * M * H);
  if (!x || !rs || !h) { free(x); free(rs); free(h); return -1; }
  for (long long m = 0; m < M; ++m)
    for (int k = 0; k < H; ++k) h[m * H + k] = h0[(idx ? idx[m] : m) * H + k];
  for (int s = 0; s < S; ++s) {
    for (long long m = 0; m < M; ++m) {
      const long long b = idx ? idx[m] : m;
      for (int k = 0; k < D; ++k) x[m * D + k] = obs[((long long)s * B + b) * D + k];
      rs[m] = reset ? reset[(long long)s * B + b] : 0.0f;
    }
    obsnorm_apply_ref(x, M, D, norm, norm_clip);
    gru_forward_ref(n_pre, pre_sizes, H, n_post, post_sizes, activation, (int)M, x, theta, rs, h, y + (long long)s * M * out_w,
                    h, s == 0 ? h_first : NULL);
    if (h_out && s + 1 == h_out_step)
      for (long long i = 0; i < M * H; ++i) h_out[i] = h[i];
  }
  free(x); free(rs); free(h);
  return 0;
}

// dtheta (gru_param_count floats, theta's packing: every block an (in + 1, out) matrix whose last
// row is the bias) and dh0 (M, H; may be NULL) from dy (T, M, out), dh_last (M, H; NULL: zeros),
// theta and the forward's saved.  reset (T, B; may be NULL) and idx as in the forward.
//   post-MLP: mlp_backward_ref over the R rows (input hn, activate_final = 0); its dx = g_post
//   cell, t descending, carry[m] = dh_last[m] (or +0) before t = T - 1:
//     g_h = g_post[r] + carry;  pob_gru_cell_grad(g_h, hin, r, z, ch, n) -> the row's four deltas
//     acc = +0; acc = fmaf(W_rz[I + i][j], delta_rz[j], acc) for j = 0 .. 2 H - 1 (delta_rz =
//       [delta_r ; delta_z]), then acc = fmaf(W_hn[i][j], delta_hn[j], acc) for j = 0 .. H - 1;
//       carry[i] = fmaf(g_h[i], z[i], acc), or +0 where reset[t][b] != 0 (a NaN too)
//     g_x[k] (under a pre-MLP): acc = +0, the same chain over W_rz[k][.] and delta_rz, then over
//       W_xn[k][.] and delta_xn
//   cell blocks of dtheta: mlp_bwd_sum over the R rows of ([xc ; hin], delta_rz), (xc, delta_xn),
//     (hin, delta_hn), the bias rows with the constant 1
//   pre-MLP: mlp_backward_ref over the R rows (input xin, activate_final = 1, dy = g_x, no dx)
//   dh0 = the carry after t = 0
// delta_out (may be NULL) receives the workspace's delta arrays (gru_seq_layout's n_delta floats).
// Returns 0, or -1 when its buffers cannot be allocated.
static inline int gru_sequence_backward_ref(const int n_pre, const int *pre_sizes, const int H, const int n_post,
                                            const int *post_sizes, const int activation, const int T, const long long M,
                                            const long long B, const int32_t *idx, const float *reset, const float *theta,
                                            const float *saved, const float *dy, const float *dh_last, float *dtheta,
                                            float *dh0, float *delta_out) {
  const int I = pre_sizes[n_pre];
  const long long R = (long long)T * M;
  const gru_seq_plan p = gru_seq_layout(n_pre, pre_sizes, H, n_post, post_sizes, R);
  float *delta = (float *)malloc(sizeof(float) * (p.n_delta + 1));
  float *g_post = (float *)malloc(sizeof(float) * R * H);
  float *g_x = (float *)malloc(sizeof(float) * (R * I + 1));
  float *carry = (float *)malloc(sizeof(float) * M * H);
  if (!delta || !g_post || !g_x || !carry) { free(delta); free(g_post); free(g_x); free(carry); return -1; }
  long long w_cell = 0;
  for (int l = 0; l < n_pre; ++l) w_cell += ((long long)pre_sizes[l] + 1) * pre_sizes[l + 1];
  const long long w_post = w_cell + 3LL * H * I + 3LL * H * H + 4 * H;
  int rc = 0;
  {
    int sizes[POB_GRU_MAX_POST + 1];
    sizes[0] = H;
    for (int l = 0; l < n_post; ++l) sizes[l + 1] = post_sizes[l];
    rc = mlp_backward_ref(n_post, sizes, activation, 0, R, saved + p.hn, theta + w_post, saved + p.post, dy, dtheta + w_post,
                          g_post, delta + p.d_post);
  }
  const float *W_rz = theta + w_cell, *W_xn = W_rz + (long long)(I + H) * 2 * H + 2 * H;
  const float *W_hn = W_xn + (long long)I * H + H;
  float *dc = delta + p.d_cell;
  for (long long e = 0; e < M * H; ++e) carry[e] = dh_last ? dh_last[e] : 0.0f;
  for (int t = T - 1; t >= 0 && !rc; --t)
    for (long long m = 0; m < M; ++m) {
      const long long row = (long long)t * M + m, b = idx ? idx[m] : m;
      const float *gt = saved + p.gate + row * 4 * H, *hin = saved + p.hin + row * H;
      float *d = dc + row * 4 * H, g_h[POB_GRU_MAX_HIDDEN];
      for (int j = 0; j < H; ++j) {
        g_h[j] = g_post[row * H + j] + carry[m * H + j];
        pob_gru_cell_grad(g_h[j], hin[j], gt[j], gt[H + j], gt[2 * H + j], gt[3 * H + j], d[j], d[H + j], d[2 * H + j],
                          d[3 * H + j]);
      }
      const bool zero = reset && reset[(long long)t * B + b] != 0.0f;
      for (int i = 0; i < H; ++i) {
        float acc = 0.0f;
        for (int j = 0; j < 2 * H; ++j) acc = MLP_FMA(W_rz[(long long)(I + i) * 2 * H + j], d[j], acc);
        for (int j = 0; j < H; ++j) acc = MLP_FMA(W_hn[(long long)i * H + j], d[3 * H + j], acc);
        carry[m * H + i] = zero ? 0.0f : MLP_FMA(g_h[i], gt[H + i], acc);
      }
      if (n_pre)
        for (int k = 0; k < I; ++k) {
          float acc = 0.0f;
          for (int j = 0; j < 2 * H; ++j) acc = MLP_FMA(W_rz[(long long)k * 2 * H + j], d[j], acc);
          for (int j = 0; j < H; ++j) acc = MLP_FMA(W_xn[(long long)k * H + j], d[2 * H + j], acc);
          g_x[row * I + k] = acc;
        }
    }
  if (!rc) {
    const float *xc = saved + p.xc, *hin = saved + p.hin;
    float *d_rz = dtheta + w_cell, *d_xn = d_rz + (long long)(I + H + 1) * 2 * H, *d_hn = d_xn + (long long)(I + 1) * H;
    for (int i = 0; i <= I + H; ++i)
      for (int j = 0; j < 2 * H; ++j) {
        const float *a = i < I ? xc + i : (i < I + H ? hin + (i - I) : NULL);
        d_rz[(long long)i * 2 * H + j] = mlp_bwd_sum(R, a, i < I ? I : H, dc + j, 4 * H, NULL);
      }
    for (int i = 0; i <= I; ++i)
      for (int j = 0; j < H; ++j) d_xn[(long long)i * H + j] = mlp_bwd_sum(R, i < I ? xc + i : NULL, I, dc + 2 * H + j, 4 * H, NULL);
    for (int i = 0; i <= H; ++i)
      for (int j = 0; j < H; ++j) d_hn[(long long)i * H + j] = mlp_bwd_sum(R, i < H ? hin + i : NULL, H, dc + 3 * H + j, 4 * H, NULL);
    if (n_pre)
      rc = mlp_backward_ref(n_pre, pre_sizes, activation, 1, R, saved + p.xin, theta, saved + p.pre, g_x, dtheta, NULL,
                            delta + p.d_pre);
    if (dh0)
      for (long long e = 0; e < M * H; ++e) dh0[e] = carry[e];
    if (delta_out)
      for (long long e = 0; e < p.n_delta; ++e) delta_out[e] = delta[e];
  }
  free(delta); free(g_post); free(g_x); free(carry);
  return rc;
}
#endif
