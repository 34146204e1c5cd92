/* pob.h -- C ABI of the MI355X-native po-brax rollout engine (libpob.so).
 *
 * The reference (po_brax, pure Python over brax v1 / JAX) has no native FFI; its
 * drop-in surface for this path is the brax ``Env`` API.  Each entry point below
 * replaces one JAX sub-graph of that surface (file:line in /root/reference):
 *
 *   pob_env_create      AntHeavenHellEnv.__init__  po_brax/envs/ant_heavenhell.py:51-73
 *                       AntGatherEnv.__init__      po_brax/envs/ant_gather.py:59-91
 *                       AntTagEnv.__init__         po_brax/envs/ant_tag.py:38-61
 *                       stock brax Ant             po_brax/envs/__init__.py:30 ('ant' ->
 *                                                  brax.envs.ant.Ant, brax <= 0.0.12) [ext]
 *                       (+ brax.System(cfg) [ext], ActionRepeatWrapper wrappers.py:16-24)
 *   pob_reset           Env.reset: ant_heavenhell.py:75-103, ant_gather.py:93-123,
 *                       ant_tag.py:63-105 ; EpisodeWrapper.reset / AutoResetWrapper.reset
 *                       [ext]; VmapGymWrapper reset closure wrappers.py:160-164
 *   pob_step            Env.step: ant_heavenhell.py:106-158, ant_gather.py:125-213,
 *                       ant_tag.py:107-181, incl. brax System.step [ext] and the
 *                       Episode/AutoReset/RandomizedAutoReset wrappers (__init__.py:59-70,
 *                       wrappers.py:30-123)
 *   pob_step_mixed      several of the above Env.step calls (different env kinds, one
 *                       batch each) fused into ONE kernel launch (BASELINE.json config 5)
 *   pob_reset_where_done AutoresetVmapGymWrapper.step tail wrappers.py:245-262 and
 *                       RandomizedAutoResetWrapperNaive/OnTerminal wrappers.py:30-80
 *   pob_reset_where_done_shard  the same tail for one rank's shard of the gym batch
 *                       (global keys split(gym_key, B_total + 1), all-reduced any-done)
 *   pob_default_qp      System.default_qp(joint_angle, joint_velocity) [ext], called at
 *                       ant_heavenhell.py:95, ant_gather.py:116, ant_tag.py:72
 *   pob_random_*        brax.jumpy.random_split / random_uniform under jit ->
 *                       jax.random.split / uniform (threefry2x32) [ext]; more_jp.py:57-77;
 *                       pob_random_split_batch = the per-env split of
 *                       RandomizedAutoResetWrapperCached.step wrappers.py:103
 *   pob_obs_gather      obs[:, idx] with the index sets of
 *                       po_brax/standard_observability_masks.py:5-67
 *   pob_env_set_obs_mask  the same gather fused into pob_step (pob_state.obs_masked)
 *
 * Conventions: every pointer argument of a compute call is DEVICE memory owned by the
 * caller (the library allocates only its static tables at create time and never per
 * step).  Layouts are the reference's batch-major pytree layouts: pos (B,N,3),
 * rot (B,N,4) wxyz, vel/ang (B,N,3), obs (B,D), keys (B,2) uint32.  `stream` is a
 * hipStream_t (NULL = default stream); calls are stream-ordered and never synchronise
 * the host.  Return value 0 = success, else a negative status; pob_last_error() gives
 * a thread-local message.
 */
#ifndef POB_H
#define POB_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POB_ABI_VERSION 8

enum pob_kind { POB_HEAVENHELL = 0, POB_GATHER = 1, POB_TAG = 2, POB_ANT = 3 };

/* storage type of the qp tensors (pos/rot/vel/ang and first_qp); compute is float32 */
enum pob_qp_storage { POB_QP_F32 = 0, POB_QP_F16 = 1 };

#define POB_MIX_MAX 4 /* envs per pob_step_mixed launch */

enum pob_status {
  POB_OK = 0,
  POB_EINVAL = -1,   /* bad argument (ValueError on the Python side) */
  POB_EHIP = -2,     /* HIP runtime error (RuntimeError) */
  POB_ENOMEM = -3,
};

/* step flags: the wrapper chain of po_brax.envs.create (__init__.py:59-70) */
enum pob_step_flags {
  POB_F_EPISODE = 1u,         /* brax EpisodeWrapper: steps += 1, time-limit done, truncation */
  POB_F_AUTORESET = 2u,       /* brax AutoResetWrapper: zero steps on prev done, first_qp/obs */
  POB_F_ZERO_STEPS_ON_DONE = 4u, /* RandomizedAutoResetWrapper*: zero steps on prev done only */
};

/* reset_where_done modes */
enum pob_reset_mode {
  POB_RESET_GYM = 0,  /* keys = split(gym_key, B+1)[1:], gym_key <- keys[0] if any done */
  POB_RESET_OWN = 1,  /* keys = state.rng (RandomizedAutoResetWrapperNaive) */
};

/* constructor kwargs of the three env classes (defaults: pob_default_params) */
typedef struct pob_params {
  float hh_heaven_hell[2][2]; /* ant_heavenhell.py:52 */
  float hh_priest[2];         /* :53 */
  float hh_visible_radius;    /* :54 */
  float hh_dying_cost;        /* :55 */
  int ga_n_apples, ga_n_bombs;        /* ant_gather.py:60-61 */
  float ga_cage_xy[2];                /* :62 */
  float ga_robot_object_spacing;      /* :63 */
  float ga_catch_range;               /* :64 */
  int ga_n_bins;                      /* :65 */
  float ga_sensor_range, ga_sensor_span, ga_dying_cost; /* :66-68 */
  float tag_tag_radius, tag_visible_radius, tag_target_step, tag_min_spawn_distance; /* ant_tag.py:39-42 */
  float tag_cage_xy[2];               /* :43 */
  float tag_dying_cost;               /* :44 */
  int action_repeat;                  /* ActionRepeatWrapper wrappers.py:16-24 */
  float solver_scale_pos, solver_scale_ang; /* PBD joint solver scales */
  int qp_storage;                     /* pob_qp_storage (engine extension; default F32) */
  int legacy_spring;                  /* 1: brax <= 0.0.12 spring dynamics (brax Ant(legacy_spring=True),
                                         the physics of notebooks/ant_tag.ipynb:449); 0: PBD */
} pob_params;

/* Env state: device pointers, batch-major.  Optional members may be NULL.  With
 * qp_storage == POB_QP_F16 the qp and first_qp pointers address IEEE binary16 arrays. */
typedef struct pob_state {
  float *pos, *rot, *vel, *ang; /* qp */
  float *obs;
  float *reward, *done;
  float *steps, *truncation;    /* EpisodeWrapper info (optional) */
  float *m0, *m1, *m2;          /* metrics: HH heavens/hells/hits, GA apples/bombs/objects, TAG hits */
  uint32_t *rng;                /* info['rng'] (B,2) */
  float *first_pos, *first_rot, *first_vel, *first_ang, *first_obs; /* AutoResetWrapper (optional) */
  uint32_t *any_done;           /* optional: step ORs 1 into *any_done when any env is done */
  /* Optional typed copies of step outputs, written by pob_step / pob_step_mixed next to the
   * float32 fields so that the caller needs no conversion kernels for the reference's dtypes
   * (ABI v5): AntTag's bool done (done != 0 as bytes 0/1, ant_tag.py:127) and int32 truncation
   * (EpisodeWrapper on a bool done [ext]); AntGather's int32 apples / bombs counts
   * (ant_gather.py:147-148) as (int32) m0 / m1.  The reset entry points ignore them. */
  uint8_t *done_u8;
  int32_t *trunc_i32;
  int32_t *m0_i32, *m1_i32;
  /* Optional (ABI v5): pob_reset_where_done[_shard] zeroes *any_done_clear, so that a caller
   * double-buffering the any-done word (step k ORs into word k % 2, its masked reset reads
   * that word and clears the other) needs no fill kernel per step. */
  uint32_t *any_done_clear;
  /* Optional (ABI v7): obs[:, idx] of the env's observation mask (pob_env_set_obs_mask), (B, K)
   * float32, written by pob_step / pob_step_mixed from the same observation rows in the same
   * launch (po_brax/standard_observability_masks.py:5-67 applied as obs[:, idx]).  Since ABI v8
   * pob_reset and pob_reset_where_done[_shard] write it too, for the rows they reset. */
  float *obs_masked;
  /* Optional (ABI v8): per-env scratch bytes (B of them, any contents on entry) for the
   * four-lane kernel's split launch: its fast launch records in ovf_mark[b] (b = the first env
   * of each 16-env wave) whether that wave's wall contacts overflowed its store, and the fix-up
   * launch right after it re-steps exactly the marked waves.  The marks live outside every
   * output, so no state the caller wrote (first_obs rows copied by AUTORESET, edited info
   * entries) can be taken for one.  NULL: the one-launch form runs instead (the same results,
   * slower at large batches).  pob_step / pob_step_mixed read it from `out`; two launches
   * that may run concurrently must not share it (slices of one buffer are fine). */
  uint8_t *ovf_mark;
} pob_state;

typedef struct pob_env pob_env;

int pob_abi_version(void);
const char *pob_last_error(void);
int pob_default_params(pob_params *p);
int pob_env_create(int kind, const pob_params *p, pob_env **out);
/* Never calls the HIP runtime (safe while a stream is being captured into a hipGraph): the
 * env's device tables (~4 KB) are KEPT until the next pob_env_create or
 * pob_release_deferred call.  The caller must not destroy an env whose launches are still
 * queued or captured in a graph it will replay. */
void pob_env_destroy(pob_env *env);
/* Free the device tables of every destroyed env now (ABI v6); returns how many buffers were
 * released.  Calls hipFree: never call it while a stream is being captured. */
int pob_release_deferred(void);
/* The env's observation mask (ABI v7): K column indices into its observation (0 <= idx < D,
 * K <= 256, host memory); K = 0 clears it.  A step whose pob_state.obs_masked is set stores
 * obs[:, idx] there.  Copies the env's device table (hipMemcpy): call it before stepping,
 * never while a stream is being captured or a launch of this env is queued. */
int pob_env_set_obs_mask(pob_env *env, const int32_t *idx, int K);
int pob_env_dims(const pob_env *env, int *n_bodies, int *obs_dim, int *act_dim);
/* host copy of default_angle() (8 floats, radians): System.default_angle [ext] */
int pob_env_default_angle(const pob_env *env, float *out8);

int pob_reset(pob_env *env, int B, const uint32_t *keys, const pob_state *out, void *stream);
int pob_step(pob_env *env, int B, const pob_state *in, const float *act, const pob_state *out,
             uint32_t flags, int episode_length, void *stream);
/* One launch stepping n (<= POB_MIX_MAX) envs, env k over its own batch B[k] with its own
 * state / action buffers; same semantics per env as pob_step.  All envs must live on the
 * same device and share qp_storage. */
int pob_step_mixed(int n, pob_env *const *envs, const int *B, const pob_state *in,
                   const float *const *act, const pob_state *out, uint32_t flags,
                   int episode_length, void *stream);
int pob_reset_where_done(pob_env *env, int B, int mode, const uint32_t *gym_key_in,
                         uint32_t *gym_key_out, const pob_state *s, void *stream);
/* gym_key_in / gym_key_out must be distinct words, and s->any_done_clear (if set) must not
 * be s->any_done (POB_EINVAL otherwise): the kernel's first block writes the outputs while
 * every block reads the inputs.
 * The same for a shard: this env batch holds rows [first, first + B) of a global batch of
 * `total` envs split over ranks (AutoresetVmapGymWrapper under index sharding).  Gym mode
 * keys are split(gym_key, total + 1)[1 + first + b]; s->any_done must then hold the GLOBAL
 * any-done flag (the caller all-reduces it, MAX, across ranks before this call). */
int pob_reset_where_done_shard(pob_env *env, int B, int total, int first, int mode,
                               const uint32_t *gym_key_in, uint32_t *gym_key_out, const pob_state *s,
                               void *stream);
int pob_default_qp(pob_env *env, int B, const float *qpos, const float *qvel, float *pos, float *rot,
                   float *vel, float *ang, void *stream);

/* jax.random on device: split(key, num) rows [first, first+count) -> out (count,2) */
int pob_random_split(const uint32_t *key, int num, int first, int count, uint32_t *out, void *stream);
/* vmap(split)(keys, num): keys (B,2) -> out (B,num,2)  (jax.vmap(jax.random.split)) */
int pob_random_split_batch(const uint32_t *keys, int B, int num, uint32_t *out, void *stream);
/* uniform(key, (n,), lo, hi) elements [first, first+count) */
int pob_random_uniform(const uint32_t *key, int n, int first, int count, float lo, float hi, float *out,
                       void *stream);
/* random_bits(key, (n,)) elements [first, first+count): the uint32 words uniform draws are made from */
int pob_random_bits(const uint32_t *key, int n, int first, int count, uint32_t *out, void *stream);
/* bench/rollout helper: key_io <- split(key_io)[0]; act = uniform(split(key_io)[1], (total,A), -1, 1)
 * rows [first, first+B) (a shard of a batch of `total` envs) */
int pob_random_actions(uint32_t *key_io, int total, int first, int B, int A, float *act, void *stream);
/* out[b, k] = obs[b, idx[k]] */
int pob_obs_gather(const float *obs, int B, int D, const int32_t *idx, int K, float *out, void *stream);

/* ---- policy networks (additive to ABI v8): po_brax/training/networks.py:34-54 (MLP),
 * :80-123 (make_model / make_models) at inference, and the tanh-normal actor of brax's PPO
 * (NormalTanhDistribution [ext]).  One launch runs every layer on the f32 matrix cores; the
 * results equal the plain-C restatement of csrc/pob_mlp.h bit for bit (DESIGN.md "Policy
 * networks": summation order, scalar functions, the head's formulas).
 *
 * Parameters: `theta` is ONE flat device float32 buffer W_0, b_0, W_1, b_1, .. where W_i is
 * row-major (sizes[i], sizes[i + 1]) -- flax Dense.kernel's (in, out) layout -- and b_i has
 * sizes[i + 1] entries; pob_mlp_param_count gives its length.  It is read at launch time
 * and never copied, so an in-place update is seen by an already captured graph.
 * Limits: 1 .. 8 layers, every width (the input's too) in 1 .. 256, any B >= 1.
 * activation: 0 relu, 1 swish, 2 tanh, applied after every layer but the last (after the last
 * too with activate_final).  pob_mlp_create / pob_mlp_destroy never call the HIP runtime. */
typedef struct pob_mlp pob_mlp;
int pob_mlp_create(int n_layers, const int *sizes /* n_layers + 1, sizes[0] = input */, int activation,
                   int activate_final, pob_mlp **out);
void pob_mlp_destroy(pob_mlp *mlp);
int pob_mlp_param_count(const pob_mlp *mlp, long long *n);
/* y (B, sizes[n_layers]) = MLP(x (B, sizes[0])) */
int pob_mlp_forward(const pob_mlp *mlp, int B, const float *x, const float *theta, float *y, void *stream);
/* The actor: logits = MLP(obs) (B, 2 A); loc, s = its halves; scale = softplus(s) + 0.001;
 * eps = sqrt(2) erfinv(u), u = uniform(split(key_io)[1], (total, A), -1, 1)[first + b, a] (this
 * batch is rows [first, first + B) of a batch of `total` envs: a shard equals the slice);
 * raw = loc + scale eps; action = tanh(raw) (B, A); logp (B) = sum_a [-eps^2 / 2 - log scale
 * - log(2 pi) / 2 - 2 (log 2 - raw - softplus(-2 raw))], a ascending.  Then key_io <-
 * split(key_io)[0] by a one-thread launch (as pob_random_actions).  deterministic = 1: action =
 * tanh(loc), raw = loc, logp untouched, key_io neither read nor advanced (may be NULL).
 * Optional outputs (NULL = skip): logp, raw (B, A), logits (B, 2 A), obs_copy (B, sizes[0]) --
 * the observation rows written out again (a trajectory slot) from the tile already loaded.
 * The last width must be even. */
int pob_policy_act(const pob_mlp *mlp, int B, int total, int first, const float *obs, const float *theta,
                   uint32_t *key_io, int deterministic, float *action, float *logp, float *raw, float *logits,
                   float *obs_copy, void *stream);

/* ---- recurrent actor (additive to ABI v8): obs (D) -> pre-MLP (0 .. 3 dense layers, the
 * activation after every one) -> GRU cell (hidden width H; input x of width I = the pre-MLP's
 * output, or D without one) -> post-MLP (1 .. 4 dense layers, the activation after all but the
 * last), every layer and the cell in one launch; results equal gru_forward_ref of
 * csrc/pob_mlp.h bit for bit (DESIGN.md "Recurrent actor").  The cell, with c = [x ; h]:
 *   r = sigmoid(b_rz[:H] + c W_rz[:, :H]),  z = sigmoid(b_rz[H:] + c W_rz[:, H:]),
 *   n = tanh(r (b_hn + h W_hn) + (b_xn + x W_xn)),  h' = z (h - n) + n.
 * `theta`: the pre-MLP's W, b pairs, W_rz (I + H, 2 H), b_rz (2 H), W_xn (I, H), b_xn (H),
 * W_hn (H, H), b_hn (H), the post-MLP's pairs; every matrix row-major (in, out).
 * Limits: every dense width and D in 1 .. 256, 1 <= H <= 128, I + H <= 256.
 * h_io (B, H) is read, then overwritten in place with h'.  reset (B, may be NULL): where
 * reset[b] != 0 (a NaN too) env b starts from h = +0.  h_in_copy (B, H, may be NULL) receives
 * the h the step started from, after the reset.  Rows >= B are never written.
 * pob_gru_create / pob_gru_destroy never call the HIP runtime. */
typedef struct pob_gru pob_gru;
int pob_gru_create(int n_pre, const int *pre_sizes /* n_pre + 1, [0] = obs width */, int hidden, int n_post,
                   const int *post_sizes /* n_post widths after the cell */, int activation, pob_gru **out);
void pob_gru_destroy(pob_gru *g);
int pob_gru_param_count(const pob_gru *g, long long *n);
/* y (B, post_sizes[n_post - 1]) */
int pob_gru_forward(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                    float *y, float *h_in_copy, void *stream);
/* pob_policy_act with the recurrent network: noise, shard indexing, deterministic, the key
 * advance and the optional outputs are pob_policy_act's.  The last post width must be even. */
int pob_gru_policy_act(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                       uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action,
                       float *logp, float *raw, float *logits, float *obs_copy, float *h_in_copy, void *stream);

/* ---- running observation normaliser (additive to ABI v8): brax PPO's normalize_observations
 * (brax <= 0.0.12 training/normalization.py [ext]); results equal obsnorm_accumulate_ref /
 * obsnorm_update_ref / pob_obsnorm_apply of csrc/pob_mlp.h bit for bit (DESIGN.md "Observation
 * normaliser": formulas, summation order).  State, all caller-owned device memory: count
 * (float64, 1 element, initially 0) and table (float32, (3, D): row 0 mean, initially 0; row 1
 * scale, initially 1; row 2 m2, the running variance sum, initially 1).  1 <= D <= 256.
 *
 * pob_obsnorm_accumulate: sums (2, D) float64 = per column sum d and sum d^2, d = obs[n][f] -
 * mean[f] in float64, over the N rows of a row-major (N, D) array, in a fixed order (chunks of
 * 1024 rows, rows ascending, then chunks ascending) that depends on N and D only.  workspace:
 * pob_obsnorm_workspace_bytes(N, D) bytes, the chunk partials; the library never allocates.
 * pob_obsnorm_update: sums is (R, 2, D), one pair per shard in rank order, n_new the row count
 * over all shards; count and table are finished in place by one block that reads nothing on
 * the host (capturable). */
int pob_obsnorm_workspace_bytes(long long N, int D, long long *bytes);
int pob_obsnorm_accumulate(const float *obs, long long N, int D, const float *table, double *workspace,
                           double *sums /* (2, D) */, void *stream);
int pob_obsnorm_update(double *count_io, float *table_io, int D, const double *sums, int R, long long n_new,
                       void *stream);
/* The forward entry points with the normaliser fused into the observation tile load: the
 * network sees clip((x - mean[f]) * scale[f], +-norm_clip) (two float32 roundings; norm_clip <= 0:
 * no clamp; a NaN stays NaN), obs_copy still receives the raw rows, the hidden state is never
 * normalised.  norm: the (3, D) table, rows 0 and 1 are read at launch time; NULL = no
 * normalisation, the results of the entry point without the suffix. */
int pob_mlp_forward_norm(const pob_mlp *mlp, int B, const float *x, const float *theta, float *y, const float *norm,
                         float norm_clip, void *stream);
int pob_policy_act_norm(const pob_mlp *mlp, int B, int total, int first, const float *obs, const float *theta,
                        uint32_t *key_io, int deterministic, float *action, float *logp, float *raw, float *logits,
                        float *obs_copy, const float *norm, float norm_clip, void *stream);
int pob_gru_forward_norm(const pob_gru *g, int B, const float *x, const float *theta, const float *reset, float *h_io,
                         float *y, float *h_in_copy, const float *norm, float norm_clip, void *stream);
int pob_gru_policy_act_norm(const pob_gru *g, int B, int total, int first, const float *obs, const float *theta,
                            uint32_t *key_io, int deterministic, const float *reset, float *h_io, float *action,
                            float *logp, float *raw, float *logits, float *obs_copy, float *h_in_copy, const float *norm,
                            float norm_clip, void *stream);

/* ---- generalised advantage estimation (ABI v8, additive): brax v1 PPO's compute_gae [ext] in one
 * launch, gae_ref of csrc/pob_mlp.h bit for bit (DESIGN.md "Critic pass and GAE": formula and
 * operation order).  All arrays row-major (T, B) float32 device memory, bootstrap (B); each env
 * on its own, t descending from T - 1 with acc = +0, v_next = vs_next = bootstrap[b]:
 *   m = 1 - truncation (NULL: 1);  term = done_input ? second m : second;  g = discount (1 - term)
 *   r = reward reward_scale;  delta = (fmaf(g, v_next, r) - v) m;  adv = (fmaf(g, vs_next, r) - v) m
 *   acc = fmaf((g m) lambda, acc, delta);  vs = acc + v;  vs_next = vs;  v_next = v
 * second is termination when done_input == 0 and done otherwise.  vs or advantages may be NULL
 * (not both); outputs must not overlap inputs.  T >= 1, B >= 1.  No allocation, no
 * synchronisation: capturable. */
int pob_gae(int T, long long B, const float *truncation /* may be NULL */, const float *second, int done_input,
            const float *reward, float reward_scale, const float *values, const float *bootstrap, float lambda,
            float discount, float *vs /* may be NULL */, float *advantages /* may be NULL */, void *stream);

/* ---- PPO loss on the tanh-normal head (ABI v8, additive): brax v1 ppo.compute_ppo_loss [ext] and
 * its gradient to the logits and the values, ppo_loss_ref of csrc/pob_mlp.h bit for bit (DESIGN.md
 * "PPO loss": formula, operation and summation order).  logits (M, 2 A) and values (M) are in
 * minibatch order; raw (N, A), old_logp, advantages, vs (N) in trajectory order: row i reads
 * trajectory row idx[i] (every entry in [0, N): not checked), or row i when idx is NULL.  The
 * entropy is sampled with u = uniform(split(key)[1], (M, A), -1, 1) of the device threefry; the
 * key is read, never advanced.  losses[4] = total, policy_loss, value_loss, entropy_loss; dlogits
 * (M, 2 A) and dvalues (M) = d total / d logits, d total / d values, either may be NULL.
 * workspace: pob_ppo_loss_workspace_bytes(M) bytes; it starts with the (ceil(M / 1024), 3) float64
 * chunk partials of the three sums.  1 <= A <= 128, M A < 2^32 - 1.  Arguments are checked before
 * any HIP call; no allocation, no synchronisation: capturable. */
int pob_ppo_loss_workspace_bytes(long long M, long long *bytes);
int pob_ppo_loss(long long M, int A, const float *logits, const float *values, const int32_t *idx /* may be NULL */,
                 const float *raw, const float *old_logp, const float *advantages, const float *vs,
                 const uint32_t *key, float entropy_cost, float ppo_epsilon,
                 float *dlogits /* may be NULL */, float *dvalues /* may be NULL */, float *losses /* 4 */,
                 double *workspace, void *stream);

/* ---- MLP backward (ABI v8, additive): the training forward of a pob_mlp, which keeps what the
 * backward needs, and the backward pass to the parameters and (optionally) the input;
 * mlp_forward_train_ref / mlp_backward_ref of csrc/pob_mlp.h bit for bit (DESIGN.md "MLP backward":
 * formulas, summation order).  Layer l is activated when l != n_layers - 1 || activate_final.
 * forward_train: y (M, sizes[n_layers]) equals pob_mlp_forward's; saved (pob_mlp_saved_bytes) receives
 * the pre-activation (M, sizes[l + 1]) row-major of every activated layer, ascending l.  backward:
 * dy (M, sizes[n_layers]) -> dtheta (param_count floats, theta's packing) and dx (M, sizes[0]; may be
 * NULL).  The workspace is opaque, caller-owned device memory of
 *   round_up_8(4 M sum_l sizes[l + 1]) + 8 ceil(M / 1024) param_count   bytes
 * (every layer's delta, then the float64 chunk partials of the parameter gradient): it grows with
 * ceil(M / 1024) * param_count * 8 bytes, about 0.3 GB for [114 -> 256 x 5 -> 1] at M = 40 960.
 * M >= 1 and (M + 1024) times the widest layer < 2^31.  Arguments are checked before any HIP call; no
 * allocation, no atomics, no synchronisation: capturable. */
int pob_mlp_saved_bytes(const pob_mlp *mlp, long long M, long long *bytes);
int pob_mlp_forward_train(const pob_mlp *mlp, long long M, const float *x, const float *theta, float *y, float *saved,
                          void *stream);
int pob_mlp_backward_workspace_bytes(const pob_mlp *mlp, long long M, long long *bytes);
int pob_mlp_backward(const pob_mlp *mlp, long long M, const float *x, const float *theta, const float *saved,
                     const float *dy, float *dtheta, float *dx /* may be NULL */, void *workspace, void *stream);

/* ---- Recurrent backward (ABI v8, additive): the training forward of a pob_gru over a window of T
 * steps and its truncated backward pass through time; gru_sequence_forward_train_ref /
 * gru_sequence_backward_ref of csrc/pob_mlp.h bit for bit (DESIGN.md "Recurrent backward": formulas,
 * operation and summation order).  obs (T, B, D) and reset (T, B; may be NULL) are trajectory arrays
 * read in place: sequence m is env idx[m] (int32, every entry in [0, B): not checked), or env m
 * without idx (then M == B); h0 (B, H) is read through idx too.  reset[t][b] != 0 (a NaN too, -0.0
 * not): env b starts step t from h = +0, and no gradient crosses that step's entry.  norm: the
 * (3, D) normaliser table of pob_gru_forward_norm, or NULL.
 * forward_train: y (T, M, out) and h_last (M, H; may be NULL) equal T chained pob_gru_forward_norm
 * calls on the gathered rows; saved (pob_gru_sequence_saved_bytes) is opaque.  backward: dy (T, M, out)
 * and dh_last (M, H; NULL: zeros) -> dtheta (param_count floats, theta's packing) and dh0 (M, H; may
 * be NULL).  idx and reset must be the forward's.  There is no gradient to the observations.  The
 * workspace is opaque, caller-owned device memory (pob_gru_sequence_backward_workspace_bytes: every
 * delta array, then 8 ceil(T M / 1024) param_count bytes of float64 chunk partials).  T >= 1, M >= 1,
 * and (T M + 1024) times the widest array (4 H included) < 2^31.  Arguments are checked before any
 * HIP call; no allocation, no atomics, no synchronisation: forward and backward capture into one graph. */
int pob_gru_sequence_saved_bytes(const pob_gru *g, int T, long long M, long long *bytes);
int pob_gru_sequence_forward_train(const pob_gru *g, int T, long long M, long long B, const float *obs,
                                   const int32_t *idx /* may be NULL */, const float *h0,
                                   const float *reset /* may be NULL */, const float *theta, float *y,
                                   float *h_last /* may be NULL */, float *saved, const float *norm /* may be NULL */,
                                   float norm_clip, void *stream);
int pob_gru_sequence_backward_workspace_bytes(const pob_gru *g, int T, long long M, long long *bytes);
int pob_gru_sequence_backward(const pob_gru *g, int T, long long M, long long B, const int32_t *idx /* may be NULL */,
                              const float *reset /* may be NULL */, const float *theta, const float *saved,
                              const float *dy, const float *dh_last /* may be NULL */, float *dtheta,
                              float *dh0 /* may be NULL */, void *workspace, void *stream);

/* ---- Recurrent window, inference only (ABI v8, additive): a pob_gru over S steps of trajectory
 * arrays in ONE launch that stores nothing but its outputs (the recurrent critic's pass: DESIGN.md
 * "Recurrent critic"); gru_sequence_forward_ref of csrc/pob_mlp.h bit for bit.  obs (S, B, D), reset
 * (S, B; may be NULL), idx, h0 (B, H) and norm as for pob_gru_sequence_forward_train; y (S, M, out)
 * equals S chained pob_gru_forward_norm calls on the gathered rows (so forward_train's y too).
 * h_first (M, H; may be NULL) receives the state step 0 started from, after step 0's reset (what
 * h_in_copy is to pob_gru_forward); h_out (M, H; may be NULL) the state after h_out_step steps
 * (1 <= h_out_step <= S, checked also when h_out is NULL), before step h_out_step's reset.  Without
 * idx h_out may be h0 itself: a tile reads its rows of h0 before it writes them; with idx it must not
 * overlap h0, and y and h_first never overlap an input.  Rows >= M are never written.  The limits
 * are forward_train's.  Arguments are checked before any HIP call; no allocation, no atomics, no
 * synchronisation: capturable. */
int pob_gru_sequence_forward(const pob_gru *g, int S, long long M, long long B, const float *obs,
                             const int32_t *idx /* may be NULL */, const float *h0,
                             const float *reset /* (S, B), may be NULL */, const float *theta,
                             float *y /* (S, M, out) */, float *h_first /* (M, H), may be NULL */,
                             float *h_out /* (M, H), may be NULL */, int h_out_step,
                             const float *norm /* may be NULL */, float norm_clip, void *stream);

/* ---- Fused Adam (ABI v8, additive): one optimiser step of up to POB_ADAM_MAX_SEG parameter
 * vectors in one launch, adam_step_ref of csrc/pob_mlp.h bit for bit (DESIGN.md "Learner on the
 * device": optax's adam [ext], the float32 operation order).  segs is a HOST array of n_seg
 * segments; it is copied into the kernel's argument, so nothing of it is read after the call
 * returns.  Per segment theta, m and v (n floats each, device memory, 4-byte aligned, any n >= 1)
 * are updated IN PLACE from grad; segments must not overlap.  state is two float64 words of device
 * memory, {beta1^t, beta2^t} as running products, 1.0 each before the first step: the call reads
 * them, applies the bias corrections of step t + 1, and a one-lane launch behind it stores the
 * advanced products, so the step count lives on the device and a replayed graph counts on.
 * Arguments are checked before any HIP call; no allocation, no atomics, no synchronisation:
 * capturable. */
#define POB_ADAM_MAX_SEG 4
typedef struct pob_adam_seg {
  float *theta;
  const float *grad;
  float *m;
  float *v;
  long long n;
} pob_adam_seg;
int pob_adam_step(const pob_adam_seg *segs, int n_seg, double *state, float lr, float beta1, float beta2, float eps,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif
