// pob_learner.hip -- the learner's streaming kernels: the observation normaliser's statistics, GAE,
// the Adam step and the PPO loss.  None of them touches the matrix-core tile code; of
// pob_mlp_tile.h they take the error helpers only.  Each section states its specification in
// pob_mlp.h and its DESIGN.md section.
#include <climits>

#include "pob_mlp_tile.h"

// ============================================================================ observation normaliser
// The statistics of pob_mlp.h obsnorm_accumulate_ref / obsnorm_update_ref (the specification; DESIGN.md
// "Observation normaliser").  k_obsnorm_accumulate: one lane per (chunk, column), consecutive lanes
// on consecutive columns of a row (coalesced), the chunk's rows in ascending order into a float64
// pair in registers, OBSNORM_STAGE loads in flight per lane; the pair goes to the workspace
// (n_chunks, 2, D).  k_obsnorm_reduce: one lane per entry of (2, D) adds the chunk partials in
// ascending chunk order.  k_obsnorm_update: one block finishes the table in place.  No atomics:
// the order depends on N and D only.
#define OBSNORM_STAGE 16
#define OBSNORM_RSTAGE 32

__global__ __launch_bounds__(256) void k_obsnorm_accumulate(const float *x, const long long N, const int D,
                                                            const float *table, double *ws, const long long n_items) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_items) return;
  const long long c = g / D;
  const int f = (int)(g - c * D);
  const long long r0 = c * POB_OBSNORM_CHUNK;
  const int rows = N - r0 < POB_OBSNORM_CHUNK ? (int)(N - r0) : POB_OBSNORM_CHUNK;
  const float mean = table[f];
  const float *p = x + (size_t)r0 * D + f;
  double S1 = 0.0, S2 = 0.0;
  int r = 0;
  for (; r + OBSNORM_STAGE <= rows; r += OBSNORM_STAGE) {
    float v[OBSNORM_STAGE];
#pragma unroll
    for (int u = 0; u < OBSNORM_STAGE; ++u) v[u] = p[(size_t)(r + u) * D];
#pragma unroll
    for (int u = 0; u < OBSNORM_STAGE; ++u) pob_obsnorm_step(v[u], mean, S1, S2);
  }
  for (; r < rows; ++r) pob_obsnorm_step(p[(size_t)r * D], mean, S1, S2);
  ws[(size_t)(2 * c) * D + f] = S1;
  ws[(size_t)(2 * c + 1) * D + f] = S2;
}

__global__ __launch_bounds__(64) void k_obsnorm_reduce(const double *ws, const long long n_chunks, const int D,
                                                       double *sums) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= 2 * D) return;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += OBSNORM_RSTAGE) {
    double v[OBSNORM_RSTAGE];
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u) v[u] = c0 + u < n_chunks ? ws[(size_t)(c0 + u) * 2 * D + e] : 0.0;
#pragma unroll
    for (int u = 0; u < OBSNORM_RSTAGE; ++u)
      if (c0 + u < n_chunks) T = T + v[u];
  }
  sums[e] = T;
}

__global__ __launch_bounds__(POB_MLP_MAX_WIDTH) void k_obsnorm_update(double *count, float *table, const int D,
                                                                      const double *sums, const int R,
                                                                      const long long n_new) {
  const int f = threadIdx.x;
  const double cnt = count[0];
  __syncthreads();  // every lane holds the old count before lane 0 replaces it
  double total = cnt;
  if (f < D) {
    double S1 = 0.0, S2 = 0.0;
    for (int r = 0; r < R; ++r) {
      S1 = S1 + sums[(size_t)(2 * r) * D + f];
      S2 = S2 + sums[(size_t)(2 * r + 1) * D + f];
    }
    float mean = table[f], scale = table[D + f], m2 = table[2 * D + f];
    total = pob_obsnorm_finish(cnt, (double)n_new, S1, S2, mean, scale, m2);
    table[f] = mean;
    table[D + f] = scale;
    table[2 * D + f] = m2;
  }
  if (f == 0) count[0] = total;
}

static int obsnorm_chunks(long long N, int D, long long *n_chunks) {
  if (D < 1 || D > POB_MLP_MAX_WIDTH) return pob_fail_msg(POB_EINVAL, "obsnorm: the observation width must be in 1 .. 256");
  if (N < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the row count must be positive");
  if (N > (1LL << 40)) return pob_fail_msg(POB_EINVAL, "obsnorm: at most 2^40 rows");
  *n_chunks = (N + POB_OBSNORM_CHUNK - 1) / POB_OBSNORM_CHUNK;
  return POB_OK;
}

extern "C" {

int pob_obsnorm_workspace_bytes(long long N, int D, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "obsnorm: bytes is NULL");
  long long n_chunks;
  const int rc = obsnorm_chunks(N, D, &n_chunks);
  if (rc != POB_OK) return rc;
  *bytes = n_chunks * 2 * D * (long long)sizeof(double);
  return POB_OK;
}

int pob_obsnorm_accumulate(const float *obs, long long N, int D, const float *table, double *workspace, double *sums,
                           void *stream) {
  long long n_chunks;
  const int rc = obsnorm_chunks(N, D, &n_chunks);
  if (rc != POB_OK) return rc;
  if (!obs || !table || !workspace || !sums) return pob_fail_msg(POB_EINVAL, "obsnorm: NULL argument (obs, table, workspace, sums)");
  hipStream_t st = (hipStream_t)stream;
  const long long n_items = n_chunks * D;
  hipLaunchKernelGGL(k_obsnorm_accumulate, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, obs, N, D, table,
                     workspace, n_items);
  hipLaunchKernelGGL(k_obsnorm_reduce, dim3((unsigned)((2 * D + 63) / 64)), dim3(64), 0, st, workspace, n_chunks, D, sums);
  return mlp_hip_check(hipGetLastError(), "k_obsnorm_accumulate launch");
}

int pob_obsnorm_update(double *count_io, float *table_io, int D, const double *sums, int R, long long n_new, void *stream) {
  if (D < 1 || D > POB_MLP_MAX_WIDTH) return pob_fail_msg(POB_EINVAL, "obsnorm: the observation width must be in 1 .. 256");
  if (R < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the shard count R must be positive");
  if (n_new < 1) return pob_fail_msg(POB_EINVAL, "obsnorm: the row count must be positive");
  if (!count_io || !table_io || !sums) return pob_fail_msg(POB_EINVAL, "obsnorm: NULL argument (count, table, sums)");
  hipLaunchKernelGGL(k_obsnorm_update, dim3(1), dim3(POB_MLP_MAX_WIDTH), 0, (hipStream_t)stream, count_io, table_io, D, sums,
                     R, n_new);
  return mlp_hip_check(hipGetLastError(), "k_obsnorm_update launch");
}

}  // extern "C"

// ============================================================================ GAE
// gae_ref of pob_mlp.h (the specification; DESIGN.md "Critic pass and GAE").  One lane per env,
// consecutive lanes on consecutive b (every load and store a coalesced row segment), t
// descending.  The carried chain is pob_gae_step's fmaf and add; the loads do not depend on it,
// so the steps are taken in chunks of POB_GAE_CHUNK whose rows are all issued before the chunk
// before them is consumed (two register images: at one or two waves per CU the loop then waits
// for HBM once per chunk, not once per step).  The newest chunk takes the (T - 1) % POB_GAE_CHUNK
// + 1 steps that make every later chunk a full one.  TRUNC = false: truncation is NULL (m = 1 - 0).
// No LDS, no atomics, no scratch.
struct gae_rows { float tr[POB_GAE_CHUNK], se[POB_GAE_CHUNK], rw[POB_GAE_CHUNK], va[POB_GAE_CHUNK]; };

// rows t_hi, t_hi - 1, .., t_hi - POB_GAE_CHUNK + 1 of lane b; a row before the first (the newest
// chunk of a T that is no multiple of the chunk) is loaded as row 0 and never used
template <bool TRUNC>
__device__ __forceinline__ void gae_load(gae_rows &r, const int t_hi, const size_t B, const size_t b,
                                         const float *truncation, const float *second, const float *reward,
                                         const float *values) {
#pragma unroll
  for (int u = 0; u < POB_GAE_CHUNK; ++u) {
    const size_t i = (size_t)(t_hi - u > 0 ? t_hi - u : 0) * B + b;
    r.tr[u] = TRUNC ? truncation[i] : 0.0f;
    r.se[u] = second[i];
    r.rw[u] = reward[i];
    r.va[u] = values[i];
  }
}

template <bool TRUNC>
__global__ __launch_bounds__(64) void k_gae(const int T, const long long B, const float *truncation, const float *second,
                                            const int done_input, const float *reward, const float reward_scale,
                                            const float *values, const float *bootstrap, const float lambda,
                                            const float discount, float *vs, float *advantages) {
  const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
  if (lane >= B) return;
  const size_t b = (size_t)lane, Bs = (size_t)B;
  float acc = 0.0f, v_next = bootstrap[b], vs_next = v_next;
  int t = T - 1;                          // the chunk in `cur` is steps t, t - 1, .., t - n + 1
  int n = (T - 1) % POB_GAE_CHUNK + 1;
  gae_rows cur, nxt;
  gae_load<TRUNC>(cur, t, Bs, b, truncation, second, reward, values);
  for (;;) {
    const bool more = t - n >= 0;  // then t - n + 1 is a multiple of the chunk: a full chunk follows
    if (more) gae_load<TRUNC>(nxt, t - n, Bs, b, truncation, second, reward, values);
#pragma unroll
    for (int u = 0; u < POB_GAE_CHUNK; ++u)
      if (u < n) {
        float adv;
        pob_gae_step(cur.tr[u], cur.se[u], done_input, cur.rw[u], reward_scale, cur.va[u], lambda, discount, acc, v_next,
                     vs_next, adv);
        const size_t i = (size_t)(t - u) * Bs + b;
        if (advantages) advantages[i] = adv;
        if (vs) vs[i] = vs_next;
      }
    if (!more) break;
    t -= n;
    n = POB_GAE_CHUNK;
    cur = nxt;
  }
}

extern "C" {

int pob_gae(int T, long long B, const float *truncation, const float *second, int done_input, const float *reward,
            float reward_scale, const float *values, const float *bootstrap, float lambda, float discount, float *vs,
            float *advantages, void *stream) {
  if (T < 1) return pob_fail_msg(POB_EINVAL, "gae: the step count T must be positive");
  if (B < 1) return pob_fail_msg(POB_EINVAL, "gae: the batch size B must be positive");
  if (B > (1LL << 36)) return pob_fail_msg(POB_EINVAL, "gae: at most 2^36 envs");
  if (!second || !reward || !values || !bootstrap)
    return pob_fail_msg(POB_EINVAL, "gae: NULL argument (second, reward, values, bootstrap)");
  if (!vs && !advantages) return pob_fail_msg(POB_EINVAL, "gae: vs and advantages are both NULL");
  const dim3 grid((unsigned)((B + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
  if (truncation)
    hipLaunchKernelGGL(k_gae<true>, grid, dim3(64), 0, st, T, B, truncation, second, done_input ? 1 : 0, reward,
                       reward_scale, values, bootstrap, lambda, discount, vs, advantages);
  else
    hipLaunchKernelGGL(k_gae<false>, grid, dim3(64), 0, st, T, B, truncation, second, done_input ? 1 : 0, reward,
                       reward_scale, values, bootstrap, lambda, discount, vs, advantages);
  return mlp_hip_check(hipGetLastError(), "k_gae launch");
}

}  // extern "C"

// ============================================================================ Adam
// adam_step_ref of pob_mlp.h (the specification; DESIGN.md "Learner on the device").  One launch
// steps every segment: the table travels BY VALUE as the kernel argument (a captured graph keeps the
// copy; no device pointer array that could go stale).  The work is streaming, 28 bytes an element: a
// lane owns ONE item, either a 16-byte group of four elements of the segment's aligned body (four
// 16-byte loads in flight, three 16-byte stores; consecutive lanes on consecutive groups) or one
// scalar element of its head or tail.  A segment's base is only 4-byte aligned: the host finds the
// head that brings theta, grad, m and v to a 16-byte boundary TOGETHER, and a segment whose four
// bases disagree modulo 16 is all head (scalar).  A block serves one segment (blk0: its first block),
// found by a select over the table, not by indexing it (no scratch).  Every lane forms the step's bias
// corrections from the state block itself (two uniform 8-byte loads, two float64 products); the
// block is advanced by k_adam_advance, one lane, after it on the same stream, so a replayed graph
// counts its own steps.  No LDS, no atomics, ordinary vector stores only.
#define ADAM_THREADS 256
struct AdamSeg {
  float *theta, *m, *v;
  const float *grad;
  long long head, nvec, nsc;  // scalar elements before the body, 16-byte groups, scalar elements in all
  unsigned blk0;
};
struct AdamTable {
  AdamSeg seg[POB_ADAM_MAX_SEG];
  int n_seg;
};

__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step(const AdamTable t, const double *state, const float lr,
                                                            const float beta1, const float beta2, const float eps) {
  AdamSeg s = t.seg[0];
#pragma unroll
  for (int k = 1; k < POB_ADAM_MAX_SEG; ++k)
    if (k < t.n_seg && blockIdx.x >= t.seg[k].blk0) s = t.seg[k];
  const long long item = (long long)(blockIdx.x - s.blk0) * ADAM_THREADS + threadIdx.x;
  if (item >= s.nvec + s.nsc) return;
  double p1, p2;
  float ic1, ic2;
  pob_adam_bias(state[0], state[1], beta1, beta2, p1, p2, ic1, ic2);
  if (item < s.nvec) {
    const size_t e = (size_t)s.head + 4 * (size_t)item;
    float4 th = *(const float4 *)(s.theta + e), m = *(const float4 *)(s.m + e), v = *(const float4 *)(s.v + e);
    const float4 g = *(const float4 *)(s.grad + e);
    pob_adam_elem(th.x, g.x, m.x, v.x, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.y, g.y, m.y, v.y, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.z, g.z, m.z, v.z, lr, beta1, beta2, eps, ic1, ic2);
    pob_adam_elem(th.w, g.w, m.w, v.w, lr, beta1, beta2, eps, ic1, ic2);
    *(float4 *)(s.theta + e) = th;
    *(float4 *)(s.m + e) = m;
    *(float4 *)(s.v + e) = v;
  } else {
    const long long k = item - s.nvec;  // scalar element k: the head's, then the tail's behind the body
    const size_t e = (size_t)(k < s.head ? k : k + 4 * s.nvec);
    float th = s.theta[e], m = s.m[e], v = s.v[e];
    pob_adam_elem(th, s.grad[e], m, v, lr, beta1, beta2, eps, ic1, ic2);
    s.theta[e] = th;
    s.m[e] = m;
    s.v[e] = v;
  }
}

__global__ void k_adam_advance(double *state, const float beta1, const float beta2) {
  double p1, p2;
  float ic1, ic2;
  pob_adam_bias(state[0], state[1], beta1, beta2, p1, p2, ic1, ic2);
  state[0] = p1;
  state[1] = p2;
}

extern "C" {

int pob_adam_step(const pob_adam_seg *segs, int n_seg, double *state, float lr, float beta1, float beta2, float eps,
                  void *stream) {
  if (n_seg < 1 || n_seg > POB_ADAM_MAX_SEG) return pob_fail_msg(POB_EINVAL, "adam: 1 .. 4 segments a launch");
  if (!segs || !state) return pob_fail_msg(POB_EINVAL, "adam: NULL argument (segs, state)");
  if (((uintptr_t)state & 7) != 0) return pob_fail_msg(POB_EINVAL, "adam: the state block must be 8-byte aligned");
  AdamTable t;
  long long blocks = 0;
  for (int k = 0; k < POB_ADAM_MAX_SEG; ++k) {
    AdamSeg &s = t.seg[k];
    if (k >= n_seg) {
      s = AdamSeg{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0u};
      continue;
    }
    const pob_adam_seg &in = segs[k];
    if (!in.theta || !in.grad || !in.m || !in.v) return pob_fail_msg(POB_EINVAL, "adam: NULL segment pointer");
    if (in.n < 1 || in.n > (1LL << 36)) return pob_fail_msg(POB_EINVAL, "adam: a segment holds 1 .. 2^36 elements");
    const uintptr_t a[4] = {(uintptr_t)in.theta, (uintptr_t)in.grad, (uintptr_t)in.m, (uintptr_t)in.v};
    for (int q = 0; q < 4; ++q)
      if (a[q] & 3) return pob_fail_msg(POB_EINVAL, "adam: segment pointers must be 4-byte aligned");
    const bool together = (a[0] & 15) == (a[1] & 15) && (a[0] & 15) == (a[2] & 15) && (a[0] & 15) == (a[3] & 15);
    long long head = together ? (long long)(((16 - (a[0] & 15)) & 15) >> 2) : in.n;
    if (head > in.n) head = in.n;
    s.theta = in.theta; s.grad = in.grad; s.m = in.m; s.v = in.v;
    s.head = head;
    s.nvec = (in.n - head) / 4;
    s.nsc = in.n - 4 * s.nvec;
    s.blk0 = (unsigned)blocks;
    blocks += (s.nvec + s.nsc + ADAM_THREADS - 1) / ADAM_THREADS;
    if (blocks > INT_MAX) return pob_fail_msg(POB_EINVAL, "adam: too many elements for one launch");
  }
  t.n_seg = n_seg;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adam_step, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, st, t, (const double *)state, lr, beta1,
                     beta2, eps);
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, state, beta1, beta2);
  return mlp_hip_check(hipGetLastError(), "k_adam_step launch");
}

}  // extern "C"

// ============================================================================ PPO loss
// ppo_loss_ref of pob_mlp.h (the specification; DESIGN.md "PPO loss").  k_ppo_loss: a block of
// 256 lanes owns a tile of R consecutive minibatch rows, R = min(256, 1024 / A), so a lane has at
// most PPO_ITEMS (row, component) items.  The tile's logits arrive in LDS as the contiguous row
// segment they are in memory (coalesced, all of a lane's loads in flight), pitch 2 A + 1 per row;
// raw is gathered by idx in whole-row segments.  Consecutive lanes take consecutive components of
// a row: every item's pob_ppo_component runs once, its five gradient factors stay in the lane's
// registers, its two terms go back into the logits' own LDS slots.  One lane per row then sums the
// terms in a ascending (the pitch is odd: conflict-free), finishes pob_ppo_row, stores dvalues and
// the row's three summands and publishes g_lp; the items form pob_ppo_grad into the same slots,
// and dlogits leaves as the contiguous segment it is.  k_ppo_chunks: one block per chunk of
// POB_PPO_CHUNK rows loads the summands coalesced into LDS and three lanes add them in ascending
// row order (the fixed order admits no tree).  k_ppo_finish: one block stages the chunk partials
// through LDS, three lanes add them in ascending order, one forms the four scalars.  No atomics,
// no scratch.
#define PPO_THREADS 256
#define PPO_ITEMS 4      // (row, component) items of a lane
#define PPO_MAX_ROWS 256 // rows of a tile: one row-phase lane each
#define PPO_ELEMS (PPO_THREADS * PPO_ITEMS)  // a tile holds at most this many components
#define PPO_FSTAGE 512   // chunk partials k_ppo_finish stages through LDS at a time

// element e of a row-major (rows, W) tile as (row, col), advanced by the block's 256 lanes at a time
struct ppo_walk {
  int row, col, dq, dr, W;
  __device__ __forceinline__ ppo_walk(const int e, const int width) : W(width) {
    row = e / W; col = e - row * W;
    dq = PPO_THREADS / W; dr = PPO_THREADS - dq * W;
  }
  __device__ __forceinline__ void next() {
    row += dq; col += dr;
    if (col >= W) { col -= W; ++row; }
  }
};

__global__ __launch_bounds__(PPO_THREADS) void k_ppo_loss(const long long M, const int A, const int R, const float *logits,
                                                          const float *values, const int32_t *idx, const float *raw,
                                                          const float *old_logp, const float *advantages, const float *vs,
                                                          const uint32_t *key, const float entropy_cost,
                                                          const float ppo_epsilon, const float inv_m, float *dlogits,
                                                          float *dvalues, float *terms) {
  __shared__ float L[2 * PPO_ELEMS + PPO_MAX_ROWS];  // (R, 2 A) at pitch 2 A + 1: logits, then terms, then dlogits
  __shared__ float X[PPO_ELEMS];                     // (R, A): raw
  __shared__ long long J[PPO_MAX_ROWS];              // the rows' trajectory rows
  __shared__ float G[PPO_MAX_ROWS];                  // the rows' g_lp
  const int tid = threadIdx.x, W = 2 * A, P = W + 1;
  const long long b0 = (long long)blockIdx.x * R;
  const int valid = M - b0 < R ? (int)(M - b0) : R;
  // the row phase's operands, loaded ahead of their use
  float r_old = 0.0f, r_adv = 0.0f, r_vs = 0.0f, r_val = 0.0f;
  if (tid < valid) {
    const long long j = idx ? (long long)idx[b0 + tid] : b0 + tid;
    J[tid] = j;
    r_old = old_logp[j]; r_adv = advantages[j]; r_vs = vs[j];
    r_val = values[b0 + tid];
  }
  {
    const float *g = logits + (size_t)b0 * W;
    const int n = valid * W;
    ppo_walk w(tid, W);
    float v[2 * PPO_ITEMS];
    int at[2 * PPO_ITEMS];
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      const bool ok = e < n;
      v[k] = ok ? g[e] : 0.0f;
      at[k] = ok ? w.row * P + w.col : -1;
      w.next();
    }
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k)
      if (at[k] >= 0) L[at[k]] = v[k];
  }
  __syncthreads();
  const int n_items = valid * A;
  {
    ppo_walk w(tid, A);
    float v[PPO_ITEMS];
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      const bool ok = tid + PPO_THREADS * k < n_items;
      v[k] = ok ? raw[(size_t)J[w.row] * A + w.col] : 0.0f;
      w.next();
    }
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k)
      if (tid + PPO_THREADS * k < n_items) X[tid + PPO_THREADS * k] = v[k];
  }
  __syncthreads();
  uint32_t s0, s1;
  tf_split(key[0], key[1], 2u, 1u, s0, s1);
  const uint32_t n_draws = (uint32_t)M * (uint32_t)A;
  float f[PPO_ITEMS][5];
  {
    ppo_walk w(tid, A);
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      if (e < n_items) {
        const int lo = w.row * P + w.col;
        const uint32_t i = (uint32_t)(b0 + w.row) * (uint32_t)A + (uint32_t)w.col;
        const float u = tf_uniform(s0, s1, n_draws, i, -1.0f, 1.0f);
        float term, ent;
        pob_ppo_component(L[lo], L[lo + A], X[e], u, term, ent, f[k][0], f[k][1], f[k][2], f[k][3], f[k][4]);
        L[lo] = term;
        L[lo + A] = ent;
      }
      w.next();
    }
  }
  __syncthreads();
  if (tid < valid) {
    float logp = 0.0f, ent = 0.0f;
    for (int a = 0; a < A; ++a) {
      logp = logp + L[tid * P + a];
      ent = ent + L[tid * P + A + a];
    }
    float neg_surr, vl, g_lp, dvalue;
    pob_ppo_row(logp, r_old, r_adv, r_vs, r_val, ppo_epsilon, inv_m, neg_surr, vl, g_lp, dvalue);
    G[tid] = g_lp;
    if (dvalues) dvalues[b0 + tid] = dvalue;
    terms[(size_t)b0 + tid] = neg_surr;
    terms[(size_t)M + b0 + tid] = vl;
    terms[2 * (size_t)M + b0 + tid] = ent;
  }
  if (!dlogits) return;
  __syncthreads();
  {
    const float g_ent = -(entropy_cost * inv_m);
    ppo_walk w(tid, A);
#pragma unroll
    for (int k = 0; k < PPO_ITEMS; ++k) {
      if (tid + PPO_THREADS * k < n_items) {
        const int lo = w.row * P + w.col;
        float d_loc, d_p;
        pob_ppo_grad(G[w.row], g_ent, f[k][0], f[k][1], f[k][2], f[k][3], f[k][4], d_loc, d_p);
        L[lo] = d_loc;
        L[lo + A] = d_p;
      }
      w.next();
    }
  }
  __syncthreads();
  {
    float *g = dlogits + (size_t)b0 * W;
    const int n = valid * W;
    ppo_walk w(tid, W);
#pragma unroll
    for (int k = 0; k < 2 * PPO_ITEMS; ++k) {
      const int e = tid + PPO_THREADS * k;
      if (e < n) g[e] = L[w.row * P + w.col];
      w.next();
    }
  }
}

// partials (n_chunks, 3) <- the float64 sums of the chunk's rows of terms (3, M), rows ascending from +0.0
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_chunks(const long long M, const float *terms, double *partials) {
  __shared__ __attribute__((aligned(16))) float T[3][POB_PPO_CHUNK];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * POB_PPO_CHUNK;
  const int rows = M - r0 < POB_PPO_CHUNK ? (int)(M - r0) : POB_PPO_CHUNK;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < POB_PPO_CHUNK / PPO_THREADS; ++k) {
      const int r = tid + PPO_THREADS * k;
      T[q][r] = r < rows ? terms[(size_t)q * M + r0 + r] : 0.0f;
    }
  __syncthreads();
  if (tid < 3) {
    double S = 0.0;
    const float4 *t4 = (const float4 *)T[tid];  // four rows a read; the adds keep the rows' order
    int r = 0;
#pragma unroll 4
    for (; r + 4 <= rows; r += 4) {
      const float4 v = t4[r >> 2];
      S = S + (double)v.x;
      S = S + (double)v.y;
      S = S + (double)v.z;
      S = S + (double)v.w;
    }
    for (; r < rows; ++r) S = S + (double)T[tid][r];
    partials[(size_t)blockIdx.x * 3 + tid] = S;
  }
}

// losses <- the chunk partials (n_chunks, 3) added per column in ascending chunk order from +0.0:
// the block stages PPO_FSTAGE chunks at a time through LDS (coalesced), three lanes add them
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_finish(const long long M, const long long n_chunks,
                                                            const double *partials, const float entropy_cost,
                                                            float *losses) {
  __shared__ double P[3 * PPO_FSTAGE];
  __shared__ double S[3];
  const int tid = threadIdx.x;
  double T = 0.0;
  for (long long c0 = 0; c0 < n_chunks; c0 += PPO_FSTAGE) {
    const int n = n_chunks - c0 < PPO_FSTAGE ? (int)(n_chunks - c0) : PPO_FSTAGE;
    for (int e = tid; e < 3 * n; e += PPO_THREADS) P[e] = partials[(size_t)c0 * 3 + e];
    __syncthreads();
    if (tid < 3) {
#pragma unroll 8
      for (int c = 0; c < n; ++c) T = T + P[3 * c + tid];
    }
    __syncthreads();
  }
  if (tid < 3) S[tid] = T;
  __syncthreads();
  if (tid == 0) pob_ppo_finish(S[0], S[1], S[2], M, entropy_cost, losses);
}

static int ppo_chunks(long long M, long long *n_chunks) {
  if (M < 1) return pob_fail_msg(POB_EINVAL, "ppo_loss: the row count M must be positive");
  if (M > 0xFFFFFFFELL) return pob_fail_msg(POB_EINVAL, "ppo_loss: too many rows (M A must be below 2^32 - 1)");
  *n_chunks = (M + POB_PPO_CHUNK - 1) / POB_PPO_CHUNK;
  return POB_OK;
}

extern "C" {

int pob_ppo_loss_workspace_bytes(long long M, long long *bytes) {
  if (!bytes) return pob_fail_msg(POB_EINVAL, "ppo_loss: bytes is NULL");
  long long n_chunks;
  const int rc = ppo_chunks(M, &n_chunks);
  if (rc != POB_OK) return rc;
  // the chunk partials (n_chunks, 3) float64, then the rows' summands (3, M) float32
  *bytes = n_chunks * 3 * (long long)sizeof(double) + ((3 * M * (long long)sizeof(float) + 7) & ~7LL);
  return POB_OK;
}

int pob_ppo_loss(long long M, int A, const float *logits, const float *values, const int32_t *idx, const float *raw,
                 const float *old_logp, const float *advantages, const float *vs, const uint32_t *key, float entropy_cost,
                 float ppo_epsilon, float *dlogits, float *dvalues, float *losses, double *workspace, void *stream) {
  long long n_chunks;
  const int rc = ppo_chunks(M, &n_chunks);
  if (rc != POB_OK) return rc;
  if (A < 1 || A > POB_PPO_MAX_A) return pob_fail_msg(POB_EINVAL, "ppo_loss: the action size A must be in 1 .. 128");
  if (M * A >= 4294967295LL) return pob_fail_msg(POB_EINVAL, "ppo_loss: too many action elements (M A must be below 2^32 - 1)");
  if (!logits || !values || !raw || !old_logp || !advantages || !vs)
    return pob_fail_msg(POB_EINVAL, "ppo_loss: NULL argument (logits, values, raw, old_logp, advantages, vs)");
  if (!key) return pob_fail_msg(POB_EINVAL, "ppo_loss: key is NULL");
  if (!losses || !workspace) return pob_fail_msg(POB_EINVAL, "ppo_loss: NULL argument (losses, workspace)");
  const int R = PPO_ELEMS / A < PPO_MAX_ROWS ? PPO_ELEMS / A : PPO_MAX_ROWS;
  const long long tiles = (M + R - 1) / R;
  hipStream_t st = (hipStream_t)stream;
  float *terms = (float *)(workspace + n_chunks * 3);
  const float inv_m = 1.0f / (float)M;
  hipLaunchKernelGGL(k_ppo_loss, dim3((unsigned)tiles), dim3(PPO_THREADS), 0, st, M, A, R, logits, values, idx, raw, old_logp,
                     advantages, vs, key, entropy_cost, ppo_epsilon, inv_m, dlogits, dvalues, terms);
  hipLaunchKernelGGL(k_ppo_chunks, dim3((unsigned)n_chunks), dim3(PPO_THREADS), 0, st, M, (const float *)terms, workspace);
  hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(PPO_THREADS), 0, st, M, n_chunks, (const double *)workspace, entropy_cost, losses);
  return mlp_hip_check(hipGetLastError(), "k_ppo_loss launch");
}

}  // extern "C"
