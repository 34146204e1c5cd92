// Host model of one collide substep of the four-lane kernel's block-cooperative wall walk,
// built on the kernel's own dealing helpers (po-brax_amd/csrc/pob_blockwalk.h): four waves x
// 64 lanes publish their items, the block deals the rounds, every owner enumerates its contact
// slots.  The flow mirrors pob_quad.h qwalls_detect_block -- publish, barrier 1, evaluate,
// barrier 2, apply -- with each wave counting the barriers it passes.
// Shared library for tests/test_block_walk_host.py; with -DBW_MAIN a stand-alone self-check.
#define POB_BW_HOST 1
#include "pob_blockwalk.h"
#include <stdint.h>
#include <string.h>

struct Rec { int lane, meta; };

// masks: [4][64][3] item masks.  dead_mask: bit w = wave w is past the batch (publishes nothing).
// Outputs: n_wave[4] published counts, evals[4][QBW_WCAP] evaluations per segment item,
// rounds[4] rounds run per wave, barriers[4], info[4] = {T, ovf, order_ok, slots_ok}.
extern "C" int bw_substep(const uint64_t *masks, int cap, int sub, int dead_mask, int *n_wave, int *evals,
                          int *rounds, int *barriers, int *info) {
  static Rec rec[QBW_WAVES][QBW_WCAP];
  static int con[QBW_WAVES][2 * QBW_WCAP];  // the (item, triangle) slot's writer: 1 + evaluating wave
  static int where[QBW_WAVES][QBW_SEG_FLOATS];  // who uses a segment dword: 1 + contact slot
  int base[QBW_WAVES][64], nl[QBW_WAVES][64];
  memset(rec, 0xff, sizeof(rec));
  memset(con, 0, sizeof(con));
  memset(where, 0, sizeof(where));
  memset(evals, 0, sizeof(int) * QBW_WAVES * QBW_WCAP);
  // ---- publish (per wave), then barrier 1
  for (int w = 0; w < QBW_WAVES; ++w) {
    uint64_t M[64][3];
    for (int t = 0; t < 64; ++t)
      for (int s = 0; s < 3; ++s) M[t][s] = ((dead_mask >> w) & 1) ? 0ull : masks[(w * 64 + t) * 3 + s];
    for (int t = 0; t < 64; ++t) nl[w][t] = bw_lane_count(M[t][0], M[t][1], M[t][2]);
    int tot = 0;
    for (int t = 0; t < 64; ++t) base[w][t] = 0;
    for (int b = 0; b < QBW_PREFIX_BITS; ++b) {
      uint64_t m = 0ull;  // the ballot
      for (int t = 0; t < 64; ++t) m |= (uint64_t)((nl[w][t] >> b) & 1) << t;
      int tt = 0;
      for (int t = 0; t < 64; ++t) { tt = tot; bw_prefix_step(m, t, b, base[w][t], tt); }
      tot = tt;
    }
    for (int t = 0; t < 64; ++t) {
      int at = base[w][t];
      for (int k = 0; k < QBW_LANE_MAX; ++k) {
        int s, bit;
        if (!bw_next_item(M[t], s, bit)) break;
        if (at < QBW_WCAP) {
          if (rec[w][at].lane != -1) return 1;  // a record slot written twice
          rec[w][at].lane = t;
          rec[w][at].meta = bw_meta(bit, s != 0, s);
        }
        ++at;
      }
    }
    n_wave[w] = tot;
    barriers[w] = 1;
  }
  // ---- the deal (block-uniform), evaluation (per wave), then barrier 2
  const BwDeal d = bw_deal(n_wave[0], n_wave[1], n_wave[2], n_wave[3], cap);
  const int R = bw_rounds(d);
  for (int w = 0; w < QBW_WAVES; ++w) {
    rounds[w] = 0;
    for (int r = bw_first_round(w, sub); r < R; r += QBW_WAVES) {
      ++rounds[w];
      for (int g = 0; g < 8; ++g) {
        const int i = 8 * r + g;
        if (i >= d.T) continue;
        int ow, j;
        bw_item_owner(d, i, ow, j);
        if (ow < 0 || ow >= QBW_WAVES || j < 0 || j >= n_wave[ow] || j >= QBW_WCAP) return 2;
        if (rec[ow][j].lane < 0) return 3;  // an item that nobody published
        ++evals[ow * QBW_WCAP + j];
        for (int t = 0; t < 2; ++t) {
          if (con[ow][2 * j + t] != 0) return 4;  // a contact slot written twice
          con[ow][2 * j + t] = 1 + w;
          // the contact record lies inside its item's slot, below the owner's meta word, and
          // shares no dword with another record
          for (int q = 0; q < QBW_CON_DW; ++q) {
            const int o = bw_con_off(2 * j + t) + q;
            if (o < bw_item_off(j) || o >= bw_meta_off(j) || o >= bw_count_off() || where[ow][o] != 0) return 5;
            where[ow][o] = 1 + 2 * j + t;
          }
        }
      }
    }
    barriers[w] += 1;
  }
  // ---- apply: every owner's enumeration, against its masks' walk order
  int order_ok = 1, slots_ok = 1;
  for (int w = 0; w < QBW_WAVES; ++w)
    for (int t = 0; t < 64; ++t) {
      int c0, c1;
      bw_apply_range(base[w][t], nl[w][t], d.ovf, c0, c1);
      uint64_t M[3];
      for (int s = 0; s < 3; ++s) M[s] = ((dead_mask >> w) & 1) ? 0ull : masks[(w * 64 + t) * 3 + s];
      long prev = -1;
      for (int c = c0; c < c1; ++c) {
        const int j = c >> 1, tri = c & 1;
        if (j >= QBW_WCAP || rec[w][j].lane != t || con[w][c] == 0) { slots_ok = 0; continue; }
        const int m = rec[w][j].meta;
        const long key = ((long)bw_meta_slot(m) * 64 + bw_meta_bit(m)) * 2 + tri;
        if (key <= prev) order_ok = 0;
        prev = key;
        if (tri == 0) {  // the item is the lane's next in walk order
          int s, bit;
          if (!bw_next_item(M, s, bit) || s != bw_meta_slot(m) || bit != bw_meta_bit(m)) order_ok = 0;
        }
      }
      if (!d.ovf && (M[0] | M[1] | M[2]) != 0ull) slots_ok = 0;  // items left unvisited
    }
  info[0] = d.T; info[1] = d.ovf ? 1 : 0; info[2] = order_ok; info[3] = slots_ok;
  return 0;
}

#ifdef BW_MAIN
#include <stdio.h>
#include <stdlib.h>
static uint64_t rnd(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main() {
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * QBW_WAVES * 64 * 3);
  int n_wave[QBW_WAVES], rounds[QBW_WAVES], barriers[QBW_WAVES], info[4];
  int *evals = (int *)malloc(sizeof(int) * QBW_WAVES * QBW_WCAP);
  int n_ovf = 0;
  for (int it = 0; it < 2000; ++it) {
    const int dens = (int)(rnd(seed) % 40);  // per-mille of lanes holding items
    for (int i = 0; i < QBW_WAVES * 64 * 3; ++i) {
      masks[i] = 0ull;
      if ((int)(rnd(seed) % 1000) < dens) masks[i] = rnd(seed) & rnd(seed) & rnd(seed) & 0xFFFFFFFFFFFFull;
    }
    if (it % 7 == 0) masks[(int)(rnd(seed) % (QBW_WAVES * 64 * 3))] = rnd(seed) & 0xFFFFFFFFFFFFull;  // one heavy lane
    const int cap = it % 3 == 0 ? 16 : QBW_CAP, sub = it % 5, dead = it % 11 == 0 ? 0xE : 0;
    const int rc = bw_substep(masks, cap, sub, dead, n_wave, evals, rounds, barriers, info);
    if (rc != 0) { printf("case %d: rc %d\n", it, rc); return 1; }
    int tot = 0, big = 0;
    for (int w = 0; w < QBW_WAVES; ++w) { tot += n_wave[w]; big |= n_wave[w] > QBW_WCAP; }
    const int ovf = tot > cap || big;
    if (info[1] != ovf || !info[2] || !info[3]) { printf("case %d: ovf %d/%d order %d slots %d\n", it, info[1], ovf, info[2], info[3]); return 1; }
    for (int w = 0; w < QBW_WAVES; ++w) {
      if (barriers[w] != 2) { printf("case %d: wave %d barriers %d\n", it, w, barriers[w]); return 1; }
      for (int j = 0; j < QBW_WCAP; ++j)
        if (evals[w * QBW_WCAP + j] != (!ovf && j < n_wave[w] ? 1 : 0)) { printf("case %d: item (%d, %d) evaluated %d times\n", it, w, j, evals[w * QBW_WCAP + j]); return 1; }
    }
    n_ovf += ovf;
  }
  printf("block walk host model: 2000 cases OK (%d overflowing)\n", n_ovf);
  free(masks); free(evals);
  return 0;
}
#endif
