// Host model of the per-body publish and apply ranges of the four-lane kernel's block-cooperative
// wall walk, built on the kernel's own helpers (po-brax_amd/csrc/pob_blockwalk.h): four waves x
// 64 lanes publish their items body by body (the loops of pob_quad.h qwalls_detect_block), the
// block deals, and every owner cuts its contact slots by body (bw_body_ranges).  Checked here
// against the walk-order publish (bw_next_item) and the whole range (bw_apply_range).
// Shared library for tests/test_body_ranges_host.py; with -DBR_MAIN a stand-alone self-check.
#define POB_BW_HOST 1
#include "pob_blockwalk.h"
#include <stdint.h>
#include <string.h>

struct Rec { int lane, meta; };

// masks: [4][64][3] item masks.  dead_mask: bit w = wave w is past the batch (publishes nothing).
// Outputs: ranges[4][64][4] = bw_body_ranges of every lane, info[4] = {ovf, tiles_ok, order_ok,
// publish_ok}:
//   tiles_ok    c[0], c[3] are bw_apply_range's c0, c1 and c[0] <= c[1] <= c[2] <= c[3];
//   order_ok    every contact slot of [c[l], c[l + 1]) belongs to an item of this lane on body l,
//               and the slots of the whole range follow the lane's walk order;
//   publish_ok  the body-by-body publish writes the records the walk-order publish writes.
extern "C" int br_substep(const uint64_t *masks, int cap, int dead_mask, int *ranges, int *info) {
  static Rec rec[QBW_WAVES][QBW_WCAP], rec_walk[QBW_WAVES][QBW_WCAP];
  int base[QBW_WAVES][64], nl[QBW_WAVES][64], nb[QBW_WAVES][64][3], n_wave[QBW_WAVES];
  memset(rec, 0xff, sizeof(rec));
  memset(rec_walk, 0xff, sizeof(rec_walk));
  for (int w = 0; w < QBW_WAVES; ++w) {
    uint64_t M[64][3];
    for (int t = 0; t < 64; ++t)
      for (int s = 0; s < 3; ++s) M[t][s] = ((dead_mask >> w) & 1) ? 0ull : masks[(w * 64 + t) * 3 + s];
    for (int t = 0; t < 64; ++t) {
      nl[w][t] = bw_lane_count(M[t][0], M[t][1], M[t][2]);
      for (int s = 0; s < 3; ++s) nb[w][t][s] = __builtin_popcountll(M[t][s]);
      base[w][t] = 0;
    }
    int tot = 0;
    for (int b = 0; b < QBW_PREFIX_BITS; ++b) {
      uint64_t m = 0ull;  // the ballot
      for (int t = 0; t < 64; ++t) m |= (uint64_t)((nl[w][t] >> b) & 1) << t;
      int tt = 0;
      for (int t = 0; t < 64; ++t) { tt = tot; bw_prefix_step(m, t, b, base[w][t], tt); }
      tot = tt;
    }
    n_wave[w] = tot;
    for (int t = 0; t < 64; ++t) {
      // the kernel's publish: three body loops, the lowest bit first
      int at = base[w][t];
      for (int l = 0; l < 3; ++l) {
        uint64_t m = M[t][l];
        while (m != 0ull) {
          const int bit = __builtin_ctzll(m);
          m &= m - 1ull;
          if (at < QBW_WCAP) {
            if (rec[w][at].lane != -1) return 1;  // a record slot written twice
            rec[w][at].lane = t;
            rec[w][at].meta = bw_meta(bit, l != 0, l);
          }
          ++at;
        }
      }
      // the walk-order publish
      uint64_t W[3] = {M[t][0], M[t][1], M[t][2]};
      at = base[w][t];
      for (int k = 0; k < QBW_LANE_MAX; ++k) {
        int s, bit;
        if (!bw_next_item(W, s, bit)) break;
        if (at < QBW_WCAP) { rec_walk[w][at].lane = t; rec_walk[w][at].meta = bw_meta(bit, s != 0, s); }
        ++at;
      }
    }
  }
  const BwDeal d = bw_deal(n_wave[0], n_wave[1], n_wave[2], n_wave[3], cap);
  // (an overflowing wave's records past a saturated lane differ in nothing that is read: the
  // block applies nothing)
  int publish_ok = 1;
  if (!d.ovf && memcmp(rec, rec_walk, sizeof(rec)) != 0) publish_ok = 0;
  int tiles_ok = 1, order_ok = 1;
  for (int w = 0; w < QBW_WAVES; ++w)
    for (int t = 0; t < 64; ++t) {
      int c[4], c0, c1;
      bw_body_ranges(base[w][t], nb[w][t][0], nb[w][t][1], nb[w][t][2], d.ovf, c);
      bw_apply_range(base[w][t], nl[w][t], d.ovf, c0, c1);
      for (int i = 0; i < 4; ++i) ranges[(w * 64 + t) * 4 + i] = c[i];
      if (c[0] != c0 || c[3] != c1 || c[0] > c[1] || c[1] > c[2] || c[2] > c[3]) tiles_ok = 0;
      long prev = -1;
      for (int l = 0; l < 3; ++l)
        for (int k = c[l]; k < c[l + 1]; ++k) {
          const int j = k >> 1;
          if (j >= QBW_WCAP || rec[w][j].lane != t || bw_meta_slot(rec[w][j].meta) != l) { order_ok = 0; continue; }
          const long key = ((long)l * 64 + bw_meta_bit(rec[w][j].meta)) * 2 + (k & 1);
          if (key <= prev) order_ok = 0;
          prev = key;
        }
    }
  info[0] = d.ovf ? 1 : 0; info[1] = tiles_ok; info[2] = order_ok; info[3] = publish_ok;
  return 0;
}

#ifdef BR_MAIN
#include <stdio.h>
#include <stdlib.h>
static uint64_t rnd(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main() {
  uint64_t seed = 0xD1B54A32D192ED03ull;
  uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * QBW_WAVES * 64 * 3);
  int *ranges = (int *)malloc(sizeof(int) * QBW_WAVES * 64 * 4);
  int info[4], n_ovf = 0;
  for (int it = 0; it < 2000; ++it) {
    const int dens = (int)(rnd(seed) % 40);  // per-mille of lanes holding items
    for (int i = 0; i < QBW_WAVES * 64 * 3; ++i) {
      masks[i] = 0ull;
      if ((int)(rnd(seed) % 1000) < dens) masks[i] = rnd(seed) & rnd(seed) & rnd(seed) & 0xFFFFFFFFFFFFull;
    }
    if (it % 7 == 0) masks[(int)(rnd(seed) % (QBW_WAVES * 64 * 3))] = rnd(seed) & 0xFFFFFFFFFFFFull;  // one heavy lane
    if (it % 97 == 0) for (int s = 0; s < 3; ++s) masks[5 * 3 + s] = 0xFFFFFFFFFFFFull;                // a saturated lane
    const int cap = it % 3 == 0 ? 16 : QBW_CAP, dead = it % 11 == 0 ? 0xE : 0;
    const int rc = br_substep(masks, cap, dead, ranges, info);
    if (rc != 0) { printf("case %d: rc %d\n", it, rc); return 1; }
    if (!info[1] || !info[2] || !info[3]) { printf("case %d: tiles %d order %d publish %d\n", it, info[1], info[2], info[3]); return 1; }
    if (info[0])
      for (int i = 0; i < QBW_WAVES * 64; ++i)
        if (ranges[4 * i] != ranges[4 * i + 3]) { printf("case %d: lane %d keeps a range in an overflowing block\n", it, i); return 1; }
    n_ovf += info[0];
  }
  printf("body ranges host model: 2000 cases OK (%d overflowing)\n", n_ovf);
  free(masks); free(ranges);
  return 0;
}
#endif
