// Host model of "the torso's items once per lane quad" in the four-lane kernel's block-cooperative
// wall walk, built on the kernel's own helpers (po-brax_amd/csrc/pob_blockwalk.h bw_quad_lead,
// bw_quad_torso_count, bw_quad_ranges): four waves x 64 lanes, a quad = lanes 4 e .. 4 e + 3 (one
// env, the torso replicated in its four lanes).  As pob_quad.h qwalls_detect_block does, every
// lane takes the torso's mask from its quad's lane 0, only that lane counts and publishes the
// torso's items, the prefix runs two steps when no lane of the wave holds four items or more and
// all seven otherwise, and every lane cuts its contact slots with bw_quad_ranges.
// Shared library for tests/test_quad_ranges_host.py; with -DQR_MAIN a stand-alone self-check.
#define POB_BW_HOST 1
#include "pob_blockwalk.h"
#include <stdint.h>
#include <string.h>

struct Rec { int lane, meta; };

// masks: [4][64][3] item masks (the torso's, [..][0], read from the quad's lane 0 only).
// dead_mask: bit w = wave w is past the batch (publishes nothing).
// Outputs: ranges[4][64][5] = bw_quad_ranges of every lane, counts[4] = the waves' published item
// counts, info[6] = {ovf, lead_ok, torso_ok, own_ok, cover_ok, prefix_ok}:
//   lead_ok    every published torso record comes from a quad's lane 0;
//   torso_ok   a lane's torso range holds exactly its quad's lane-0 torso records, in walk order;
//   own_ok     a lane's own ranges hold exactly its Aux, then its lower-leg records, in walk order;
//   cover_ok   every contact slot of every published item lies in the torso range of exactly the
//              four lanes of the publishing quad (a torso item) or in an own range of exactly the
//              publishing lane (an Aux / lower-leg item), and in no other range;
//   prefix_ok  the shortened prefix gives the bases and the total of all seven steps.
extern "C" int qr_substep(const uint64_t *masks, int cap, int dead_mask, int *ranges, int *counts, int *info) {
  static Rec rec[QBW_WAVES][QBW_WCAP];
  static int cover_t[QBW_WAVES][2 * QBW_WCAP][4], cover_o[QBW_WAVES][2 * QBW_WCAP];
  int base[QBW_WAVES][64], n0[QBW_WAVES][64], nb[QBW_WAVES][64][3], n_wave[QBW_WAVES];
  memset(rec, 0xff, sizeof(rec));
  memset(cover_t, 0, sizeof(cover_t));
  memset(cover_o, 0, sizeof(cover_o));
  int lead_ok = 1, prefix_ok = 1;
  for (int w = 0; w < QBW_WAVES; ++w) {
    uint64_t M[64][3];
    int nl[64];
    for (int t = 0; t < 64; ++t)
      for (int s = 0; s < 3; ++s) M[t][s] = ((dead_mask >> w) & 1) ? 0ull : masks[(w * 64 + t) * 3 + s];
    for (int t = 0; t < 64; ++t) {
      const uint64_t m0q = M[t & ~3][0];  // the quad broadcast of lane 0's torso mask
      n0[w][t] = __builtin_popcountll(m0q);
      M[t][0] = bw_quad_lead(t) ? m0q : 0ull;
      nb[w][t][0] = bw_quad_torso_count(t, n0[w][t]);
      nb[w][t][1] = __builtin_popcountll(M[t][1]);
      nb[w][t][2] = __builtin_popcountll(M[t][2]);
      if (nb[w][t][0] != __builtin_popcountll(M[t][0])) return 2;
      nl[t] = bw_lane_count(M[t][0], M[t][1], M[t][2]);
    }
    // the prefix: steps 0 and 1 when no lane holds four items or more, else all seven
    bool big = false;
    for (int t = 0; t < 64; ++t) big |= nl[t] >= 4;
    int tot = 0, tot_full = 0, base_full[64];
    for (int t = 0; t < 64; ++t) { base[w][t] = 0; base_full[t] = 0; }
    for (int b = 0; b < QBW_PREFIX_BITS; ++b) {
      uint64_t m = 0ull;  // the ballot
      for (int t = 0; t < 64; ++t) m |= (uint64_t)((nl[t] >> b) & 1) << t;
      int tt = 0, tf = 0;
      for (int t = 0; t < 64; ++t) {
        tf = tot_full; bw_prefix_step(m, t, b, base_full[t], tf);
        if (big || b < 2) { tt = tot; bw_prefix_step(m, t, b, base[w][t], tt); }
      }
      tot_full = tf;
      if (big || b < 2) tot = tt;
    }
    if (tot != tot_full || memcmp(base[w], base_full, sizeof(base_full)) != 0) prefix_ok = 0;
    n_wave[w] = tot;
    counts[w] = tot;
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
            if (l == 0 && !bw_quad_lead(t)) lead_ok = 0;
          }
          ++at;
        }
      }
    }
  }
  const BwDeal d = bw_deal(n_wave[0], n_wave[1], n_wave[2], n_wave[3], cap);
  int torso_ok = 1, own_ok = 1, cover_ok = 1;
  for (int w = 0; w < QBW_WAVES; ++w)
    for (int t = 0; t < 64; ++t) {
      int c[5];
      bw_quad_ranges(t, base[w][t & ~3], n0[w][t], base[w][t], nb[w][t][1], nb[w][t][2], d.ovf, c);
      for (int i = 0; i < 5; ++i) ranges[(w * 64 + t) * 5 + i] = c[i];
      if (c[0] > c[1] || c[2] > c[3] || c[3] > c[4] || c[0] < 0 || c[2] < 0) return 3;
      if (!d.ovf && (c[1] - c[0] != 2 * n0[w][t] || c[3] - c[2] != 2 * nb[w][t][1] || c[4] - c[3] != 2 * nb[w][t][2])) {
        torso_ok = 0; own_ok = 0;
      }
      long prev = -1;
      for (int k = c[0]; k < c[1]; ++k) {  // the torso's slots: the quad's lane 0 published them
        const int j = k >> 1;
        if (j >= QBW_WCAP || rec[w][j].lane != (t & ~3) || bw_meta_slot(rec[w][j].meta) != 0) { torso_ok = 0; continue; }
        const long key = (long)bw_meta_bit(rec[w][j].meta) * 2 + (k & 1);
        if (key <= prev) torso_ok = 0;
        prev = key;
        ++cover_t[w][k][t & 3];
      }
      prev = -1;
      for (int l = 1; l < 3; ++l)
        for (int k = c[l + 1]; k < c[l + 2]; ++k) {
          const int j = k >> 1;
          if (j >= QBW_WCAP || rec[w][j].lane != t || bw_meta_slot(rec[w][j].meta) != l) { own_ok = 0; continue; }
          const long key = ((long)l * 64 + bw_meta_bit(rec[w][j].meta)) * 2 + (k & 1);
          if (key <= prev) own_ok = 0;
          prev = key;
          ++cover_o[w][k];
        }
    }
  for (int w = 0; w < QBW_WAVES; ++w)
    for (int k = 0; k < 2 * QBW_WCAP; ++k) {
      const int j = k >> 1;
      const bool published = !d.ovf && j < n_wave[w];
      const int ct = cover_t[w][k][0] + cover_t[w][k][1] + cover_t[w][k][2] + cover_t[w][k][3];
      if (!published) {
        if (ct != 0 || cover_o[w][k] != 0) cover_ok = 0;
        continue;
      }
      if (bw_meta_slot(rec[w][j].meta) == 0) {
        for (int q = 0; q < 4; ++q)
          if (cover_t[w][k][q] != 1) cover_ok = 0;  // once in each lane of the owning quad
        if (cover_o[w][k] != 0) cover_ok = 0;
      } else if (ct != 0 || cover_o[w][k] != 1) cover_ok = 0;
    }
  info[0] = d.ovf ? 1 : 0; info[1] = lead_ok; info[2] = torso_ok; info[3] = own_ok; info[4] = cover_ok; info[5] = prefix_ok;
  return 0;
}

#ifdef QR_MAIN
#include <stdio.h>
#include <stdlib.h>
static uint64_t rnd(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main() {
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * QBW_WAVES * 64 * 3);
  int *ranges = (int *)malloc(sizeof(int) * QBW_WAVES * 64 * 5);
  int info[6], counts[QBW_WAVES], n_ovf = 0, n_torso = 0;
  for (int it = 0; it < 2000; ++it) {
    const int dens = (int)(rnd(seed) % 40);  // per-mille of masks holding items
    for (int i = 0; i < QBW_WAVES * 64 * 3; ++i) {
      masks[i] = 0ull;
      if ((int)(rnd(seed) % 1000) < dens) masks[i] = rnd(seed) & rnd(seed) & rnd(seed) & 0xFFFFFFFFFFFFull;
    }
    for (int i = 0; i < QBW_WAVES * 64; ++i) masks[3 * i] = masks[3 * (i & ~3)];  // the torso's mask: equal within a quad
    if (it % 7 == 0) masks[(int)(rnd(seed) % (QBW_WAVES * 64 * 3))] = rnd(seed) & 0xFFFFFFFFFFFFull;  // one heavy lane (a torso mask in one lane only: lane 0's still decides)
    if (it % 97 == 0) for (int s = 0; s < 3; ++s) masks[4 * 3 + s] = 0xFFFFFFFFFFFFull;                // a saturated quad lane 0
    const int cap = it % 3 == 0 ? 16 : QBW_CAP, dead = it % 11 == 0 ? 0xE : 0;
    const int rc = qr_substep(masks, cap, dead, ranges, counts, info);
    if (rc != 0) { printf("case %d: rc %d\n", it, rc); return 1; }
    if (!info[1] || !info[2] || !info[3] || !info[4] || !info[5]) {
      printf("case %d: lead %d torso %d own %d cover %d prefix %d\n", it, info[1], info[2], info[3], info[4], info[5]);
      return 1;
    }
    for (int i = 0; i < QBW_WAVES * 64; ++i) {
      const int *c = ranges + 5 * i;
      if (info[0] && (c[0] != c[1] || c[2] != c[4])) { printf("case %d: lane %d keeps a range in an overflowing block\n", it, i); return 1; }
      n_torso += c[1] - c[0];
    }
    n_ovf += info[0];
  }
  printf("quad ranges host model: 2000 cases OK (%d overflowing, %d torso slot reads)\n", n_ovf, n_torso);
  free(masks); free(ranges);
  return 0;
}
#endif
