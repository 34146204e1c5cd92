// pob_blockwalk.h -- the dealing arithmetic of the four-lane kernel's block-cooperative wall
// walk (pob_quad.h qwalls_detect_block): plain integer code, compiled for the device and, with
// POB_BW_HOST, for the host (tests/test_block_walk_host.py drives it for four waves x 64 lanes).
//
// A 256-thread block's four waves pool the face items of a collide substep.  Each wave owns a
// segment of the exchange area (its own LDS region's former contact pool): QBW_WCAP item slots
// of QBW_SLOT_DW dwords and the wave's item count.  An item slot holds
//   * after the publish: the item's record in dwords 0 .. 7 (the owner's segment end points A,
//     B, its radius, and meta = face bit | capsule flag << 6 | body slot << 7) and meta again
//     in dword 10 -- written by the owner wave, lane by lane in lane order, each lane's items
//     in its walk order (slot, then bit);
//   * after the evaluation: the two triangles' contact records of QBW_CON_DW floats (tau, n,
//     dist -- dist's bit pattern QBW_NO_CONTACT for a triangle without a contact) in dwords
//     0 .. 4 and 5 .. 9, over the record, which only the evaluating group read (its eight lanes
//     read it at the top of the round and write at its end, in one wave's program order), and
//     meta still in dword 10 for the owner -- contact slot c = 2 j + t for triangle t of item j.
// The block's items are numbered wave by wave (item i = segment w's item j, i = off[w] + j);
// round r holds items 8 r .. 8 r + 7, one per group of eight lanes, and wave w evaluates the
// rounds r = (w + substep) mod 4, + 4, + 8, ..
#pragma once
#include <stdint.h>
#ifdef POB_BW_HOST
#define POB_BW_D static inline
#else
#define POB_BW_D __device__ __forceinline__
#endif

#define QBW_WAVES 4
#define QBW_WCAP 50     // items of a wave's segment
#define QBW_SLOT_DW 11
#define QBW_CON_DW 5
#define QBW_LANE_MAX 64  // a lane's item count saturates here (> QBW_WCAP: its wave overflows)
#define QBW_CAP (QBW_WAVES * QBW_WCAP)  // the block's item capacity (a launch may lower it)
#define QBW_SEG_FLOATS (QBW_WCAP * QBW_SLOT_DW + 1)
#define QBW_NO_CONTACT (-1)  // (int bits of dist: a NaN no contact carries)

// offsets (floats) inside a wave's segment
POB_BW_D constexpr int bw_item_off(const int j) { return QBW_SLOT_DW * j; }
POB_BW_D constexpr int bw_meta_off(const int j) { return QBW_SLOT_DW * j + 2 * QBW_CON_DW; }
POB_BW_D constexpr int bw_con_off(const int c) { return QBW_SLOT_DW * (c >> 1) + QBW_CON_DW * (c & 1); }  // c = 2 j + t
POB_BW_D constexpr int bw_count_off() { return QBW_WCAP * QBW_SLOT_DW; }

// meta word of an item record
POB_BW_D constexpr int bw_meta(const int bit, const bool seg, const int slot) { return bit | (seg ? 64 : 0) | (slot << 7); }
POB_BW_D constexpr int bw_meta_bit(const int m) { return m & 63; }
POB_BW_D constexpr bool bw_meta_seg(const int m) { return (m & 64) != 0; }
POB_BW_D constexpr int bw_meta_slot(const int m) { return (m >> 7) & 3; }

// a lane's item count as published (saturated)
POB_BW_D int bw_lane_count(const uint64_t m0, const uint64_t m1, const uint64_t m2) {
  const int n = __builtin_popcountll(m0) + __builtin_popcountll(m1) + __builtin_popcountll(m2);
  return n < QBW_LANE_MAX ? n : QBW_LANE_MAX;
}
// The wave's exclusive prefix of the lanes' counts, one ballot per bit of the count: after
// step b = 0 .. 6 with m = the ballot of (count >> b) & 1, base = the items of the lanes below
// this one, tot = the wave's
POB_BW_D void bw_prefix_step(const uint64_t m, const int lane, const int b, int &base, int &tot) {
  base += __builtin_popcountll(m & ((1ull << lane) - 1ull)) << b;
  tot += __builtin_popcountll(m) << b;
}
#define QBW_PREFIX_BITS 7  // (QBW_LANE_MAX = 64 needs bits 0 .. 6)
// a wave none of whose lanes holds 4 items or more needs steps 0 and 1 only (the ballots of the
// higher bits are empty: their steps add nothing)
#define QBW_PREFIX_SHORT_BITS 2
POB_BW_D constexpr bool bw_prefix_needs_all(const int count) { return count >= (1 << QBW_PREFIX_SHORT_BITS); }

// the lane's next item in walk order -- the lowest set bit of the first slot with one -- taken
// out of M; false when the lane has none left
POB_BW_D bool bw_next_item(uint64_t (&M)[3], int &slot, int &bit) {
  const bool h0 = M[0] != 0ull, h1 = M[1] != 0ull, h2 = M[2] != 0ull;
  const bool has = h0 | h1 | h2;
  slot = h0 ? 0 : (h1 ? 1 : 2);
  const uint64_t ml = h0 ? M[0] : (h1 ? M[1] : M[2]);
  bit = has ? __builtin_ctzll(ml) : 0;
  const uint64_t pop = has ? ml & (0ull - ml) : 0ull;
  M[0] = h0 ? M[0] & ~pop : M[0];
  M[1] = (!h0 & h1) ? M[1] & ~pop : M[1];
  M[2] = (!h0 & !h1) ? M[2] & ~pop : M[2];
  return has;
}

// The block's deal of a collide substep, from the four waves' counts (every wave computes it
// from the same four LDS words, so it is block-uniform): the segments' first item numbers,
// the total, and whether the block overflows -- a wave's count above its segment, or the total
// above cap.  An overflowing block evaluates and applies nothing (T = 0) and goes to the fix-up
// launch after its last substep.
struct BwDeal {
  int off[QBW_WAVES];
  int T;     // items to evaluate
  bool ovf;
};
POB_BW_D BwDeal bw_deal(const int n0, const int n1, const int n2, const int n3, const int cap) {
  BwDeal d;
  d.off[0] = 0; d.off[1] = n0; d.off[2] = n0 + n1; d.off[3] = n0 + n1 + n2;
  const int T = n0 + n1 + n2 + n3;
  d.ovf = (T > cap) | (n0 > QBW_WCAP) | (n1 > QBW_WCAP) | (n2 > QBW_WCAP) | (n3 > QBW_WCAP);
  d.T = d.ovf ? 0 : T;
  return d;
}
POB_BW_D int bw_rounds(const BwDeal &d) { return (d.T + 7) >> 3; }
// wave w's first round of collide substep sub (its rounds follow at a stride of QBW_WAVES)
POB_BW_D int bw_first_round(const int w, const int sub) { return (w + sub) & (QBW_WAVES - 1); }
// item i (< d.T) -> its segment (the owner wave) and its number there
POB_BW_D void bw_item_owner(const BwDeal &d, const int i, int &w, int &j) {
  w = (i >= d.off[1] ? 1 : 0) + (i >= d.off[2] ? 1 : 0) + (i >= d.off[3] ? 1 : 0);
  j = i - (w == 0 ? 0 : (w == 1 ? d.off[1] : (w == 2 ? d.off[2] : d.off[3])));
}
// the owner's enumeration: the contact slots [c0, c1) of a lane holding n items from segment
// item base on -- item by item in walk order, triangle 0 then 1 -- none in an overflowing block
POB_BW_D void bw_apply_range(const int base, const int n, const bool ovf, int &c0, int &c1) {
  c0 = 2 * base;
  c1 = ovf ? c0 : 2 * (base + n);
}
// the same range cut by body: a lane publishes its items slot by slot (bw_next_item), so the
// contact slots of body l's n_l items are [c[l], c[l + 1]), c[0] = c0 and c[3] = c1 of
// bw_apply_range (n = n0 + n1 + n2: a count that saturates overflows its wave) -- all four
// equal in an overflowing block
POB_BW_D void bw_body_ranges(const int base, const int n0, const int n1, const int n2, const bool ovf, int (&c)[4]) {
  c[0] = 2 * base;
  c[1] = ovf ? c[0] : c[0] + 2 * n0;
  c[2] = ovf ? c[0] : c[1] + 2 * n1;
  c[3] = ovf ? c[0] : c[2] + 2 * n2;
}

// The torso's items once per lane quad (pob_quad.h qwalls_detect_block): the four lanes of a
// quad (lanes 4 e .. 4 e + 3 of a wave: one env) hold bit-identical replicas of the torso, so
// only the quad's lane 0 counts and publishes the torso's items -- n0 of them, from its own
// base base0 on -- and all four lanes apply the torso's contacts from those slots.
POB_BW_D constexpr bool bw_quad_lead(const int lane) { return (lane & 3) == 0; }
// the torso items a lane publishes and counts into its lane count
POB_BW_D constexpr int bw_quad_torso_count(const int lane, const int n0) { return bw_quad_lead(lane) ? n0 : 0; }
// The ranges of a lane: the torso's contact slots [c[0], c[1]) -- the quad's lane-0 slots, base0
// that lane's prefix base -- and the lane's own Aux and lower-leg slots [c[2], c[3]) and
// [c[3], c[4]), which start at the lane's own base (behind the torso's in the quad's lane 0).
// All empty in an overflowing block.
POB_BW_D void bw_quad_ranges(const int lane, const int base0, const int n0, const int base, const int n1, const int n2,
                             const bool ovf, int (&c)[5]) {
  c[0] = 2 * base0;
  c[1] = ovf ? c[0] : c[0] + 2 * n0;
  c[2] = 2 * (base + bw_quad_torso_count(lane, n0));
  c[3] = ovf ? c[2] : c[2] + 2 * n1;
  c[4] = ovf ? c[2] : c[3] + 2 * n2;
}

// One hit scan per collide substep (pob_quad.h qwalls_detect_block): after the evaluation a lane
// reads the two dist words of each item of a body once and keeps "triangle t of the body's item
// i holds a contact" as bit 2 i + t of a 32-bit mask; both apply passes walk the mask's set bits
// (contact slot = the body's first slot + the bit's number), lowest first: the walk order.  A
// body with more than QBW_HIT_ITEMS items (a launch may lower it) does not fit: its wave
// publishes an overflowing count (bw_hit_count), so the block applies nothing and goes to the
// fix-up launch.
#define QBW_HIT_ITEMS 16
POB_BW_D constexpr uint32_t bw_hit_bits(const bool h0, const bool h1, const int i) {
  return ((h0 ? 1u : 0u) | (h1 ? 2u : 0u)) << (2 * i);
}
// the wave's count as published: wide = some lane of the wave holds a body past the mask's width
POB_BW_D constexpr int bw_hit_count(const int tot, const bool wide) { return wide && tot <= QBW_WCAP ? QBW_WCAP + 1 : tot; }
