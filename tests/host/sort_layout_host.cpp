// The radix sort's workspace layout (pob_sort_layout_of of po-brax_amd/csrc/pob_sort.h) walked on the
// host: for n over 1 .. 3 TILE + 1 and a few large values up to 2^31 - 1 every region is aligned,
// inside the workspace, disjoint from the others, and large enough for what the kernels keep in it.
// A stand-alone program: tests/test_sort_api.py builds it with -fsanitize=address,undefined.
#include <cstdio>

#include "pob_sort.h"

static int check(long long n) {
  const pob_sort_layout L = pob_sort_layout_of(n);
  const long long tiles = (n + POB_SORT_TILE - 1) / POB_SORT_TILE;
  const long long off[7] = {L.subs, L.totals, L.counts, L.keys[0], L.keys[1], L.vals[0], L.vals[1]};
  const long long len[7] = {POB_SORT_MAX_ROUNDS * 2 * 4LL, POB_SORT_RADIX * 4LL, POB_SORT_RADIX * tiles * 4LL,
                            4 * n, 4 * n, 4 * n, 4 * n};
  if (L.tiles != tiles || L.subs != 0 || L.bytes <= 0) return 1;
  for (int a = 0; a < 7; ++a) {
    if (off[a] < 0 || off[a] % POB_SORT_ALIGN != 0 || off[a] + len[a] > L.bytes) return 2;
    for (int b = 0; b < a; ++b)
      if (off[a] < off[b] + len[b] && off[b] < off[a] + len[a]) return 3;
  }
  return 0;
}

int main() {
  long long cases = 0, last = 0;
  for (long long n = 1; n <= 3 * POB_SORT_TILE + 1; ++n, ++cases) {
    const int rc = check(n);
    if (rc) return printf("n = %lld: layout check %d failed\n", n, rc), 1;
    const long long bytes = pob_sort_layout_of(n).bytes;
    if (bytes < last) return printf("n = %lld: workspace shrinks\n", n), 1;
    last = bytes;
  }
  const long long large[] = {POB_SORT_SCAN_CHUNK * (long long)POB_SORT_TILE + 1, 1310720, (1LL << 24) - 1, 1LL << 30,
                             (1LL << 31) - POB_SORT_TILE, (1LL << 31) - 1};
  for (long long n : large) {
    const int rc = check(n);
    if (rc) return printf("n = %lld: layout check %d failed\n", n, rc), 1;
    ++cases;
  }
  printf("%lld cases OK\n", cases);
  return 0;
}
