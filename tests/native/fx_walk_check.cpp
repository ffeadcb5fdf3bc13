// The walk order of the persistent stage 1 (pypulsar_amd/csrc/fx_walk.h) on
// the CPU: for a spread of group counts NG, element-block counts and grid
// sizes, the queues of the 8 XCD shares hand out every (group, element block)
// item exactly once, whichever workgroups drain them, and fx_walk_group is a
// bijection that gives each XCD share 32 adjacent groups of a 256-group run.
// Plain C++, no HIP, no GPU (tests/test_fx_walk.py builds it, also with
// -fsanitize=address,undefined):
//   c++ -std=c++17 -O2 -Ipypulsar_amd/csrc -o build/fx_walk_check tests/native/fx_walk_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fx_walk.h"

using namespace pdd;

// The kernel's queue discipline (fx_take in pdd_sweep.hip): ticket t of queue
// x is item t * 8 + x; an exhausted queue sends the workgroup to the next one.
static int64_t take(std::vector<uint32_t>& queue, int xcd, int64_t n_items) {
  for (int t = 0; t < kFxXcds; ++t) {
    const int x = (xcd + t) % kFxXcds;
    const int64_t i = (int64_t)queue[x]++ * kFxXcds + x;
    if (i < n_items) return i;
  }
  return -1;
}

static int check(int NG, int64_t nblk, int n_wg, unsigned seed) {
  const int64_t n_items = (int64_t)NG * nblk;
  std::vector<int> seen((size_t)n_items, 0);
  std::vector<uint32_t> queue(kFxXcds, 0);
  std::vector<char> live((size_t)n_wg, 1);
  std::vector<int64_t> walked((size_t)n_wg, 0);
  int n_live = n_wg;
  // workgroups take turns in a scrambled order (the hardware's is unknown)
  while (n_live > 0) {
    seed = seed * 1664525u + 1013904223u;
    int w = (int)((seed >> 8) % (unsigned)n_wg);
    while (!live[(size_t)w]) w = (w + 1) % n_wg;
    const int64_t i = take(queue, fx_walk_xcd(w), n_items);
    if (i < 0) {
      live[(size_t)w] = 0;
      --n_live;
      continue;
    }
    const FxWalkItem it = fx_walk_item(i, NG);
    if (it.group < 0 || it.group >= NG || it.block < 0 || it.block >= nblk) {
      fprintf(stderr, "NG %d nblk %lld: item %lld -> (%d, %lld) out of range\n", NG, (long long)nblk,
              (long long)i, it.group, (long long)it.block);
      return 1;
    }
    ++seen[(size_t)(it.block * NG + it.group)];
    ++walked[(size_t)w];
  }
  for (int64_t c = 0; c < n_items; ++c)
    if (seen[(size_t)c] != 1) {
      fprintf(stderr, "NG %d nblk %lld grid %d: (group %lld, block %lld) visited %d times\n", NG,
              (long long)nblk, n_wg, (long long)(c % NG), (long long)(c / NG), seen[(size_t)c]);
      return 1;
    }
  // a grid larger than the item count leaves workgroups without an item
  int64_t total = 0;
  for (int64_t n : walked) total += n;
  if (total != n_items) return 1;
  // the XCD share of a slot: inside whole 256-group runs slot s (walked by XCD
  // s % 8 when the grid is a multiple of 8) maps into the run's 32-group line
  // s % 8; the tail maps to itself
  for (int s = 0; s < NG; ++s) {
    const int g = fx_walk_group(s, NG);
    const bool whole = s < NG / kFxWalkRun * kFxWalkRun;
    if (whole ? (g / kFxWalkRun != s / kFxWalkRun || g % kFxWalkRun / kFxWalkLine != s % kFxXcds)
              : g != s) {
      fprintf(stderr, "NG %d: slot %d -> group %d\n", NG, s, g);
      return 1;
    }
  }
  return 0;
}

int main() {
  const int ngs[] = {1, 3, 7, 8, 16, 33, 61, 255, 256, 257, 300, 512, 1000, 1024};
  const int64_t blocks[] = {1, 2, 5, 33, 257};
  const int grids[] = {1, 5, 8, 64, 1000, 1024};
  int n = 0;
  for (int NG : ngs)
    for (int64_t nblk : blocks)
      for (int grid : grids) {
        if (check(NG, nblk, grid, 12345u + (unsigned)n)) return 1;
        ++n;
      }
  printf("fx_walk ok: %d cases\n", n);
  return 0;
}
