// Walk order of the persistent stage 1 (k_fx_stage1_p, pdd_sweep.hip): plain
// C++, usable on the host and in kernels.  The stage's work is NG groups x
// nblk element blocks = NG * nblk ITEMS, item index i = blk * NG + slot with
// the slot (group) index fastest; workgroup w of a grid of n_wg walks items
// w, w + n_wg, w + 2 n_wg, ...  (tests/native/fx_walk_check.cpp checks that
// every item is visited exactly once.)
//
// Slots map to groups through a permutation inside runs of kFxWalkRun = 256
// slots: workgroup ids go round-robin over the kFxXcds = 8 XCDs, so (with a
// grid that is a multiple of 8) slot s is walked by XCD s % 8; the
// permutation hands each XCD 32 ADJACENT groups of the run -- with 4-channel
// groups of 8-bit time-major input the 32 groups that share a 128-byte line
// of every spectrum, which then passes through one XCD's L2 only.  A
// performance assumption: any bijection gives the same pattern image.  The
// last NG % 256 slots map to themselves.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDD_FX_HD __host__ __device__
#else
#define PDD_FX_HD
#endif

namespace pdd {

constexpr int kFxXcds = 8;
constexpr int kFxWalkLine = 32;                      // adjacent groups per XCD share
constexpr int kFxWalkRun = kFxXcds * kFxWalkLine;    // slots per permuted run

// Group of slot s (0 <= s < NG): a bijection of [0, NG).
PDD_FX_HD inline int fx_walk_group(int s, int NG) {
  const int full = NG / kFxWalkRun * kFxWalkRun;
  if (s >= full) return s;
  const int r = s % kFxWalkRun;
  return s - r + (r % kFxXcds) * kFxWalkLine + r / kFxXcds;
}

struct FxWalkItem {
  int group;
  int64_t block;
};
// Item i (0 <= i < NG * nblk) -> (group, element block).
PDD_FX_HD inline FxWalkItem fx_walk_item(int64_t i, int NG) {
  return {fx_walk_group((int)(i % NG), NG), i / NG};
}

// XCD that runs workgroup w (hardware dispatch order, MI300 / MI355X).
PDD_FX_HD inline int fx_walk_xcd(int64_t w) { return (int)(w % kFxXcds); }

}  // namespace pdd
