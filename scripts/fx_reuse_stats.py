#!/usr/bin/env python
"""CPU-only figures behind DESIGN.md's "modelled, not built" stage-2 rows,
from the delay table alone (pypulsar_amd.delays.sweep_table): how much of a
factorised stage 2's LDS reads adjacent trials could share, and what larger
channel groups would cost stage 1.

    python scripts/fx_reuse_stats.py [--config config3|northstar] [--block 96] [--wave 8]

A (trial, group) CELL is one pattern read of stage 2: trial d reads its
pattern of group G at the group's base shift.  With delay-aligned tiles the
LDS offset of the read is the base shift minus the trial's skew (its delay at
a mid-band reference group), so two trials read the same LDS words when they
use the same pattern at the same skewed shift.

Printed, per group size g:
  patterns            distinct relative-shift patterns over all groups
                      (= stage-1 rows; g = 4 is the plan's n_pat)
  stage-1 bytes       relative to g = 4
  stage-2 reads       relative to g = 4 (one read per cell: 4 / g)
and, for the plan's g = 4 with `block`-trial blocks and `wave` consecutive
trials per wave:
  same offset         cells whose pattern and skewed shift equal the previous
                      trial's (a read that could be skipped)
  same pattern +-1    ... equal pattern, skewed shift differs by one element
  pattern changes     adjacent trial pairs (inside a wave) whose pattern differs
  wave / block reuse  cells whose (pattern, skewed shift) any earlier trial
                      of the same wave / block already read
  rare patterns       patterns used by <= 64 trials, and the cells they cover
The 10-bit element's op count is arithmetic, printed for the record.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pypulsar_amd import delays  # noqa: E402

CONFIGS = {"config3": (4096, 4096, 1000.0), "northstar": (4096, 2048, 1000.0)}


def band(C, lo=1250.0, hi=1550.0):
    foff = -(hi - lo) / C
    return (hi + foff / 2.0) + foff * np.arange(C)


def pattern_ids(tab, g, c_lo=0, c_hi=None):
    """[D, groups] pattern id of every cell (ids are per group) and the count."""
    D, C = tab.shape
    c_hi = C if c_hi is None else c_hi
    ids = np.empty((D, (c_hi - c_lo) // g), dtype=np.int64)
    n = 0
    for k, c0 in enumerate(range(c_lo, c_hi - g + 1, g)):
        rel = tab[:, c0:c0 + g] - tab[:, c0:c0 + 1]
        _, inv = np.unique(rel, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        ids[:, k] = inv + n
        n += int(inv.max()) + 1
    return ids, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(CONFIGS))
    ap.add_argument("--block", type=int, default=96)
    ap.add_argument("--wave", type=int, default=8)
    a = ap.parse_args()
    C, D, dm_hi = CONFIGS[a.config]
    freqs = band(C)
    tab = delays.sweep_table(np.linspace(0.0, dm_hi, D), freqs, 64e-6)
    print("%s: %d channels x %d trials, max bin %d" % (a.config, C, D, tab.max()))

    base = {}
    for g in (4, 6, 8):
        c_hi = C // g * g
        ids, n = pattern_ids(tab, g, 0, c_hi)
        base[g] = n
        print("g = %d: %6d patterns over %4d groups; stage-1 bytes %.2f x, stage-2 reads %.3f x"
              % (g, n, c_hi // g, n / float(base[4]), 4.0 / g))
    # g = 8 on the top quarter of the band (the highest frequencies: fewest patterns), 4 elsewhere
    q = C // 4
    _, n8 = pattern_ids(tab, 8, 0, q)
    _, n4 = pattern_ids(tab, 4, q, C)
    print("g = 8 on the top quarter, 4 elsewhere: %d patterns (%.2f x), stage-2 reads %.3f x"
          % (n8 + n4, (n8 + n4) / float(base[4]), (q / 8.0 + (C - q) / 4.0) / (C / 4.0)))

    ids, n_pat = pattern_ids(tab, 4)
    NG = ids.shape[1]
    shift = tab[:, ::4]                                    # base shift of every cell
    # delay-aligned tiles: skew = delay at a mid-band reference group, relative
    # to the trial block's minimum
    ref = shift[:, NG // 2]
    blk = np.arange(D) // a.block
    skew = ref - np.array([ref[blk == b].min() for b in range(blk.max() + 1)])[blk]
    off = shift - skew[:, None]
    wave = np.arange(D) // a.wave
    adj = wave[1:] == wave[:-1]                            # pairs inside one wave
    same_pat = ids[1:] == ids[:-1]
    same_off = same_pat & (off[1:] == off[:-1])
    near = same_pat & (np.abs(off[1:] - off[:-1]) == 1)
    cells = float(D * NG)
    print("cells: %d (trial, group); %d-trial blocks, %d trials per wave" % (cells, a.block, a.wave))
    print("same offset as the previous trial:    %5.1f %% of the reads" % (100 * same_off[adj].sum() / cells))
    print("same pattern at +-1 element:           %5.1f %%" % (100 * near[adj].sum() / cells))
    print("adjacent pairs that change pattern:    %5.1f %% inside a wave, %.1f %% of all cells"
          % (100 * (~same_pat[adj]).sum() / float(adj.sum() * NG), 100 * (~same_pat[adj]).sum() / cells))
    key = ids * (int(off.max() - off.min()) + 1) + (off - off.min())
    for name, part in (("wave", wave), ("block", blk)):
        reuse = 0
        for p in range(int(part.max()) + 1):
            k = key[part == p]
            reuse += k.size - sum(len(np.unique(k[:, j])) for j in range(NG))
        print("any-to-any reuse inside a %-5s:        %5.1f %%" % (name, 100 * reuse / cells))
    uses = np.bincount(ids.reshape(-1), minlength=n_pat)
    rare = uses <= 64
    print("patterns used by <= 64 trials: %.1f %% of %d, covering %.1f %% of the cells"
          % (100 * rare.mean(), n_pat, 100 * uses[rare].sum() / cells))
    print("10-bit element (12 samples per 16-byte read): 8 unpack ops + 4 v_add3 + 1 address op "
          "= 13 VALU ops = 6.5 CU-cycles per read, against 4 LDS cycles; 20 registers per 24 "
          "samples against 12 per 16")


if __name__ == "__main__":
    main()
