"""Brute-force restatement of the single-pulse candidate grouping (test
infrastructure: no product path imports it; it imports nothing of the
product).

Restates what pypulsar_amd/spgroup.py and pypulsar_amd/csrc/pdd_spgroup.hip
implement, on purpose without any of their reasoning about windows, cells or
reach: the full k x k link matrix straight from the two inequalities,
components by scipy, summaries by plain loops.  Fine up to a few thousand
candidates.

A candidate list is an int32 [k, 4] array {row, start, width, float32 bits of
the S/N}.

* ``canonical_order``  ascending (start // 1024, row, start, width, S/N bits);
* ``link_matrix``      |row_a - row_b| <= row_tol and
                       max(start_a, start_b) - min(end_a, end_b) <= time_tol;
* ``labels``           label = smallest index of the connected component;
* ``summaries``        the [k, 8] group records of pdd_spg_summarise;
* ``group``            all of it for a list in any order;
* ``bow_ties`` / ``noise`` / ``per_cell``  the lists the tests share.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

WINDOW = 1024
WIDTHS = (1, 2, 3, 4, 6, 9, 14, 20, 30, 45, 70, 100, 150, 300, 600, 1025)


def cands(rows, starts, widths, snrs):
    """int32 [k, 4] records from columns."""
    c = np.empty((len(rows), 4), dtype=np.int32)
    c[:, 0], c[:, 1], c[:, 2] = rows, starts, widths
    c[:, 3] = np.asarray(snrs, dtype=np.float32).view(np.int32)
    return c


def canonical_order(c):
    c = np.asarray(c, dtype=np.int32).reshape(-1, 4)
    # np.lexsort: the LAST key is the primary one
    return np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0], c[:, 1] // WINDOW))


def link_matrix(c, row_tol, time_tol):
    c = np.asarray(c, dtype=np.int64).reshape(-1, 4)
    r, s, e = c[:, 0], c[:, 1], c[:, 1] + c[:, 2]
    near = np.abs(r[:, None] - r[None, :]) <= row_tol
    gap = np.maximum(s[:, None], s[None, :]) - np.minimum(e[:, None], e[None, :])
    return near & (gap <= time_tol)


def labels(c, row_tol, time_tol):
    """label[i] = the smallest index of i's component (c as given)."""
    k = len(c)
    if k == 0:
        return np.empty(0, dtype=np.int32)
    _, comp = connected_components(csr_matrix(link_matrix(c, row_tol, time_tol)), directed=False)
    first = {}
    for i in range(k):
        first.setdefault(int(comp[i]), i)
    return np.asarray([first[int(comp[i])] for i in range(k)], dtype=np.int32)


def summaries(c, label):
    c = np.asarray(c, dtype=np.int32).reshape(-1, 4)
    snr = c[:, 3].view(np.float32)
    out = np.zeros((len(c), 8), dtype=np.int32)
    for g in sorted(set(int(x) for x in label)):
        members = [i for i in range(len(c)) if label[i] == g]
        best = members[0]
        for i in members:
            if snr[i] > snr[best]:
                best = i
        out[g] = (len(members), best, min(int(c[i, 0]) for i in members),
                  max(int(c[i, 0]) for i in members), min(int(c[i, 1]) for i in members),
                  max(int(c[i, 1]) + int(c[i, 2]) for i in members), c[best, 3], 0)
    return out


def group(c, row_tol=2, time_tol=3):
    """(order, label, groups) of a list in any order: order maps canonical
    index to input index; label and groups are in canonical indices."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 4)
    order = canonical_order(c)
    cs = c[order]
    lab = labels(cs, row_tol, time_tol)
    return order, lab, summaries(cs, lab)


def partition(order, label):
    """The grouping as a set of frozensets of INPUT indices (order free)."""
    parts = {}
    for ci, g in enumerate(label):
        parts.setdefault(int(g), []).append(int(order[ci]))
    return set(frozenset(v) for v in parts.values())


# ---- the lists the tests share ----

def noise(seed, rows=64, windows=96, occupancy=0.02, taken=None):
    """One candidate in a fraction `occupancy` of the (window, row) cells not
    in `taken`, at a uniform start within the window."""
    rng = np.random.default_rng(seed)
    out = []
    for K in range(windows):
        for r in range(rows):
            if rng.random() < occupancy and (taken is None or (K, r) not in taken):
                out.append((r, K * WINDOW + int(rng.integers(0, WINDOW)),
                            WIDTHS[int(rng.integers(0, 6))], 6.0 + float(rng.exponential(0.5))))
    a = np.asarray(out, dtype=np.float64).reshape(-1, 4)
    return cands(a[:, 0], a[:, 1], a[:, 2], a[:, 3])


def bow_ties(seed, rows=64, windows=96, events=40, occupancy=0.02):
    """`events` bow ties -- members at rows r0 + dr, |dr| <= 20, a fifth of
    them dropped, width growing and S/N falling with |dr|, start drifting by
    `slope` samples a row -- plus noise; the first comer keeps a cell."""
    rng = np.random.default_rng(seed)
    n = windows * WINDOW
    taken, out = set(), []
    for _ in range(events):
        r0, t0 = int(rng.integers(0, rows)), int(rng.integers(0, n))
        slope, peak = int(rng.integers(-8, 9)), float(rng.uniform(10.0, 40.0))
        for dr in range(-20, 21):
            r = r0 + dr
            drop = rng.random() < 0.2
            if drop or not 0 <= r < rows:
                continue
            w = min(x for x in WIDTHS if x >= 1 + 6 * abs(dr))
            s = t0 + slope * dr - w // 2
            if s < 0 or s >= n or (s // WINDOW, r) in taken:
                continue
            taken.add((s // WINDOW, r))
            out.append((r, s, w, 6.0 + peak * np.exp(-(dr / 8.0) ** 2)))
    a = np.asarray(out, dtype=np.float64).reshape(-1, 4)
    ties = cands(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    return np.concatenate([ties, noise(seed + 1, rows, windows, occupancy, taken)])


def per_cell(seed, rows=32, windows=16, n=3, fraction=1.0 / 3):
    """`n` candidates in a fraction of the cells (merged lists, or a plane
    searched at a t0 that is no multiple of 1024)."""
    rng = np.random.default_rng(seed)
    out = []
    for K in range(windows):
        for r in range(rows):
            if rng.random() < fraction:
                for _ in range(n):
                    out.append((r, K * WINDOW + int(rng.integers(0, WINDOW)),
                                WIDTHS[int(rng.integers(0, len(WIDTHS)))],
                                6.0 + float(rng.integers(0, 8)) / 2))
    a = np.asarray(out, dtype=np.float64).reshape(-1, 4)
    return cands(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
