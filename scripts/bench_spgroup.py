#!/usr/bin/env python
"""Times the single-pulse candidate grouping (pypulsar_amd/spgroup.py,
csrc/pdd_spgroup.hip) and writes profiles/spgroup_bench.json stamped with the
library's source digest.

With HIP events, the median and the spread of ``--repeats`` timed runs after
``--warmup`` untimed ones, separately for the canonical sort (torch), for
``pdd_spg_label`` and for ``pdd_spg_summarise``, on

* synthetic lists of 2^14, 2^17 and 2^20 candidates: bow ties plus noise on
  1024 rows, the generator of tests/spgroup_oracle.py scaled (the same
  density of events and of noise per cell);
* the candidates of one ``SinglePulseSearch`` of a 1024 x 2^20 float32 plane
  of noise with injected bursts, beside the time of that search
  (k_sp_stats + k_sp_search).

Beside each, the wall clock of a CPU cell-lookup implementation (NumPy +
scipy, below) on the same list; its labels and summaries must equal the
device's.

Needs a GPU; there is no fallback.

    python scripts/bench_spgroup.py [--rows 1024] [--log2n 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 1024
WIDTHS = np.asarray((1, 2, 3, 4, 6, 9, 14, 20, 30, 45, 70, 100, 150, 300, 600, 1025))


def synthetic(k_target, rows=1024, seed=1):
    """About k_target candidates: 40 bow ties and 2 % noise cells per 64 x 96
    cells (0.2 candidates a cell), one candidate a cell."""
    rng = np.random.default_rng(seed)
    windows = max(4, int(round(k_target / 0.207 / rows)))
    n = windows * WINDOW
    E = max(1, int(round(40.0 * rows * windows / (64 * 96))))
    r0, t0 = rng.integers(0, rows, E), rng.integers(0, n, E)
    slope, peak = rng.integers(-8, 9, E), rng.uniform(10.0, 40.0, E)
    dr = np.arange(-20, 21)
    r = r0[:, None] + dr[None, :]
    w = WIDTHS[np.searchsorted(WIDTHS, 1 + 6 * np.abs(dr))][None, :] + 0 * r
    s = t0[:, None] + slope[:, None] * dr[None, :] - w // 2
    snr = 6.0 + peak[:, None] * np.exp(-(dr[None, :] / 8.0) ** 2)
    ok = (rng.random(r.shape) >= 0.2) & (r >= 0) & (r < rows) & (s >= 0) & (s < n)
    r, s, w, snr = r[ok], s[ok], w[ok], snr[ok]
    # noise: one candidate in 2 % of the cells
    cellsn = np.flatnonzero(rng.random(rows * windows) < 0.02)
    rn, Kn = cellsn % rows, cellsn // rows
    sn = Kn * WINDOW + rng.integers(0, WINDOW, len(cellsn))
    r, s = np.concatenate([r, rn]), np.concatenate([s, sn])
    w = np.concatenate([w, WIDTHS[rng.integers(0, 6, len(cellsn))]])
    snr = np.concatenate([snr, 6.0 + rng.exponential(0.5, len(cellsn))])
    # the first comer keeps a cell
    _, first = np.unique((s // WINDOW) * rows + r, return_index=True)
    first = np.sort(first)
    c = np.empty((len(first), 4), dtype=np.int32)
    c[:, 0], c[:, 1], c[:, 2] = r[first], s[first], w[first]
    c[:, 3] = snr[first].astype(np.float32).view(np.int32)
    return c[rng.permutation(len(c))]


def cpu_group(c, nrows, row_tol, time_tol):
    """Cell lookup on the CPU: the canonical sort, the partners of every
    candidate in the key ranges of windows K - 2 .. K (lower indices only) by
    searchsorted, the link test on the expanded pairs, components by scipy,
    summaries by ufunc.at.  Returns (order, label, groups) as the device."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    c = np.asarray(c, dtype=np.int64)
    k = len(c)
    order = np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0], c[:, 1] // WINDOW))
    cs = c[order]
    r, s, e = cs[:, 0], cs[:, 1], cs[:, 1] + cs[:, 2]
    K = s // WINDOW
    key = K * nrows + r
    idx = np.arange(k)
    rlo, rhi = np.maximum(r - row_tol, 0), np.minimum(r + row_tol, nrows - 1)
    src, dst = [], []
    for back in (2, 1, 0):
        W = K - back
        j0 = np.searchsorted(key, W * nrows + rlo)
        j1 = np.searchsorted(key, W * nrows + rhi + 1) if back else idx
        j0, j1 = np.minimum(j0, idx), np.minimum(j1, idx)
        cnt = np.where(W >= 0, np.maximum(j1 - j0, 0), 0)
        a = np.repeat(idx, cnt)
        b = np.repeat(j0, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        link = (np.abs(r[a] - r[b]) <= row_tol) & \
            (np.maximum(s[a], s[b]) - np.minimum(e[a], e[b]) <= time_tol)
        src.append(a[link])
        dst.append(b[link])
    src, dst = np.concatenate(src), np.concatenate(dst)
    _, comp = connected_components(coo_matrix((np.ones(len(src), dtype=np.int8), (src, dst)),
                                              shape=(k, k)), directed=False)
    first = np.full(comp.max() + 1, k, dtype=np.int64)
    np.minimum.at(first, comp, idx)
    label = first[comp]
    grp = np.zeros((k, 8), dtype=np.int64)
    grp[first, 2], grp[first, 4] = 1 << 40, 1 << 40
    np.add.at(grp[:, 0], label, 1)
    np.minimum.at(grp[:, 2], label, r)
    np.maximum.at(grp[:, 3], label, r)
    np.minimum.at(grp[:, 4], label, s)
    np.maximum.at(grp[:, 5], label, e)
    snr = cs[:, 3].astype(np.int32).view(np.float32)
    # best: highest snr, smallest index on a tie -- the first in (snr desc, index asc)
    o = np.lexsort((idx, -snr.astype(np.float64)))
    lab_o = label[o]
    _, pos = np.unique(lab_o, return_index=True)
    grp[lab_o[pos], 1] = o[pos]
    grp[first, 6] = cs[grp[first, 1], 3]
    return order, label.astype(np.int32), grp.astype(np.int32)


def timed(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def bench_list(cands, nrows, row_tol, time_tol, warmup, repeats, cpu_check=None):
    """Times of the three steps on a device candidate tensor; cpu_check: the
    host copy, grouped on the CPU too and compared."""
    import torch
    from pypulsar_amd import spgroup
    from pypulsar_amd._lib import call, ptr, stream_ptr
    k = cands.shape[0]
    res = {"k": int(k), "nrows": int(nrows)}
    res["sort"] = timed(lambda: spgroup.canonical_order(cands, nrows), warmup, repeats)
    order = spgroup.canonical_order(cands, nrows)
    cs = cands[order].contiguous()
    label = torch.empty(k, dtype=torch.int32, device=cands.device)
    groups = torch.empty((k, 8), dtype=torch.int32, device=cands.device)
    res["pdd_spg_label"] = timed(lambda: call("pdd_spg_label", ptr(cs), k, nrows, row_tol,
                                              time_tol, ptr(label), stream_ptr()),
                                 warmup, repeats)
    res["pdd_spg_summarise"] = timed(lambda: call("pdd_spg_summarise", ptr(cs), ptr(label), k,
                                                  ptr(groups), stream_ptr()), warmup, repeats)
    g = groups.cpu().numpy()
    members = g[:, 0][g[:, 0] > 0]
    res.update(groups=int(len(members)), largest=int(members.max()),
               groups_ge_10=int(np.sum(members >= 10)))
    if cpu_check is not None:
        t0 = time.perf_counter()
        o_c, lab_c, grp_c = cpu_group(cpu_check, nrows, row_tol, time_tol)
        res["cpu_cell_lookup_ms"] = 1e3 * (time.perf_counter() - t0)
        assert np.array_equal(cpu_check[o_c], cs.cpu().numpy()), "canonical order mismatch"
        assert np.array_equal(lab_c, label.cpu().numpy()), "label mismatch"
        assert np.array_equal(grp_c, g), "summary mismatch"
        res["equals_cpu"] = True
    return res


def show(name, r):
    print("%-14s k %8d groups %7d largest %5d | sort %8.4f  label %8.4f  summarise %8.4f ms"
          " | cpu %9.1f ms" % (name, r["k"], r["groups"], r["largest"], r["sort"]["ms"],
                               r["pdd_spg_label"]["ms"], r["pdd_spg_summarise"]["ms"],
                               r.get("cpu_cell_lookup_ms", float("nan"))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--row-tol", type=int, default=2)
    ap.add_argument("--time-tol", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=6.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgroup_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.search import SinglePulseSearch
    assert torch.cuda.is_available(), "bench_spgroup.py needs a GPU"
    res = {}
    cpu_group(synthetic(1 << 10, 64), 64, a.row_tol, a.time_tol)  # (imports scipy: not timed)

    for log2k in (14, 17, 20):
        c = synthetic(1 << log2k, a.rows)
        r = bench_list(torch.from_numpy(c).cuda(), a.rows, a.row_tol, a.time_tol, a.warmup,
                       a.repeats, cpu_check=c)
        res["synthetic_2^%d" % log2k] = r
        show("synthetic 2^%d" % log2k, r)

    # ---- the candidates of one search of the bench plane ----
    D, n = a.rows, 1 << a.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(0.0, 1.0, generator=gen)
    rng = np.random.default_rng(2)
    nburst = 64
    for _ in range(nburst):  # bow ties: amplitude falls, width grows with |row - r0|
        r0, t0, peak = int(rng.integers(0, D)), int(rng.integers(2048, n - 2048)), \
            float(rng.uniform(15.0, 60.0))
        for dr in range(-20, 21):
            if 0 <= r0 + dr < D:
                w = 2 + 2 * abs(dr)
                plane[r0 + dr, t0 - w // 2:t0 - w // 2 + w] += \
                    peak / (1.0 + abs(dr) / 3.0) / float(np.sqrt(w))
    sp = SinglePulseSearch(threshold=a.threshold)
    found = {}

    def search():
        found["c"], found["n"] = sp.raw(plane)

    r = timed(search, 1, max(3, a.repeats // 3))
    k = int(found["n"].item())
    assert k <= sp.max_cands
    r.update(candidates=k, threshold=a.threshold, bursts=nburst,
             note="k_sp_stats + k_sp_search (and the allocation of the candidate buffer)")
    res["SinglePulseSearch.raw"] = r
    print("SinglePulseSearch.raw  %8.3f ms (%.3f-%.3f)  %d candidates" % (
        r["ms"], r["ms_min"], r["ms_max"], k))
    cands = found["c"][:k].contiguous()
    del plane
    r = bench_list(cands, D, a.row_tol, a.time_tol, a.warmup, a.repeats,
                   cpu_check=cands.cpu().numpy())
    res["search_plane"] = r
    show("search plane", r)
    tot = r["sort"]["ms"] + r["pdd_spg_label"]["ms"] + r["pdd_spg_summarise"]["ms"]
    res["group_over_search"] = tot / res["SinglePulseSearch.raw"]["ms"]
    print("grouping / search = %.5f" % res["group_over_search"])

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "row_tol": a.row_tol, "time_tol": a.time_tol, "warmup": a.warmup,
           "repeats": a.repeats, "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
