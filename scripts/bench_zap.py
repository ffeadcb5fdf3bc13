#!/usr/bin/env python
"""Times the birdie zapper (pypulsar_amd/zap.py, csrc/pdd_zap.hip) and writes
profiles/zap_bench.json stamped with the library's source digest (DESIGN.md
§6i):

* ``pdd_zap_percentile`` on R = 33 rows of nn = 2^19 whitened powers and
  ``pdd_zap_apply`` for 100 intervals on 1024 rows, with HIP events: the
  median and the spread of ``--repeats`` timed launches after ``--warmup``
  untimed ones; for the percentile the bytes the algorithm needs, (R + 1) nn 4,
  over the time as a fraction of the 6.2 TB/s achievable read rate DESIGN.md
  uses, and the same for R = 1 .. 64 with 20 launches back to back between
  one pair of events (a single launch of this length is a quarter launch
  overhead);
* ``BirdieFinder.find`` end to end (row gather, prep, FFT, whitening,
  percentile, the copy of nn floats to the host and the flagging there) on a
  configs[1]-sized plane (1024 rows x 2^20 samples, float32) beside one
  ``PeriodicitySearch`` of that plane, both by the wall clock between device
  synchronisations.

Needs a GPU; there is no fallback.

    python scripts/bench_zap.py [--rows 1024] [--log2n 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_RATE = 6.2e12  # B/s, the achievable read rate DESIGN.md §6b uses


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


def wall(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"ms": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--percentile-rows", type=int, default=33)
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zap_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib, zap
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.periodicity import PeriodicitySearch
    assert torch.cuda.is_available(), "bench_zap.py needs a GPU"

    D, n = a.rows, 1 << a.log2n
    nfft, nn = n, n // 2
    dt = 64e-6
    R = a.percentile_rows
    res = {}

    # ---- the kernels, on preallocated buffers ----
    gen = torch.Generator(device="cuda").manual_seed(1)
    powers = torch.empty((D, nn), dtype=torch.float32, device="cuda")
    powers.exponential_(1.0, generator=gen)
    bf = zap.BirdieFinder(rows=R)
    rank = bf.rank(R)
    pct = torch.empty(nn, dtype=torch.float32, device="cuda")
    r = timed(lambda: call("pdd_zap_percentile", ptr(powers), R, nn, nn, rank, ptr(pct),
                           stream_ptr()), a.warmup, a.repeats)
    nbytes = 4 * (R + 1) * nn
    r.update(rows=R, rank=rank, algorithmic_bytes=nbytes,
             fraction_of_read_rate=nbytes / (r["ms"] * 1e-3) / READ_RATE,
             note="R rows read once + the percentile spectrum written")
    res["pdd_zap_percentile"] = r
    print("pdd_zap_percentile     %8.4f ms (%.4f-%.4f)  %6.3f GB  %.2f of 6.2 TB/s" % (
        r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_read_rate"]))
    # the same against NumPy, once
    want = np.sort(powers[:R].cpu().numpy(), axis=0)[rank - 1]
    assert np.array_equal(pct.cpu().numpy(), want), "percentile mismatch"
    # against the number of rows (bytes, and the network of the row class), 20
    # launches between one pair of events: the launch overhead is amortised
    sweep = {}
    for Rk in (1, 8, 16, 24, 32, 33, 40, 48, 56, 64):
        def burst():
            for _ in range(20):
                call("pdd_zap_percentile", ptr(powers), Rk, nn, nn, (Rk + 1) // 2, ptr(pct),
                     stream_ptr())
        r = timed(burst, 1, a.repeats)
        r = {k: v / 20.0 for k, v in r.items()}
        r["algorithmic_bytes"] = 4 * (Rk + 1) * nn
        r["fraction_of_read_rate"] = r["algorithmic_bytes"] / (r["ms"] * 1e-3) / READ_RATE
        sweep[str(Rk)] = r
        print("  R %2d back to back   %8.4f ms (%.4f-%.4f)  %.2f of 6.2 TB/s" % (
            Rk, r["ms"], r["ms_min"], r["ms_max"], r["fraction_of_read_rate"]))
    res["pdd_zap_percentile_back_to_back"] = sweep

    # 100 intervals of 1 .. 19 bins spread over the spectrum
    lo = np.linspace(1000, nn - 1000, a.intervals).astype(np.int64)
    iv = np.stack((lo, lo + np.arange(a.intervals) % 19), axis=1).astype(np.int32)
    zb = zap.device_bins(iv, nn, "cuda")
    spec = torch.zeros((D, nn), dtype=torch.complex64, device="cuda")
    sr = torch.view_as_real(spec)
    for name, sp in (("pdd_zap_apply", None), ("pdd_zap_apply+spectrum", sr)):
        r = timed(lambda: call("pdd_zap_apply", ptr(powers), nn, ptr(sp), nn, D, nn, ptr(zb),
                               len(iv), stream_ptr()), a.warmup, a.repeats)
        r.update(rows=D, intervals=len(iv), bins=int(np.sum(iv[:, 1] - iv[:, 0] + 1)))
        res[name] = r
        print("%-22s %8.4f ms (%.4f-%.4f)  %d intervals, %d bins, %d rows" % (
            name, r["ms"], r["ms_min"], r["ms_max"], r["intervals"], r["bins"], D))
    del powers, spec, sr

    # ---- the finder beside one search of the same plane ----
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(524288.0, 1024.0, generator=gen)
    plane.round_()
    plane[::64, ::4096] += 8192.0     # a pulse train in every 64th row
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    plane += (40.0 * torch.sin(2.0 * np.pi * 50.0 * dt * t)).float()[None, :]  # a 50 Hz line
    del t
    ps = PeriodicitySearch()
    found = {}

    def find():
        found["zl"] = bf.find(ps, plane, dt, nfft=nfft)

    r = wall(find, 1, a.repeats)
    b = found["zl"].bins(nfft, dt)
    r.update(rows_used=len(bf.select_rows(D)), intervals=len(b),
             bins=int(np.sum(b[:, 1] - b[:, 0] + 1)), intervals_list=b.tolist()[:16])
    res["BirdieFinder.find"] = r
    print("BirdieFinder.find      %8.3f ms (%.3f-%.3f)  %d intervals %s" % (
        r["ms"], r["ms_min"], r["ms_max"], len(b), b.tolist()[:6]))
    for name, kw in (("PeriodicitySearch", {}), ("PeriodicitySearch(zap)", {"zap": found["zl"]})):
        cnt = {}

        def search():
            cnt["n"] = len(ps(plane, np.arange(D, dtype=np.float64), dt, nfft=nfft, **kw))

        r = wall(search, 1, max(3, a.repeats // 3))
        r["candidates"] = cnt["n"]
        res[name] = r
        print("%-22s %8.3f ms (%.3f-%.3f)  %d candidates" % (name, r["ms"], r["ms_min"],
                                                             r["ms_max"], cnt["n"]))
    res["find_over_search"] = res["BirdieFinder.find"]["ms"] / res["PeriodicitySearch"]["ms"]
    print("find / search = %.4f (rows used / rows = %.4f)" % (
        res["find_over_search"], len(bf.select_rows(D)) / float(D)))

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "nfft": nfft, "nn": nn, "warmup": a.warmup, "repeats": a.repeats,
           "read_rate_Bps": READ_RATE, "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
