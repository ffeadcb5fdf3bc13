#!/usr/bin/env python
"""Times the two entry points of the fold (pypulsar_amd/fold.py,
csrc/pdd_fold.hip) with HIP events on one stream: pdd_fold_rows and
pdd_fold_search for 256 jobs on a 1024 x 2^20 float32 plane (npart = 32,
nbins = 64, A = B = 64), and writes profiles/fold_bench.json stamped with the
library's source digest.

Per entry point: the median and the spread of ``--repeats`` timed launches
after ``--warmup`` untimed ones.  For the fold, the bytes it must read (J rows
of n float32) over the time as a fraction of the 6.29 TB/s measured HBM read
rate; for the search, the LDS bytes its inner loop reads (12 bytes per trial,
part and bin) over the time.  Needs a GPU; there is no fallback.

    python scripts/bench_fold.py [--rows 1024] [--log2n 20] [--jobs 256] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_RATE = 6.29e12  # B/s, the measured HBM read rate (float4 copy)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=256)
    ap.add_argument("--npart", type=int, default=32)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--ntrial", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.fold import Folder
    assert torch.cuda.is_available(), "bench_fold.py needs a GPU"

    D, n, J = a.rows, 1 << a.log2n, a.jobs
    dt = 64e-6
    folder = Folder(a.npart, a.nbins, a.ntrial, a.ntrial)
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(524288.0, 1024.0, generator=gen)
    plane.round_()
    plane[::4, ::4099] += 8192.0     # a pulse train in every folded row
    # every fourth row, at periods between 1 ms and 1 s
    rows = (np.arange(J) * 4) % D
    freqs = np.geomspace(1.0, 1000.0, J)
    freqs[0] = 1.0 / (4099 * dt)
    jobs = folder.jobs(rows, freqs, 0.0, dt)
    jd = torch.from_numpy(jobs).cuda()
    prof = torch.empty((J, a.npart, a.nbins), dtype=torch.float64, device="cuda")
    cnt = torch.empty((J, a.npart, a.nbins), dtype=torch.int32, device="cuda")
    sumsq = torch.empty((J, a.npart), dtype=torch.float64, device="cuda")
    na = 2 * a.ntrial + 1
    chi2 = torch.empty((J, na, na), dtype=torch.float64, device="cuda")
    best = torch.empty((J, 2), dtype=torch.int32, device="cuda")
    bchi = torch.empty((J,), dtype=torch.float64, device="cuda")
    bprof = torch.empty((J, a.nbins), dtype=torch.float64, device="cuda")
    bcnt = torch.empty((J, a.nbins), dtype=torch.int32, device="cuda")

    res = {}
    r = timed(lambda: call("pdd_fold_rows", ptr(plane), D, n, plane.stride(0),
                           jobs.ctypes.data_as(ctypes.c_void_p), ptr(jd), J, a.npart, a.nbins,
                           ptr(prof), ptr(cnt), ptr(sumsq), stream_ptr()), a.warmup, a.repeats)
    nbytes = 4 * J * (n // a.npart) * a.npart
    r["algorithmic_bytes"] = int(nbytes)
    r["fraction_of_read_rate"] = nbytes / (r["ms"] * 1e-3) / READ_RATE
    r["note"] = ("J rows read once; includes the zeroing of the outputs (one launch) and one "
                 "atomic per non-empty bin and workgroup")
    res["pdd_fold_rows"] = r
    print("pdd_fold_rows   %8.3f ms (%.3f-%.3f)  %.2f GB  %.2f of 6.29 TB/s" % (
        r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_read_rate"]))

    r = timed(lambda: call("pdd_fold_search", ptr(prof), ptr(cnt), ptr(sumsq), J, a.npart,
                           a.nbins, a.ntrial, a.ntrial, ptr(chi2), ptr(best), ptr(bchi),
                           ptr(bprof), ptr(bcnt), stream_ptr()), a.warmup, a.repeats)
    lds = 12 * J * na * na * a.npart * a.nbins
    r["lds_bytes_read"] = int(lds)
    r["lds_read_rate_Bps"] = lds / (r["ms"] * 1e-3)
    r["trials"] = J * na * na
    r["note"] = "float64 + int32 read from LDS per (trial, part, bin); includes k_fold_best"
    res["pdd_fold_search"] = r
    print("pdd_fold_search %8.3f ms (%.3f-%.3f)  %.1f GB from LDS  %.2f TB/s" % (
        r["ms"], r["ms_min"], r["ms_max"], lds / 1e9, r["lds_read_rate_Bps"] / 1e12))
    torch.cuda.synchronize()
    b = best.cpu().numpy()
    print("job 0 (the injected period): best trial (%d, %d), reduced chi2 %.1f" % (
        b[0, 0], b[0, 1], float(bchi[0])))

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "jobs": J, "npart": a.npart, "nbins": a.nbins, "A": a.ntrial,
           "B": a.ntrial, "warmup": a.warmup, "repeats": a.repeats, "read_rate_Bps": READ_RATE,
           "kernels": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
