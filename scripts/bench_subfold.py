#!/usr/bin/env python
"""Times the subband fold (pypulsar_amd/subfold.py, csrc/pdd_subfold.hip) with
HIP events on one stream and writes profiles/subfold_bench.json stamped with
the library's source digest.

pdd_subfold for 1, 8 and 64 jobs on a 1024-channel x 2^20 8-bit block and for
8 jobs on a 4096-channel one (periods 1 ms - 1 s, DM 50 and 500, npart 32,
nsub 32, nbins 64): the median and the spread of ``--repeats`` timed launches
after ``--warmup`` untimed ones, the time per job, and the n C bytes a job
must read over that time as a fraction of the 6.29 TB/s measured HBM read
rate.  Beside it pdd_fold_rows on nsub float32 rows of the same length --
what the fold would cost if the subband series existed already -- and
pdd_subfold_dm on the cubes.  Nothing here passes or fails: the script
records what it measures.  Needs a GPU; there is no fallback.

    python scripts/bench_subfold.py [--log2n 20] [--out FILE]
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
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--npart", type=int, default=32)
    ap.add_argument("--nsub", type=int, default=32)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subfold_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.fold import Folder
    from pypulsar_amd.subfold import SubbandFolder
    assert torch.cuda.is_available(), "bench_subfold.py needs a GPU"

    n, dt = 1 << a.log2n, 64e-6
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = []
    last = None
    for C, J, dm in ((1024, 1, 50.0), (1024, 8, 50.0), (1024, 64, 50.0), (1024, 8, 500.0),
                     (4096, 8, 50.0)):
        foff = 300.0 / C
        freqs = 1550.0 - foff / 2 - foff * np.arange(C)
        if last is None or last.shape[1] != C:
            last = None
            last = torch.randint(64, 192, (n, C), dtype=torch.uint8, device="cuda", generator=gen)
        block = last
        sf = SubbandFolder(freqs, dt, a.npart, a.nsub, a.nbins)
        f = np.geomspace(1.0, 1000.0, J) if J > 1 else np.array([1.0 / (4099 * dt)])
        jobs = sf.plan(n, np.full(J, dm), f)
        out = sf.empty(J)

        def fold():
            # (adds to the outputs: the sums grow over the launches, the work does not)
            sf.fold(block, 0, n, jobs, out=out)

        r = timed(fold, a.warmup, a.repeats)
        nbytes = n * C
        r.update(channels=C, jobs=J, dm=dm, bmax=int(jobs.bmax.max()), ms_per_job=r["ms"] / J,
                 bytes_per_job=int(nbytes),
                 fraction_of_read_rate=nbytes * J / (r["ms"] * 1e-3) / READ_RATE,
                 note="each job reads the n C bytes of the block once; includes the upload of "
                      "the job and delay tables, not the zeroing")
        res.append(r)
        print("pdd_subfold C %4d J %2d DM %3.0f  %9.3f ms (%.3f-%.3f)  %8.3f ms/job  %.3f of "
              "6.29 TB/s" % (C, J, dm, r["ms"], r["ms_min"], r["ms_max"], r["ms_per_job"],
                             r["fraction_of_read_rate"]))
        if (C, J) == (1024, 64):
            d = timed(lambda: sf.refine(*out, jobs), a.warmup, a.repeats)
            d.update(jobs=J, ndm=sf.ndm, ms_per_job=d["ms"] / J,
                     note="default ladder; includes the upload of the shift table")
            print("pdd_subfold_dm J %d ndm %d  %.3f ms (%.3f-%.3f)" % (
                J, sf.ndm, d["ms"], d["ms_min"], d["ms_max"]))
            dm_res = d
            # the fold of nsub float32 rows of the same length, one job a row in turn
            folder = Folder(a.npart, a.nbins)
            nout = n - int(jobs.bmax.max())
            plane = torch.empty((a.nsub, nout), dtype=torch.float32, device="cuda")
            plane.normal_(4096.0, 64.0, generator=gen)
            rows = np.arange(J * a.nsub) % a.nsub
            fj = folder.jobs(rows, np.repeat(f, a.nsub), 0.0, dt)
            jd = torch.from_numpy(fj).cuda()
            JJ = len(fj)
            prof = torch.empty((JJ, a.npart, a.nbins), dtype=torch.float64, device="cuda")
            cnt = torch.empty((JJ, a.npart, a.nbins), dtype=torch.int32, device="cuda")
            sumsq = torch.empty((JJ, a.npart), dtype=torch.float64, device="cuda")
            fr = timed(lambda: call("pdd_fold_rows", ptr(plane), a.nsub, nout, plane.stride(0),
                                    fj.ctypes.data_as(ctypes.c_void_p), ptr(jd), JJ, a.npart,
                                    a.nbins, ptr(prof), ptr(cnt), ptr(sumsq), stream_ptr()),
                       a.warmup, a.repeats)
            fr.update(jobs=J, rows_per_job=a.nsub, ms_per_job=fr["ms"] / J,
                      bytes_per_job=int(4 * a.nsub * nout),
                      note="pdd_fold_rows of nsub float32 rows per job: the fold alone, had the "
                           "subband series existed")
            print("pdd_fold_rows  %d x %d rows  %.3f ms (%.3f-%.3f)  %.3f ms/job" % (
                J, a.nsub, fr["ms"], fr["ms_min"], fr["ms_max"], fr["ms_per_job"]))
            rows_res = fr
        del out
    torch.cuda.synchronize()
    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0), "n": n,
           "dt": dt, "npart": a.npart, "nsub": a.nsub, "nbins": a.nbins, "warmup": a.warmup,
           "repeats": a.repeats, "read_rate_Bps": READ_RATE,
           "loads": "8-bit blocks with 4-byte aligned rows: chunks of 256 samples of a 64-channel "
                    "tile staged in LDS with 4-byte loads; otherwise per-lane loads, 8 rows in "
                    "flight (DESIGN.md 6l has the per-lane times of the same cases)",
           "pdd_subfold": res, "pdd_subfold_dm": dm_res, "pdd_fold_rows": rows_res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
