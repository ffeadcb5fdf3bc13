#!/usr/bin/env python
"""Times the candidate cut-outs (pypulsar_amd/cutout.py, csrc/pdd_cutout.hip)
and writes profiles/cutout_bench.json stamped with the library's source digest
(DESIGN.md §6k).

With HIP events, the median and the spread of ``--repeats`` timed runs after
``--warmup`` untimed ones, of ``pdd_cutout_ft`` and ``pdd_cutout_dmt`` each, on
a block of 4096 channels of 8-bit noise: nbin = nsub = ndm = 256, candidates
at DM 500 (trial DMs 0 .. 1000), f in {1, 8, 64}, batches of 1 and of 64 jobs
(their windows start at different rows of the block), the box-sum scratch
bounded as ``Cutouts`` bounds it by default.  Both images of the first job
are compared with a NumPy restatement of the definition at 16 bins.

Beside them, as wall clock around a device synchronisation:

* the ``Spectra`` chain for ONE frequency-time image -- the window's host
  bytes to ``Spectra``, ``dedisperse``, ``subband``, ``downsample``;
* one block of 2^18 spectra of ``StreamingSearch`` (1024 trial DMs 0 .. 1000,
  downsampling 2) in the steady state of a stream.

Needs a GPU; there is no fallback.

    python scripts/bench_cutout.py [--channels 4096] [--jobs 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 64e-6


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
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    ms.sort()
    return {"ms": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def records(J, dm, f, first, step):
    """J candidates at DM ``dm`` with W = 2 f whose windows start ``step``
    raw samples apart."""
    from pypulsar_amd.search import CAND_DTYPE
    rec = np.zeros(J, dtype=CAND_DTYPE)
    rec["DM"], rec["Downfact"] = dm, 1
    rec["Sample"] = first + step * np.arange(J)
    return rec


def check_first(block, freqs, jobs, ft, dmt, nb=16):
    """The first job's images, first ``nb`` bins, against NumPy."""
    from pypulsar_amd.delays import sweep_table
    x = block.cpu().numpy()
    t0, f, C = int(jobs.t0[0]), int(jobs.f[0]), len(freqs)
    tab = sweep_table(jobs.dms[0], freqs, DT)
    cols = np.arange(C)
    k = np.arange(nb * f)

    def row(bins):  # [C, nb] per-channel box sums
        idx = t0 + bins[None, :] + k[:, None]
        assert idx.min() >= 0 and idx.max() < x.shape[0]
        return x[idx, cols[None, :]].astype(np.int64).reshape(nb, f, C).sum(axis=1).T

    want_ft = row(tab[jobs.ndm // 2]).reshape(jobs.nsub, C // jobs.nsub, nb).sum(axis=1)
    assert np.array_equal(ft[0, :, :nb].cpu().numpy(), want_ft.astype(np.float32)), "ft mismatch"
    for d in (0, jobs.ndm // 2, jobs.ndm - 1):
        assert np.array_equal(dmt[0, d, :nb].cpu().numpy(),
                              row(tab[d]).sum(axis=0).astype(np.float32)), "dmt mismatch"


def bench_kernels(block, freqs, jobs, work_bytes, warmup, repeats):
    """The two entry points on prepared device arguments (what Cutouts passes)."""
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    C, J, nbin, nsub, ndm = len(freqs), len(jobs), jobs.nbin, jobs.nsub, jobs.ndm
    n = block.shape[0]
    table = torch.from_numpy(jobs.tables().reshape(J * ndm, C)).cuda()
    jb = np.zeros((J, 5), dtype=np.int64)
    jb[:, 0], jb[:, 1], jb[:, 2] = jobs.t0, jobs.f, np.arange(J) * ndm
    jb[:, 3], jb[:, 4] = jobs.bmin, jobs.bmax
    jft = jb.copy()
    jft[:, 2] += ndm // 2
    djb, djft = torch.from_numpy(jb).cuda(), torch.from_numpy(jft).cuda()
    fmax, span = int(jobs.f.max()), int(jobs.span.max())
    one = span * C * (2 if fmax * 255 <= 65535 else 4)
    per_pass = min(J, max(work_bytes // one, 1))
    work = torch.empty(per_pass * one, dtype=torch.uint8, device="cuda")
    ft = torch.empty((J, nsub, nbin), dtype=torch.float32, device="cuda")
    dmt = torch.empty((J, ndm, nbin), dtype=torch.float32, device="cuda")

    def run_ft():
        call("pdd_cutout_ft", ptr(block), _lib.U8, n, C, block.stride(0), ptr(djft), J, ptr(table),
             J * ndm, None, nbin, nsub, fmax, ptr(ft), stream_ptr())

    def run_dmt():
        call("pdd_cutout_dmt", ptr(block), _lib.U8, n, C, block.stride(0), ptr(djb), J, ptr(table),
             J * ndm, None, nbin, ndm, fmax, span, ptr(work), work.numel(), ptr(dmt), stream_ptr())

    res = {"jobs": J, "f": fmax, "span": span, "box_sum_bytes_per_job": one,
           "jobs_per_pass": per_pass, "pdd_cutout_ft": timed(run_ft, warmup, repeats),
           "pdd_cutout_dmt": timed(run_dmt, warmup, repeats)}
    check_first(block, freqs, jobs, ft, dmt)
    res["equals_numpy"] = True
    for k in ("pdd_cutout_ft", "pdd_cutout_dmt"):
        res[k]["ms_per_job"] = res[k]["ms"] / J
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--dm", type=float, default=500.0)
    ap.add_argument("--size", type=int, default=256, help="nbin = nsub = ndm")
    ap.add_argument("--factors", default="1,8,64", help="samples per image bin, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--work-bytes", type=int, default=1 << 30)
    ap.add_argument("--no-stream", action="store_true", help="skip the StreamingSearch block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cutout_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.cutout import plan_jobs
    from pypulsar_amd.formats.spectra import Spectra
    assert torch.cuda.is_available(), "bench_cutout.py needs a GPU"
    C, S = a.channels, a.size
    foff = -300.0 / C  # 1250-1550 MHz, descending (bench.py's band)
    freqs = 1550.0 + foff / 2.0 + foff * np.arange(C)
    res = {}

    for f in [int(v) for v in a.factors.split(",")]:
        # a block that holds every window: the ladder's delays, the images, the jobs' offsets
        probe = plan_jobs(records(1, a.dm, f, 0, 0), 1, freqs, DT, S, S, S, factor=f)
        step = 37
        first = int(-probe.lo[0]) + 16
        n = first + int(probe.hi[0]) + step * a.jobs + 16
        gen = torch.Generator(device="cuda").manual_seed(f)
        block = torch.empty((n, C), dtype=torch.float32, device="cuda").normal_(
            128.0, 16.0, generator=gen).round_().clamp_(0, 255).to(torch.uint8)
        for J in (1, a.jobs):
            jobs = plan_jobs(records(J, a.dm, f, first, step), 1, freqs, DT, S, S, S, factor=f)
            assert jobs.lo.min() >= 0 and jobs.hi.max() <= n
            r = bench_kernels(block, freqs, jobs, a.work_bytes, a.warmup, a.repeats)
            r["block_rows"] = n
            res["f%d_jobs%d" % (f, J)] = r
            print("f %3d jobs %3d | ft %9.4f ms (%.4f / job)  dmt %9.4f ms (%.4f / job) | "
                  "box sums %.1f MB / job, %d jobs a pass"
                  % (f, J, r["pdd_cutout_ft"]["ms"], r["pdd_cutout_ft"]["ms_per_job"],
                     r["pdd_cutout_dmt"]["ms"], r["pdd_cutout_dmt"]["ms_per_job"],
                     r["box_sum_bytes_per_job"] / 1e6, r["jobs_per_pass"]))
        # the Spectra chain for one frequency-time image of the first job
        j0 = plan_jobs(records(1, a.dm, f, first, step), 1, freqs, DT, S, S, S, factor=f)
        lo = int(j0.t0[0])
        hi = lo + S * f + int(j0.tables()[0, S // 2].max())
        win = block[lo:hi].cpu().numpy()

        def chain():
            s = Spectra(freqs, DT, win.T)
            s.dedisperse(a.dm, padval=0)
            s.subband(S)
            s.trim(win.shape[0] - S * f)
            s.downsample(f)
            return s.device_data

        r = wall(chain, 2, max(3, a.repeats // 2))
        r["window_rows"] = int(win.shape[0])
        res["spectra_chain_f%d" % f] = r
        print("f %3d Spectra chain, one frequency-time image: %.3f ms (%.3f-%.3f), wall clock"
              % (f, r["ms"], r["ms_min"], r["ms_max"]))
        del block

    if not a.no_stream:
        from pypulsar_amd.search import StreamingSearch
        T, steps = 1 << 18, 4
        dms = np.linspace(0.0, 1000.0, 1024)
        chunks = []
        for i in range(2):
            x = torch.empty((T, C), dtype=torch.float32, device="cuda").normal_(128.0, 16.0)
            h = torch.empty((T, C), dtype=torch.uint8, pin_memory=True)
            h.copy_(x.round_().clamp_(0, 255).to(torch.uint8))
            chunks.append(h)
        del x
        ss = StreamingSearch(dms, freqs, DT, block=T, downsamp=2, dtype=torch.uint8, threshold=7.0)
        total, done, t0 = a.warmup + steps + 1, 0, None
        for _c in ss((chunks[i % 2] for i in range(total))):
            done += 1
            if done == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if done == a.warmup + steps:
                torch.cuda.synchronize()
                res["StreamingSearch_block"] = {
                    "ms": 1e3 * (time.perf_counter() - t0) / steps, "spectra": T, "numdms": 1024,
                    "downsamp": 2, "blocks": steps,
                    "note": "wall clock per block in the steady state of a stream"}
                break
        ss.close()
        print("StreamingSearch, one block of 2^18 spectra: %.2f ms"
              % res["StreamingSearch_block"]["ms"])

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0), "channels": C,
           "nbin": S, "nsub": S, "ndm": S, "dm": a.dm, "dt": DT, "factors": a.factors,
           "warmup": a.warmup,
           "repeats": a.repeats, "work_bytes": a.work_bytes, "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
