#!/usr/bin/env python
"""Times the kernels of the periodicity search (pypulsar_amd/periodicity.py,
csrc/pdd_period.hip), and the FFT between them separately, with HIP events on
a configs[1]-sized plane (1024 rows x 2^20 samples, float32), and writes
profiles/period_bench.json stamped with the library's source digest
(DESIGN.md §6d).

Per kernel: the median and the spread of ``--repeats`` timed launches after
``--warmup`` untimed ones, the bytes the algorithm needs (computed from the
shapes below), and that traffic over the time as a fraction of the 6.2 TB/s
achievable read rate DESIGN.md uses.  Needs a GPU; there is no fallback.

    python scripts/bench_period.py [--rows 1024] [--log2n 20] [--out FILE]
"""
import argparse
import json
import os
import sys

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "period_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.periodicity import PeriodicitySearch, deredden_table
    assert torch.cuda.is_available(), "bench_period.py needs a GPU"

    D, n = a.rows, 1 << a.log2n
    nfft, nn = n, n // 2
    dt = 64e-6
    ps = PeriodicitySearch()  # sigma 6, harms (1, 2, 4, 8, 16), flo 1 Hz
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(524288.0, 1024.0, generator=gen)
    plane.round_()
    # a pulse train in every 64th row, so the search stores candidates
    plane[::64, ::4096] += 8192.0
    B = len(deredden_table(nn)[0])

    res = {}

    def rec(name, fn, nbytes, note):
        r = timed(fn, a.warmup, a.repeats)
        r["algorithmic_bytes"] = int(nbytes)
        r["fraction_of_read_rate"] = nbytes / (r["ms"] * 1e-3) / READ_RATE
        r["note"] = note
        res[name] = r
        print("%-22s %8.3f ms (%.3f-%.3f)  %6.2f GB  %.2f of 6.2 TB/s" % (
            name, r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_read_rate"]))

    # the entry points themselves, on preallocated buffers (no allocation or
    # fill inside a timed window)
    from pypulsar_amd._lib import call, ptr, stream_ptr
    import ctypes
    padded = torch.empty((D, nfft), dtype=torch.float32, device="cuda")
    rec("pdd_ps_prep", lambda: call("pdd_ps_prep", ptr(plane), D, n, plane.stride(0), nfft,
                                    ptr(padded), stream_ptr()),
        4 * D * (n + nfft), "plane read once + padded rows written (the kernel reads the plane "
        "twice: mean, then subtraction)")
    rec("rfft (rocFFT)", lambda: torch.fft.rfft(padded, dim=1),
        4 * D * nfft + 8 * D * (nfft // 2 + 1), "padded rows read + spectrum written")
    spec = torch.fft.rfft(padded, dim=1)
    del padded
    f, ld = torch.view_as_real(spec), spec.stride(0)
    offs, lens = ps._table(nn, spec.device)
    med = torch.empty((D, B), dtype=torch.float32, device="cuda")
    powers = torch.empty((D, nn), dtype=torch.float32, device="cuda")
    rec("pdd_ps_block_medians",
        lambda: call("pdd_ps_block_medians", ptr(f), D, nn, ld, ptr(offs), ptr(lens), B, ptr(med),
                     stream_ptr()),
        8 * D * nn + 4 * D * B, "spectrum read + block levels written")
    rec("pdd_ps_normalise",
        lambda: call("pdd_ps_normalise", ptr(f), D, nn, ld, ptr(offs), ptr(lens), B, ptr(med),
                     ptr(powers), None, stream_ptr()),
        8 * D * nn + 4 * D * nn + 4 * D * B, "spectrum and levels read + powers written")
    del spec, f
    hs = torch.empty((D, nn // 16), dtype=torch.float32, device="cuda")
    rec("pdd_ps_harmsum(16)",
        lambda: call("pdd_ps_harmsum", ptr(powers), D, nn, nn, 16, ptr(hs), stream_ptr()),
        4 * D * (16 * (nn // 16) + nn // 16), "16 gathered harmonics per output + output written")
    gathered = sum(int(h - hp) * (nn // int(h))
                   for h, hp in zip(ps.harms, [0] + list(ps.harms[:-1])))
    cands = torch.empty((ps.max_cands, 4), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rlo = ps.rlo(nfft, dt)

    def search():
        count.zero_()  # (a fill of 8 bytes inside the timed window)
        call("pdd_ps_search", ptr(powers), D, nn, nn, ps.harms.ctypes.data_as(ctypes.c_void_p),
             len(ps.harms), ps.thr.ctypes.data_as(ctypes.c_void_p), rlo, ptr(cands),
             ps.max_cands, ptr(count), stream_ptr())

    rec("pdd_ps_search", search, 4 * D * nn,
        "every power read once (the gather touches %d elements per row, at stride h)"
        % gathered)
    search()
    ncand = int(count.item())
    res["pdd_ps_search"]["gathered_bytes"] = 4 * D * int(gathered)
    res["pdd_ps_search"]["candidates"] = ncand
    assert ncand <= ps.max_cands, "candidate overflow: the timed search stored a part only"

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "nfft": nfft, "nn": nn, "blocks": B,
           "harms": [int(h) for h in ps.harms], "warmup": a.warmup, "repeats": a.repeats,
           "read_rate_Bps": READ_RATE, "kernels": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("%d candidates; wrote %s" % (ncand, a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
