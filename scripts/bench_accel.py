#!/usr/bin/env python
"""Times the two kernels of the acceleration search (pypulsar_amd/accel.py,
csrc/pdd_accel.hip) with HIP events at nfft = 2^20, zmax = 50 (51 z trials),
harmonic stages (1, 2, 4, 8), on as many rows as keep the workspace within
4 GiB (AccelSearch.row_batch), and writes profiles/accel_bench.json stamped
with the library's source digest.

Per kernel: the median and the range of ``--repeats`` timed launches after
``--warmup`` untimed ones.  For pdd_acc_correlate the complex multiply-adds
per second and, at 8 flop each, the fraction of the 157.3 TF float32 vector
peak; for pdd_acc_search the plane's bytes, read once, over the time, as a
fraction of the 6.2 TB/s achievable read rate DESIGN.md uses.  Needs a GPU;
there is no fallback.

    python scripts/bench_accel.py [--log2n 20] [--zmax 50] [--rows R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_period import READ_RATE, timed  # noqa: E402

F32_PEAK = 157.3e12  # flop/s, the float32 vector peak
FLOP_PER_MAC = 8     # a complex multiply-add


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--zmax", type=int, default=50)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.accel import AccelSearch
    assert torch.cuda.is_available(), "bench_accel.py needs a GPU"

    n = nfft = 1 << a.log2n
    nn, dt = nfft // 2, 64e-6
    acc = AccelSearch(zmax=a.zmax, harms=(1, 2, 4, 8))  # sigma 6, dz 2, flo 1 Hz
    D = acc.row_batch(nfft) if a.rows is None else a.rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(524288.0, 1024.0, generator=gen)
    plane.round_()
    plane[::4, ::4096] += 8192.0  # a pulse train in every 4th row: candidates are stored
    _, white = acc.ps.normalise(acc.ps.spectrum(plane, nfft), want_spectrum=True)
    del plane
    taps, hw, M = acc._bank(n, nfft, white.device)
    nz, ni = acc.nz, 2 * nn
    powers = torch.empty((D, nz, ni), dtype=torch.float32, device="cuda")
    f = torch.view_as_real(white)
    res = {}

    macs = D * ni * int(sum(2 * int(h) + 1 for h in hw))
    r = timed(lambda: call("pdd_acc_correlate", ptr(f), D, nn, white.stride(0), ptr(taps),
                           hw.ctypes.data_as(ctypes.c_void_p), nz, M, ptr(powers), stream_ptr()),
              a.warmup, a.repeats)
    r["complex_macs"] = macs
    r["complex_macs_per_s"] = macs / (r["ms"] * 1e-3)
    r["fraction_of_f32_peak"] = FLOP_PER_MAC * r["complex_macs_per_s"] / F32_PEAK
    r["bytes_written"] = 4 * D * nz * ni
    r["note"] = "D 2nn sum_j (2 hw_j + 1) complex multiply-adds at 8 flop; powers written once"
    res["pdd_acc_correlate"] = r
    print("pdd_acc_correlate %9.3f ms (%.3f-%.3f)  %.3g cmac/s  %.3f of the f32 peak" % (
        r["ms"], r["ms_min"], r["ms_max"], r["complex_macs_per_s"], r["fraction_of_f32_peak"]))

    cands = torch.empty((acc.max_cands, 6), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rlo = acc.rlo(nfft, dt)

    def search():
        count.zero_()  # (a fill of 8 bytes inside the timed window)
        call("pdd_acc_search", ptr(powers), D, nz, ni, acc.harms.ctypes.data_as(ctypes.c_void_p),
             len(acc.harms), acc.thr.ctypes.data_as(ctypes.c_void_p), rlo, ptr(cands),
             acc.max_cands, ptr(count), stream_ptr())

    r = timed(search, a.warmup, a.repeats)
    nbytes = 4 * D * nz * ni
    r["algorithmic_bytes"] = nbytes
    r["fraction_of_read_rate"] = nbytes / (r["ms"] * 1e-3) / READ_RATE
    r["loads"] = D * nz * ni * int(sum(int(h) for h in acc.harms))
    # harmonic h of stage H walks the fraction h / H of the columns and of the
    # z rows: it touches between (h / H)^2 of the plane (every repeated row
    # served on chip) and h / H of it (none)
    lo = sum((h / float(H)) ** 2 for H in acc.harms for h in range(1, int(H) + 1))
    hi = sum(h / float(H) for H in acc.harms for h in range(1, int(H) + 1))
    r["touched_bytes_range"] = [int(lo * nbytes), int(hi * nbytes)]
    r["touched_fraction_of_read_rate_range"] = [
        lo * nbytes / (r["ms"] * 1e-3) / READ_RATE, hi * nbytes / (r["ms"] * 1e-3) / READ_RATE]
    r["note"] = ("algorithmic: the plane read once; one launch per stage, each reading the "
                 "plane again: touched bytes between sum (h/H)^2 and sum h/H planes")
    search()
    ncand = int(count.item())
    r["candidates"] = ncand
    assert ncand <= acc.max_cands, "candidate overflow: the timed search stored a part only"
    res["pdd_acc_search"] = r
    print("pdd_acc_search    %9.3f ms (%.3f-%.3f)  %6.2f GB  %.3f of 6.2 TB/s  %d candidates" % (
        r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_read_rate"], ncand))
    print("                  touched %.1f-%.1f GB: %.2f-%.2f of 6.2 TB/s" % (
        lo * nbytes / 1e9, hi * nbytes / 1e9, r["touched_fraction_of_read_rate_range"][0],
        r["touched_fraction_of_read_rate_range"][1]))

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "nfft": nfft, "nn": nn, "zmax": a.zmax, "dz": acc.dz, "nz": nz,
           "half_widths": [int(hw.min()), int(hw.max())], "harms": [int(h) for h in acc.harms],
           "warmup": a.warmup, "repeats": a.repeats, "f32_peak_flops": F32_PEAK,
           "read_rate_Bps": READ_RATE, "ms_per_row": {k: v["ms"] / D for k, v in res.items()},
           "kernels": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
