#!/usr/bin/env python
"""Times the jerk search (pypulsar_amd/jerk.py, csrc/pdd_jerk.hip) with HIP
events at nfft = 2^20, zmax = 50, wmax = 100 (51 x 11 templates), harmonic
stages (1, 2, 4, 8), on as many rows as keep the workspace within
JerkSearch's default 32 GiB, and writes profiles/jerk_bench.json stamped with
the library's source digest.

Timed, each as the median and the range of ``--repeats`` launches after
``--warmup`` untimed ones:

* the correlation: ``pdd_acc_correlate`` once per w slab (complex
  multiply-adds per second and the fraction of the float32 vector peak, as
  scripts/bench_accel.py);
* ``pdd_jerk_search`` on the volume;
* the yardstick: ``pdd_acc_search`` over the same nw slabs one at a time --
  the same stage sums on the same bytes, in-slab maxima only.  The two
  searches alternate inside the timed loop.

For both searches the bytes of the volume the stage sums touch (between sum
(h / H)^3 volumes, every repeated row and slab served on chip, and sum h / H,
none) and, for the jerk search, the bytes of its ring of stage slabs (every S
written once and read twice; stage 1 reads the volume itself twice more) over
the time, as fractions of the 6.2 TB/s achievable read rate DESIGN.md uses.
Needs a GPU; there is no fallback.

    python scripts/bench_jerk.py [--log2n 20] [--zmax 50] [--wmax 100] [--rows R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_accel import F32_PEAK, FLOP_PER_MAC  # noqa: E402
from bench_period import READ_RATE, timed  # noqa: E402


def timed_pair(fa, fb, warmup, repeats):
    """``timed`` of two functions whose launches alternate."""
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = []
    for m in ms:
        m.sort()
        out.append({"ms": m[len(m) // 2], "ms_min": m[0], "ms_max": m[-1]})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--zmax", type=int, default=50)
    ap.add_argument("--wmax", type=int, default=100)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jerk_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.jerk import JerkSearch
    assert torch.cuda.is_available(), "bench_jerk.py needs a GPU"

    n = nfft = 1 << a.log2n
    nn, dt = nfft // 2, 64e-6
    js = JerkSearch(zmax=a.zmax, wmax=a.wmax, harms=(1, 2, 4, 8))  # sigma 6, dz 2, dw 20, flo 1 Hz
    D = js.row_batch(nfft) if a.rows is None else a.rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(524288.0, 1024.0, generator=gen)
    plane.round_()
    plane[::4, ::4096] += 8192.0  # a pulse train in every 4th row: candidates are stored
    _, white = js.ps.normalise(js.ps.spectrum(plane, nfft), want_spectrum=True)
    del plane
    taps, hw, M = js._bank(n, nfft, white.device)
    nw, nz, ni = js.nw, js.nz, 2 * nn
    vol = torch.empty((nw, D, nz, ni), dtype=torch.float32, device="cuda")
    f = torch.view_as_real(white)
    res = {}

    def correlate():
        for l in range(nw):
            call("pdd_acc_correlate", ptr(f), D, nn, white.stride(0), ptr(taps[l]),
                 hw[l].ctypes.data_as(ctypes.c_void_p), nz, M, ptr(vol[l]), stream_ptr())

    macs = D * ni * int(sum(2 * int(h) + 1 for h in hw.ravel()))
    r = timed(correlate, a.warmup, a.repeats)
    r["complex_macs"] = macs
    r["complex_macs_per_s"] = macs / (r["ms"] * 1e-3)
    r["fraction_of_f32_peak"] = FLOP_PER_MAC * r["complex_macs_per_s"] / F32_PEAK
    r["bytes_written"] = 4 * nw * D * nz * ni
    r["note"] = "nw launches of pdd_acc_correlate; D 2nn sum_lj (2 hw_lj + 1) complex multiply-adds"
    res["correlate"] = r
    print("correlate (%2d slabs) %9.3f ms (%.3f-%.3f)  %.3g cmac/s  %.3f of the f32 peak" % (
        nw, r["ms"], r["ms_min"], r["ms_max"], r["complex_macs_per_s"],
        r["fraction_of_f32_peak"]))

    scratch = torch.empty(3 * D * nz * ni, dtype=torch.float32, device="cuda")
    cands = torch.empty((js.max_cands, 8), dtype=torch.int32, device="cuda")
    cands6 = torch.empty((js.max_cands, 6), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    count6 = torch.zeros(1, dtype=torch.int64, device="cuda")
    rlo = js.rlo(nfft, dt)
    hp, tp = js.harms.ctypes.data_as(ctypes.c_void_p), js.thr.ctypes.data_as(ctypes.c_void_p)

    def jerk():
        count.zero_()  # (a fill of 8 bytes inside the timed window)
        call("pdd_jerk_search", ptr(vol), D, nw, nz, ni, hp, len(js.harms), tp, rlo, ptr(scratch),
             scratch.numel(), ptr(cands), js.max_cands, ptr(count), stream_ptr())

    def per_slab():
        count6.zero_()
        for l in range(nw):
            call("pdd_acc_search", ptr(vol[l]), D, nz, ni, hp, len(js.harms), tp, rlo, ptr(cands6),
                 js.max_cands, ptr(count6), stream_ptr())

    rj, ry = timed_pair(jerk, per_slab, a.warmup, a.repeats)
    vbytes = 4 * nw * D * nz * ni
    harms = [int(H) for H in js.harms]
    lo = sum((h / float(H)) ** 3 for H in harms for h in range(1, H + 1))
    lo2 = sum((h / float(H)) ** 2 for H in harms for h in range(1, H + 1))
    hi = sum(h / float(H) for H in harms for h in range(1, H + 1))
    # the ring: per stage every S of [ilo, ni) written once, read as slab s by one
    # launch and as slab s - 1 by the next (nw and nw - 1 slabs); H = 1 writes
    # nothing and reads the volume's own slabs in their place
    ring = sum(4 * D * nz * (ni - 2 * H * rlo) * ((3 if H > 1 else 2) * nw - 1) for H in harms)
    for r, name, extra, low in ((rj, "pdd_jerk_search", ring, lo), (ry, "pdd_acc_search_per_slab",
                                                                    0, lo2)):
        r["volume_bytes"] = vbytes
        r["fraction_of_read_rate"] = vbytes / (r["ms"] * 1e-3) / READ_RATE
        r["loads"] = nw * D * nz * ni * int(sum(harms))
        r["touched_bytes_range"] = [int(low * vbytes) + extra, int(hi * vbytes) + extra]
        r["touched_fraction_of_read_rate_range"] = [
            b / (r["ms"] * 1e-3) / READ_RATE for b in r["touched_bytes_range"]]
        res[name] = r
    rj["ring_bytes"] = ring
    rj["launches"] = len(harms) * (nw + 1)
    rj["note"] = ("touched: the stage sums' bytes of the volume, between sum (h/H)^3 and sum h/H "
                  "volumes, plus the ring (every S written once, read twice; H = 1: the volume "
                  "read twice more, nothing written)")
    ry["launches"] = len(harms) * nw
    ry["note"] = ("the yardstick: pdd_acc_search on each of the nw slabs in turn (in-slab maxima "
                  "only); touched between sum (h/H)^2 and sum h/H volumes")
    jerk()
    per_slab()
    ncand, ncand6 = int(count.item()), int(count6.item())
    rj["candidates"], ry["candidates"] = ncand, ncand6
    assert ncand <= js.max_cands and ncand6 <= js.max_cands, "candidate overflow"
    ratio = rj["ms"] / ry["ms"]
    for r, name in ((rj, "pdd_jerk_search"), (ry, "pdd_acc_search x slabs")):
        print("%-22s %9.3f ms (%.3f-%.3f)  volume %6.2f GB  touched %.1f-%.1f GB: %.2f-%.2f of "
              "6.2 TB/s  %d candidates" % (
                  name, r["ms"], r["ms_min"], r["ms_max"], vbytes / 1e9,
                  r["touched_bytes_range"][0] / 1e9, r["touched_bytes_range"][1] / 1e9,
                  r["touched_fraction_of_read_rate_range"][0],
                  r["touched_fraction_of_read_rate_range"][1], r["candidates"]))
    print("pdd_jerk_search / per-slab pdd_acc_search: %.3f" % ratio)

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "rows": D, "n": n, "nfft": nfft, "nn": nn, "zmax": a.zmax, "dz": js.dz, "nz": nz,
           "wmax": a.wmax, "dw": js.dw, "nw": nw, "half_widths": [int(hw.min()), int(hw.max())],
           "harms": harms, "warmup": a.warmup, "repeats": a.repeats, "f32_peak_flops": F32_PEAK,
           "read_rate_Bps": READ_RATE, "ms_per_row": {k: v["ms"] / D for k, v in res.items()},
           "jerk_search_over_per_slab_acc_search": ratio, "kernels": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
