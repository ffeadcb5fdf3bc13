#!/usr/bin/env python
"""Times the orbit resampler (pypulsar_amd/orbit.py, csrc/pdd_orbit.hip) with
HIP events: one row of 2^20 samples demodulated by 1024 circular templates into
a [1024, 2^20] plane, and writes profiles/orbit_bench.json stamped with the
library's source digest.

Two banks: a wide one (orbits of three observation lengths; the knot rule gives
K = 256, 9 float64 position solves a workgroup) and a tight one (130 orbits in
the observation; K <= 8, 257 solves or more a workgroup).  Per bank: the median
and the range of ``--repeats`` timed launches of pdd_orbit_resample in both
sampling modes after ``--warmup`` untimed ones, beside three yardsticks:

* a bytes floor: the T n 4 output bytes written once at the 6.2 TB/s DESIGN.md
  uses (the input row is read through L2);
* the ``PeriodicitySearch`` (prep, FFT, whitening, harmonic sums) of the same
  [T, n] rows: what a template costs after it is resampled;
* the same arithmetic composed from torch calls -- float64 ``sin``, six rounds of
  the fixed-point inversion ``p = j + (D(p dt) - D(0)) / dt`` (its error
  shrinks by beta <= 0.1 a round), ``floor`` and ``gather`` -- in batches of
  ``--compose-rows`` templates: what the resampling would cost without the
  kernel.

The number that matters is the resampler's share of a template's whole cost,
resample / (resample + search).  Needs a GPU; there is no fallback.

    python scripts/bench_orbit.py [--templates 1024] [--log2n 20] [--out FILE]
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

WRITE_RATE = READ_RATE  # B/s: DESIGN.md prices one write of a block at the same 6.2 TB/s


def banks(T, n, dt):
    """name -> float64 [T, 5] circular templates."""
    import numpy as np
    span = n * dt
    u = (np.arange(T, dtype=np.float64) + 0.5) / T
    wide = np.zeros((T, 5))
    wide[:, 0] = span * (2.5 + u)                 # 2.5 .. 3.5 observation lengths
    wide[:, 1] = 0.5 + u                          # 0.5 .. 1.5 light-seconds
    wide[:, 4] = wide[:, 0] * ((7.0 * u) % 1.0)
    tight = np.zeros((T, 5))
    tight[:, 0] = span / (120.0 + 20.0 * u)       # 120 .. 140 orbits in the observation
    tight[:, 1] = 0.08 * tight[:, 0] / (2.0 * np.pi) * (0.5 + 0.5 * u)   # beta 0.04 .. 0.08
    tight[:, 4] = tight[:, 0] * ((7.0 * u) % 1.0)
    return {"wide": wide, "tight": tight}


def compose(row, bank, dt, fill, rows, rounds=6):
    """Nearest-mode demodulation from torch calls; returns the [T, n] plane."""
    import torch
    n = row.shape[0]
    j = torch.arange(n, dtype=torch.float64, device=row.device)
    out = torch.empty((len(bank), n), dtype=torch.float32, device=row.device)
    src = torch.cat((row, row.new_full((1,), fill)))       # index n: the fill value
    for a in range(0, len(bank), rows):
        o = torch.from_numpy(bank[a:a + rows]).to(row.device)
        w, x, t0 = (2.0 * torch.pi / o[:, 0])[:, None], o[:, 1][:, None], o[:, 4][:, None]
        d0 = x * torch.sin(-w * t0)
        p = j[None, :].expand(len(o), n)
        for _ in range(rounds):
            p = j[None, :] + (x * torch.sin(w * (p * dt - t0)) - d0) / dt
        idx = torch.floor(p + 0.5).to(torch.int64)
        idx = torch.where((p >= 0) & (p <= n - 1), idx, torch.full_like(idx, n))
        out[a:a + rows] = src[idx]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--compose-rows", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbit_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd import orbit as orb
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.periodicity import PeriodicitySearch
    assert torch.cuda.is_available(), "bench_orbit.py needs a GPU"

    T, n, dt = a.templates, 1 << a.log2n, 64e-6
    gen = torch.Generator(device="cuda").manual_seed(1)
    row = torch.empty(n, dtype=torch.float32, device="cuda")
    row.normal_(0.0, 1.0, generator=gen)
    fill = float(row.double().mean().item())
    out = torch.empty((T, n), dtype=torch.float32, device="cuda")
    ps = PeriodicitySearch()  # sigma 6, harms 1..16, flo 1 Hz
    dms = np.zeros(T)
    floor_ms = 4.0 * T * n / WRITE_RATE * 1e3
    res = {}
    for name, bank in banks(T, n, dt).items():
        bank = orb.validate(bank)
        K = orb.knot_spacing(bank, dt)
        dev = torch.from_numpy(bank).cuda()
        r = {"K": K, "beta_max": float(orb.beta(bank).max()), "bytes_floor_ms": floor_ms}
        for mode in ("nearest", "linear"):
            def kernel(mode=mode):
                call("pdd_orbit_resample", ptr(row), n, ctypes.c_double(dt), ptr(dev), T, K,
                     orb.MODES[mode], ctypes.c_float(fill), ptr(out), out.stride(0), None,
                     stream_ptr())
            t = timed(kernel, a.warmup, a.repeats)
            t["times_the_bytes_floor"] = t["ms"] / floor_ms
            t["write_TBps"] = 4.0 * T * n / (t["ms"] * 1e-3) / 1e12
            r[mode] = t
        call("pdd_orbit_resample", ptr(row), n, ctypes.c_double(dt), ptr(dev), T, K,
             orb.MODES["nearest"], ctypes.c_float(fill), ptr(out), out.stride(0), None,
             stream_ptr())
        s = timed(lambda: ps(out, dms, dt), 1, 3)
        r["periodicity_search"] = s
        r["resampler_share_of_a_template"] = r["nearest"]["ms"] / (r["nearest"]["ms"] + s["ms"])
        c = timed(lambda: compose(row, bank, dt, fill, a.compose_rows), 1, 2)
        r["composition"] = c
        r["composition_over_kernel"] = c["ms"] / r["nearest"]["ms"]
        ref = compose(row, bank, dt, fill, a.compose_rows)
        r["composition_samples_that_differ"] = int((ref != out).sum().item())
        del ref
        res[name] = r
        print("%-5s K = %3d  nearest %7.3f ms (%.3f-%.3f) = %4.2f x the bytes floor  linear %7.3f "
              "ms  search %7.3f ms  share %.3f  composition %9.3f ms = %5.1f x the kernel "
              "(%d of %d samples differ)"
              % (name, K, r["nearest"]["ms"], r["nearest"]["ms_min"], r["nearest"]["ms_max"],
                 r["nearest"]["times_the_bytes_floor"], r["linear"]["ms"], s["ms"],
                 r["resampler_share_of_a_template"], c["ms"], r["composition_over_kernel"],
                 r["composition_samples_that_differ"], T * n))
    doc = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "templates": T, "n": n, "dt": dt, "warmup": a.warmup, "repeats": a.repeats,
           "compose_rows": a.compose_rows, "write_rate_Bps": WRITE_RATE, "banks": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(doc, fo, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
