#!/usr/bin/env python
"""Times the sideband search (pypulsar_amd/sideband.py, csrc/pdd_sideband.hip)
with HIP events on a 1024-row x 2^19-bin plane of whitened powers (nfft =
2^20) over the default ladder of mini-FFT lengths 32..16384 (shift 2, stages
(1, 2, 4), sigma 6, the automatic clip), and writes
profiles/sideband_bench.json stamped with the library's source digest
(DESIGN.md §6q).

Per length ``L``: the median and the range of ``--repeats`` timed launches of
pdd_sb_search after ``--warmup`` untimed ones, beside two yardsticks:

* a bytes floor: the powers read once at the 6.2 TB/s achievable read rate
  DESIGN.md uses;
* the same computation composed from library calls -- ``Tensor.unfold`` for the
  overlapped segments, ``torch.fft.rfft`` (rocFFT), elementwise normalisation
  and interbinning, the stage sums and ``nonzero`` -- in batches of
  ``--compose-rows`` rows: what the search would cost without the kernel.

Totals over the ladder, and the ladder as a fraction of one plain periodicity
search (prep, FFT, whitening, harmonic sums) of the same plane.  The kernel's
ladder total must not exceed the composition's (exit status 1 otherwise).
Needs a GPU; there is no fallback.

    python scripts/bench_sideband.py [--rows 1024] [--log2n 20] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_period import READ_RATE, timed  # noqa: E402

INTERBIN = math.pi ** 2 / 16.0


def compose(powers, rlo, L, shift, clip, harms, thr, qlo, rows):
    """The definition of DESIGN.md §6q from torch calls; returns the number of
    candidates (``nonzero`` brings the indices to the host, as a search
    without the kernel would have to)."""
    import torch
    import torch.nn.functional as F
    stride = L >> shift
    found = 0
    for r0 in range(0, powers.shape[0], rows):
        x = powers[r0:r0 + rows, rlo:]
        if clip > 0:
            x = x.clamp(max=clip)
        seg = x.unfold(1, L, stride)                       # [rows, nseg, L], a view
        A = torch.fft.rfft(seg, dim=2)                     # [rows, nseg, L / 2 + 1]
        a0 = A[..., :1].real
        scale = torch.where(a0 > 0, float(L) / (a0 * a0), torch.zeros_like(a0))
        M = torch.empty(seg.shape, dtype=torch.float32, device=powers.device)
        lo, hi = A[..., :-1], A[..., 1:]
        M[..., 0::2] = (lo.real * lo.real + lo.imag * lo.imag) * scale
        d = lo - hi
        M[..., 1::2] = (d.real * d.real + d.imag * d.imag) * (scale * INTERBIN)
        for H, t in zip(harms, thr):
            nout = L // int(H)
            S = M[..., :nout].clone()
            for h in range(2, int(H) + 1):
                S += M[..., 0:h * nout:h]
            S = S[..., qlo:]
            if S.shape[-1] == 0:
                continue
            P = F.pad(S, (1, 1), value=float("-inf"))
            hit = (S >= float(t)) & (S > P[..., :-2]) & (S >= P[..., 2:])
            found += int(hit.nonzero().shape[0])
    return found


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--compose-rows", type=int, default=64)
    ap.add_argument("--compose-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sideband_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.periodicity import PeriodicitySearch
    from pypulsar_amd.sideband import SidebandSearch, nseg
    assert torch.cuda.is_available(), "bench_sideband.py needs a GPU"

    D, n = a.rows, 1 << a.log2n
    nfft, nn, dt = n, n // 2, 64e-6
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(0.0, 1.0, generator=gen)
    ps = PeriodicitySearch()  # sigma 6, harms 1..16, flo 1 Hz
    dms = np.arange(D, dtype=np.float64)
    plain = timed(lambda: ps(plane, dms, dt), 1, 2)
    print("plain periodicity search of the plane %9.3f ms (%.3f-%.3f)" % (
        plain["ms"], plain["ms_min"], plain["ms_max"]))
    # the whitened powers of that plane, batch by batch
    powers = torch.empty((D, nn), dtype=torch.float32, device="cuda")
    step = ps.row_batch(nfft)
    for r0 in range(0, D, step):
        powers[r0:r0 + step] = ps.normalise(ps.spectrum(plane[r0:r0 + step], nfft))
    del plane
    torch.cuda.empty_cache()

    sb = SidebandSearch(ps=ps)
    rlo = sb.rlo(nfft, dt)
    cands = torch.empty((sb.max_cands, 6), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    floor_ms = 4.0 * D * nn / READ_RATE * 1e3
    res = {}
    for e in sb.log2s:
        L = 1 << e
        if not nseg(nn, rlo, L, sb.shift):
            continue

        def kernel(e=e):
            count.zero_()  # (a fill of 8 bytes inside the timed window)
            sb._search(powers, rlo, e, None, cands, sb.max_cands, count)

        r = timed(kernel, a.warmup, a.repeats)
        kernel()
        r["candidates"] = int(count.item())
        r["segments_per_row"] = nseg(nn, rlo, L, sb.shift)
        r["bytes_floor_ms"] = floor_ms
        r["times_the_bytes_floor"] = r["ms"] / floor_ms
        c = timed(lambda: compose(powers, rlo, L, sb.shift, sb.clip, sb.harms, sb.thr, sb.qlo,
                                  a.compose_rows), 1, a.compose_repeats)
        r["composition_ms"] = c["ms"]
        r["composition_ms_range"] = [c["ms_min"], c["ms_max"]]
        r["composition_candidates"] = compose(powers, rlo, L, sb.shift, sb.clip, sb.harms, sb.thr,
                                              sb.qlo, a.compose_rows)
        r["composition_over_kernel"] = c["ms"] / r["ms"]
        res[str(L)] = r
        print("L = %5d  kernel %8.3f ms (%.3f-%.3f) = %5.1f x the bytes floor; composition "
              "%9.3f ms = %5.1f x the kernel; candidates %d / %d" % (
                  L, r["ms"], r["ms_min"], r["ms_max"], r["times_the_bytes_floor"], c["ms"],
                  r["composition_over_kernel"], r["candidates"], r["composition_candidates"]))
    k_total = sum(r["ms"] for r in res.values())
    c_total = sum(r["composition_ms"] for r in res.values())
    print("ladder: kernel %.3f ms, composition %.3f ms (%.1f x), bytes floor %.3f ms; the ladder "
          "is %.2f of one plain periodicity search" % (
              k_total, c_total, c_total / k_total, floor_ms * len(res), k_total / plain["ms"]))
    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0), "rows": D,
           "nfft": nfft, "nn": nn, "rlo": rlo, "shift": sb.shift,
           "harms": [int(h) for h in sb.harms], "sigma": sb.sigma_threshold, "clip": sb.clip,
           "qlo": sb.qlo, "warmup": a.warmup, "repeats": a.repeats,
           "compose_rows": a.compose_rows, "read_rate_Bps": READ_RATE,
           "plain_periodicity_search": plain, "lengths": res,
           "ladder": {"kernel_ms": k_total, "composition_ms": c_total,
                      "composition_over_kernel": c_total / k_total,
                      "bytes_floor_ms": floor_ms * len(res),
                      "fraction_of_plain_search": k_total / plain["ms"],
                      "losing_lengths": [int(L) for L, r in res.items()
                                         if r["ms"] > r["composition_ms"]]}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
    print("wrote %s" % a.out)
    if k_total > c_total:
        print("FAIL: the kernel's ladder total exceeds the library composition's")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
