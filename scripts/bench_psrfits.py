#!/usr/bin/env python
"""Times the PSRFITS stream decode (pdd_psrfits_block, csrc/pdd_psrfits.hip)
and the stream fed from SUBINT rows (StreamingSweep(decoder=...)) with HIP
events and writes profiles/psrfits_bench.json stamped with the library's
source digest.

* ``pdd_psrfits_block`` on ``--chans`` channels x 2^``--log2t`` spectra in
  subints of ``--nsblk``: uint8 from 4- and 8-bit rows, float32 from 8-, 16-
  and 32-bit rows with scales, offsets and weights, and AABB summed from
  8-bit.  The shapes are warmed up, then timed ``--repeats`` times in turn
  (shape by shape within a repeat, so drift hits all alike); per shape the
  median and the spread, the bytes the algorithm needs and that traffic over
  the time as a share of the 6.2 TB/s HBM read rate.
* the BASELINE configs[4] stream (StreamingSweep, 2^18-spectra blocks, the
  default zero-DM, pinned H2D included) per block fed from PSRFITS rows in
  integer mode beside the existing 8-bit chunk stream of the same values,
  legs alternating in one process, the chunk leg repeated for the spread;
  and the float-mode row stream beside a float32 chunk stream.

The rows are built on the device from a seed with the usual columns
(TSUBINT, OFFS_SUB, TEL_AZ, TEL_ZEN, DAT_FREQ, DAT_WTS, DAT_OFFS, DAT_SCL,
DATA: data_off = 24 + 20 nchan for one polarisation).  Needs a GPU; there is
no fallback.

    python scripts/bench_psrfits.py [--log2t 18] [--chans 4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.2e12  # B/s, the HBM read rate the other sections use


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    ms = sorted(ms)
    return {"ms": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def make_rows(nsub, nsblk, C, nbits, npol, gen, unit):
    """(device rows uint8 [nsub, row_bytes], decoder keywords).  ``unit``:
    scales 1, offsets 0, weights 1 (an integer-mode file)."""
    import torch
    wts_off = 24 + 8 * C
    offs_off = wts_off + 4 * C
    scl_off = offs_off + 4 * npol * C
    data_off = scl_off + 4 * npol * C
    row_bytes = data_off + nsblk * npol * C * nbits // 8
    rows = torch.empty((nsub, row_bytes), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 28) // row_bytes)
    for r in range(0, nsub, step):
        part = rows[r:r + step]
        part.copy_(torch.randint(0, 256, part.shape, dtype=torch.uint8, device="cuda",
                                 generator=gen))

    def put(off, vals):   # big-endian float32 column
        b = vals.contiguous().view(torch.uint8).reshape(nsub, -1, 4).flip(2)
        rows[:, off:off + b.shape[1] * 4] = b.reshape(nsub, -1)

    def rnd(n, lo, hi):
        return lo + (hi - lo) * torch.rand((nsub, n), device="cuda", generator=gen)
    put(wts_off, torch.ones((nsub, C), device="cuda") if unit else rnd(C, 0.5, 1.0))
    put(offs_off, torch.zeros((nsub, npol * C), device="cuda") if unit else rnd(npol * C, -4, 4))
    put(scl_off, torch.ones((nsub, npol * C), device="cuda") if unit else rnd(npol * C, 0.5, 2))
    if nbits == 32:   # finite samples: every byte pattern of a float32 is not
        for r in range(nsub):
            v = torch.randn(nsblk * npol * C, device="cuda", generator=gen)
            rows[r, data_off:] = v.view(torch.uint8).reshape(-1, 4).flip(1).reshape(-1)
    return rows, dict(row_bytes=row_bytes, data_off=data_off, scl_off=scl_off, offs_off=offs_off,
                      wts_off=wts_off, nbits=nbits, nsblk=nsblk, nchan=C, npol=npol)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=18)
    ap.add_argument("--chans", type=int, default=4096)
    ap.add_argument("--nsblk", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numdms", type=int, default=2048)
    ap.add_argument("--stream-steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--no-float-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psrfits_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.formats.psrfits import PsrfitsDecoder
    from pypulsar_amd.stream import StreamingSweep
    assert torch.cuda.is_available(), "bench_psrfits.py needs a GPU"

    T, C, nsblk = 1 << a.log2t, a.chans, a.nsblk
    assert T % nsblk == 0
    nsub = T // nsblk
    gen = torch.Generator(device="cuda").manual_seed(1)
    kernels = {}

    def decoder(kw, integer, npol_sum=1, nsubints=nsub):
        return PsrfitsDecoder(kw["row_bytes"], kw["data_off"], -1 if integer else kw["scl_off"],
                              -1 if integer else kw["offs_off"], kw["wts_off"], kw["nbits"],
                              kw["nsblk"], kw["nchan"], kw["npol"], 0, npol_sum, nsubints,
                              "uint8" if integer else "float32")

    # ---- the kernel: (name, nbits, npol, integer output, bytes per sample)
    shapes = [("u8 from 4-bit", 4, 1, True, 1.5), ("u8 from 8-bit", 8, 1, True, 2.0),
              ("f32 from 8-bit", 8, 1, False, 5.0), ("f32 from 16-bit", 16, 1, False, 6.0),
              ("f32 from 32-bit", 32, 1, False, 8.0), ("f32 from 8-bit AABB summed", 8, 2, False, 6.0)]
    runs = []
    for name, nbits, npol, integer, bps in shapes:
        rows, kw = make_rows(nsub, nsblk, C, nbits, npol, gen, unit=integer)
        dec = decoder(kw, integer, npol_sum=npol)
        out = torch.empty((T, C), dtype=dec.torch_dtype, device="cuda")
        runs.append((name, bps, (lambda d=dec, r=rows, o=out: d.decode(r, nsub, 0, T, o)), []))
    for _ in range(a.warmup):
        for _, _, fn, _ in runs:
            fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, _, fn, ms in runs:
            ms.append(event_ms(fn))
    for name, bps, _, ms in runs:
        r = summary(ms)
        r["algorithmic_bytes"] = int(bps * T * C)
        r["fraction_of_hbm_read_rate"] = bps * T * C / (r["ms"] * 1e-3) / HBM_RATE
        kernels["pdd_psrfits_block, " + name] = r
        print("%-44s %8.3f ms (%.3f-%.3f)  %6.3f GB  %.3f of 6.2 TB/s" % (
            name, r["ms"], r["ms_min"], r["ms_max"], bps * T * C / 1e9,
            r["fraction_of_hbm_read_rate"]))
        sys.stdout.flush()
    del runs

    # ---- the stream
    stream = {}
    if not a.no_stream:
        dms = np.linspace(0.0, 1000.0, a.numdms)
        foff = -300.0 / C  # 1250-1550 MHz, descending (bench.py's band)
        freqs = 1550.0 + foff / 2.0 + foff * np.arange(C)
        total = a.warmup + a.stream_steps + 1
        for mode in ("integer",) + (() if a.no_float_stream else ("float",)):
            integer = mode == "integer"
            tdt = torch.uint8 if integer else torch.float32
            hrows, hx, kw = [], [], None
            for i in range(2):   # two different chunks, alternated
                rows, kw = make_rows(nsub, nsblk, C, 8, 1, gen, unit=integer)
                x = torch.empty((T, C), dtype=tdt, device="cuda")
                decoder(kw, integer).decode(rows, nsub, 0, T, x)
                hrows.append(torch.empty(rows.shape, dtype=torch.uint8, pin_memory=True).copy_(rows))
                hx.append(torch.empty(x.shape, dtype=tdt, pin_memory=True).copy_(x))
                del rows, x
            legs = {"chunks": [], "rows": []}
            for _ in range(a.rounds):
                for leg in ("chunks", "rows"):
                    skw = {"dtype": tdt}
                    if leg == "rows":
                        skw = {"decoder": decoder(kw, integer, nsubints=nsub * total)}
                    st = StreamingSweep(dms, freqs, 64e-6, block=T, downsamp=2, **skw)
                    assert st.exact == integer
                    planes = [torch.empty((st.D, st.n_out_block), dtype=torch.float32,
                                          device="cuda") for _ in range(3)]
                    src = hrows if leg == "rows" else hx
                    done, t0 = 0, None
                    for _item in st((src[i % 2] for i in range(total)), planes=planes):
                        done += 1
                        if done == a.warmup:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        if done == a.warmup + a.stream_steps:
                            break
                    torch.cuda.synchronize()
                    legs[leg].append(1e3 * (time.perf_counter() - t0) / a.stream_steps)
                    st.close()
                    del st, planes
                    print("stream %s mode, %-6s leg %.2f ms per block" % (mode, leg, legs[leg][-1]))
                    sys.stdout.flush()
            stream[mode] = {
                "ms_per_block": legs,
                "h2d_bytes_per_block": {"chunks": T * C * (1 if integer else 4),
                                        "rows": nsub * kw["row_bytes"]},
                "spread_chunks_ms": max(legs["chunks"]) - min(legs["chunks"]),
            }
            del hrows, hx

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "spectra": T, "channels": C, "nsblk": nsblk, "warmup": a.warmup, "repeats": a.repeats,
           "hbm_read_rate_Bps": HBM_RATE, "kernels": kernels,
           "stream": None if a.no_stream else dict(
               stream, blocks_timed=a.stream_steps, numdms=a.numdms, rounds=a.rounds,
               note="configs[4]: default zero-DM + downsample 2 + sweep, pinned H2D on the copy "
                    "stream; 'chunks' is the existing [n, nchan] chunk stream (the baseline), "
                    "'rows' the same values as PSRFITS rows decoded on the device; legs "
                    "alternated, the chunk leg repeated for the spread")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
