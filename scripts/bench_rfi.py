#!/usr/bin/env python
"""Times the RFI excision steps (pypulsar_amd/rfi.py, csrc/pdd_rfi.hip) with
HIP events on a stream-sized block (2^18 spectra x 4096 channels, 8 bits,
intervals of 2^14 samples) and writes profiles/rfi_bench.json stamped with the
library's source digest:

* pass (a) (pdd_rfi_stats_prep), the FFT (rocFFT through torch.fft.rfft) and
  reduction (b) (pdd_rfi_stats_power) on one workspace batch of channels, and
  the whole ``RFIFind.stats`` of the block;
* ``pdd_rfi_apply`` on the block with an empty mask, a typical mask (2 % of
  the channels everywhere, one interval entirely, 0.5 % scattered cells) and
  a mask of every cell;
* the BASELINE configs[4] stream (StreamingSweep, pinned H2D included) per
  block with and without that typical mask, alternated ``--rounds`` times.

Per kernel: the median and the spread of ``--repeats`` timed launches after
``--warmup`` untimed ones, the bytes the algorithm needs (computed from the
shapes), and that traffic over the time as a fraction of the 6.2 TB/s
achievable read rate DESIGN.md uses.  Needs a GPU; there is no fallback.

    python scripts/bench_rfi.py [--log2t 18] [--chans 4096] [--out FILE]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=18)
    ap.add_argument("--chans", type=int, default=4096)
    ap.add_argument("--log2p", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numdms", type=int, default=2048)
    ap.add_argument("--stream-steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rfi_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.rfi import RFIFind, RFIMask
    assert torch.cuda.is_available(), "bench_rfi.py needs a GPU"

    T, C, P = 1 << a.log2t, a.chans, 1 << a.log2p
    nint = T // P
    gen = torch.Generator(device="cuda").manual_seed(1)
    block = torch.empty((T, C), dtype=torch.float32, device="cuda")
    block = block.normal_(128.0, 16.0, generator=gen).round_().clamp_(0, 255).to(torch.uint8)
    finder = RFIFind(P)
    G = finder.chan_batch(nint, C, torch.uint8)
    L = P // 2 + 1
    res = {}

    def rec(name, fn, nbytes, note):
        r = timed(fn, a.warmup, a.repeats)
        r["algorithmic_bytes"] = int(nbytes)
        r["fraction_of_read_rate"] = nbytes / (r["ms"] * 1e-3) / READ_RATE
        r["note"] = note
        res[name] = r
        print("%-34s %8.3f ms (%.3f-%.3f)  %7.3f GB  %.3f of 6.2 TB/s" % (
            name, r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_read_rate"]))

    # one workspace batch of G channels: the entry points on preallocated buffers
    rows = torch.empty((G * nint, P), dtype=torch.float32, device="cuda")
    nvar = torch.empty(G * nint, dtype=torch.float64, device="cuda")
    avg = torch.empty((nint, C), dtype=torch.float64, device="cuda")
    std, pw = torch.empty_like(avg), torch.empty_like(avg)
    rec("pdd_rfi_stats_prep (a), %d ch" % G,
        lambda: call("pdd_rfi_stats_prep", ptr(block), _lib.U8, nint, C, block.stride(0), P, 0, G,
                     ptr(rows), ptr(avg), ptr(std), ptr(nvar), stream_ptr()),
        nint * P * G * (1 + 4), "raw bytes of the batch read once + float rows written")
    rec("rfft (rocFFT), %d ch" % G, lambda: torch.fft.rfft(rows, dim=1),
        G * nint * (4 * P + 8 * L), "float rows read + spectrum written")
    spec = torch.view_as_real(torch.fft.rfft(rows, dim=1))
    rec("pdd_rfi_stats_power (b), %d ch" % G,
        lambda: call("pdd_rfi_stats_power", ptr(spec), G * nint, P, ptr(nvar), nint, C, 0, ptr(pw),
                     stream_ptr()),
        G * nint * 8 * L, "spectrum read once")
    del spec, rows, nvar
    rec("RFIFind.stats, whole block", lambda: finder.stats(block),
        T * C * (1 + 4 + 4 + 8 + 8), "raw + rows written and read + spectrum written and read "
        "(%d batches of %d channels)" % (-(-C // G), G))

    # the mask application
    rng = np.random.default_rng(3)
    fill = np.full(C, 128.0)
    empty = np.zeros((nint, C), dtype=bool)
    typical = rng.random((nint, C)) < 0.005
    typical[:, rng.choice(C, max(1, C // 50), replace=False)] = True
    typical[nint // 2, :] = True
    masks = {"empty": empty, "typical": typical, "full": np.ones((nint, C), dtype=bool)}
    W = -(-C // 32)
    for name, m in masks.items():
        rm = RFIMask(m, P, fill)
        rm.to_device()
        rm.fill_device(torch.uint8)
        frac = float(m.mean())
        rec("pdd_rfi_apply, %s mask" % name, lambda rm=rm: rm.apply(block, 0),
            T * W * 4 + 2 * frac * T * C,
            "one bitmap word per (row, 32 channels) (cached: %d words) + masked cells read and "
            "written (%.2f%% masked; 16-byte pieces, so up to 16 x that for scattered cells)"
            % (nint * W, 100 * frac))
    del block

    stream = None
    if not a.no_stream:
        from pypulsar_amd.stream import StreamingSweep
        dms = np.linspace(0.0, 1000.0, a.numdms)
        foff = -300.0 / C  # 1250-1550 MHz, descending (bench.py's band)
        freqs = 1550.0 + foff / 2.0 + foff * np.arange(C)
        # the mask of a long stream: the typical pattern, repeated
        reps = a.warmup + a.stream_steps + 2
        rm = RFIMask(np.tile(typical, (reps, 1)), P, fill)
        chunks = []
        for i in range(2):
            x = torch.empty((T, C), dtype=torch.float32, device="cuda").normal_(128.0, 16.0,
                                                                                generator=gen)
            h = torch.empty((T, C), dtype=torch.uint8, pin_memory=True)
            h.copy_(x.round_().clamp_(0, 255).to(torch.uint8))
            chunks.append(h)
        del x
        runs = {"plain": [], "masked": []}
        for _ in range(a.rounds):
            for name, mask in (("plain", None), ("masked", rm)):
                st = StreamingSweep(dms, freqs, 64e-6, block=T, downsamp=2, rfimask=mask)
                planes = [torch.empty((st.D, st.n_out_block), dtype=torch.float32, device="cuda")
                          for _ in range(3)]
                total = a.warmup + a.stream_steps + 1
                done, t0 = 0, None
                for _item in st((chunks[i % 2] for i in range(total)), planes=planes):
                    done += 1
                    if done == a.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    if done == a.warmup + a.stream_steps:
                        break
                torch.cuda.synchronize()
                runs[name].append(1e3 * (time.perf_counter() - t0) / a.stream_steps)
                st.close()
                del st, planes
                print("stream %-6s %.2f ms per block" % (name, runs[name][-1]))
        stream = {"ms_per_block": runs, "blocks_timed": a.stream_steps, "numdms": a.numdms,
                  "note": "configs[4]: 8-bit blocks, zero-DM 'wrap' + downsample 2 + sweep, pinned "
                          "H2D on the copy stream; plain and masked runs alternated"}

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "spectra": T, "channels": C, "ptsperint": P, "nint": nint, "chan_batch": G,
           "warmup": a.warmup, "repeats": a.repeats, "read_rate_Bps": READ_RATE, "kernels": res,
           "stream": stream}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
