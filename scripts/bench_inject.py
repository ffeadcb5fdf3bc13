#!/usr/bin/env python
"""Times the injector (pypulsar_amd/inject.py, csrc/pdd_inject.hip) with HIP
events on a stream-sized block (2^18 spectra x 4096 channels), 8-bit and
float32, and writes profiles/inject_bench.json stamped with the library's
source digest:

* 1, 4 and 16 pulsars at B = 1024 (fd = fdd = 0: the integer phase alone),
  4 pulsars with fd and fdd (the float64 drift per cell), 1 and 64 bursts
  (B = 256 for the 64, which keeps their tables at 270 MB), an empty job list;
* 1 and 4 pulsars in Keplerian orbits (pdd_inject_orbit), wide (pb about a
  quarter of the block, circular, a table of 2^m + 1 knots with m about 13)
  and tight (pb about 600 s, e = 0.9, f = 500 Hz: m = 21, a table of 16 MB
  per pulsar);
* beside the block-bytes floor: one read and one write of the block at the
  6.2 TB/s achievable rate DESIGN.md uses;
* the BASELINE configs[4] stream (StreamingSweep, pinned H2D included) per
  block with and without ``injector=`` (4 pulsars), alternated ``--rounds``
  times.

Per case: the median and the spread of ``--repeats`` timed launches after
``--warmup`` untimed ones.  Needs a GPU; there is no fallback.

    python scripts/bench_inject.py [--log2t 18] [--chans 4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE = 6.2e12  # B/s, the achievable rate DESIGN.md §6b uses
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=18)
    ap.add_argument("--chans", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numdms", type=int, default=2048)
    ap.add_argument("--stream-steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inject_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.inject import BurstSignal, Injector, PulsarSignal
    assert torch.cuda.is_available(), "bench_inject.py needs a GPU"

    T, C = 1 << a.log2t, a.chans
    foff = -300.0 / C  # 1250-1550 MHz, descending (bench.py's band)
    freqs = 1550.0 + foff / 2.0 + foff * np.arange(C)
    rng = np.random.default_rng(2)

    def pulsars(k, curved=False):
        return [PulsarSignal(f=float(rng.uniform(2, 500)), dm=float(rng.uniform(5, 300)),
                             amp=float(rng.uniform(0.05, 0.5)), width=float(rng.uniform(0.02, 0.1)),
                             fd=1e-3 if curved else 0.0, fdd=1e-6 if curved else 0.0)
                for _ in range(k)]

    def binaries(k, tight):
        out = []
        for i in range(k):
            if tight:
                orb = dict(pb=600.0 + 7.0 * i, x=0.5, e=0.9, omega=1.0, t0=100.0 + i)
                f = 500.0 - i
            else:
                orb = dict(pb=T * DT / 4.0 * (1.0 + 0.1 * i), x=0.01, t0=0.3 * i)
                f = float(rng.uniform(50, 500))
            out.append(PulsarSignal(f=f, dm=float(rng.uniform(5, 300)),
                                    amp=float(rng.uniform(0.05, 0.5)),
                                    width=float(rng.uniform(0.02, 0.1)), **orb))
        return out

    def bursts(k):
        return [BurstSignal(t=float(rng.uniform(0.05, 0.8)) * T * DT, dm=float(rng.uniform(20, 300)),
                            amp=float(rng.uniform(1, 20)), width=float(rng.uniform(5e-4, 4e-3)))
                for _ in range(k)]

    cases = [("empty job list", [], 1024), ("1 pulsar", pulsars(1), 1024),
             ("4 pulsars", pulsars(4), 1024), ("16 pulsars", pulsars(16), 1024),
             ("4 pulsars, fd and fdd", pulsars(4, True), 1024), ("1 burst", bursts(1), 1024),
             ("64 bursts (B = 256)", bursts(64), 256),
             ("1 pulsar in a wide orbit", binaries(1, False), 1024),
             ("4 pulsars in wide orbits", binaries(4, False), 1024),
             ("1 pulsar in a tight orbit", binaries(1, True), 1024),
             ("4 pulsars in tight orbits", binaries(4, True), 1024)]
    res = {}
    gen = torch.Generator(device="cuda").manual_seed(1)
    stream_inj = None
    for name, sigs, B in cases:
        t0 = time.perf_counter()
        it = Injector(sigs, freqs, DT, nbins=B)
        host_s = time.perf_counter() - t0
        if name == "4 pulsars":
            stream_inj = it
        for tdt, tag in ((torch.uint8, "u8"), (torch.float32, "f32")):
            block = torch.empty((T, C), dtype=torch.float32, device="cuda")
            block.normal_(128.0, 16.0, generator=gen)
            if tdt == torch.uint8:
                block = block.round_().clamp_(0, 255).to(torch.uint8)
            nbytes = 2 * block.numel() * block.element_size()
            floor_ms = 1e3 * nbytes / RATE
            r = timed(lambda: it.apply(block, 0), a.warmup, a.repeats)
            if sigs:
                lo = np.clip(np.stack([j.lo for j in it.jobs]), 0, T)
                hi = np.clip(np.stack([j.hi for j in it.jobs]), 0, T)
                r["job_cells"] = int(np.maximum(hi - lo, 0).sum())
            else:
                r["job_cells"] = 0
            r.update(block_bytes_floor_ms=floor_ms, fraction_of_floor=floor_ms / r["ms"],
                     ns_per_job_cell=(1e6 * r["ms"] / r["job_cells"]) if r["job_cells"] else None,
                     nbins=B, table_bytes=len(sigs) * C * (B + 1) * 4, host_build_s=host_s)
            if it.has_orbits():
                r.update(orbit_m=[int(s.m) for s in sigs],
                         orbit_table_bytes=int(it.orbit_arrays()[2].nbytes))
            res["%s, %s" % (name, tag)] = r
            print("%-30s %-3s %8.3f ms (%.3f-%.3f)  floor %.3f ms (%.3f of it)  %s ns per job cell"
                  % (name, tag, r["ms"], r["ms_min"], r["ms_max"], floor_ms, r["fraction_of_floor"],
                     "%.4f" % r["ns_per_job_cell"] if r["job_cells"] else "-"))
            del block
        del it

    stream = None
    if not a.no_stream:
        from pypulsar_amd.stream import StreamingSweep
        dms = np.linspace(0.0, 1000.0, a.numdms)
        chunks = []
        for i in range(2):
            x = torch.empty((T, C), dtype=torch.float32, device="cuda").normal_(128.0, 16.0,
                                                                                generator=gen)
            h = torch.empty((T, C), dtype=torch.uint8, pin_memory=True)
            h.copy_(x.round_().clamp_(0, 255).to(torch.uint8))
            chunks.append(h)
        del x
        runs = {"plain": [], "injected": []}
        for _ in range(a.rounds):
            for name, inj in (("plain", None), ("injected", stream_inj)):
                st = StreamingSweep(dms, freqs, DT, block=T, downsamp=2, injector=inj)
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
                print("stream %-8s %.2f ms per block" % (name, runs[name][-1]))
        stream = {"ms_per_block": runs, "blocks_timed": a.stream_steps, "numdms": a.numdms,
                  "note": "configs[4]: 8-bit blocks, zero-DM 'wrap' + downsample 2 + sweep, pinned "
                          "H2D on the copy stream; plain and injected (4 pulsars, B = 1024) runs "
                          "alternated"}

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "spectra": T, "channels": C, "warmup": a.warmup, "repeats": a.repeats,
           "rate_Bps": RATE, "cases": res, "stream": stream}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
