#!/usr/bin/env python
"""Times the 1-, 2- and 4-bit filterbank path (csrc/pdd_lowbit.hip,
pypulsar_amd/stream.py) with HIP events on a stream-sized block (2^18 spectra
x 4096 channels) and writes profiles/lowbit_bench.json stamped with the
library's source digest.  For nbits 1, 2 and 4:

* ``pdd_unpack_bits`` of the packed block into the 8-bit block;
* ``pdd_zdm_packed_int_downsample`` (integer zero-DM, factor 2) on the packed
  block beside ``pdd_zdm_int_downsample`` on the same values as 8 bits, the
  two alternating launch by launch in one run;
* the BASELINE configs[4] stream (StreamingSweep, pinned H2D included) per
  block on packed pinned chunks beside the 8-bit stream of the same values,
  both with zero_dm="int": legs 8-bit, packed, 8-bit, packed, ... so the
  repeated 8-bit leg gives the run-to-run spread the margin is judged by.

The data are seeded uniformly random packed bytes (every field value equally
likely); the 8-bit twin is their device unpack, spot-checked here against the
host codec.  Per kernel: the median and the spread of ``--repeats`` timed
launches after ``--warmup`` untimed ones, the bytes the algorithm needs
(read + written, computed from the shapes), and that traffic over the time as
a fraction of the 6.3 TB/s achievable HBM rate.  Needs a GPU; there is no
fallback.

    python scripts/bench_lowbit.py [--log2t 18] [--chans 4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.3e12  # B/s, the achievable HBM rate (float4 copy)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=18)
    ap.add_argument("--chans", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--numdms", type=int, default=2048)
    ap.add_argument("--stream-steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowbit_bench.json"))
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.stream import StreamingSweep, unpack_bits
    assert torch.cuda.is_available(), "bench_lowbit.py needs a GPU"

    T, C, ds = 1 << a.log2t, a.chans, 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    kernels, stream = {}, {}

    def rec(name, ms, nbytes, note):
        r = summary(ms)
        r["algorithmic_bytes"] = int(nbytes)
        r["fraction_of_hbm_rate"] = nbytes / (r["ms"] * 1e-3) / HBM_RATE
        r["note"] = note
        kernels[name] = r
        print("%-44s %8.3f ms (%.3f-%.3f)  %6.3f GB  %.3f of 6.3 TB/s" % (
            name, r["ms"], r["ms_min"], r["ms_max"], nbytes / 1e9, r["fraction_of_hbm_rate"]))
        sys.stdout.flush()

    x8 = torch.empty((T, C), dtype=torch.uint8, device="cuda")
    img = torch.empty((C, T // ds), dtype=torch.int16, device="cuda")
    for nbits in (1, 2, 4):
        rb = C * nbits // 8
        vmax = (1 << nbits) - 1
        packed = torch.randint(0, 256, (T, rb), dtype=torch.uint8, device="cuda", generator=gen)
        unpack_bits(packed, nbits, C, x8)
        # the twin is this library's own unpack: check a slice against the host codec
        assert np.array_equal(x8[:64].cpu().numpy(),
                              sigproc.unpack_bits(packed[:64].cpu().numpy(), nbits))

        def unpack():
            call("pdd_unpack_bits", ptr(packed), nbits, T, C, rb, ptr(x8), C, stream_ptr())

        def fused():
            call("pdd_zdm_packed_int_downsample", ptr(packed), nbits, T, C, rb, ds, _lib.ZDM_INT,
                 vmax * ds, ptr(img), img.stride(0), stream_ptr())

        def eight():
            call("pdd_zdm_int_downsample", ptr(x8), _lib.U8, T, C, C, ds, _lib.ZDM_INT, 255 * ds,
                 ptr(img), img.stride(0), stream_ptr())

        for _ in range(a.warmup):
            unpack()
        torch.cuda.synchronize()
        rec("pdd_unpack_bits, %d-bit" % nbits, [event_ms(unpack) for _ in range(a.repeats)],
            T * rb + T * C, "packed rows read + 8-bit rows written")
        for _ in range(a.warmup):
            eight()
            fused()
        torch.cuda.synchronize()
        t8, tp = [], []
        for _ in range(a.repeats):   # alternating launch by launch
            t8.append(event_ms(eight))
            tp.append(event_ms(fused))
        out_bytes = C * (T // ds) * 2
        rec("pdd_zdm_int_downsample, 8-bit twin of %d-bit" % nbits, t8, T * C + out_bytes,
            "8-bit rows read once + 16-bit image written (the mean pass reads the rows again)")
        rec("pdd_zdm_packed_int_downsample, %d-bit" % nbits, tp, T * rb + out_bytes,
            "packed rows read once + 16-bit image written (the mean pass reads the rows again)")

        if a.no_stream:
            del packed
            continue
        dms = np.linspace(0.0, 1000.0, a.numdms)
        foff = -300.0 / C  # 1250-1550 MHz, descending (bench.py's band)
        freqs = 1550.0 + foff / 2.0 + foff * np.arange(C)
        h8 = [torch.empty((T, C), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        hp = [torch.empty((T, rb), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        for i in range(2):
            hp[i].copy_(packed)
            h8[i].copy_(x8)
            if i == 0:   # a second, different chunk
                packed = torch.randint(0, 256, (T, rb), dtype=torch.uint8, device="cuda",
                                       generator=gen)
                unpack_bits(packed, nbits, C, x8)
        del packed
        runs = {"8bit": [], "packed": []}
        for _ in range(a.rounds):
            for name, chunks, kw in (("8bit", h8, {}), ("packed", hp, {"nbits": nbits})):
                st = StreamingSweep(dms, freqs, 64e-6, block=T, downsamp=ds, zero_dm="int", **kw)
                assert st.exact and st.fused == (name == "packed")
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
                print("stream %d-bit values, %-6s leg %.2f ms per block" % (nbits, name,
                                                                            runs[name][-1]))
                sys.stdout.flush()
        stream["%d-bit" % nbits] = {
            "ms_per_block": runs,
            "h2d_bytes_per_block": {"8bit": T * C, "packed": T * rb},
            "spread_8bit_ms": max(runs["8bit"]) - min(runs["8bit"]),
        }
        del h8, hp

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0),
           "spectra": T, "channels": C, "downsamp": ds, "warmup": a.warmup, "repeats": a.repeats,
           "hbm_rate_Bps": HBM_RATE, "kernels": kernels,
           "stream": None if a.no_stream else dict(
               stream, blocks_timed=a.stream_steps, numdms=a.numdms, rounds=a.rounds,
               note="configs[4]: zero-DM 'int' + downsample 2 + the exact 16-bit sweep, pinned "
                    "H2D on the copy stream; 8-bit and packed legs alternated, the 8-bit leg "
                    "repeated for the spread")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
