#!/usr/bin/env python
"""Times the fast-folding search (pypulsar_amd/ffa.py, csrc/pdd_ffa.hip) with
HIP events on one stream -- one step of the plan and the whole 0.5 .. 10 s plan
on a 1024 x 2^20 float32 plane (dt = 64 us) -- and writes
profiles/ffa_bench.json stamped with the library's source digest (DESIGN.md
§6h).

Every launch of the search is bracketed by device events (FFASearch.events);
a kernel's time is the sum over its launches, the median of ``--repeats``
runs after ``--warmup`` untimed ones.  From the shapes alone (nothing measured
by counters):

* the float32 adds of each transform pass (Mp p0 per stage and problem, zero
  rows included) and, at two LDS reads of 4 bytes per add, their fraction of
  the LDS read roof of ds_read_b32 (256 CUs x 128 B/clk x 2.4 GHz);
* the HBM bytes the passes move per sample and base period (the series read
  once, the workspace written and read once per pass boundary, 5 bytes per
  trial written) against the two-pass minimum of 12 (read, write, read of
  float32), over the 6.29 TB/s measured copy rate;
* the last pass again without its score (no S/N asked for): what the
  prefix sums and the widths cost.

Needs a GPU; there is no fallback.

    python scripts/bench_ffa.py [--rows 1024] [--log2n 20] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12                    # B/s, the measured HBM copy rate (float4 copy)
LDS_READ_ROOF = 256 * 128 * 2.4e9      # B/s, ds_read_b32 on every CU at the maximum clock


def step_counts(fs, n, step):
    """Adds per pass and HBM bytes of one step and row, from the shapes."""
    f, b_lo, b_hi = step
    n_ds = n // f
    adds, hbm, samples, trials = {}, 0, 0, 0
    for p0 in range(b_lo, b_hi):
        M, K, kpass, npass = fs.plan_info(n_ds, p0)
        Mp = 1 << K
        for p in range(npass):
            k = min(kpass, K - p * kpass)
            adds[p] = adds.get(p, 0) + Mp * p0 * k
        hbm += 4 * M * p0 + 2 * 4 * Mp * p0 * (npass - 1) + 5 * (Mp - 1)
        samples += M * p0
        trials += Mp - 1
    return adds, hbm, samples, trials


def run(fs, plane, dt, plan, score=True):
    """One periodogram of `plan`; {kernel: ms} summed over its launches."""
    import torch
    fs.events = []
    fs.plan = lambda n, dt_: plan
    if score:
        snr, widx, _ = fs.periodogram(plane, dt)
        fs.raw(snr, widx)
    else:
        # the passes alone, the last one without a score: the same batches
        orig = fs._passes

        def bare(y, p_lo, np_, npass, slot, **kw):
            return orig(y, p_lo, np_, npass, slot)
        fs._passes = bare
        fs.periodogram(plane, dt)
        del fs._passes
    torch.cuda.synchronize()
    ms = {}
    for key, a, b in fs.events:
        ms[key] = ms.get(key, 0.0) + a.elapsed_time(b)
    fs.events = None
    del fs.plan
    return ms


def median_runs(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    runs = [fn() for _ in range(repeats)]
    out = {}
    for key in runs[0]:
        v = sorted(r[key] for r in runs)
        out[key] = {"ms": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--pmin", type=float, default=0.5)
    ap.add_argument("--pmax", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffa_bench.json"))
    a = ap.parse_args(argv)

    import torch
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    from pypulsar_amd.ffa import FFASearch
    assert torch.cuda.is_available(), "bench_ffa.py needs a GPU"

    D, n, dt = a.rows, 1 << a.log2n, 64e-6
    fs = FFASearch(a.pmin, a.pmax)
    plan = fs.plan(n, dt)
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane = torch.empty((D, n), dtype=torch.float32, device="cuda")
    plane.normal_(8192.0, 128.0, generator=gen)
    plane.round_()
    plane[::4, ::23437] += 1024.0     # a 1.5 s pulse train in every fourth row

    out = {"digest": _lib.loaded_digest(), "device": torch.cuda.get_device_name(0), "rows": D,
           "n": n, "dt": dt, "period_min": a.pmin, "period_max": a.pmax, "plan": plan,
           "warmup": a.warmup, "repeats": a.repeats, "copy_rate_Bps": COPY_RATE,
           "lds_read_roof_Bps": LDS_READ_ROOF, "workspace_bytes": fs.workspace_bytes}
    for name, steps in (("one_step", plan[:1]), ("full_plan", plan)):
        res = median_runs(lambda: run(fs, plane, dt, steps), a.warmup, a.repeats)
        bare = median_runs(lambda: run(fs, plane, dt, steps, score=False), a.warmup, a.repeats)
        adds, hbm, samples, trials = {}, 0, 0, 0
        for st in steps:
            ad, hb, sm, tr = step_counts(fs, n, st)
            for p, v in ad.items():
                adds[p] = adds.get(p, 0) + v * D
            hbm, samples, trials = hbm + hb * D, samples + sm * D, trials + tr * D
        tpass = 0.0
        for p, v in sorted(adds.items()):
            r = res["pass%d" % p]
            r["adds"] = int(v)
            r["adds_per_s"] = v / (r["ms"] * 1e-3)
            r["ms_without_score"] = bare["pass%d" % p]["ms"]
            r["adds_per_s_without_score"] = v / (bare["pass%d" % p]["ms"] * 1e-3)
            r["fraction_of_lds_read_roof"] = 8.0 * r["adds_per_s_without_score"] / LDS_READ_ROOF
            tpass += r["ms"]
            print("%-9s pass%d %9.3f ms (%.3f-%.3f; %.3f without the score)  %.3g adds  "
                  "%.3g adds/s  %.3f of the LDS read roof" % (
                      name, p, r["ms"], r["ms_min"], r["ms_max"], r["ms_without_score"], v,
                      r["adds_per_s_without_score"], r["fraction_of_lds_read_roof"]))
        for key in ("downsample", "detrend", "search"):
            r = res[key]
            print("%-9s %-10s %9.3f ms (%.3f-%.3f)" % (name, key, r["ms"], r["ms_min"],
                                                      r["ms_max"]))
        tot = sum(r["ms"] for r in res.values())
        hb = {"bytes": int(hbm), "samples_x_base_periods": int(samples),
              "bytes_per_sample_and_base_period": hbm / float(samples),
              "two_pass_minimum": 12.0, "passes_ms": tpass,
              "fraction_of_copy_rate": hbm / (tpass * 1e-3) / COPY_RATE}
        print("%-9s HBM (from the shapes) %.2f B per sample and base period (minimum 12): "
              "%.2f GB in %.1f ms of passes, %.3f of the copy rate" % (
                  name, hb["bytes_per_sample_and_base_period"], hbm / 1e9, tpass,
                  hb["fraction_of_copy_rate"]))
        print("%-9s total %.1f ms for %d rows: %.3g trials, %.3g trials/s" % (
            name, tot, D, trials, trials / (tot * 1e-3)))
        out[name] = {"steps": steps, "kernels": res, "hbm": hb, "total_ms": tot,
                     "trials": int(trials), "trials_per_s": trials / (tot * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
