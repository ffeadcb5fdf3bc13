"""Records tests/golden/golden_sweep_plans.json: the sweep planner's output
(scalars, cost model, table digests) for the grids of tests/test_sweep_plan.py.

The expected values must come from the commit BEFORE the planner under test:
the oracle program is that commit's pdd_sweep.hip + pdd_ops.hip, patched to
print its host vectors just before their upload, linked with a small main that
takes plan_dump's arguments (table file, n_grp D C dtype flags) and prints the
same JSON object.  Usage:

    python tests/golden/make_golden_sweep_plans.py /path/to/oracle_main
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_sweep_plan as tsp  # noqa: E402

F32, U8, U16 = 0, 1, 2
FACTOR, FORCE, G2, G4, NO_SKEW = 1, 2, 4, 8, 16


def grid(C, dms, descending=True):
    return {"C": C, "descending": descending, "dms": dms}


def cases():
    out = []

    def add(name, dtype, flags, *groups):
        out.append({"name": name, "dtype": dtype, "flags": flags, "groups": list(groups)})

    # the ladder of tests/test_gpu_parity.py: rung i takes candidate i
    from test_gpu_parity import LADDER
    for dt, code in (("f32", F32), ("u8", U8)):
        for i, d in enumerate(LADDER[dt]):
            add("ladder_%s_%d" % (dt, i), code, FACTOR, grid(32, {"arange": [64, d]}))
    add("u16_dense", U16, FACTOR, grid(32, {"arange": [64, 1.0]}))
    add("u16_too_sparse", U16, FACTOR, grid(32, {"arange": [64, 15.0]}))
    # (the last rung has one trial per block, span 0: no single-group table
    # fails it, however sparse -- "too sparse for one LDS tile" is unreachable)
    add("u8_very_sparse_last_rung", U8, FACTOR, grid(32, {"arange": [64, 4000.0]}))
    add("f32_very_sparse_last_rung", F32, FACTOR, grid(32, {"arange": [64, 4000.0]}))
    # short and grouped starts
    add("u8_short_single_starts_at_1", U8, FACTOR, grid(32, {"linspace": [0.0, 40.0, 44]}))
    add("u8_grouped_short", U8, 0, *[grid(24, {"linspace": [5.0 * k, 5.0 * k + 30.0, 40]})
                                      for k in range(4)])
    add("f32_grouped_short", F32, 0, *[grid(24, {"linspace": [5.0 * k, 5.0 * k + 30.0, 50]})
                                       for k in range(2)])
    # C x 255 > 255 x 2^15: kU8Short's byte-wide carry counts are not allowed
    add("u8_grouped_short_forbidden", U8, 0, *[grid(32769, {"linspace": [0.0, 1.0 + k, 40]})
                                               for k in range(2)])
    # forced factorisation, the grids of tests/test_gpu_factor.py
    for C, g in ((32, 4), (36, 4), (36, 2), (34, 2)):
        for desc in (True, False):
            for skew in (True, False):
                add("fx_u8_C%d_g%d_%s_%s" % (C, g, "desc" if desc else "asc", "skew" if skew else "noskew"),
                    U8, FACTOR | FORCE | (G4 if g == 4 else G2) | (0 if skew else NO_SKEW),
                    grid(C, {"linspace": [0.0, 3.0 if C == 32 else 4.0, 64]}, desc))
    for C, g in ((36, 4), (34, 2)):
        for desc in (True, False):
            for skew in (True, False):
                add("fx_f32_C%d_g%d_%s_%s" % (C, g, "desc" if desc else "asc", "skew" if skew else "noskew"),
                    F32, FACTOR | FORCE | (G4 if g == 4 else G2) | (0 if skew else NO_SKEW),
                    grid(C, {"linspace": [0.0, 3.0 if g == 4 else 4.0, 64]}, desc))
    add("fx_u16_C36_g4", U16, FACTOR | FORCE | G4, grid(36, {"linspace": [0.0, 4.0, 64]}))
    add("fx_u16_C36_g2", U16, FACTOR | FORCE | G2, grid(36, {"linspace": [0.0, 4.0, 64]}))
    # the automatic choice on the configs[1] geometry: groups of 2
    add("fx_u8_config1_auto", U8, FACTOR, grid(1024, {"linspace": [0.0, 1000.0, 1024]}))
    # ... and on the configs[3] grid (plans in ~2.5 s on a CPU): groups of 4
    add("fx_u8_config3_auto", U8, FACTOR, grid(4096, {"linspace": [0.0, 1000.0, 4096]}))
    # a grouped grid too sparse for any interleaved tiling
    add("u8_grouped_too_sparse", U8, 0, *[grid(32, {"arange": [64, 40.0]}) for k in range(2)])
    # the two rarer branches (test_case_set_conditions).  A narrow grid at a
    # high DM: small windows, but groups of 4 whose relative shifts span more
    # than kFxRspan bins (no gtab) ...
    add("fx_u8_gtab_empty", U8, FACTOR | FORCE | G4, grid(32, {"linspace": [400.0, 404.0, 64]}))
    # ... and two trial blocks whose pair order costs > PDD_FX_PAIR_MAX chunks
    add("fx_u8_pair_order_dropped_g4", U8, FACTOR | FORCE | G4, grid(48, {"linspace": [0.0, 16.0, 128]}))
    add("fx_u8_pair_order_dropped_g2", U8, FACTOR | FORCE | G2, grid(48, {"linspace": [0.0, 32.0, 128]}))
    return out


def main():
    oracle = sys.argv[1]
    rec = []
    for c in cases():
        tab = tsp.case_table(c)
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            tab.tofile(f)
            f.flush()
            got = subprocess.run([oracle, f.name] + tsp.case_args(c, tab), check=True,
                                 stdout=subprocess.PIPE, universal_newlines=True).stdout
        c["table_sha256"] = tsp.table_digest(tab)
        c["want"] = json.loads(got.strip().splitlines()[-1])
        rec.append(c)
        w = c["want"]
        print(c["name"], w["status"], w.get("variant"), w.get("fx"), w.get("gtab_empty"),
              w.get("pair_ratio"), w["message"])
    with open(os.path.join(HERE, "golden_sweep_plans.json"), "w") as f:
        json.dump({"cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
