"""The sweep planner (pypulsar_amd/csrc/pdd_sweep_plan.hip, sweep_plan.h) on
the CPU: tests/native/plan_dump.cpp links the planner as plain C++ (no HIP, no
GPU) and prints every scalar of the finished plan, the factorised cost model's
figures and a digest of each table the library would upload.  The expected
values of tests/golden/golden_sweep_plans.json were recorded from the commit
before the planner became a unit of its own (tests/golden/
make_golden_sweep_plans.py), so every case pins the tables bit for bit."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, band
from oracle import spectra_oracle as orc

DT = 64e-6
CSRC = os.path.join(ROOT, "pypulsar_amd", "csrc")
PLAN_DUMP = os.path.join(ROOT, "build", "plan_dump")
PLAN_SOURCES = [os.path.join(ROOT, "tests", "native", "plan_dump.cpp"),
                os.path.join(CSRC, "pdd_sweep_plan.hip")]
FX_RSPAN = 512        # sweep_plan.h kFxRspan
FX_PAIR_MAX = 1.06    # sweep_plan.h PDD_FX_PAIR_MAX


def _cxx():
    for c in ("c++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")


@functools.lru_cache(maxsize=None)
def build_plan_dump():
    """build/plan_dump, rebuilt when older than the planner's sources: the
    plain-C++ compile line (no ROCm include path) is the proof that the
    planner has no HIP dependency."""
    deps = PLAN_SOURCES + [os.path.join(CSRC, "sweep_plan.h"), os.path.join(ROOT, "include", "pdd.h")]
    if not os.path.exists(PLAN_DUMP) or os.path.getmtime(PLAN_DUMP) < max(map(os.path.getmtime, deps)):
        os.makedirs(os.path.dirname(PLAN_DUMP), exist_ok=True)
        tmp = "%s.%d.tmp" % (PLAN_DUMP, os.getpid())
        subprocess.check_call([_cxx(), "-x", "c++", "-std=c++17", "-O3", "-ffp-contract=off",
                               "-I" + CSRC, "-o", tmp] + PLAN_SOURCES)
        os.replace(tmp, PLAN_DUMP)
    return PLAN_DUMP


def case_table(case):
    """int32 [n_grp, D, C] delay table of a fixture case."""
    tabs = []
    for g in case["groups"]:
        (kind, a), = g["dms"].items()
        dms = np.arange(a[0]) * a[1] if kind == "arange" else np.linspace(a[0], a[1], a[2])
        tabs.append(orc.sweep_table(dms, band(g["C"], g["descending"]), DT))
    return np.ascontiguousarray(np.stack(tabs), dtype="<i4")


def case_args(case, tab):
    n_grp, D, C = tab.shape
    return [str(v) for v in (n_grp, D, C, case["dtype"], case["flags"])]


def table_digest(tab):
    return hashlib.sha256(tab.tobytes()).hexdigest()


def run_plan(tab, dtype, flags, exe=None):
    """The real planner's answer (plan_dump's JSON object) for an int32
    [n_grp, D, C] or [D, C] table; dtype 0 / 1 / 2 = f32 / u8 / u16."""
    tab = np.ascontiguousarray(tab, dtype="<i4")
    if tab.ndim == 2:
        tab = tab[None]
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        tab.tofile(f)
        f.flush()
        out = subprocess.run([exe or build_plan_dump(), f.name] + [str(v) for v in tab.shape] +
                             [str(dtype), str(flags)], check=True, stdout=subprocess.PIPE,
                             universal_newlines=True).stdout
    return json.loads(out)


with open(os.path.join(GOLDEN, "golden_sweep_plans.json")) as _f:
    CASES = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def plan_dump():
    return build_plan_dump()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_golden(plan_dump, case):
    tab = case_table(case)
    assert table_digest(tab) == case["table_sha256"], "the input table drifted (oracle), not the planner"
    got = run_plan(tab, case["dtype"], case["flags"], plan_dump)
    want = case["want"]
    if want["status"] != 0:
        assert (got["status"], got["message"]) == (want["status"], want["message"])
        return
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_ladder_cases_take_every_tiling_in_order():
    by_name = {c["name"]: c["want"] for c in CASES}
    for dt, n in (("f32", 4), ("u8", 5)):
        assert [by_name["ladder_%s_%d" % (dt, i)]["variant"] for i in range(n)] == list(range(n))
        assert "ladder_%s_%d" % (dt, n) not in by_name
    assert by_name["u8_short_single_starts_at_1"]["variant"] == 1
    assert by_name["u8_grouped_short"]["variant"] == 100 and by_name["u8_grouped_short"]["DB"] == 40
    assert by_name["f32_grouped_short"]["variant"] == 100 and by_name["f32_grouped_short"]["DB"] == 52
    assert by_name["u8_grouped_short_forbidden"]["variant"] != 100
    assert by_name["fx_u8_config1_auto"]["fx"] == 2
    assert by_name["fx_u8_config3_auto"]["fx"] == 4 and by_name["fx_u8_config3_auto"]["n_pat"] > 1024
    assert "16-bit-input tile" in by_name["u16_too_sparse"]["message"]
    assert by_name["u8_very_sparse_last_rung"]["variant"] == 4
    assert by_name["f32_very_sparse_last_rung"]["variant"] == 3
    assert by_name["u8_grouped_too_sparse"]["status"] == -1


def test_case_set_conditions():
    """The fixture reaches the planner's two rarer branches: a group whose
    relative-shift range exceeds kFxRspan (no gtab: stage 1 without LDS), and
    a pair order costing more than PDD_FX_PAIR_MAX (tables rebuilt without
    it; pair_ratio is the pair-order build's)."""
    fx = [c["want"] for c in CASES if c["want"]["status"] == 0 and c["want"]["fx"]]
    assert any(w["gtab_empty"] and w["fx_rspan"] > FX_RSPAN for w in fx)
    assert any(w["pair_ratio"] > FX_PAIR_MAX for w in fx)
