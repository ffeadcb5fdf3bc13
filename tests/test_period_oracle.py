"""The periodicity search without a GPU: the NumPy restatement
(tests/period_oracle.py) against fixtures made by running the reference
(tests/golden/make_golden_period.py), the product's block table and
significance function, sifting, the ``.accelcands`` writer / reader, and the
argument checks of the new entry points."""
import json
import os
import re

import numpy as np
import pytest

import period_oracle as po
from conftest import GOLDEN

HARMS = (1, 2, 3, 4, 8, 16)


@pytest.fixture(scope="module")
def gp():
    return np.load(os.path.join(GOLDEN, "golden_period.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def gh():
    return np.load(os.path.join(GOLDEN, "golden_period_hsum.npz"), allow_pickle=False)


def _cases(gp):
    return [tuple(int(v) for v in c) for c in gp["cases"]]


def test_cases_and_tables(gp):
    from pypulsar_amd.periodicity import deredden_table
    assert _cases(gp) == [(19, 6, 200), (2048, 6, 200), (2500, 6, 200), (16384, 40, 200)]
    for nn, ibl, mbl in _cases(gp):
        offs, lens = gp["nn%d_offs" % nn], gp["nn%d_lens" % nn]
        for o, n in (po.table(nn, ibl, mbl), deredden_table(nn, ibl, mbl)):
            assert o.dtype == np.int32 and n.dtype == np.int32
            np.testing.assert_array_equal(o, offs)
            np.testing.assert_array_equal(n, lens)
    assert gp["nn16384_lens"].max() == 200  # the case that reaches the cap
    assert gp["nn2048_lens"].max() < 200
    assert len(gp["nn19_offs"]) == 2


def test_table_needs_a_corrected_block():
    from pypulsar_amd.periodicity import deredden_table
    with pytest.raises(AssertionError):
        deredden_table(18)
    with pytest.raises(AssertionError):
        deredden_table(4096, 6, 257)


def test_oracle_harmonic_sum_bit_exact(gp, gh):
    for nn, _, _ in _cases(gp):
        powers = gh["nn%d_hsum1" % nn]
        np.testing.assert_array_equal(powers, np.abs(gp["nn%d_spec" % nn]) ** 2)
        for H in HARMS:
            want = gh["nn%d_hsum%d" % (nn, H)]
            assert want.shape == (3, nn // H) and want.dtype == np.float32
            for r in range(3):
                got = po.harmonic_sum(powers[r], H)
                assert got.dtype == np.float32
                np.testing.assert_array_equal(got.view(np.int32), want[r].view(np.int32))


def test_oracle_deredden(gp):
    for nn, ibl, mbl in _cases(gp):
        spec, want = gp["nn%d_spec" % nn], gp["nn%d_dered" % nn]
        for r in range(3):
            got = po.deredden(spec[r], ibl, mbl)
            assert got.dtype == np.complex64
            assert got[0] == 1.0 + 0.0j
            err = np.abs(got.astype(np.complex128) - want[r]) / np.abs(want[r])
            assert err.max() <= 1e-6, (nn, r, err.max())


def test_oracle_candidates_rule():
    p = np.ones((1, 64), dtype=np.float32)
    p[0, 10] = 9.0            # single peak
    p[0, 20] = p[0, 21] = 7.0  # plateau: the first bin of equal neighbours wins
    p[0, 3] = 50.0            # below rlo
    p[0, 63] = 8.0            # last bin: the right neighbour is outside
    got = po.candidates(p, (1,), (5.0,), 4)
    assert {(k, H) for _, k, H, _ in got} == {(10, 1), (20, 1), (63, 1)}
    got2 = po.candidates(p, (1, 2), (5.0, 9.5), 4)
    # S_2[k] = P[k] + P[2k]: k = 10 -> 9 + 7 = 16; k = 5 -> 1 + 9 = 10
    assert {(k, H) for _, k, H, _ in got2 if H == 2} == {(5, 2), (10, 2)}


def test_sigma_function():
    from scipy.stats import norm
    from pypulsar_amd import periodicity as pp
    assert abs(pp.sigma(-np.log(norm.sf(5.0)), 1) - 5.0) <= 1e-9
    for H in (1, 2, 4, 8, 16, 32):
        S = np.concatenate(([0.01, 0.5], np.geomspace(1.0, 1e6, 400)))
        s = pp.sigma(S, H)
        assert np.all(np.isfinite(s)), H
        assert np.all(np.diff(s) > 0), H
        # against the restatement, over and past the underflow of chi2.sf
        for v in (3.0, 40.0, 300.0, 649.0, 651.0, 800.0, 5e4, 1e6):
            a, b = pp.sigma(v + H, H), po.sigma(v + H, H)
            assert abs(a - b) <= 1e-8 * max(1.0, abs(b)), (H, v, a, b)
        for sg in (3.0, 6.0, 12.5, 40.0):
            t = pp.threshold_power(sg, H)
            assert abs(pp.sigma(t, H) - sg) <= 1e-9, (H, sg)
        assert abs(pp.threshold_power(6.0, H) - po.threshold_power(6.0, H)) <= 1e-7 * H


def _recs(rows):
    from pypulsar_amd.periodicity import CAND_DTYPE
    out = np.zeros(len(rows), dtype=CAND_DTYPE)
    for i, (dm, row, r, nh, power, sg) in enumerate(rows):
        out[i] = (dm, row, r, r / 10.0, 10.0 / r, nh, power, sg)
    return out


def test_sift():
    from pypulsar_amd.periodicity import sift
    c = _recs([(10.0, 0, 500, 8, 40.0, 9.0),
               (12.0, 1, 500, 8, 60.0, 14.0),
               (14.0, 2, 501, 8, 45.0, 10.0),    # within 1.5 bins
               (12.0, 1, 1000, 4, 30.0, 8.0),    # 2 r: absorbed (same DM: no new hit)
               (12.0, 1, 250, 16, 33.0, 8.5),    # r / 2: absorbed
               (10.0, 0, 1499, 2, 20.0, 6.5),    # 3 r - 1: absorbed, weaker at DM 10
               (14.0, 2, 777, 1, 25.0, 7.0),     # unrelated: kept
               (14.0, 2, 8500, 1, 25.0, 6.8)])   # 17 r: beyond max_ratio, kept
    s = sift(c)
    assert [round(x.r) for x in s] == [500, 777, 8500]
    top = s[0]
    assert (top.dm, top.sigma, top.numharm, top.row) == (12.0, 14.0, 8, 1)
    assert top.hits == [(10.0, 9.0), (12.0, 14.0), (14.0, 10.0)]
    assert s[1].hits == [(14.0, 7.0)] and s[2].hits == [(14.0, 6.8)]
    assert [round(x.r) for x in sift(c, max_ratio=17)] == [500, 777]
    assert [round(x.r) for x in sift(c, rtol_bins=0.5)] == [500, 501, 777, 8500, 1499]
    assert sift(c[:0]) == []


def test_accelcands_golden(tmp_path):
    from pypulsar_amd.periodicity import SiftedCandidate, read_accelcands, write_accelcands
    golden = open(os.path.join(GOLDEN, "golden_accelcands.txt")).read()
    with open(os.path.join(GOLDEN, "golden_accelcands.json")) as f:
        params = json.load(f)["candidates"]
    cl = []
    for p in params:
        c = SiftedCandidate(p["dm"], p["r"], p["period"], p["numharm"], p["ipow"], p["sigma"],
                            accelfile=p["accelfile"], candnum=p["candnum"])
        c.hits = [tuple(h) for h in reversed(p["hits"])]  # (the writer sorts them)
        cl.append(c)
    fn = str(tmp_path / "a.accelcands")
    write_accelcands(cl, fn)
    assert open(fn).read() == golden
    back = read_accelcands(fn)
    want = sorted(params, key=lambda p: -p["sigma"])
    assert len(back) == len(want)
    for b, p in zip(back, want):
        assert (b.accelfile, b.candnum, b.numharm) == (p["accelfile"], p["candnum"], p["numharm"])
        assert abs(b.dm - p["dm"]) <= 0.005 and abs(b.sigma - p["sigma"]) <= 0.005
        assert abs(b.power - p["ipow"]) <= 0.05 and abs(b.r - p["r"]) <= 0.005
        assert abs(b.period - p["period"]) <= 0.5e-9
        assert len(b.hits) == len(p["hits"])
        for (dm, sg), (dm0, sg0) in zip(b.hits, sorted(map(tuple, p["hits"]))):
            assert abs(dm - dm0) <= 0.005 and abs(sg - sg0) <= 0.005
    fn2 = str(tmp_path / "b.accelcands")
    write_accelcands(back, fn2)
    assert open(fn2).read() == golden


def test_default_names(tmp_path):
    from pypulsar_amd.periodicity import read_accelcands, sift, write_accelcands
    s = sift(_recs([(60.0, 3, 512, 16, 400.0, 30.0), (62.0, 4, 512, 16, 200.0, 20.0)]))
    fn = str(tmp_path / "c.accelcands")
    write_accelcands(s, fn, basename="obs")
    (b,) = read_accelcands(fn)
    assert (b.accelfile, b.candnum) == ("obs_DM60.00_ACCEL_0", 1)
    assert b.hits == [(60.0, 30.0), (62.0, 20.0)]


def test_entry_points_reject_null_without_gpu():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first
    calls = {
        "pdd_ps_prep": [(None, 2, 8, 8, 8, one, None), (one, 2, 8, 8, 8, None, None)],
        "pdd_ps_block_medians": [(None, 2, 32, 33, one, one, 3, one, None),
                                 (one, 2, 32, 33, None, one, 3, one, None),
                                 (one, 2, 32, 33, one, one, 3, None, None)],
        "pdd_ps_normalise": [(None, 2, 32, 33, one, one, 3, one, one, None, None),
                             (one, 2, 32, 33, one, one, 3, one, None, None, None)],
        "pdd_ps_harmsum": [(None, 2, 32, 32, 2, one, None), (one, 2, 32, 32, 2, None, None)],
        "pdd_ps_search": [(None, 2, 32, 32, one, 1, one, 1, one, 4, one, None),
                          (one, 2, 32, 32, None, 1, one, 1, one, 4, one, None),
                          (one, 2, 32, 32, one, 1, one, 1, one, 4, None, None)],
    }
    for name, argsets in calls.items():
        assert name in _lib.EXPORTS
        for args in argsets:
            st = getattr(h, name)(*args)
            assert st < 0, name
            assert name.encode() in h.pdd_last_error(), name
            assert b"null pointer" in h.pdd_last_error(), name
    # bad shapes and stage lists are refused before any HIP call, too
    harms = (ctypes.c_int32 * 2)(2, 2)
    thr = (ctypes.c_float * 2)(1.0, 1.0)
    assert h.pdd_ps_search(one, 2, 32, 32, harms, 2, thr, 1, one, 4, one, None) < 0
    assert b"ascend" in h.pdd_last_error()
    assert h.pdd_ps_harmsum(one, 2, 32, 32, 33, one, None) < 0
    assert h.pdd_ps_normalise(one, 2, 32, 33, one, one, 1, one, one, None, None) < 0
    assert h.pdd_ps_prep(one, 2, 8, 8, 4, one, None) < 0


def test_product_does_not_import_the_restatement():
    from conftest import ROOT
    pkg = os.path.join(ROOT, "pypulsar_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\S*period_oracle", txt, re.M), f
