"""The fold's host side without a GPU: the exact phase model
(fold.phase_steps), the NumPy oracle (tests/fold_oracle.py) against a fixture
made by running the reference's Datfile.pulses / Pulse.downsample_Nbins /
SummedPulse.__iadd__ (tests/golden/make_golden_fold.py), the integer shift
formula, the trial -> (f, fd) map on a synthetic pulse train, the .bestprof
text round trip and Folder's argument validation."""
import os
from fractions import Fraction

import numpy as np
import pytest

import fold_oracle as fo
from conftest import GOLDEN

FLOAT_BAR = 1e-5  # the project's float bar (conftest.rel_err)


@pytest.mark.parametrize("f,fd,dt,phi0", [
    (23.4567, 0.0, 64e-6, 0.0), (1234.5678, -3.25e-3, 81.92e-6, 0.999999),
    (0.731, 7.5e-2, 1e-3, 0.5), (15625.0 / 7, 1e-9, 64e-6, 0.25)])
def test_phase_steps_exact(f, fd, dt, phi0):
    from pypulsar_amd.fold import phase_steps
    P0, step, accel = phase_steps(f, fd, dt, phi0)
    M = 1 << 64
    for v in (P0, step, accel):
        assert isinstance(v, int) and 0 <= v < M
    # each value rounded once from the exact rational value of the floats
    es = Fraction(f) * Fraction(dt) * M
    ea = Fraction(fd) * Fraction(dt) * Fraction(dt) * M
    s = step if step - es < M // 2 else step - M
    assert abs(Fraction(s) - es) <= Fraction(1, 2)
    a = accel if accel < M // 2 else accel - M      # signed
    assert abs(Fraction(a) - ea) <= Fraction(1, 2)
    assert (a < 0) == (fd < 0) or a == 0
    p = (P0 - step // 2) % M
    assert abs(Fraction(p) - Fraction(phi0) * M) <= Fraction(1, 2)
    assert (P0, step, accel) == fo.phase_steps(f, fd, dt, phi0)


def test_phase_whole_sample_period_has_no_edge_sample():
    # a period of 8 samples, 4 bins: step is exact and every sample sits at
    # the centre of its half bin, never on an edge
    from pypulsar_amd.fold import phase_steps
    P0, step, accel = phase_steps(1.0 / (8 * 0.5), 0.0, 0.5)
    assert step == 1 << 61 and accel == 0 and P0 == 1 << 60
    assert fo.bins_python(P0, step, accel, 16, 4) == [0, 0, 1, 1, 2, 2, 3, 3] * 2


@pytest.mark.parametrize("f,fd,phi0", [(777.7, 0.0, 0.0), (91.3, 4.0e4, 0.9999), (5.1, -3.0e4, 0.3)])
def test_uint64_phases_equal_python_integers(f, fd, phi0):
    # (the accelerations wrap the quadratic term past 2^64 many times)
    from pypulsar_amd.fold import phase_steps
    n, nbins, dt = 5003, 50, 64e-6
    P0, step, accel = phase_steps(f, fd, dt, phi0)
    got = fo.bins_of(fo.phases(P0, step, accel, n), nbins)
    assert got.tolist() == fo.bins_python(P0, step, accel, n, nbins)
    assert got.min() >= 0 and got.max() < nbins


def test_oracle_against_reference_fold():
    from pypulsar_amd.fold import phase_steps
    g = np.load(os.path.join(GOLDEN, "golden_fold.npz"), allow_pickle=False)
    dt = float(g["dt"])
    for k, (m, nbins, turns) in enumerate(g["cases"].tolist()):
        x, want = g["x%d" % k], g["prof%d" % k]
        per = m * nbins
        assert len(x) > per * turns and want.shape == (nbins,)
        job = (0,) + phase_steps(1.0 / (per * dt), 0.0, dt)
        prof, cnt, sumsq = fo.fold_rows(x[None, :per * turns], [job], 1, nbins)
        assert np.all(cnt == m * turns)
        # the reference sums the turns' bin MEANS (over m samples): exact equality
        np.testing.assert_array_equal(prof[0, 0] / m, want)
        assert sumsq[0, 0] == np.sum(x[:per * turns].astype(np.float64) ** 2)


def test_fold_parts_and_remainder():
    rng = np.random.default_rng(4)
    x = np.round(rng.normal(50, 5, (2, 1003))).astype(np.float32)
    jobs = [(1,) + fo.phase_steps(300.0, 0.0, 64e-6, 0.1)]
    prof, cnt, sumsq = fo.fold_rows(x, jobs, 7, 10)
    L = 1003 // 7
    assert cnt.sum() == 7 * L and np.all(cnt.sum(axis=2) == L)
    assert prof.sum() == x[1, :7 * L].astype(np.float64).sum()
    b = fo.bins_python(*jobs[0][1:], 7 * L, 10)
    for p in (0, 6):
        want = np.zeros(10)
        for i in range(p * L, (p + 1) * L):
            want[b[i]] += float(x[1, i])
        np.testing.assert_array_equal(prof[0, p], want)


def test_shift_formula_is_nearest_bin():
    from pypulsar_amd.fold import trial_shift
    for N in (1, 2, 5, 16):
        for p in range(N):
            u = Fraction(2 * p + 1 - N, 2 * N)
            for ia in range(-9, 10):
                for ib in range(-9, 10):
                    x = ia * u + 4 * ib * u * u
                    s = fo.shift(ia, ib, p, N)
                    # round to nearest; a half-integer goes up (floor(x + 1/2))
                    assert s == (x + Fraction(1, 2)).__floor__()
                    assert abs(s - x) <= Fraction(1, 2)
                    assert trial_shift(ia, ib, p, N) == s
    assert all(fo.shift(ia, ib, 0, 1) == 0 for ia in (-7, 0, 7) for ib in (-7, 0, 7))


def test_trial_to_ffdot_recovers_the_pulse_train():
    from pypulsar_amd.fold import trial_to_ffdot
    c = fo.search_case()
    ia, ib = c["best"]
    f1, fd1 = trial_to_ffdot(ia, ib, c["f"], c["fd"], c["nbins"], c["T"])
    df, dfd = 1.0 / (c["nbins"] * c["T"]), 8.0 / (c["nbins"] * c["T"] ** 2)
    print("best trial (%d, %d): f' - f0 = %.3g steps, fd' - fd0 = %.3g steps, chi2 %.1f" % (
        ia, ib, (f1 - c["f0"]) / df, (fd1 - c["fd0"]) / dfd, c["best_chi2"]))
    assert abs(fd1 - c["fd0"]) <= dfd
    assert abs(f1 - c["f0"]) <= df
    assert 0 < abs(ia) < c["A"] and 0 < abs(ib) < c["B"]   # (the fold was offset)
    # the maximum is isolated: the best non-adjacent trial is lower by more
    # than twice the float bar (so the device's argmax can be compared)
    chi2 = c["chi2"].copy()
    assert chi2[ia + c["A"], ib + c["B"]] == c["best_chi2"] == chi2.max()
    chi2[max(0, ia + c["A"] - 1):ia + c["A"] + 2, max(0, ib + c["B"] - 1):ib + c["B"] + 2] = -1.0
    second = chi2.max()
    print("second best non-adjacent chi2 %.3f" % second)
    assert c["best_chi2"] - second > 2 * FLOAT_BAR * c["best_chi2"]
    # the trial (0, 0) is the plain sum of the parts
    S0, C0 = fo.summed(c["prof"][0], c["cnt"][0], 0, 0)
    np.testing.assert_array_equal(S0, c["prof"][0].sum(axis=0))
    assert C0.sum() == c["npart"] * (c["n"] // c["npart"])


def test_search_degenerate_inputs():
    # a constant row: var == 0, chi-square 0 everywhere, best = trial (0, 0)
    x = np.full((1, 4096), 37.0, dtype=np.float32)
    prof, cnt, sumsq = fo.fold_rows(x, [(0,) + fo.phase_steps(100.0, 0.0, 64e-6)], 4, 8)
    chi2, best, bc, S, C = fo.search(prof[0], cnt[0], sumsq[0], 3, 2)
    assert chi2.shape == (7, 5) and np.all(chi2 == 0.0) and best == (0, 0) and bc == 0.0
    # ties go to the smallest |ib|, then |ia|, then the negative sign
    assert fo.better((1.0, 1, -1), (1.0, 0, 2)) and fo.better((1.0, 0, 2), (1.0, 5, -3))
    assert fo.better((1.0, -1, 1), (1.0, 1, 1)) and fo.better((1.0, 1, -1), (1.0, -1, 1))
    assert fo.better((2.0, 9, 9), (1.0, 0, 0))


def test_bestprof_round_trip(tmp_path):
    from pypulsar_amd.fold import FoldedCandidate, mean_profile, read_bestprof, write_bestprof
    c = fo.search_case()
    fc = FoldedCandidate(dm=12.375, row=3, f=23.456712345678, fd=-1.25e-3,
                         period=1.0 / 23.456712345678, chi2=float(c["best_chi2"]),
                         profile=c["S"], counts=c["C"], nsamp=int(c["C"].sum()),
                         data_avg=101.23456789, data_var=17.5, dt=c["dt"])
    fn = str(tmp_path / "cand1.bestprof")
    write_bestprof(fc, fn, infile="obs.fil", candname="obs_cand1")
    hdr, prof = read_bestprof(fn)
    assert hdr["Input file"] == "obs.fil" and hdr["Candidate"] == "obs_cand1"
    assert hdr["T_sample"] == c["dt"] and hdr["Data Folded"] == fc.nsamp
    assert hdr["Data Avg"] == fc.data_avg and hdr["Data StdDev"] == np.sqrt(17.5)
    assert hdr["Profile Bins"] == c["nbins"] == len(prof)
    want = mean_profile(fc)
    np.testing.assert_array_equal(prof, want)      # (%.17g: the text is exact)
    assert hdr["Profile Avg"] == want.mean() and hdr["Profile StdDev"] == want.std()
    assert hdr["Reduced chi-sqr"] == fc.chi2 and hdr["Best DM"] == 12.375
    assert hdr["P_topo (ms)"] == 1000.0 * fc.period
    assert hdr["P'_topo (s/s)"] == -fc.fd / (fc.f * fc.f)
    lines = open(fn).read().splitlines()
    assert all(l.startswith("# ") for l in lines[:13]) and set(lines[13]) == {"#"}
    assert len(lines) == 14 + c["nbins"]


def test_sigma_finite_where_probability_underflows():
    from pypulsar_amd.fold import chi2_sigma
    s = chi2_sigma(np.array([0.5, 1.0, 2.0, 50.0, 5000.0]), 64)
    assert np.all(np.isfinite(s)) and np.all(np.diff(s) > 0)
    assert s[0] < 0 < s[2] and s[4] > 38.0   # (norm.sf(38.6) is the smallest float64)
    from scipy.stats import chi2, norm
    assert abs(s[2] - norm.isf(chi2.sf(2.0 * 63, 63))) < 1e-9


def test_folder_validation():
    from pypulsar_amd.fold import Folder
    fd = Folder()
    assert (fd.npart, fd.nbins, fd.A, fd.B) == (32, 64, 64, 64)
    assert (Folder(1, 2).A, Folder(32, 256).B, Folder(128, 64, 3, 0).B) == (2, 256, 0)
    for bad in ((32, 1), (32, 257), (0, 64), (129, 64), (128, 128), (64, 129)):
        with pytest.raises(ValueError):
            Folder(*bad)
    for kw in ({"ntrial_f": 257}, {"ntrial_fd": -1}):
        with pytest.raises(ValueError):
            Folder(**kw)
    with pytest.raises(ValueError):
        fd.jobs([0], 10.0)                       # no sample time
    jobs = fd.jobs([3, 1], [10.0, 20.0], 0.0, 64e-6, 0.25)
    assert jobs.shape == (2, 4) and jobs.dtype == np.int64 and jobs[:, 0].tolist() == [3, 1]
    assert tuple(int(v) for v in jobs[1, 1:].view(np.uint64)) == fo.phase_steps(20.0, 0.0, 64e-6, 0.25)
    assert fd.span(1000, 0.5) == 32 * 31 * 0.5
