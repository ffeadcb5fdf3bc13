"""The NumPy restatement of the fast-folding search (tests/ffa_oracle.py)
checked against itself: the butterfly against the direct sum of shifted rows,
the plan's tiling, the noise statistics of the score and a detection.  CPU
only."""
import numpy as np
import pytest

import ffa_oracle as fo


# ---- butterfly and shifts ----

@pytest.mark.parametrize("Mp", [2, 4, 8, 16, 32, 64, 128, 256])
def test_butterfly_is_direct_sum(Mp):
    p0 = 13
    # (integer-valued rows: the float32 butterfly and the float64 sum are exact)
    x = np.random.default_rng(Mp).integers(-50, 50, (Mp, p0)).astype(np.float32)
    got = fo.butterfly(x)
    if Mp <= 64:
        np.testing.assert_array_equal(got, fo.butterfly_recursive(x))
    for s in range(Mp):
        assert fo.shift(s, 0, Mp) == 0 and fo.shift(s, Mp - 1, Mp) == s
    for s in sorted(set([0, 1, Mp // 2, Mp - 2, Mp - 1]) | set(range(0, Mp, 7))):
        np.testing.assert_array_equal(got[s].astype(np.float64), fo.direct(x, s))


def _max_deviation(Mp):
    """Largest |shift(s, r) - s r / (Mp - 1)| over all trials and rows, by
    the recursion applied to whole arrays (shift[s, r])."""
    sh = np.zeros((1, 1), dtype=np.int64)
    m = 1
    while m < Mp:
        m *= 2
        s = np.arange(m)
        half = sh[s >> 1]                                   # [m, m / 2]
        sh = np.concatenate([half, ((s + 1) >> 1)[:, None] + half], axis=1)
    s, r = np.arange(Mp)[:, None], np.arange(Mp)[None, :]
    return float(np.max(np.abs(sh - s * r / float(Mp - 1))))


def test_shift_deviation_from_the_line():
    # array form == scalar closed form
    for Mp in (2, 8, 32):
        sh = np.asarray([[fo.shift(s, r, Mp) for r in range(Mp)] for s in range(Mp)])
        s, r = np.arange(Mp)[:, None], np.arange(Mp)[None, :]
        assert np.max(np.abs(sh - s * r / float(Mp - 1))) == pytest.approx(_max_deviation(Mp))
    for Mp in (4, 8, 16, 32, 64):
        dev = _max_deviation(Mp)
        print("Mp = %d: largest deviation of a row's shift from the line %.3f bin" % (Mp, dev))
        assert dev <= 1.0
    # recorded, not bounded: 2.000 bins at Mp = 4096
    print("Mp = 4096: largest deviation %.3f bin" % _max_deviation(4096))


# ---- plan ----

@pytest.mark.parametrize("n,dt,pmin,pmax,bmin,bmax", [
    (1 << 20, 64e-6, 0.5, 10.0, 250, 500),
    (1 << 20, 64e-6, 0.016, 0.3, 250, 500),
    (20000, 1e-3, 0.016, 0.1, 16, 40),
    (1 << 16, 1e-3, 0.3, 2.9, 100, 333),
])
def test_plan_tiles_the_range(n, dt, pmin, pmax, bmin, bmax):
    plan = fo.ffa_plan(n, dt, pmin, pmax, bmin, bmax)
    assert len(plan) >= 1
    P, fprev = pmin, 0
    for f, b_lo, b_hi in plan:
        dts = f * dt
        assert f >= max(1, fprev)                      # f never descends
        assert bmin <= b_lo < b_hi <= bmax             # every p0 in [bins_min, bins_max)
        assert b_lo * dts <= P * (1 + 1e-12) < (b_lo + 1) * dts   # no gap at the step's start
        assert n // f >= 2 * b_hi
        P, fprev = b_hi * dts, f
    assert P >= pmax                                    # ... and none at the end
    per, p0, s, f, M = fo.trial_table(n, dt, plan)
    # ascending period within a step; a new step starts at most one of its bins
    # below the end of the one before
    new = np.flatnonzero(np.diff(f) != 0) + 1
    for seg in np.split(per, new):
        assert np.all(np.diff(seg) > 0)
    for i in new:
        assert per[i - 1] - f[i] * dt < per[i] <= per[i - 1] + f[i] * dt
    assert per[0] <= pmin * (1 + 1e-12) and per[-1] < P


def test_plan_refuses_a_short_series():
    with pytest.raises(ValueError):
        fo.ffa_plan(4096, 1e-3, 0.5, 3.0, 250, 500)    # 3 s needs 2 x 3 s of data
    with pytest.raises(ValueError):
        fo.ffa_plan(1 << 20, 64e-6, 0.001, 1.0)        # period_min below bins_min * dt
    with pytest.raises(ValueError):
        fo.ffa_plan(1 << 20, 64e-6, 0.5, 10.0, 4, 500)


# ---- score ----

def test_score_noise_statistics():
    n, p0 = 1 << 16, 64
    x = np.random.default_rng(5).normal(0.0, 1.0, n).astype(np.float32)
    yp, sig = fo.prep(x[None, :], 1, n)                 # one chunk: mean removal
    prof = fo.transform(yp[0], p0)[:-1]
    sw = fo.boxcar_snr(prof, n // p0, sig[0])
    assert len(sw) == 6                                 # widths 1 .. 9 of 64 bins at ducy 0.2
    # S_w is the LARGEST of the p0 boxcar sums of a trial (the maximum of p0
    # correlated unit Gaussians, mean about 2); the unit Gaussian the
    # normalisation promises is the boxcar at a given phase, so the statistic
    # is taken over all trials and all phases of each width
    P2 = np.concatenate([prof, prof], axis=1).astype(np.float64)
    c = np.concatenate([np.zeros((len(prof), 1)), np.cumsum(P2, axis=1)], axis=1)
    tot = prof.astype(np.float64).sum(axis=1)
    for wi, w in enumerate(fo.DEFAULT_WIDTHS[:6]):
        S = c[:, w:w + p0] - c[:, 0:p0]                 # [trial, phase]
        z = (S - w * tot[:, None] / p0) / (sig[0] * np.sqrt((n // p0) * w * (1.0 - w / p0)))
        print("w = %d: mean %.4f std %.4f (largest-phase mean %.3f)" % (w, z.mean(), z.std(),
                                                                        sw[wi].mean()))
        assert abs(z.mean()) <= 0.05 and abs(z.std() - 1.0) <= 0.05
        np.testing.assert_allclose(sw[wi], z.max(axis=1), rtol=0, atol=1e-4)


def test_constant_row_scores_zero():
    x = np.full((1, 4096), 5.0, dtype=np.float32)
    yp, sig = fo.prep(x, 3, 1000)
    assert sig[0] == 0.0 and not np.any(yp)
    snr, wid, _ = fo.score(fo.transform(yp[0], 50)[:-1], len(yp[0]) // 50, sig[0])
    assert not np.any(snr) and not np.any(wid) and np.all(np.isfinite(snr))


# ---- detection ----

def test_detection():
    n, p0, s_true, width = 4096, 50, 37, 3
    M = n // p0
    Mp = fo.mp_of(M)
    period = p0 + s_true / float(Mp - 1)
    x = np.random.default_rng(11).normal(0.0, 1.0, n)
    ph = (np.arange(n) / period) % 1.0
    x[ph * period < width] += 1.0                       # 1 sigma per sample, 3 bins wide
    yp, sig = fo.prep(x[None, :].astype(np.float32), 1, n)
    snr, wid, _ = fo.score(fo.transform(yp[0], p0)[:-1], M, sig[0])
    best = int(np.argmax(snr))
    print("best trial s = %d, width %d, S/N %.2f" % (best, fo.DEFAULT_WIDTHS[wid[best]],
                                                      snr[best]))
    assert abs(best - s_true) <= width + 1
    assert fo.DEFAULT_WIDTHS[wid[best]] in (3, 4)
    assert snr[best] > 8.0
