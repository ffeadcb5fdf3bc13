"""NumPy restatement of the birdie finder and the zap (test infrastructure:
no product path imports it; it imports nothing of the product).

Restates, freshly, what pypulsar_amd/zap.py and pypulsar_amd/csrc/pdd_zap.hip
implement:

* ``order_statistic``   the rank-th smallest value of every column
                        (``np.sort(P, axis=0)[rank - 1]``);
* ``rank`` / ``threshold``  the order statistic of a percentile and the power
                        it exceeds under Exp(1) noise with probability
                        ``norm.sf(nsig)``;
* ``flag``              thresholding, run growing and merging;
* ``to_bins`` / ``from_bins``  the frequency <-> bin rules of a zaplist;
* ``fill``              the zap of powers and spectrum;
* ``whiten`` / ``find``  the finder on a host plane, whitened by
                        tests/period_oracle.py;
* ``synthetic_plane``   the plane the CPU and GPU tests share.
"""
import math

import numpy as np

import period_oracle as po


def order_statistic(P, rank):
    P = np.asarray(P, dtype=np.float32)
    assert 1 <= rank <= P.shape[0]
    return np.sort(P, axis=0)[rank - 1]


def select_rows(D, rows=33):
    return np.unique(np.round(np.linspace(0, D - 1, min(rows, D)))).astype(np.int64)


def rank(R, percent=50.0):
    return max(1, int(math.ceil(percent * R / 100.0)))


def threshold(R, percent=50.0, nsig=5.0):
    """x with P(j-th of R Exp(1) order statistics > x) = norm.sf(nsig): the
    j-th smallest exceeds x when at least R - j + 1 of the R values do, each
    with probability q = exp(-x), so the binomial tail is solved for q."""
    from scipy.optimize import brentq
    from scipy.stats import binom, norm
    j = rank(R, percent)
    p = norm.sf(nsig)
    q = brentq(lambda lq: binom.logsf(R - j, R, math.exp(lq)) - math.log(p), -60.0, -1e-12,
               xtol=1e-14, rtol=1e-14)
    return -q


def merge(iv):
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in iv):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def flag(pct, R, rlo, percent=50.0, nsig=5.0, grow=1):
    """Intervals of the bins k >= rlo with pct[k] > threshold, every run
    grown by ``grow`` within [1, nn - 1], merged."""
    pct = np.asarray(pct, dtype=np.float64)
    nn = len(pct)
    thr = threshold(R, percent, nsig)
    iv = []
    k = max(1, int(rlo))
    while k < nn:
        if pct[k] > thr:
            e = k
            while e + 1 < nn and pct[e + 1] > thr:
                e += 1
            iv.append((max(1, k - grow), min(nn - 1, e + grow)))
            k = e + 1
        else:
            k += 1
    return merge(iv)


def to_bins(freqs, widths, nfft, dt, nn):
    T = nfft * dt
    iv = []
    for f, w in zip(freqs, widths):
        lo = max(1, int(math.floor((f - w / 2.0) * T + 1e-6)))
        hi = min(nn - 1, int(math.ceil((f + w / 2.0) * T - 1e-6)))
        if lo <= hi:
            iv.append((lo, hi))
    return merge(iv)


def from_bins(bins, nfft, dt):
    T = nfft * dt
    b = np.asarray(bins, dtype=np.float64).reshape(-1, 2)
    return (b[:, 0] + b[:, 1]) / (2.0 * T), (b[:, 1] - b[:, 0]) / T


def fill(powers, bins, spectrum=None):
    """Copies of powers [D, nn] (and the complex64 spectrum) with the bins of
    the inclusive intervals at the whitened mean level."""
    p = np.array(powers, dtype=np.float32, copy=True)
    s = None if spectrum is None else np.array(spectrum, dtype=np.complex64, copy=True)
    for lo, hi in np.asarray(bins).reshape(-1, 2):
        p[:, lo:hi + 1] = np.float32(1.0)
        if s is not None:
            s[:, lo:hi + 1] = np.complex64(np.float32(0.70710677) + 1j * np.float32(0.70710677))
    return p if s is None else (p, s)


def whiten(plane, nfft):
    """float32 whitened powers [D, nfft // 2] of host plane rows: mean removed
    in float64, zero padded, transformed, whitened as by period_oracle."""
    plane = np.asarray(plane, dtype=np.float32)
    D, n = plane.shape
    nn = nfft // 2
    out = np.empty((D, nn), dtype=np.float32)
    for d in range(D):
        x = np.zeros(nfft, dtype=np.float32)
        x[:n] = (plane[d].astype(np.float64) - plane[d].astype(np.float64).mean()).astype(
            np.float32)
        w = po.deredden(np.fft.rfft(x.astype(np.float64))[:nn].astype(np.complex64))
        out[d] = w.real.astype(np.float32) ** 2 + w.imag.astype(np.float32) ** 2
    return out


def find(powers, rlo, rows=33, percent=50.0, nsig=5.0, grow=1):
    """(intervals, percentile spectrum) of whitened powers [D, nn]."""
    sel = select_rows(powers.shape[0], rows)
    R = len(sel)
    pct = order_statistic(powers[sel], rank(R, percent))
    return flag(pct, R, rlo, percent, nsig, grow), pct


# ---- the synthetic plane of the CPU and GPU tests ----

SHAPES = ((9, 4096, 4096), (33, 3000, 4096))   # (D, n, nfft)
BIRDIE_BIN = 517
PULSAR_ROW, PULSAR_PERIOD = 4, 64              # the pulsar's bin: nfft // 64
DT = 64e-6


def synthetic_plane(D, n, nfft, A, seed=0):
    """float32 [D, n]: rounded noise of level 524288 and sigma 1024, a birdie
    ``A sin(2 pi 517 t / nfft)`` in every row and a pulse train of period 64
    samples in row 4 only."""
    rng = np.random.default_rng(seed)
    x = np.round(524288.0 + rng.normal(0.0, 1024.0, (D, n)))
    t = np.arange(n)
    x += A * np.sin(2.0 * np.pi * BIRDIE_BIN * t / nfft)[None, :]
    x[PULSAR_ROW] += 4000.0 * ((t % PULSAR_PERIOD) < 2)
    return x.astype(np.float32)
