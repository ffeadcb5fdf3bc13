"""NumPy float64 restatement of the RFI statistics and of the mask decision
(DESIGN.md §6g), written from the definitions, independently of
pypulsar_amd/rfi.py and of the device code; plus the seeded test inputs.

x: time-major [T, C]; intervals of P samples; nint = T // P (ragged tail
ignored).  Per (interval i, channel c), over the N = P samples of the cell:
    avg = sum x / N
    var = population variance;  std = sqrt(var)
    pow = max_{k=1..P//2} |rfft(x - avg)[k]|^2 / (P var),  0 where var == 0
8-bit input: S1 = sum x, S2 = sum x^2 as exact integers,
    avg = float(S1) / float(N),  var = float(N S2 - S1 S1) / float(N N)
(each conversion and division one IEEE double operation).
"""
import math

import numpy as np
from scipy.stats import norm


def stats(x, P, fft_dtype=np.float64):
    """(avg, std, pow), float64 [nint, C].  fft_dtype=float32 does the
    transform (input, butterflies, |.|^2) in single precision: the yardstick
    of the device's float32 transform."""
    x = np.asarray(x)
    T, C = x.shape
    nint = T // P
    cells = x[:nint * P].reshape(nint, P, C)
    if x.dtype == np.uint8:
        v = cells.astype(np.int64)
        s1 = v.sum(axis=1)
        s2 = (v * v).sum(axis=1)
        avg = s1.astype(np.float64) / float(P)
        var = (P * s2 - s1 * s1).astype(np.float64) / float(P * P)
    else:
        v = cells.astype(np.float64)
        avg = v.mean(axis=1)
        var = ((v - avg[:, None, :]) ** 2).mean(axis=1)
    std = np.sqrt(var)
    d = cells.astype(np.float64) - avg[:, None, :]
    if fft_dtype == np.float32:
        import scipy.fft
        f = scipy.fft.rfft(d.astype(np.float32), axis=1)
        assert f.dtype == np.complex64
        p = (f.real * f.real + f.imag * f.imag)[:, 1:P // 2 + 1].max(axis=1).astype(np.float64)
    else:
        f = np.fft.rfft(d, axis=1)
        p = (f.real ** 2 + f.imag ** 2)[:, 1:P // 2 + 1].max(axis=1)
    pw = np.zeros_like(var)
    nz = var > 0
    pw[nz] = p[nz] / (P * var[nz])
    return avg, std, pw


def pthr(freq_sig, P):
    nb = P // 2
    return -math.log(1.0 - (1.0 - norm.sf(freq_sig)) ** (1.0 / nb))


def _med_mad(v):
    med = float(np.median(v))
    return med, 1.4826 * float(np.median(np.abs(np.asarray(v) - med)))


def decide(avg, std, pw, P, time_sig=10.0, freq_sig=4.0, chan_sig=6.0, chan_window=16,
           chantrigfrac=0.7, inttrigfrac=0.3, margins=None):
    """bool [nint, C].  margins: optional list that receives, for every cell
    left unflagged by steps 1-2, the ratios value / threshold of its three
    tests (pow / pthr, |avg dev| / (time_sig scatter), |std dev| / (...))."""
    nint, C = avg.shape
    thr = pthr(freq_sig, P)
    bad = np.zeros((nint, C), dtype=bool)
    for i in range(nint):
        for c in range(C):
            bad[i, c] = pw[i, c] > thr or std[i, c] == 0
    flag = bad.copy()
    ratios = np.zeros((nint, C, 3))
    ratios[:, :, 0] = pw / thr
    for c in range(C):
        keep = [i for i in range(nint) if not bad[i, c]]
        if not keep:
            continue
        ma, sa = _med_mad(avg[keep, c])
        ms, ss = _med_mad(std[keep, c])
        for i in range(nint):
            da, ds = abs(avg[i, c] - ma), abs(std[i, c] - ms)
            if da > time_sig * sa or ds > time_sig * ss:
                flag[i, c] = True
            ratios[i, c, 1] = da / (time_sig * sa) if sa > 0 else (np.inf if da > 0 else 0.0)
            ratios[i, c, 2] = ds / (time_sig * ss) if ss > 0 else (np.inf if ds > 0 else 0.0)
    if margins is not None:
        margins.extend(ratios[~flag].ravel().tolist())
    m = [None] * C
    for c in range(C):
        keep = [i for i in range(nint) if not flag[i, c]]
        if keep:
            m[c] = float(np.median(std[keep, c]))
    whole = []
    for c in range(C):
        if m[c] is None:
            whole.append(c)
            continue
        near = [m[k] for k in range(max(0, c - chan_window), min(C, c + chan_window + 1))
                if m[k] is not None]
        med, scat = _med_mad(near)
        if abs(m[c] - med) > chan_sig * scat:
            whole.append(c)
    for c in whole:
        flag[:, c] = True
    for c in range(C):
        if flag[:, c].sum() > chantrigfrac * nint:
            flag[:, c] = True
    for i in range(nint):
        if flag[i, :].sum() > inttrigfrac * C:
            flag[i, :] = True
    return flag


def fill(avg, mask):
    C = avg.shape[1]
    out = np.full(C, np.nan)
    for c in range(C):
        keep = ~mask[:, c]
        if keep.any():
            out[c] = np.median(avg[keep, c])
    ok = ~np.isnan(out)
    out[~ok] = np.median(out[ok]) if ok.any() else 0.0
    return out


# ---- the seeded inputs: 8-bit noise with a sinusoidal bandpass and five
# injections.  (P, nint, C, seed): the seed of each shape is the one for which
# test_rfi_oracle.py asserts exact recovery with >= 1 % margins.
SIGMA = 8.0
CASES = {"p256": (256, 16, 64, 1), "p1024": (1024, 12, 48, 1)}


def make_input(P, nint, C, seed, dtype=np.uint8):
    """(x [nint P + 37, C], injected bool [nint, C]).  Injections: a noisy
    channel (sigma x 2.5), a dead channel (constant), a level-jumped interval
    (+25 in every channel), a tone of amplitude 1.5 sigma in one cell, a
    4-sample burst of +120 in one cell."""
    rng = np.random.default_rng(seed)
    T = nint * P + 37
    level = 110.0 + 30.0 * np.sin(2 * np.pi * np.arange(C) / C)
    x = rng.normal(0.0, SIGMA, (T, C))
    want = np.zeros((nint, C), dtype=bool)
    c_noisy, c_dead, i_jump = C // 5, C // 2, nint // 3
    x[:, c_noisy] *= 2.5
    want[:, c_noisy] = True
    x += level
    x[i_jump * P:(i_jump + 1) * P] += 25.0
    want[i_jump] = True
    it, ct = nint - 2, C // 3
    x[it * P:(it + 1) * P, ct] += 1.5 * SIGMA * np.sin(2 * np.pi * 0.1173 * np.arange(P))
    want[it, ct] = True
    ib, cb = 1, C - 5
    x[ib * P + 50:ib * P + 54, cb] += 120.0
    want[ib, cb] = True
    x[:, c_dead] = 97.0
    want[:, c_dead] = True
    if dtype == np.uint8:
        return np.clip(np.rint(x), 0, 255).astype(np.uint8), want
    return x.astype(np.float32), want


def small_input():
    """8-bit noise [5 * 100, 24]: its first 16 columns are the block with a
    non-power-of-two interval (100), row stride > C and C % 32 != 0."""
    rng = np.random.default_rng(2)
    return np.clip(np.rint(rng.normal(120.0, 9.0, (500, 24))), 0, 255).astype(np.uint8)
