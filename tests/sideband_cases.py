"""Shared inputs of the sideband tests (host only: NumPy and the oracles).

``recovery_series``: the phase-modulated signal of DESIGN.md §6q's recovery
case -- ``amp cos(2 pi f0 (t - x sin(2 pi t / Porb + 0.7)))`` in unit Gaussian
noise with ``n = nfft = 8192``, ``dt = 1e-3``, ``f0 = 2500.4 / T``, ``Porb = T
/ 8.37``, modulation index ``beta = 2 pi f0 x = 6`` and ``amp = 0.22``: a comb
of about 12 lines none of which reaches 6 sigma.
"""
import numpy as np

import period_oracle as po
import sideband_oracle as so

N, DT = 8192, 1e-3
T = N * DT
F0 = 2500.4 / T
NORB = 8.37            # orbits in the observation
PORB = T / NORB
BETA, AMP = 6.0, 0.22
FLO = 1.0
HARMS = (1, 2, 4)
QLO = 4


def recovery_series(seed, n=N, dt=DT, amp=AMP):
    rng = np.random.default_rng(seed)
    t = np.arange(n) * dt
    x = BETA / (2.0 * np.pi * F0)
    sig = amp * np.cos(2.0 * np.pi * F0 * (t - x * np.sin(2.0 * np.pi * t / PORB + 0.7)))
    return rng.standard_normal(n) + sig


def whitened_powers(series):
    """float32 whitened powers [n // 2] by the periodicity oracle."""
    x = np.asarray(series, dtype=np.float64)
    x = (x - x.mean()).astype(np.float32)
    spec = np.fft.rfft(x.astype(np.float64))[:len(x) // 2].astype(np.complex64)
    w = po.deredden(spec)
    return (w.real.astype(np.float32) ** 2 + w.imag.astype(np.float32) ** 2).astype(np.float32)


def rlo(nfft=N, dt=DT, flo=FLO):
    return max(1, int(np.ceil(flo * nfft * dt)))


def oracle_search(powers, sigma_threshold=6.0, harms=HARMS, qlo=QLO, shift=2, clip=None,
                  log2s=range(5, 15), r_lo=None):
    """Every candidate of the oracle over the ladder: a list of (sigma, L, lo,
    q, H, power) by descending sigma.  ``clip`` None: the single-bin
    threshold."""
    r_lo = rlo() if r_lo is None else r_lo
    thr = np.asarray([po.threshold_power(sigma_threshold, h) for h in harms], dtype=np.float32)
    clip = po.threshold_power(sigma_threshold, 1) if clip is None else clip
    out = []
    for e in log2s:
        L = 1 << e
        los = so.segments(len(powers), r_lo, L, shift)
        if not len(los):
            continue
        M = so.mini(powers, r_lo, L, shift, clip).astype(np.float32)
        for j, q, H, bits in so.candidates(M, harms, thr, qlo):
            p = float(np.asarray([bits], dtype=np.int32).view(np.float32)[0])
            out.append((po.sigma(p, H), L, int(los[j]), q, H, p))
    return sorted(out, key=lambda c: (-c[0], c[1:]))
