"""Shared inputs of the orbit tests (host only: NumPy and the oracles).

``ORBITS``: four orbits ``(pb, x, e, omega, t0)`` on ``n = 16384`` samples of
``dt = 1e-3`` (``T = n dt``): a circular one, an eccentric one, a tight one
(many orbits in the row, the smallest knot spacing) and a wide one (a third of
an orbit, the largest excursion: 61 output samples at its end lie beyond the
row).  ``recovery_bank`` / ``derived_bank``: template banks for the recovery
series of tests/sideband_cases.py.  ``channel_data``: the 16-channel 8-bit
file of tests/test_gpu_sideband_cli.py.
"""
import numpy as np

import sideband_cases as sc

N, DT = 16384, 1e-3
T = N * DT
ORBITS = {
    "circ": (T / 2.3, 0.020, 0.0, 0.0, -0.11 * (T / 2.3)),
    "ecc": (T / 1.7, 0.015, 0.4, 1.1, 0.23 * (T / 1.7)),
    "tight": (T / 37.3, 0.001, 0.0, 0.0, 0.0),
    "wide": (3.1 * T, 0.5, 0.0, 0.0, 0.4 * (3.1 * T)),
}
NAMES = ("circ", "ecc", "tight", "wide")
KNOT_K = {"circ": 16, "ecc": 16, "tight": 4, "wide": 16}   # the rule's spacing, one orbit a launch
FILL_COUNT = {"circ": 0, "ecc": 0, "tight": 1, "wide": 61}  # outputs whose position leaves the row
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)                         # x = 0: the row itself

# the recovery signal's own orbit: x sin(2 pi t / PORB + 0.7)
PSI = 0.7
X_TRUE = sc.BETA / (2.0 * np.pi * sc.F0)
W0 = 2.0 * np.pi / sc.PORB
MISMATCH = 0.05


def circular(x, w, psi):
    """(pb, x, 0, 0, t0) of the delay ``x sin(w t + psi)``."""
    pb = 2.0 * np.pi / w
    return (pb, x, 0.0, 0.0, -psi * pb / (2.0 * np.pi))


TRUE_ORBIT = circular(X_TRUE, W0, PSI)


def recovery_bank(m=MISMATCH):
    """The 3 x 5 x 3 bank around the truth, off its nodes: ``dx = 2 m / F0``,
    ``x_i = x + (i + .3) dx``, ``psi = .7 + (k + .3) 2 m / (F0 x_i)``, ``W = W0 +
    (l - .3) 2 m / (F0 x T)``; float64 [45, 5]."""
    Tr = sc.N * sc.DT
    dx = 2.0 * m / sc.F0
    out = []
    for i in (-1, 0, 1):
        xi = X_TRUE + (i + 0.3) * dx
        for k in (-2, -1, 0, 1, 2):
            psi = PSI + (k + 0.3) * 2.0 * m / (sc.F0 * xi)
            for l in (-1, 0, 1):
                out.append(circular(xi, W0 + (l - 0.3) * 2.0 * m / (sc.F0 * X_TRUE * Tr), psi))
    return np.asarray(out, dtype=np.float64)


def derived_bank_args(L=256, q=61, lo=2377, numharm=1, n=sc.N, dt=sc.DT):
    """(porb_lo, porb_hi, x_max, f_top, T) of the bank that follows a sideband
    candidate ``(L, q)`` whose segment starts at bin ``lo``: ``porb = q n dt /
    (2 L)`` +- ``porb / q``, ``x_max = (f_hi - f_lo) porb / (4 pi f_lo)``,
    ``f_top = numharm f_hi``."""
    Tr = n * dt
    porb = q * Tr / (2.0 * L)
    f_lo, f_hi = lo / Tr, (lo + L) / Tr
    return (porb - porb / q, porb + porb / q, (f_hi - f_lo) * porb / (4.0 * np.pi * f_lo),
            numharm * f_hi, Tr)


# ---- the file of the command-line test ----

C, SIGMA_CH = 16, 16.0


def channel_data(seed=3):
    """[C, n] uint8: noise of SIGMA_CH counts a channel around 128 and, in
    every channel (DM 0), the recovery signal with the amplitude that gives the
    channel sum the plane case's ratio of amplitude to noise."""
    rng = np.random.default_rng(seed)
    a = sc.AMP * SIGMA_CH / np.sqrt(C)
    t = np.arange(sc.N) * sc.DT
    sig = a * np.cos(2.0 * np.pi * sc.F0 * (t - X_TRUE * np.sin(2.0 * np.pi * t / sc.PORB + PSI)))
    data = rng.normal(128.0, SIGMA_CH, (C, sc.N)) + sig[None, :]
    return np.clip(np.round(data), 0, 255).astype(np.uint8)
