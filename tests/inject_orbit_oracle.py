"""NumPy restatement of the injector's Keplerian orbits (pypulsar_amd/inject.py,
pdd_inject_orbit), on top of tests/inject_oracle.py.

Two layers, as there:

* ``inject_arrays``: the cell arithmetic of pdd_inject_orbit on the job tables
  in the layouts of include/pdd.h (uint64 wrapping, float64 operations one by
  one) -- what the kernel is compared with, bit for bit;
* ``orbit_consts`` / ``qtab`` / ``build``: the orbital phase constants from the
  exact rational orbital phase at samples 0 and 1, and the table from a Kepler
  solver of its own (bisection), compared with ``Injector.orbit_arrays``.

An orbit is the tuple (pb, x, e, omega, t0) of pypulsar_amd.orbit; a signal
dict carries it under the keys of the same names.
"""
import math
from fractions import Fraction

import numpy as np

import inject_oracle as io

M64 = 1 << 64
MIN_M, MAX_M = 6, 22
BUDGET = 1e-6  # turns


# ---------------------------------------------------------------- the cell arithmetic
def orbital_term(i_abs, ophase_j, m, ostep, table):
    """float64 [n, C]: q of one job at absolute samples ``i_abs``; ``table``
    its 2^m + 1 knots."""
    i = np.asarray(i_abs, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        psi = ophase_j[None, :] + i[:, None] * np.uint64(ostep)
    k = (psi >> np.uint64(64 - m)).astype(np.int64)
    w = ((psi >> np.uint64(32 - m)) & np.uint64(0xffffffff)).astype(np.float64) * 2.0 ** -32
    qa, qb = table[k], table[k + 1]
    d = qb - qa
    return qa + d * w


def job_phases(i_abs, j, phase, drift, ophase, ometa, qtab):
    """uint64 [n, C]: the phase p of job j at absolute samples ``i_abs``."""
    p = io.phases(i_abs, phase[j], drift[j])
    m = int(ometa[j, 0])
    if m >= 0:
        assert MIN_M <= m <= MAX_M and ometa[j, 2] % 8 == 0
        at = int(ometa[j, 2]) // 8
        table = qtab[at:at + (1 << m) + 1]
        assert table.size == (1 << m) + 1
        ostep = int(np.array(ometa[j, 1], dtype=np.int64).view(np.uint64))
        q = orbital_term(i_abs, ophase[j], m, ostep, table)
        with np.errstate(over="ignore"):
            p = p - io.frac_u64(q)
    return p


def inject_arrays(x, t0, phase, drift, rng, tab, ophase, ometa, qtab, B, seed, vmax=255):
    """The block ``x`` [n, C] (uint8 or float32) after pdd_inject_orbit at
    ``t0``: inject_oracle.inject_arrays with the orbital term in the phase."""
    x = np.asarray(x)
    n, C = x.shape
    lb = int(B).bit_length() - 1
    assert 1 << lb == B and tab.shape[1:] == (C, B + 1)
    i = int(t0) + np.arange(n, dtype=np.int64)
    acc = np.zeros((n, C), dtype=np.float32)
    cov = np.zeros((n, C), dtype=bool)
    cc = np.arange(C)[None, :]
    for j in range(phase.shape[0]):
        lo, hi = rng[j, :C, 0], rng[j, :C, 1]
        m = (i[:, None] >= lo[None, :]) & (i[:, None] < hi[None, :])
        if not m.any():
            continue
        p = job_phases(i, j, phase, drift, ophase, ometa, qtab)
        b = (p >> np.uint64(64 - lb)).astype(np.int64)
        w = ((p >> np.uint64(40 - lb)) & np.uint64(0xffffff)).astype(np.float32) \
            * np.float32(2.0 ** -24)
        ta, tb = tab[j][cc, b], tab[j][cc, b + 1]
        v = ta + (tb - ta) * w
        assert v.dtype == np.float32
        acc = np.where(m, acc + v, acc)
        cov |= m
    if x.dtype == np.float32:
        return np.where(cov, x + acc, x)
    assert x.dtype == np.uint8
    y = (x.astype(np.float32) + acc) + io.dither(i, C, seed)
    y = np.minimum(np.float32(vmax), np.maximum(np.float32(0), np.floor(y)))
    return np.where(cov, y.astype(np.uint8), x)


# ---------------------------------------------------------------- the orbit model
def orbit_of(sig):
    """(pb, x, e, omega, t0) of a signal dict, or None."""
    if sig.get("pb") is None:
        return None
    return tuple(float(sig.get(k) or 0.0) for k in ("pb", "x", "e", "omega", "t0"))


def eccentric_anomaly(M, e):
    """E of ``E - e sin E = M`` by bisection on [0, 2 pi) per element (the
    left side is increasing in E), 60 halvings."""
    M = np.asarray(M, dtype=np.float64)
    turns = np.floor(M / (2.0 * np.pi))
    a = M - 2.0 * np.pi * turns
    lo, hi = np.zeros_like(a), np.full_like(a, 2.0 * np.pi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = mid - e * np.sin(mid) < a
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi) + 2.0 * np.pi * turns


def roemer(orb, t):
    """D(t) in seconds."""
    pb, x, e, om, t0 = orb
    E = eccentric_anomaly(2.0 * np.pi * (np.asarray(t, dtype=np.float64) - t0) / pb, e)
    return x * ((np.cos(E) - e) * math.sin(om) + np.sin(E) * math.sqrt(1.0 - e * e) * math.cos(om))


def table_bits(f, orb):
    """The smallest m in 6..22 whose table keeps f x (2 pi)^2 / (1 - e)^3 / (8
    M^2) within the budget; None when none does."""
    A = f * orb[1] * (2.0 * math.pi) ** 2 / (1.0 - orb[2]) ** 3
    for m in range(MIN_M, MAX_M + 1):
        if A / (8.0 * 4.0 ** m) <= BUDGET:
            return m
    return None


def qtab(f, orb, m):
    """float64 [2^m + 1]: f (D(t0 + k pb / M) - D(0)) in turns."""
    M = 1 << m
    k = np.arange(M + 1, dtype=np.float64)
    k[M] = 0.0
    return f * (roemer(orb, orb[4] + k * (orb[0] / M)) - roemer(orb, 0.0))


def exact_psi(orb, dt, delta, i):
    """The orbital phase ((i + 1/2) dt - delta - t0) / pb as an exact rational."""
    t = (Fraction(int(i)) + Fraction(1, 2)) * Fraction(float(dt)) - Fraction(float(delta))
    return (t - Fraction(float(orb[4]))) / Fraction(float(orb[0]))


def orbit_consts(orb, dt, delta):
    """(O0, ostep) as Python ints from the exact phase at samples 0 and 1."""
    y0, y1 = exact_psi(orb, dt, delta, 0), exact_psi(orb, dt, delta, 1)
    return round(y0 * M64) % M64, round((y1 - y0) * M64) % M64


def orbit_arrays(signals, freqs, dt):
    """ophase, ometa, qtab of include/pdd.h for signal dicts."""
    J, C = len(signals), len(freqs)
    ophase = np.zeros((J, C), dtype=np.uint64)
    ometa = np.zeros((J, 3), dtype=np.int64)
    ometa[:, 0] = -1
    tabs, at = [], 0
    for j, sig in enumerate(signals):
        orb = orbit_of(sig) if sig["kind"] == "pulsar" else None
        if orb is None:
            continue
        delta = io.lags(float(sig["dm"]), freqs)
        m = table_bits(float(sig["f"]), orb)
        assert m is not None
        step = 0
        for c in range(C):
            O0, step = orbit_consts(orb, dt, delta[c])
            ophase[j, c] = O0
        ometa[j] = (m, int(np.array(step, dtype=np.uint64).view(np.int64)), 8 * at)
        tabs.append(qtab(float(sig["f"]), orb, m))
        at += tabs[-1].size
    return ophase, ometa, (np.concatenate(tabs) if tabs else np.zeros(0))


def build(signals, freqs, dt, B=1024):
    """(the four arrays of inject_oracle.build, the three orbit arrays)."""
    _, arr = io.build(signals, freqs, dt, B)
    return arr, orbit_arrays(signals, freqs, dt)


def inject(x, t0, signals, freqs, dt, B=1024, seed=0, vmax=255):
    """``x`` [n, C] with the signals (dicts) added, its row 0 being sample ``t0``."""
    arr, orb = build(signals, freqs, dt, B)
    return inject_arrays(x, t0, *arr, *orb, B=B, seed=seed, vmax=vmax)
