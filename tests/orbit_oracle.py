"""NumPy restatement of the orbit demodulation (include/pdd.h, DESIGN.md §6r;
host only, float64 unless said otherwise).

Orbit ``(pb, x, e, omega, t0)``; Roemer delay ``D(t) = x [(cos E - e) sin omega
+ sin E sqrt(1 - e^2) cos omega]`` with ``E - e sin E = 2 pi (t - t0) / pb``.
Output sample ``j`` is taken at the input position ``p_j`` (samples) with ``p_j
- (D(p_j dt) - D(0)) / dt = j``.  The device evaluates ``p`` at the knots ``j =
k K`` and interpolates between them; the two sampling modes read the row at
``p``."""
import math

import numpy as np

NEAREST, LINEAR = 0, 1


def kepler(M, e):
    """The eccentric anomaly ``E`` of mean anomaly ``M``: Newton's iteration
    from ``M + e sin M`` (from pi for e >= 0.8), to round-off."""
    M = np.asarray(M, dtype=np.float64)
    turns = np.rint(M / (2.0 * np.pi))
    a = M - 2.0 * np.pi * turns
    sign = np.where(a < 0.0, -1.0, 1.0)
    a = np.abs(a)
    E = a + e * np.sin(a) if e < 0.8 else np.full_like(a, np.pi)
    for _ in range(60):
        d = (E - e * np.sin(E) - a) / (1.0 - e * np.cos(E))
        E = E - d
        if np.all(np.abs(d) <= 1e-15):
            break
    return sign * E + 2.0 * np.pi * turns


def delay(orbit, t):
    """(D(t), dD/dt) in s and s/s."""
    pb, x, e, om, t0 = (float(v) for v in orbit)
    t = np.asarray(t, dtype=np.float64)
    nb = 2.0 * np.pi / pb
    E = kepler(nb * (t - t0), e)
    s, c = np.sin(E), np.cos(E)
    q = math.sqrt(1.0 - e * e)
    D = x * ((c - e) * math.sin(om) + s * q * math.cos(om))
    dD = x * (-s * math.sin(om) + c * q * math.cos(om)) * nb / (1.0 - e * c)
    return D, dD


def beta(orbit):
    pb, x, e = (float(v) for v in orbit[:3])
    return x * (2.0 * np.pi / pb) / (1.0 - e)


def positions(orbit, j, dt):
    """``p_j`` in samples for the output samples ``j`` (any array)."""
    j = np.asarray(j, dtype=np.float64)
    D0 = float(delay(orbit, 0.0)[0])
    p = j.copy()
    for _ in range(30):
        D, dD = delay(orbit, p * dt)
        d = ((p - j) - (D - D0) / dt) / (1.0 - dD)
        p = p - d
        if np.all(np.abs(d) <= 1e-12):
            break
    return p


def knot_count(n, K):
    return (int(n) - 1) // int(K) + 2


def knots(orbit, n, K, dt):
    """The exact positions at ``j = k K``, ``k < nk``."""
    return positions(orbit, np.arange(knot_count(n, K), dtype=np.float64) * K, dt)


def spacing(orbits, dt, budget=1e-3):
    """The largest power of two ``K <= 256`` with ``A K^2 / 8 <= budget`` for
    all orbits, ``A = x (2 pi / pb)^2 dt / ((1 - e)^3 (1 - beta)^3)``."""
    A = max(o[1] * (2.0 * np.pi / o[0]) ** 2 * dt / ((1.0 - o[2]) ** 3 * (1.0 - beta(o)) ** 3)
            for o in orbits)
    K = 256
    while K > 1 and A * K * K / 8.0 > budget:
        K //= 2
    return K


def interpolate(knot, n, K):
    """``p_j``, ``j < n``, from a knot table: ``p_k + (p_{k+1} - p_k) (i / K)``
    for ``j = k K + i``, one IEEE float64 operation each, in this order."""
    knot = np.asarray(knot, dtype=np.float64)
    j = np.arange(int(n))
    k, i = j // K, j % K
    w = i.astype(np.float64) / float(K)
    return knot[k] + (knot[k + 1] - knot[k]) * w


def sample(row, p, mode, fill):
    """float32 [len(p)]: ``row`` read at the positions ``p`` by ``mode``; a
    position outside ``[0, n - 1]`` gives ``fill``."""
    row = np.asarray(row, dtype=np.float32)
    n = len(row)
    p = np.asarray(p, dtype=np.float64)
    inside = (p >= 0.0) & (p <= float(n - 1))
    q = np.where(inside, p, 0.0)
    if mode == NEAREST:
        val = row[np.floor(q + 0.5).astype(np.int64)]
    else:
        fl = np.floor(q)
        i0 = fl.astype(np.int64)
        f = (q - fl).astype(np.float32)
        a, b = row[i0], row[np.minimum(i0 + 1, n - 1)]
        val = np.where(i0 < n - 1, (a + (b - a) * f).astype(np.float32), a)
    return np.where(inside, val, np.float32(fill)).astype(np.float32)


def resample(row, orbit, dt, K, mode, fill, knot=None):
    """One template's output row; ``knot``: the knot table to interpolate
    (default: the exact one)."""
    n = len(row)
    knot = knots(orbit, n, K, dt) if knot is None else knot
    return sample(row, interpolate(knot, n, K), mode, fill)


def bank_counts(porb_lo, porb_hi, x_max, f_top, T, m=0.05):
    """(x_k, Npsi_k, NW_k) of the circular bank: ``dx = 2 m / f_top``, ``x_k =
    k dx`` for ``k = 1 .. ceil(x_max / dx)``, ``Npsi = max(1, ceil(2 pi f_top
    x_k / (2 m)))``, ``NW = max(1, ceil((W_hi - W_lo) f_top x_k T / (2 m)))``
    with ``W = 2 pi / porb``."""
    dx = 2.0 * m / f_top
    w_lo, w_hi = 2.0 * np.pi / porb_hi, 2.0 * np.pi / porb_lo
    out = []
    for k in range(1, int(math.ceil(x_max / dx)) + 1):
        x = k * dx
        out.append((x, max(1, int(math.ceil(2.0 * np.pi * f_top * x / (2.0 * m)))),
                    max(1, int(math.ceil((w_hi - w_lo) * f_top * x * T / (2.0 * m))))))
    return out
