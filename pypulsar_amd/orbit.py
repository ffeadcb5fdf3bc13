"""Coherent orbit search: one DM row demodulated over a bank of Keplerian
templates on the device (the reference's ``bin/demodulate.py``, which takes a
time series into the pulsar's frame by dropping and duplicating samples, for
many trial orbits at once).

The sideband search (``pypulsar_amd.sideband``) reports an orbital period and a
frequency range and stops there: the comb's power stays spread over about ``2
beta`` sidebands.  Here the row is resampled by every template of a bank into
a ``[templates, n]`` plane (pdd_orbit_resample, pypulsar_amd/csrc/pdd_orbit.hip;
restated in tests/orbit_oracle.py); ``PeriodicitySearch`` treats
that plane exactly like a DM-time plane -- the right template puts the comb's
power back into one bin -- and ``Folder`` folds the best row.

An orbit is ``(pb, x, e, omega, t0)``: the period in s, the projected
semi-major axis in light-seconds, the eccentricity in [0, 1), the longitude of
periastron in rad and the time of periastron in s after the row's first sample
(for ``e = 0``: the ascending node).  The Roemer delay is ``D(t) = x [(cos E -
e) sin omega + sin E sqrt(1 - e^2) cos omega]`` with ``E - e sin E = 2 pi (t -
t0) / pb``; for ``e = omega = 0`` that is ``x sin(2 pi t / pb + psi)``, ``psi =
-2 pi t0 / pb``.  Output sample ``j`` is taken at the input position ``p_j =
t_j / dt`` with ``t_j - (D(t_j) - D(0)) = j dt``, so ``p_0 = 0``.  A template
with ``beta = x (2 pi / pb) / (1 - e)``, a bound on ``|dD/dt|``, above 0.1 is
refused (real binaries stay below 0.01): below it ``p`` is strictly
increasing.  No CPU fallback: the helpers below that work on the host
(``roemer``, ``positions``, ``knot_spacing``, ``circular_bank``) describe and
plan; the resampling itself is the kernel's.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import periodicity as _per
from ._lib import call, ptr, stream_ptr

Orbit = collections.namedtuple("Orbit", "pb x e omega t0")

MODES = {"nearest": _lib.ORBIT_NEAREST, "linear": _lib.ORBIT_LINEAR}
BETA_MAX = 0.1          # largest accepted bound on |dD/dt|
KNOT_BUDGET = 1e-3      # samples: the interpolation error between knots
MAX_K = 256             # largest knot spacing (kOrbMaxK in pdd_orbit.hip)
MIN_TILE = 2044         # fewest output samples a workgroup takes (K = 1; pdd_orbit.hip)

ORBCAND_DTYPE = np.dtype(_per.CAND_DTYPE.descr + [("template", "i8"), ("pb", "f8"), ("x", "f8"),
                                                  ("e", "f8"), ("omega", "f8"), ("t0", "f8")])
SIFTED_DTYPE = np.dtype(ORBCAND_DTYPE.descr + [("ntemplates", "i8"), ("nhits", "i4")])
_ORDER = ("template", "numharm", "r")
_ELEMENTS = ("pb", "x", "e", "omega", "t0")
# the columns of a .orbcands line, in order
ORBCANDS_COLUMNS = ("sigma", "DM", "freq", "period", "r", "numharm", "power", "template", "pb",
                    "x", "e", "omega", "t0", "ntemplates", "nhits")


# ---- orbits (host, float64) ----

def as_orbits(orbits):
    """An ``Orbit``, a sequence of them or an array -> float64 [T, 5]."""
    a = np.asarray(orbits, dtype=np.float64)
    if a.ndim == 1:
        a = a[None, :]
    assert a.ndim == 2 and a.shape[1] == 5, "orbits are (pb, x, e, omega, t0)"
    return np.ascontiguousarray(a)


def beta(orbits):
    """``x (2 pi / pb) / (1 - e)`` per template: a bound on ``|dD/dt|``."""
    o = as_orbits(orbits)
    return o[:, 1] * (2.0 * np.pi / o[:, 0]) / (1.0 - o[:, 2])


def validate(orbits):
    """float64 [T, 5] of ``orbits``; ValueError unless every value is finite,
    ``pb > 0``, ``x >= 0``, ``0 <= e < 1`` and ``beta <= 0.1``."""
    o = as_orbits(orbits)
    if not np.all(np.isfinite(o)):
        raise ValueError("orbit: every element must be finite")
    if np.any(o[:, 0] <= 0.0):
        raise ValueError("orbit: pb must be > 0")
    if np.any(o[:, 1] < 0.0):
        raise ValueError("orbit: x must be >= 0")
    if np.any(o[:, 2] < 0.0) or np.any(o[:, 2] >= 1.0):
        raise ValueError("orbit: e must be in [0, 1)")
    b = beta(o)
    if np.any(b > BETA_MAX):
        raise ValueError("orbit: beta = x (2 pi / pb) / (1 - e) = %.3g exceeds %.1f"
                         % (float(b.max()), BETA_MAX))
    return o


def _anomaly(M, e):
    """(sin E, cos E) of ``E - e sin E = M`` by Newton's iteration."""
    M = M - 2.0 * np.pi * np.rint(M / (2.0 * np.pi))
    a = np.abs(M)
    E = np.where(e < 0.8, a + e * np.sin(a), np.pi)
    for _ in range(40):
        d = (E - e * np.sin(E) - a) / (1.0 - e * np.cos(E))
        E = E - d
        if not np.any(np.abs(d) > 1e-13):
            break
    return np.where(M < 0.0, -np.sin(E), np.sin(E)), np.cos(E)


def _delay(o, t):
    """(D, dD/dt) of orbits ``o`` [T, 5] at times ``t`` [..., T] or scalar."""
    pb, x, e, om, t0 = (o[:, k] for k in range(5))
    nb = 2.0 * np.pi / pb
    s, c = _anomaly(nb * (t - t0), e)
    so, co = np.sin(om), np.sqrt(1.0 - e * e) * np.cos(om)
    return x * ((c - e) * so + s * co), x * (c * co - s * so) * (nb / (1.0 - e * c))


def roemer(orbits, t):
    """The Roemer delay ``D(t)`` in s: [T, len(t)] (one orbit: [len(t)])."""
    o = as_orbits(orbits)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    D = _delay(o, t[:, None])[0].T
    return D[0] if np.ndim(orbits) == 1 else D


def positions(orbit, n, dt, j=None):
    """Input positions ``p_j`` (float64, in samples) of the output samples
    ``j`` (default: all of ``0..n-1``) of one orbit: ``p - (D(p dt) - D(0)) /
    dt = j``, Newton's iteration to well below 1e-9 samples."""
    o = validate(orbit)
    assert len(o) == 1, "one orbit"
    dt = float(dt)
    j = np.arange(int(n), dtype=np.float64) if j is None else np.asarray(j, dtype=np.float64)
    D0 = _delay(o, np.zeros(1))[0][0]
    p = j.copy()
    for _ in range(16):
        D, dD = _delay(o, (p * dt)[:, None])
        d = ((p - j) - (D[:, 0] - D0) / dt) / (1.0 - dD[:, 0])
        p = p - d
        if not np.any(np.abs(d) > 1e-11):
            break
    return p


def curvature(orbits, dt):
    """``A = x (2 pi / pb)^2 dt / ((1 - e)^3 (1 - beta)^3)`` per template: a
    bound on ``|d2p/dj2|`` in samples per sample squared."""
    o = as_orbits(orbits)
    return o[:, 1] * (2.0 * np.pi / o[:, 0]) ** 2 * float(dt) / \
        ((1.0 - o[:, 2]) ** 3 * (1.0 - beta(o)) ** 3)


def knot_spacing(orbits, dt, budget=KNOT_BUDGET):
    """The largest power of two ``K`` in 1..256 with ``A K^2 / 8 <= budget``
    samples for every template: the error of the linear interpolation of ``p``
    between knots ``K`` samples apart.  The budget of 1e-3 samples is 1/500 of
    the +-0.5-sample jitter that the drop / duplicate rule itself accepts, and
    a phase error of at most 3e-3 rad at the Nyquist frequency."""
    A = float(np.max(curvature(orbits, dt))) if len(as_orbits(orbits)) else 0.0
    K = MAX_K
    while K > 1 and A * K * K / 8.0 > budget:
        K >>= 1
    return K


# ---- the resampler (device) ----

class Resampler(object):
    """``Resampler(mode="nearest")(row, orbits, dt)`` -> [T, n] float32 device
    tensor: ``row`` (a 1-D float32 device view of unit stride, e.g. a plane
    row) in the frame of every orbit of ``orbits`` (``Orbit``s or a [T, 5]
    array).  ``mode``: "nearest" takes the sample at ``floor(p + 0.5)`` (the
    reference's drop / duplicate), "linear" interpolates between the two
    neighbours in float32.  ``fill``: the value of an output sample whose
    position lies outside the row (default: the row's mean).  ``K``: the knot
    spacing (default: ``knot_spacing`` over all the call's templates).  With
    ``want_knots`` returns (out, knots float64 [T, (n - 1) // K + 2]).  All
    device work is queued on torch's current stream."""

    def __init__(self, mode="nearest"):
        _lib.require_gpu()
        if mode not in MODES:
            raise ValueError("mode must be one of %s" % ", ".join(sorted(MODES)))
        self.mode = mode

    def __call__(self, row, orbits, dt, fill=None, want_knots=False, K=None, out=None):
        assert row.is_cuda and row.dtype == torch.float32 and row.dim() == 1
        assert row.stride(0) == 1 or row.shape[0] <= 1, "row must have unit stride"
        o = validate(orbits)
        T, n, dt = len(o), int(row.shape[0]), float(dt)
        K = knot_spacing(o, dt) if K is None else int(K)
        if fill is None:
            fill = float(row.double().mean().item())
        if out is None:
            out = torch.empty((T, n), dtype=torch.float32, device=row.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.shape == (T, n)
        assert out.stride(1) == 1 or n <= 1
        nk = (n - 1) // K + 2
        knots = torch.empty((T, nk), dtype=torch.float64, device=row.device) if want_knots else None
        dev = torch.from_numpy(o).to(row.device)
        step = max(1, ((1 << 31) - 1) // (-(-n // MIN_TILE)))  # the grid limit of one launch
        for a in range(0, T, step):
            b = min(T, a + step)
            call("pdd_orbit_resample", ptr(row), n, ctypes.c_double(dt), ptr(dev[a:b]), b - a, K,
                 MODES[self.mode], ctypes.c_float(fill), ptr(out[a:b]), out.stride(0),
                 ptr(knots[a:b]) if want_knots else None, stream_ptr())
        return (out, knots) if want_knots else out


def demodulated(row, orbit, dt):
    """``row`` in the pulsar's frame of one orbit ("nearest", the reference's
    demodulate.py): the [n] float32 row that ``Folder`` folds."""
    o = as_orbits(orbit)
    assert len(o) == 1, "one orbit"
    return Resampler("nearest")(row, o, dt)[0]


# ---- template banks (host) ----

def circular_bank(porb_lo, porb_hi, x_max, f_top, T, mismatch=0.05, max_templates=1 << 20):
    """float64 [Nt, 5] circular templates (``e = omega = 0``) that cover
    orbital periods ``porb_lo .. porb_hi`` (s), ``0 < x <= x_max`` (light
    seconds) and every orbital phase, for an observation of ``T`` s.  The
    steps keep the Roemer-delay error between neighbours to the fraction ``m =
    mismatch`` of the shortest searched period ``1 / f_top``:

    * ``dx = 2 m / f_top``, ``x_k = k dx``, ``k = 1 .. ceil(x_max / dx)``;
    * per ``x_k``, ``ceil(2 pi f_top x_k / (2 m))`` phases ``psi = 2 pi i /
      Npsi`` (``t0 = -psi pb / (2 pi)``);
    * per ``x_k``, ``ceil((W_hi - W_lo) f_top x_k T / (2 m))`` angular
      frequencies ``W = 2 pi / pb`` at the midpoints of equal cells of ``[W_lo,
      W_hi]`` (a phase error of ``dW T`` at the end of the observation);

    each count at least 1; ordered by x, then W, then psi.  ValueError, with
    the count, when there are more than ``max_templates``."""
    porb_lo, porb_hi, f_top, T, m = (float(v) for v in (porb_lo, porb_hi, f_top, T, mismatch))
    assert 0.0 < porb_lo <= porb_hi and x_max >= 0.0 and f_top > 0.0 and T > 0.0 and m > 0.0
    dx = 2.0 * m / f_top
    w_lo, w_hi = 2.0 * np.pi / porb_hi, 2.0 * np.pi / porb_lo
    xs = dx * np.arange(1, int(math.ceil(float(x_max) / dx)) + 1, dtype=np.float64)
    npsi = np.maximum(1, np.ceil(2.0 * np.pi * f_top * xs / (2.0 * m))).astype(np.int64)
    nw = np.maximum(1, np.ceil((w_hi - w_lo) * f_top * xs * T / (2.0 * m))).astype(np.int64)
    total = int(np.sum(npsi * nw))
    if total > int(max_templates):
        raise ValueError("circular_bank: %d templates exceed max_templates=%d"
                         % (total, int(max_templates)))
    bank = np.zeros((total, 5), dtype=np.float64)
    at = 0
    for x, a, b in zip(xs, npsi, nw):
        w = w_lo + (np.arange(b, dtype=np.float64) + 0.5) * ((w_hi - w_lo) / b)
        psi = 2.0 * np.pi * np.arange(a, dtype=np.float64) / a
        pb = np.repeat(2.0 * np.pi / w, a)
        part = bank[at:at + a * b]
        part[:, 0] = pb
        part[:, 1] = x
        part[:, 4] = -np.tile(psi, b) * pb / (2.0 * np.pi)
        at += a * b
    return bank


# ---- the search over a bank (device) ----

class OrbitSearch(object):
    """``OrbitSearch(sigma_threshold=6.0)(row, dm, dt, bank)`` -> candidates
    (ORBCAND_DTYPE records: those of the periodicity search plus the template
    and its five elements).

    ``row``: a 1-D float32 device row of a plane, ``dm`` its DM, ``dt`` its
    sample time, ``bank`` a [Nt, 5] array of orbits.  The templates are taken
    in batches sized like ``PeriodicitySearch.row_batch``; each batch is
    resampled (``mode``, one knot spacing for the whole bank, fill: the row's
    mean) and handed to ``PeriodicitySearch.__call__`` unchanged, the templates
    playing the part of DM rows.  ``flo`` .. ``fhi``: the searched band in Hz
    (candidates above ``fhi`` are dropped on the host; None: no upper edge).
    ``ps``: the ``PeriodicitySearch`` to use (default: one made from
    ``sigma_threshold``, ``harms`` and ``flo``)."""

    def __init__(self, sigma_threshold=6.0, harms=_per.DEFAULT_HARMS, mode="nearest", flo=1.0,
                 fhi=None, max_cands=1 << 20, ps=None):
        self.ps = ps if ps is not None else _per.PeriodicitySearch(
            sigma_threshold, harms, flo=flo, max_cands=max_cands)
        self.resampler = Resampler(mode)
        self.fhi = None if fhi is None else float(fhi)

    def __call__(self, row, dm, dt, bank, nfft=None, row_batch=None, plane_row=0):
        bank = validate(bank)
        n = int(row.shape[0])
        nfft = self.ps.default_nfft(n) if nfft is None else int(nfft)
        step = self.ps.row_batch(nfft) if row_batch is None else int(row_batch)
        assert step >= 1
        K = knot_spacing(bank, dt)
        fill = float(row.double().mean().item()) if n else 0.0
        parts = []
        for a in range(0, len(bank), step):
            part = bank[a:a + step]
            plane = self.resampler(row, part, dt, fill=fill, K=K)
            c = self.ps(plane, np.full(len(part), float(dm)), dt, nfft=nfft)
            del plane
            if self.fhi is not None:
                c = c[c["freq"] <= self.fhi]
            parts.append(to_records(c, bank, a, plane_row))
        return merge(parts)


def to_records(cands, bank, template0=0, plane_row=0):
    """Periodicity records of a resampled batch whose row 0 is template
    ``template0`` of ``bank`` -> ORBCAND_DTYPE records (``row``: the plane row
    the time series came from)."""
    out = np.empty(len(cands), dtype=ORBCAND_DTYPE)
    for name in _per.CAND_DTYPE.names:
        out[name] = cands[name]
    out["template"] = cands["row"].astype(np.int64) + int(template0)
    out["row"] = int(plane_row)
    for k, name in enumerate(_ELEMENTS):
        out[name] = np.asarray(bank)[out["template"], k] if len(out) else []
    return out


def merge(parts):
    """Concatenate candidate arrays of several batches, sorted by (template,
    numharm, r)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=ORBCAND_DTYPE)
    return np.sort(np.concatenate(parts), order=_ORDER)


# ---- sifting and .orbcands files (host) ----

def sift(cands, ntemplates=0, rtol_bins=1.5, max_ratio=16):
    """Group candidate records across templates and harmonics: in order of
    descending sigma a candidate is absorbed into the first stronger one whose
    ``r`` it matches within ``rtol_bins``, or in an integer ratio up to
    ``max_ratio`` within ``rtol_bins`` (the rule of ``periodicity.sift``).
    The kept ones gain ``ntemplates`` (how many were searched) and ``nhits``
    (members, itself included).  Returns SIFTED_DTYPE records by descending
    sigma."""
    cands = np.asarray(cands)
    order = np.argsort(-cands["sigma"], kind="stable")
    kept, hits, kept_r = [], [], np.empty(0)
    m = np.arange(1, int(max_ratio) + 1, dtype=np.float64)
    for i in order:
        r = float(cands["r"][i])
        j = -1
        if kept:
            big, small = np.maximum(kept_r, r), np.minimum(kept_r, r)
            hit = np.flatnonzero(np.any(np.abs(big[:, None] - m[None, :] * small[:, None])
                                        <= rtol_bins, axis=1))
            if len(hit):
                j = int(hit[0])
        if j < 0:
            kept.append(i)
            hits.append(1)
            kept_r = np.append(kept_r, r)
        else:
            hits[j] += 1
    out = np.empty(len(kept), dtype=SIFTED_DTYPE)
    for name in ORBCAND_DTYPE.names:
        out[name] = cands[name][kept] if len(kept) else []
    out["ntemplates"] = int(ntemplates)
    out["nhits"] = hits
    return out


ORBCANDS_HEADER = "# " + " ".join(ORBCANDS_COLUMNS) + \
    "   (freq in Hz, period, pb and t0 in s, x in light-seconds, omega in rad)\n"


def _sorted(sifted):
    s = np.asarray(sifted)
    return s[np.argsort(-s["sigma"], kind="stable")]


def write_orbcands(sifted, fn):
    """Write sifted candidates as ``<base>.orbcands``: one line each, by
    descending sigma, of the ORBCANDS_COLUMNS -- every number in its shortest
    exact form, so ``read_orbcands`` returns what was written."""
    with open(fn, "w") as f:
        f.write(ORBCANDS_HEADER)
        for c in _sorted(sifted):
            f.write(" ".join(repr(c[n].item()) if SIFTED_DTYPE[n] == np.dtype("f8") else str(c[n])
                             for n in ORBCANDS_COLUMNS) + "\n")


def read_orbcands(fn):
    """Inverse of write_orbcands: records with the ORBCANDS_COLUMNS."""
    dtype = np.dtype([(n, SIFTED_DTYPE[n]) for n in ORBCANDS_COLUMNS])
    rows = []
    for line in open(fn):
        t = line.partition("#")[0].split()
        if t:
            assert len(t) == len(ORBCANDS_COLUMNS), "%s: bad line %r" % (fn, line)
            rows.append(tuple(t))
    out = np.empty(len(rows), dtype=dtype)
    for i, n in enumerate(ORBCANDS_COLUMNS):
        out[n] = [np.dtype(dtype[n]).type(r[i]) for r in rows] if rows else []
    return out


def write_orbcands_npz(sifted, fn):
    """``<base>_orbcands.npz``: the columns of the ``.orbcands`` file, by
    descending sigma."""
    s = _sorted(sifted)
    np.savez(fn, **{n: np.asarray(s[n], dtype=SIFTED_DTYPE[n]) for n in ORBCANDS_COLUMNS})
