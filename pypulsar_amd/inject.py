"""Synthetic pulsars and bursts added to raw time-major blocks on the device
(pdd_inject, csrc/pdd_inject.hip; restated in
tests/inject_oracle.py).

The reference has no injector: the definition is this project's own.

The injected value of a cell is a pure function of (absolute sample i,
channel c), so a file injected whole, block by block with overlaps, or from a
resumed run holds the same bytes.

Signal model (host, float64 and exact rationals)
------------------------------------------------
Times are seconds from file sample 0; sample i covers [i dt, (i + 1) dt) and
is evaluated at its centre.  ``t``, ``phi0`` and ``f`` refer to arrival at the
highest channel frequency; channel c lags by ``delta_c = delay_from_DM(dm,
f_c) - delay_from_DM(dm, max f)`` (float64, never rounded to bins).  ``width``
is the FWHM (turns for a pulsar, seconds for a burst); ``amp`` the intrinsic
peak in data units at ``ref_freq`` (default: the band centre); channel c is
scaled by ``(f_c / ref_freq)^spectral_index``.

Per job j and channel c a profile table ``T[j][c][0..B-1]`` (float32 cast of
float64), B a power of two in 64..4096, is the inverse real DFT of the
product of

* the intrinsic profile's Fourier coefficient (Gaussian of unit peak:
  ``sigma sqrt(2 pi) exp(-2 pi^2 sigma^2 k^2)``, sigma = width / (2 sqrt(2 ln
  2)); a tabulated profile: its DFT, peak scaled to 1),
* ``sinc(k s_c)``, ``s_c = dm_smear(dm, |foff|, f_c)``: the intra-channel smear,
* ``sinc(k dt)``: the integration over a sample,
* ``1 / (1 + 2 pi i k tau_c)``, ``tau_c = tau (f_c / ref_freq)^tau_index``: a
  one-sided exponential,

all lengths in turns (np.sinc: sin(pi x) / (pi x)).  ``T[b]`` is the
sample-integrated profile at phase b / B.  A pulsar's turn is its period 1 / f;
a burst's "turn" is a window of W seconds that the host places around the
burst so that what falls outside is below 1e-6 of the table's peak, and the
burst only touches the samples ``[lo_c, hi_c)`` of a channel in which the
phase stays inside [0, 1).  A pulsar touches the samples [start, stop).

Phase of job j at absolute sample i in channel c: ``Phi(t) = phi0 + f t + fd
t^2 / 2 + fdd t^3 / 6`` at ``t = (i + 1/2) dt - delta_c``, expanded as ``k0_c +
k1_c i + k2_c i^2 + k3 i^3`` in exact rationals of the float arguments;
``P0_c = round(k0_c 2^64) mod 2^64``, ``step_c = round(k1_c 2^64) mod 2^64``,
k2_c and k3 rounded to float64.  ``phase = P0_c + i step_c`` (wrapping uint64)
``+ U(x x (k2_c + x k3))``, ``x = (double) i``, ``U(d) = (uint64)((d -
floor(d)) 2^64)`` (a difference that rounds to 1.0 counts as 0), every
operation one IEEE operation in this order.

Orbits.  A pulsar may carry a Keplerian orbit ``(pb, x, e, omega, t0)``: the
elements, units and Roemer delay ``D(t)`` of ``pypulsar_amd.orbit`` and of
pdd_orbit_resample (include/pdd.h); ``orbit.validate`` is applied (``beta = x
(2 pi / pb) / (1 - e) <= 0.1``).  Its phase is

    Phi(t) = phi0 + f t + fd t^2 / 2 + fdd t^3 / 6 - f (D(t) - D(0)),

the cubic evaluated at the pulsar time ``t - (D(t) - D(0))`` with the cross
terms of ``fd`` and ``fdd`` with ``D`` dropped (``fd D`` is at most ``fd x``
turns).  With ``fd = fdd = 0`` this is exactly the map pdd_orbit_resample
inverts (``p_0 = 0``): a row injected with an orbit and demodulated with the
same orbit is the orbit-free pulsar.  ``Q(psi) = f (D(t0 + psi pb) - D(0))``,
in turns, is periodic in the orbital phase ``psi = (t - t0) / pb``, so one
orbit is tabulated -- ``qtab[k] = Q(k / M)``, k = 0..M, ``qtab[M] = qtab[0]``,
``M = 2^m`` -- and psi is carried like the spin phase: ``O0_c = round(((dt / 2
- delta_c - t0) / pb) 2^64) mod 2^64`` per channel and ``ostep = round((dt /
pb) 2^64) mod 2^64`` per job, each rounded once from the exact rationals of
the float arguments.  Per cell ``psi = O0_c + i ostep`` (wrapping), ``k = psi
>> (64 - m)``, ``w = (double)((psi >> (32 - m)) & 0xffffffff) 2^-32`` (exact),
``q = qtab[k] + (qtab[k + 1] - qtab[k]) w`` (float64, one IEEE operation each)
and ``U(q)`` is taken off the phase.  ``m`` is the smallest of 6..22 with ``A /
(8 M^2) <= 1e-6`` turns, ``A = f x (2 pi)^2 / (1 - e)^3`` a bound on ``|d2Q /
dpsi2|`` (the analytic bound, not the table's own second differences): the
linear interpolation stays within 1e-3 of a bin of the default 1024-bin
table.  An orbit that would need ``m > 22`` is refused.  Bursts take no orbit.

Lookup: ``b = phase >> (64 - log2 B)``, ``wgt = float32((phase >> (40 - log2
B)) & 0xffffff) 2^-24``, ``v_j = T[b] + (T[b + 1] - T[b]) wgt`` in float32,
``T[B]`` being ``T[0]`` for a pulsar and 0 for a burst.  The values of the
jobs that cover the cell are summed in float32 in job order into ``acc``.

float32 blocks become ``x + acc``; 8-bit blocks ``min(vmax, max(0,
floor((float(x) + acc) + u)))`` with the dither ``u = float32(h >> 8) 2^-24``,
``h = fmix(fmix(fmix(lo ^ seed) ^ hi ^ 0x9e3779b9) ^ (c 0x27d4eb2f))`` over the
32-bit halves (lo, hi) of the absolute sample index (fmix: MurmurHash3's
32-bit finaliser).  A cell no job covers keeps its value.
"""
import json
import math
from fractions import Fraction

import numpy as np

from . import delays

_M64 = 1 << 64
MAX_JOBS = 64
NBINS_MIN, NBINS_MAX = 64, 4096
GROUP = 256          # channels of one envelope entry of the device `range` array
RANGE_MAX = 1 << 62  # "everything": the default stop of a pulsar
FWHM_TO_SIGMA = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))
_ORBIT_KEYS = ("pb", "x", "e", "omega", "t0")
_PULSAR_KEYS = ("f", "dm", "amp", "fd", "fdd", "phi0", "width", "profile", "spectral_index",
                "tau", "tau_index", "ref_freq", "start", "stop") + _ORBIT_KEYS
ORBIT_MIN_M, ORBIT_MAX_M = 6, 22  # log2 of the knots of an orbit's table (include/pdd.h)
ORBIT_BUDGET = 1e-6               # turns: the interpolation error of the orbital term


def orbit_table_bits(f, x, e):
    """The smallest ``m`` in 6..22 with ``f x (2 pi)^2 / (1 - e)^3 / (8 (2^m)^2)
    <= 1e-6`` turns; ValueError when 22 does not do."""
    A = float(f) * float(x) * (2.0 * math.pi) ** 2 / (1.0 - float(e)) ** 3
    for m in range(ORBIT_MIN_M, ORBIT_MAX_M + 1):
        if A / (8.0 * float(1 << m) ** 2) <= ORBIT_BUDGET:
            return m
    raise ValueError("orbit: f = %r Hz, x = %r lt-s, e = %r need a table of more than 2^%d knots "
                     "for %g turns" % (float(f), float(x), float(e), ORBIT_MAX_M, ORBIT_BUDGET))


def orbit_table(f, orb, m):
    """float64 [2^m + 1]: ``f (D(t0 + k pb / M) - D(0))`` in turns, k = 0..M,
    the last knot repeating the first.  ``orb``: (pb, x, e, omega, t0)."""
    from . import orbit as _orbit  # (imports torch: only signals with an orbit need it)
    M = 1 << int(m)
    pb, t0 = float(orb[0]), float(orb[4])
    t = t0 + np.arange(M, dtype=np.float64) * (pb / M)
    D = _orbit.roemer(tuple(orb), np.concatenate([t, [0.0]]))
    q = np.empty(M + 1, dtype=np.float64)
    q[:M] = float(f) * (D[:M] - D[M])
    q[M] = q[0]
    return q
_BURST_KEYS = ("t", "dm", "amp", "width", "spectral_index", "tau", "tau_index", "ref_freq")


class PulsarSignal(object):
    """A periodic signal: frequency ``f`` (Hz) and derivatives ``fd``, ``fdd``
    at t = 0, phase ``phi0`` (turns) at t = 0, ``width`` the FWHM in turns of a
    Gaussian ``profile`` (or ``profile`` a 1-D array: one period, any length),
    present in the samples [start, stop).  ``pb`` (s) and ``x`` (light
    seconds) together put it into a Keplerian orbit of eccentricity ``e``,
    longitude of periastron ``omega`` (rad) and time of periastron ``t0`` (s
    after sample 0; ``e = 0``: the ascending node), the elements of
    ``pypulsar_amd.orbit``: the phase loses ``f (D(t) - D(0))`` turns (the
    module docstring; the cross term ``fd D``, at most ``fd x`` turns, is
    dropped)."""
    kind = "pulsar"

    def __init__(self, f, dm, amp, fd=0.0, fdd=0.0, phi0=0.0, width=0.05, profile="gauss",
                 spectral_index=0.0, tau=0.0, tau_index=-4.0, ref_freq=None, start=None, stop=None,
                 pb=None, x=None, e=None, omega=None, t0=None):
        self.f, self.dm, self.amp = float(f), float(dm), float(amp)
        self.fd, self.fdd, self.phi0 = float(fd), float(fdd), float(phi0)
        self.width = float(width)
        if isinstance(profile, str):
            if profile != "gauss":
                raise ValueError("profile must be 'gauss' or a 1-D array, got %r" % (profile,))
            self.profile = profile
        else:
            self.profile = np.asarray(profile, dtype=np.float64)
            if self.profile.ndim != 1 or self.profile.size < 2 or not self.profile.max() > 0:
                raise ValueError("a tabulated profile is a 1-D array with a positive peak")
        self.spectral_index, self.tau, self.tau_index = float(spectral_index), float(tau), float(tau_index)
        self.ref_freq = None if ref_freq is None else float(ref_freq)
        self.start = 0 if start is None else int(start)
        self.stop = RANGE_MAX if stop is None else int(stop)
        if not self.f > 0:
            raise ValueError("a pulsar needs f > 0")
        if isinstance(self.profile, str) and not self.width > 0:
            raise ValueError("width must be positive")
        if self.tau < 0 or not 0 <= self.start <= self.stop <= RANGE_MAX:
            raise ValueError("tau >= 0 and 0 <= start <= stop are required")
        self.orbit, self.m, self.qtab = None, -1, None
        if (pb is None) != (x is None):
            raise ValueError("an orbit needs pb and x together")
        if pb is None:
            if not (e is None and omega is None and t0 is None):
                raise ValueError("e, omega and t0 need an orbit (pb and x)")
            return
        from . import orbit as _orbit  # (imports torch: only signals with an orbit need it)
        orb = tuple(0.0 if v is None else float(v) for v in (pb, x, e, omega, t0))
        _orbit.validate(orb)
        self.orbit = _orbit.Orbit(*orb)
        self.m = orbit_table_bits(self.f, self.orbit.x, self.orbit.e)
        self.qtab = orbit_table(self.f, self.orbit, self.m)
        self.beta = float(_orbit.beta(orb)[0])
        # max |dD/dt| from the table's own differences: the apparent frequency
        # stays inside [f_lo, f_hi]
        v = float(np.max(np.abs(np.diff(self.qtab)))) * (1 << self.m) / (self.f * self.orbit.pb)
        self.f_lo, self.f_hi = self.f * (1.0 - v), self.f * (1.0 + v)

    def params(self):
        d = self._params()
        if self.orbit is not None:
            d.update(self.orbit._asdict())
            d.update(beta=self.beta, f_lo=self.f_lo, f_hi=self.f_hi)
        return d

    def _params(self):
        d = dict(kind="pulsar", f=self.f, dm=self.dm, amp=self.amp, fd=self.fd, fdd=self.fdd,
                 phi0=self.phi0, width=self.width, spectral_index=self.spectral_index,
                 tau=self.tau, tau_index=self.tau_index, ref_freq=self.ref_freq,
                 start=self.start, stop=None if self.stop == RANGE_MAX else self.stop)
        d["profile"] = self.profile if isinstance(self.profile, str) else self.profile.tolist()
        return d


class BurstSignal(object):
    """A single dispersed pulse arriving at ``t`` seconds (at the highest
    channel frequency), Gaussian of FWHM ``width`` seconds."""
    kind = "burst"

    def __init__(self, t, dm, amp, width, spectral_index=0.0, tau=0.0, tau_index=-4.0,
                 ref_freq=None):
        self.t, self.dm, self.amp, self.width = float(t), float(dm), float(amp), float(width)
        self.spectral_index, self.tau, self.tau_index = float(spectral_index), float(tau), float(tau_index)
        self.ref_freq = None if ref_freq is None else float(ref_freq)
        if not self.width > 0 or self.tau < 0:
            raise ValueError("a burst needs width > 0 and tau >= 0")

    def params(self):
        return dict(kind="burst", t=self.t, dm=self.dm, amp=self.amp, width=self.width,
                    spectral_index=self.spectral_index, tau=self.tau, tau_index=self.tau_index,
                    ref_freq=self.ref_freq)


def channel_lags(dm, freqs):
    """delta_c (float64 seconds): the lag of every channel behind the highest
    channel frequency, the reference of delays.sweep_table."""
    freqs = np.asarray(freqs, dtype=np.float64)
    return delays.delay_from_DM(dm, freqs) - delays.delay_from_DM(dm, np.max(freqs))


def phase_coefficients(f, fd, fdd, phi0, dt, delta):
    """(P0, step, k2, k3) of ``Phi((i + 1/2) dt - delta)`` as a cubic in i:
    P0 and step Python ints in [0, 2^64) (each rounded once from the exact
    rational value of the float arguments), k2 and k3 floats."""
    f, fd, fdd, phi0, dt, delta = (Fraction(float(v)) for v in (f, fd, fdd, phi0, dt, delta))
    a = dt / 2 - delta
    k0 = phi0 + f * a + fd * a * a / 2 + fdd * a * a * a / 6
    k1 = dt * (f + fd * a + fdd * a * a / 2)
    k2 = dt * dt * (fd + fdd * a) / 2
    k3 = fdd * dt * dt * dt / 6
    return round(k0 * _M64) % _M64, round(k1 * _M64) % _M64, float(k2), float(k3)


def burst_window(width, smear_max, dt, tau_max):
    """(W, lead) seconds: the window of a burst's table and the distance of
    the burst's arrival behind the window's start.  The Gaussian is cut 7
    sigma out (e^-24.5), widened by half the two boxcars; the exponential
    e^-16 behind that."""
    half = 7.0 * width * FWHM_TO_SIGMA + 0.5 * (smear_max + dt)
    return 2.0 * half + 16.0 * tau_max, half


def intrinsic_coefficients(profile, width, K):
    """Fourier coefficients c_0..c_K of the unit-peak intrinsic profile,
    ``p(phi) = sum_k c_k e^{2 pi i k phi}``; lengths in turns."""
    k = np.arange(K + 1, dtype=np.float64)
    if isinstance(profile, str):
        sigma = width * FWHM_TO_SIGMA
        return (sigma * math.sqrt(2.0 * math.pi) * np.exp(-2.0 * math.pi ** 2 * sigma ** 2 * k * k)
                ).astype(np.complex128)
    p = np.asarray(profile, dtype=np.float64) / np.max(profile)
    spec = np.fft.rfft(p) / p.size
    out = np.zeros(K + 1, dtype=np.complex128)
    m = min(K + 1, spec.size)
    out[:m] = spec[:m]
    return out


def profile_tables(intrinsic, scale, smear, dt_turns, tau, shift, B):
    """float64 [C, B]: per channel the inverse DFT of ``scale_c intrinsic_k
    sinc(k smear_c) sinc(k dt) / (1 + 2 pi i k tau_c) e^{-2 pi i k shift}``
    (all lengths in turns), k = 0..B/2."""
    K = B // 2
    k = np.arange(K + 1, dtype=np.float64)
    coef = (np.asarray(scale, dtype=np.float64)[:, None] * intrinsic[None, :]
            * np.sinc(k[None, :] * np.asarray(smear, dtype=np.float64)[:, None])
            * np.sinc(k * dt_turns)[None, :]
            / (1.0 + 2j * math.pi * k[None, :] * np.asarray(tau, dtype=np.float64)[:, None])
            * np.exp(-2j * math.pi * k * shift)[None, :])
    return np.fft.irfft(coef * B, n=B, axis=1)


class _Job(object):
    __slots__ = ("signal", "tables", "P0", "step", "k2", "k3", "lo", "hi", "window", "lead", "scale",
                 "O0", "ostep")


class Injector(object):
    """``Injector(signals, freqs, dt).apply(block, t0)`` adds the signals, in
    place, to a time-major device block [n, C] (8-bit or float32) whose first
    row is absolute sample ``t0``.  Everything but ``apply`` runs on the host
    (no GPU needed)."""

    def __init__(self, signals, freqs, dt, nbins=1024, seed=0, vmax=255):
        self.freqs = np.asarray(freqs, dtype=np.float64).reshape(-1).copy()
        self.C = self.freqs.size
        self.dt = float(dt)
        self.B = int(nbins)
        if self.B < NBINS_MIN or self.B > NBINS_MAX or self.B & (self.B - 1):
            raise ValueError("nbins must be a power of two in %d..%d" % (NBINS_MIN, NBINS_MAX))
        self.seed = int(seed)
        if not 0 <= self.seed < (1 << 32):
            raise ValueError("seed must fit 32 bits")
        self.vmax = int(vmax)
        if not 1 <= self.vmax <= 255:
            raise ValueError("vmax must be in 1..255")
        self.signals = list(signals)
        if len(self.signals) > MAX_JOBS:
            raise ValueError("at most %d signals per injector" % MAX_JOBS)
        if self.C < 1 or not self.dt > 0 or not np.all(self.freqs > 0):
            raise ValueError("freqs must be positive and dt > 0")
        self.foff = abs(self.freqs[1] - self.freqs[0]) if self.C > 1 else 0.0
        self.sigma_chan, self.n_samples = None, None
        self.jobs = [self._build(s) for s in self.signals]
        self._dev = {}

    # ---- host model
    def _ref_freq(self, s):
        return 0.5 * (self.freqs.max() + self.freqs.min()) if s.ref_freq is None else s.ref_freq

    def _build(self, s):
        job = _Job()
        job.signal = s
        C, B, dt = self.C, self.B, self.dt
        ref = self._ref_freq(s)
        delta = channel_lags(s.dm, self.freqs)
        job.scale = s.amp * (self.freqs / ref) ** s.spectral_index
        smear = np.abs(delays.dm_smear(s.dm, self.foff, self.freqs))
        tau = s.tau * (self.freqs / ref) ** s.tau_index
        job.P0 = np.zeros(C, dtype=np.uint64)
        job.step = np.zeros(C, dtype=np.uint64)
        job.k2 = np.zeros(C, dtype=np.float64)
        job.k3 = 0.0
        job.O0, job.ostep = np.zeros(C, dtype=np.uint64), 0
        if s.kind == "pulsar":
            job.window, job.lead = 1.0 / s.f, 0.0
            turn = s.f  # turns per second
            intr = intrinsic_coefficients(s.profile, s.width, B // 2)
            job.tables = profile_tables(intr, job.scale, smear * turn, dt * turn, tau * turn, 0.0, B)
            for c in range(C):
                P0, step, k2, job.k3 = phase_coefficients(s.f, s.fd, s.fdd, s.phi0, dt, delta[c])
                job.P0[c], job.step[c], job.k2[c] = P0, step, k2
            job.lo = np.full(C, s.start, dtype=np.int64)
            job.hi = np.full(C, s.stop, dtype=np.int64)
            if s.orbit is not None:
                dtf, pbf, t0f = Fraction(dt), Fraction(s.orbit.pb), Fraction(s.orbit.t0)
                job.ostep = round(dtf / pbf * _M64) % _M64
                for c in range(C):
                    job.O0[c] = round((dtf / 2 - Fraction(float(delta[c])) - t0f) / pbf * _M64) % _M64
            return job
        W, lead = burst_window(s.width, float(smear.max()), dt, float(tau.max()))
        job.window, job.lead = W, lead
        intr = intrinsic_coefficients("gauss", s.width / W, B // 2)
        job.tables = profile_tables(intr, job.scale, smear / W, dt / W, tau / W, lead / W, B)
        job.lo = np.zeros(C, dtype=np.int64)
        job.hi = np.zeros(C, dtype=np.int64)
        Wf, dtf = Fraction(W), Fraction(dt)
        k1 = dtf / Wf
        step = round(k1 * _M64) % _M64
        for c in range(C):
            # phase = (t_i - delta_c - (t - lead)) / W
            k0 = (dtf / 2 - Fraction(float(delta[c])) - (Fraction(s.t) - Fraction(lead))) / Wf
            P0 = round(k0 * _M64) % _M64
            lo = max(0, math.ceil(-k0 / k1))
            hi = max(lo, math.ceil((1 - k0) / k1))
            # the rounded integer phase must agree at both ends (no wrap)
            while lo < hi and (P0 + lo * step) % _M64 >= (1 << 63):
                lo += 1
            while hi > lo and (P0 + (hi - 1) * step) % _M64 < (1 << 63):
                hi -= 1
            job.P0[c], job.step[c], job.lo[c], job.hi[c] = P0, step, lo, min(hi, RANGE_MAX)
        return job

    @property
    def tables(self):
        """float32 [J, C, B] profile tables."""
        if not self.jobs:
            return np.zeros((0, self.C, self.B), dtype=np.float32)
        return np.stack([j.tables.astype(np.float32) for j in self.jobs])

    def host_arrays(self):
        """The job tables in the layouts pdd_inject takes (include/pdd.h):
        phase uint64 [J, C, 2] (P0, step); drift float64 [J, C, 2] (k2, k3);
        range int64 [J, C + G, 2] (lo, hi; the G = ceil(C / 256) trailing
        entries are the envelopes of 256 channels); tables float32 [J, C, B +
        1] (entry B: T[0] of a pulsar, 0 of a burst)."""
        J, C, B = len(self.jobs), self.C, self.B
        G = -(-C // GROUP)
        phase = np.zeros((J, C, 2), dtype=np.uint64)
        drift = np.zeros((J, C, 2), dtype=np.float64)
        rng = np.zeros((J, C + G, 2), dtype=np.int64)
        tab = np.zeros((J, C, B + 1), dtype=np.float32)
        for j, job in enumerate(self.jobs):
            phase[j, :, 0], phase[j, :, 1] = job.P0, job.step
            drift[j, :, 0], drift[j, :, 1] = job.k2, job.k3
            rng[j, :C, 0], rng[j, :C, 1] = job.lo, job.hi
            for g in range(G):
                lo, hi = job.lo[g * GROUP:(g + 1) * GROUP], job.hi[g * GROUP:(g + 1) * GROUP]
                ok = hi > lo
                rng[j, C + g] = (lo[ok].min(), hi[ok].max()) if ok.any() else (0, 0)
            tab[j, :, :B] = job.tables.astype(np.float32)
            if job.signal.kind == "pulsar":
                tab[j, :, B] = tab[j, :, 0]
        return phase, drift, rng, tab

    def has_orbits(self):
        return any(getattr(j.signal, "orbit", None) is not None for j in self.jobs)

    def orbit_arrays(self):
        """The orbit tables in the layouts pdd_inject_orbit takes
        (include/pdd.h): ophase uint64 [J, C] (O0; 0 for a job without an
        orbit); ometa int64 [J, 3] (m, or -1: no orbit; ostep, the uint64's
        bits; the byte offset of the job's table in qtab); qtab float64, the
        tables of the jobs with an orbit one after the other (``2^m + 1``
        knots each; empty when no job has an orbit)."""
        J, C = len(self.jobs), self.C
        ophase = np.zeros((J, C), dtype=np.uint64)
        ometa = np.zeros((J, 3), dtype=np.int64)
        ometa[:, 0] = -1
        tabs, at = [], 0
        for j, job in enumerate(self.jobs):
            s = job.signal
            if getattr(s, "orbit", None) is None:
                continue
            ophase[j] = job.O0
            ometa[j] = (s.m, np.array(job.ostep, dtype=np.uint64).view(np.int64), 8 * at)
            tabs.append(s.qtab)
            at += s.qtab.size
        qtab = np.concatenate(tabs) if tabs else np.zeros(0, dtype=np.float64)
        return ophase, ometa, qtab

    def _sigma_sum(self, sigma_chan):
        s = np.broadcast_to(np.asarray(sigma_chan, dtype=np.float64), (self.C,))
        return math.sqrt(float(np.sum(s * s)))

    def matched_snr(self, sigma_chan, n_samples):
        """Per signal, the S/N a matched filter recovers from noise of
        standard deviation ``sigma_chan`` (scalar or [C]) per channel sample:
        with E the aligned channel sum of the float64 tables, sqrt(n
        var_phi(E)) / sqrt(sum sigma_c^2) for a pulsar over n = the samples
        of [start, stop) within ``n_samples``, sqrt((W / dt) mean_phi(E^2)) /
        sqrt(sum sigma_c^2) for a burst.  An orbit does not enter: it changes
        the number of samples per turn by at most beta <= 0.1 (in practice
        below 0.02) and not the energy per turn, so the figure is the
        orbit-free pulsar's, good to that fraction."""
        noise = self._sigma_sum(sigma_chan)
        if not noise > 0:
            raise ValueError("a matched S/N needs a noise level: sigma_chan is 0 in every channel "
                             "(1.4826 MAD of coarsely quantised data can be); give amp, not snr")
        out = []
        for job in self.jobs:
            E = job.tables.sum(axis=0)
            if job.signal.kind == "pulsar":
                n = max(0, min(int(n_samples), job.signal.stop) - job.signal.start)
                out.append(math.sqrt(n * float(np.var(E))) / noise)
            else:
                out.append(math.sqrt(job.window / self.dt * float(np.mean(E * E))) / noise)
        return out

    def truth(self, sigma_chan=None, n_samples=None):
        """One dict per signal: its parameters, ``matched_snr`` (None without
        a noise level) and ``sample``: the arrival at the highest channel
        frequency in samples (a pulsar: of its first pulse at or after t =
        0)."""
        sigma_chan = self.sigma_chan if sigma_chan is None else sigma_chan
        n_samples = self.n_samples if n_samples is None else n_samples
        known = (sigma_chan is not None and n_samples is not None
                 and self._sigma_sum(sigma_chan) > 0)
        snr = self.matched_snr(sigma_chan, n_samples) if known else [None] * len(self.jobs)
        out = []
        for job, m in zip(self.jobs, snr):
            s = job.signal
            d = s.params()
            d["matched_snr"] = m
            t = s.t if s.kind == "burst" else ((-s.phi0) % 1.0) / s.f
            d["sample"] = t / self.dt
            out.append(d)
        return out

    @classmethod
    def from_spec(cls, spec, freqs, dt, sigma_chan=None, n_samples=None, **kw):
        """An Injector from a JSON file (or its parsed list / {"signals": [...],
        nbins, seed} dict).  Every signal is a dict with ``kind`` ("pulsar" or
        "burst"; default: "burst" when it has ``t``) and the constructor's
        arguments, the strength as ``amp`` or as ``snr``: the matched S/N
        (needs ``sigma_chan``, for a pulsar ``n_samples`` too)."""
        if isinstance(spec, str):
            with open(spec) as f:
                spec = json.load(f)
        if isinstance(spec, dict):
            for key in ("nbins", "seed", "vmax"):
                if key in spec:
                    kw.setdefault(key, spec[key])
            spec = spec.get("signals")
        if not isinstance(spec, list):
            raise ValueError("an injection spec is a list of signals")
        signals, want = [], []
        for i, d in enumerate(spec):
            if not isinstance(d, dict):
                raise ValueError("signal %d is not an object" % i)
            d = dict(d)
            kind = d.pop("kind", "burst" if "t" in d else "pulsar")
            if kind not in ("pulsar", "burst"):
                raise ValueError("signal %d: unknown kind %r" % (i, kind))
            keys = _PULSAR_KEYS if kind == "pulsar" else _BURST_KEYS
            snr = d.pop("snr", None)
            if (snr is None) == ("amp" not in d):
                raise ValueError("signal %d needs exactly one of amp and snr" % i)
            bad = sorted(set(d) - set(keys))
            if bad:
                raise ValueError("signal %d (%s): unknown field(s) %s" % (i, kind, ", ".join(bad)))
            if snr is not None:
                if sigma_chan is None or (kind == "pulsar" and n_samples is None):
                    raise ValueError("signal %d gives snr: the noise level (sigma_chan, n_samples) "
                                     "is needed" % i)
                d["amp"] = 1.0
            try:
                signals.append(PulsarSignal(**d) if kind == "pulsar" else BurstSignal(**d))
            except TypeError as e:
                raise ValueError("signal %d (%s): %s" % (i, kind, e))
            want.append(snr)
        if any(w is not None for w in want):
            unit = cls(signals, freqs, dt, **kw).matched_snr(sigma_chan, n_samples or 0)
            for s, w, u in zip(signals, want, unit):
                if w is not None:
                    if not u > 0:
                        raise ValueError("a signal of zero matched S/N cannot be scaled")
                    s.amp = float(w) / u
        inj = cls(signals, freqs, dt, **kw)
        inj.sigma_chan, inj.n_samples = sigma_chan, n_samples
        return inj

    # ---- device
    def _device_arrays(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            phase, drift, rng, tab = self.host_arrays()
            self._dev[key] = (torch.from_numpy(phase.view(np.int64)).to(device),
                              torch.from_numpy(drift).to(device),
                              torch.from_numpy(rng).to(device),
                              torch.from_numpy(tab).to(device))
        return self._dev[key]

    def _device_orbit_arrays(self, device):
        """(ophase, qtab) on the device, ometa on the host."""
        import torch
        key = "orbit:" + str(device)
        if key not in self._dev:
            ophase, ometa, qtab = self.orbit_arrays()
            self._dev[key] = (torch.from_numpy(ophase.view(np.int64)).to(device),
                              np.ascontiguousarray(ometa), torch.from_numpy(qtab).to(device))
        return self._dev[key]

    def apply(self, block, t0=0, stream=None, vmax=None):
        """Add the signals, in place, to the time-major device block [n, C]
        (8-bit or float32) whose first row is sample ``t0``; returns the
        block.  ``vmax`` overrides the injector's 8-bit clip."""
        import torch
        from . import _lib
        from ._lib import call, ptr, stream_ptr
        codes = {torch.uint8: _lib.U8, torch.float32: _lib.F32}
        if block.dtype not in codes:
            raise TypeError("Injector.apply: 8-bit or float32 blocks only, got %s" % block.dtype)
        assert block.is_cuda and block.dim() == 2 and block.shape[1] == self.C
        assert block.stride(1) == 1 or block.shape[1] == 1
        n = block.shape[0]
        if n == 0 or not self.jobs:
            return block
        phase, drift, rng, tab = self._device_arrays(block.device)
        args = (ptr(block), codes[block.dtype], n, self.C, block.stride(0), int(t0),
                ptr(phase), ptr(drift), ptr(rng), ptr(tab), len(self.jobs), self.B, self.seed,
                self.vmax if vmax is None else int(vmax))
        if self.has_orbits():
            ophase, ometa, qtab = self._device_orbit_arrays(block.device)
            call("pdd_inject_orbit", *(args + (ptr(ophase), ometa.ctypes.data, ptr(qtab),
                                               qtab.numel(), stream_ptr(stream))))
        else:
            call("pdd_inject", *(args + (stream_ptr(stream),)))
        return block


def amp_for_snr(signal, snr, freqs, dt, sigma_chan, n_samples, nbins=1024):
    """The ``amp`` at which ``signal`` has matched S/N ``snr`` (matched_snr is
    linear in amp)."""
    keep = signal.amp
    signal.amp = 1.0
    try:
        unit = Injector([signal], freqs, dt, nbins=nbins).matched_snr(sigma_chan, n_samples)[0]
    finally:
        signal.amp = keep
    return float(snr) / unit


SIGMA_SPECTRA = 1 << 16  # spectra the command-line tools take the noise level from


def file_sigma(fb, nmax=SIGMA_SPECTRA):
    """``robust_sigma`` of the first min(N, nmax) spectra of an opened search
    file (SIGPROC of any supported bit depth, or PSRFITS)."""
    n = min(int(fb.number_of_samples), int(nmax))
    if hasattr(fb, "read_device"):
        head = fb.read_device(0, n).cpu().numpy()
    elif fb.packed:
        import torch
        from .stream import unpack_bits
        host = np.empty((n, fb.bytes_per_spectrum), dtype=np.uint8)
        n = fb.read_packed_into(0, host)
        head = unpack_bits(torch.from_numpy(host[:n]).cuda(), fb.nbits, fb.nchans).cpu().numpy()
    else:
        host = np.empty((n, fb.nchans), dtype=np.dtype(fb.dtype))
        n = fb.read_block_into(0, host)
        head = host[:n]
    return robust_sigma(head)


def injector_for_file(spec, fb, **kw):
    """The Injector of the JSON ``spec`` for an opened search file: ``snr``
    entries are scaled by the file's own noise level (file_sigma) and length."""
    return Injector.from_spec(spec, fb.freqs, fb.tsamp, sigma_chan=file_sigma(fb),
                              n_samples=int(fb.number_of_samples), **kw)


def robust_sigma(block):
    """1.4826 MAD per channel of a host block [n, C]: the noise level the
    command-line tools scale ``snr`` by."""
    x = np.asarray(block, dtype=np.float64)
    med = np.median(x, axis=0)
    return 1.4826 * np.median(np.abs(x - med[None, :]), axis=0)
