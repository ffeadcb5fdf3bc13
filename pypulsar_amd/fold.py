"""Folding of periodicity candidates on the DM-time plane and refinement of
their period, period derivative and DM.

The third consumer of the sweep's plane (after ``SinglePulseSearch`` and
``PeriodicitySearch``): the time series of every trial DM is on the device
already, so a candidate's row and its DM neighbours are folded there
(pdd_fold_rows), the folds are searched over period and period-derivative
offsets (pdd_fold_search) and only profiles come back.  The reference folds
on the host: ``Datfile.pulses`` (formats/datfile.py:231-275) cuts single
turns, ``Pulse.downsample_Nbins`` and ``SummedPulse.__iadd__``
(formats/pulse.py:197-215, 425-482) bin and sum them.  The arithmetic is
stated in include/pdd.h and restated in tests/fold_oracle.py.

Phase is a 64-bit unsigned fraction of a turn with wrap-around arithmetic, so
the bin of every sample is the same in Python integers, NumPy ``uint64`` and
on the GPU.  No CPU fallback.
"""
import ctypes
from fractions import Fraction

import numpy as np

MAX_BINS, MAX_PART, MAX_CELLS, MAX_TRIAL = 256, 128, 8192, 256
_M64 = 1 << 64


def phase_steps(f, fd, dt, phi0=0.0):
    """(P0, step, accel), Python ints in [0, 2^64), of a fold at frequency
    ``f`` (Hz), derivative ``fd`` (Hz/s), sample time ``dt`` and start phase
    ``phi0`` (turns): ``step = round(f dt 2^64)``, ``accel = round(fd dt dt
    2^64)`` (signed), ``P0 = round(phi0 2^64) + step // 2``, all mod 2^64 and
    each rounded once, from the exact rational value of the float arguments.
    Sample i has phase ``P0 + i step + (i (i - 1) // 2) accel`` (mod 2^64):
    the phase at the centre of the sample."""
    f, fd, dt, phi0 = (Fraction(float(v)) for v in (f, fd, dt, phi0))
    step = round(f * dt * _M64) % _M64
    accel = round(fd * dt * dt * _M64) % _M64
    return (round(phi0 * _M64) + step // 2) % _M64, step, accel


def trial_shift(ia, ib, p, npart):
    """Bins by which part ``p`` of ``npart`` is shifted in trial (ia, ib):
    the nearest bin to ``ia u + 4 ib u u``, ``u = (2 p + 1 - npart) / (2
    npart)``, as ``floor((ia m N + 2 ib m m + N N) / (2 N N))``."""
    N = int(npart)
    m = 2 * int(p) + 1 - N
    return (int(ia) * m * N + 2 * int(ib) * m * m + N * N) // (2 * N * N)


def trial_to_ffdot(ia, ib, f, fd, nbins, T):
    """(f', fd') of trial (ia, ib) of a fold at (f, fd) over ``T`` seconds
    (``T = npart L dt``): ``ia`` bins of linear and ``ib`` bins of quadratic
    drift of the PULSE across the span.  Part p is read ``s_p`` bins further
    on, so a positive trial follows a pulse that arrives later and later in
    the fold: a signal slower than the fold.  Hence
    ``fd' = fd - 8 ib / (nbins T^2)`` and, f' being the frequency at t = 0,
    ``f' = f - ia / (nbins T) + 4 ib / (nbins T)``."""
    T = float(T)
    return (f - ia / (nbins * T) + 4.0 * ib / (nbins * T), fd - 8.0 * ib / (nbins * T * T))


def align(prof, ia, ib):
    """[npart, nbins] sub-integrations rotated by the shifts of trial (ia, ib)
    (row p: ``out[p, b] = prof[p, (b + s_p) mod nbins]``)."""
    prof = np.asarray(prof)
    return np.stack([np.roll(prof[p], -trial_shift(ia, ib, p, prof.shape[0]))
                     for p in range(prof.shape[0])])


def chi2_sigma(chi2, nbins):
    """Equivalent Gaussian deviate of ``chi2 (nbins - 1) ~ chi-square(nbins -
    1)``; finite where the probability underflows."""
    from scipy.special import gammaln
    from scipy.stats import chi2 as chi2_dist
    from .periodicity import _sigma_of_logp
    c = np.asarray(chi2, dtype=np.float64)
    k = nbins - 1
    x2 = np.atleast_1d(c) * k
    logp = chi2_dist.logsf(x2, k)
    # where scipy's survival function has underflowed: the leading terms of
    # ln Q(a, x) = -x + (a - 1) ln x - ln Gamma(a) + ln(1 + (a-1)/x + (a-1)(a-2)/x^2 + ...)
    # (there x > a by far, and the positive terms j < a descend)
    low = ~(logp > -700.0) & (x2 > 0)
    if np.any(low):
        a, x = 0.5 * k, 0.5 * x2[low]
        s, term = np.ones_like(x), np.ones_like(x)
        for j in range(1, int(np.ceil(a))):
            term = term * (a - j) / x
            s = s + term
        logp[low] = -x + (a - 1.0) * np.log(x) - gammaln(a) + np.log(s)
    r = _sigma_of_logp(logp).reshape(c.shape)
    return float(r) if r.ndim == 0 else r


class FoldedCandidate(object):
    """One folded and refined candidate (all arrays on the host).

    ``dm``, ``row``: the best DM trial; ``f``, ``fd``, ``period``: refined
    frequency (at the first sample), derivative and period; ``f_fold``: the
    frequency it was folded at; ``trial``: the best (ia, ib); ``chi2``: its
    reduced chi-square; ``dms`` / ``rows`` / ``chi2_vs_dm``: the folded DM
    trials and the best chi-square of each; ``chi2_plane`` [2A+1, 2B+1] of
    the best row; ``subints`` [npart, nbins] aligned by the best trial's
    shifts, ``subint_counts`` likewise; ``profile`` / ``counts``: the summed
    profile and its sample counts; ``sigma``; ``data_avg`` / ``data_var`` /
    ``nsamp``: statistics of the folded samples; ``T``: the folded span (s)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "FoldedCandidate(DM=%.2f, P=%.9g s, fd=%.3g Hz/s, chi2=%.2f, sigma=%.1f)" % (
            self.dm, self.period, self.fd, self.chi2, self.sigma)


class Folder(object):
    """``Folder(npart=32, nbins=64)(plane, dms, dt, cands)`` -> FoldedCandidates.

    ``npart`` sub-integrations of ``nbins`` bins; the search covers
    ``ntrial_f`` bins of linear and ``ntrial_fd`` bins of quadratic drift on
    each side (default ``nbins`` each).  All device work is queued on torch's
    current stream."""

    def __init__(self, npart=32, nbins=64, ntrial_f=None, ntrial_fd=None):
        self.npart, self.nbins = int(npart), int(nbins)
        if not 2 <= self.nbins <= MAX_BINS:
            raise ValueError("nbins must be in 2..%d" % MAX_BINS)
        if not 1 <= self.npart <= MAX_PART:
            raise ValueError("npart must be in 1..%d" % MAX_PART)
        if self.npart * self.nbins > MAX_CELLS:
            raise ValueError("npart * nbins must not exceed %d" % MAX_CELLS)
        self.A = min(self.nbins, MAX_TRIAL) if ntrial_f is None else int(ntrial_f)
        self.B = min(self.nbins, MAX_TRIAL) if ntrial_fd is None else int(ntrial_fd)
        if not (0 <= self.A <= MAX_TRIAL and 0 <= self.B <= MAX_TRIAL):
            raise ValueError("ntrial_f and ntrial_fd must be in 0..%d" % MAX_TRIAL)

    def jobs(self, rows, f, fd=0.0, dt=None, phi0=0.0):
        """int64 [J, 4] {row, P0, step, accel} (the unsigned values' bits)."""
        if dt is None or not dt > 0:
            raise ValueError("dt (the plane's sample time) is required")
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        f, fd, phi0 = (np.broadcast_to(np.asarray(v, dtype=np.float64), rows.shape)
                       for v in (f, fd, phi0))
        out = np.empty((len(rows), 4), dtype=np.uint64)
        for j in range(len(rows)):
            for q, v in enumerate(phase_steps(f[j], fd[j], dt, phi0[j])):
                out[j, 1 + q] = np.uint64(v)
        out = out.view(np.int64)
        out[:, 0] = rows
        return out

    def span(self, n, dt):
        """Seconds folded of a row of n samples: npart (n // npart) dt."""
        return self.npart * (int(n) // self.npart) * float(dt)

    def fold(self, plane, rows, f, fd=0.0, dt=None, phi0=0.0):
        """Fold ``plane[rows[j]]`` at (f[j], fd[j], phi0[j]) (scalars
        broadcast).  Device tensors (prof float64 [J, npart, nbins], cnt int32
        [J, npart, nbins], sumsq float64 [J, npart]); does not synchronise."""
        import torch
        from . import _lib
        _lib.require_gpu()
        assert plane.is_cuda and plane.dtype == torch.float32 and plane.dim() == 2
        assert plane.stride(1) == 1
        D, n = plane.shape
        if n < self.npart:
            raise ValueError("rows of %d samples cannot be cut into %d parts" % (n, self.npart))
        jobs = self.jobs(rows, f, fd, dt, phi0)
        J = len(jobs)
        prof = torch.empty((J, self.npart, self.nbins), dtype=torch.float64, device=plane.device)
        cnt = torch.empty((J, self.npart, self.nbins), dtype=torch.int32, device=plane.device)
        sumsq = torch.empty((J, self.npart), dtype=torch.float64, device=plane.device)
        if J:
            # (the library checks the rows on the host copy before it launches)
            jd = torch.from_numpy(jobs).to(plane.device)
            _lib.call("pdd_fold_rows", _lib.ptr(plane), D, n, plane.stride(0),
                      jobs.ctypes.data_as(ctypes.c_void_p), _lib.ptr(jd), J, self.npart,
                      self.nbins, _lib.ptr(prof), _lib.ptr(cnt), _lib.ptr(sumsq),
                      _lib.stream_ptr())
        return prof, cnt, sumsq

    def search(self, prof, cnt, sumsq):
        """Search folds over the trials [-A, A] x [-B, B].  Device tensors
        (chi2 float64 [J, 2A+1, 2B+1], best int32 [J, 2] = (ia, ib),
        best_chi2 float64 [J], best_prof float64 [J, nbins], best_cnt int32
        [J, nbins]); does not synchronise."""
        import torch
        from . import _lib
        _lib.require_gpu()
        J = prof.shape[0]
        assert prof.is_cuda and prof.dtype == torch.float64 and prof.is_contiguous()
        assert cnt.dtype == torch.int32 and cnt.is_contiguous() and cnt.shape == prof.shape
        assert sumsq.dtype == torch.float64 and sumsq.is_contiguous()
        assert tuple(prof.shape[1:]) == (self.npart, self.nbins)
        assert tuple(sumsq.shape) == (J, self.npart)
        dev = prof.device
        chi2 = torch.empty((J, 2 * self.A + 1, 2 * self.B + 1), dtype=torch.float64, device=dev)
        best = torch.empty((J, 2), dtype=torch.int32, device=dev)
        best_chi2 = torch.empty((J,), dtype=torch.float64, device=dev)
        best_prof = torch.empty((J, self.nbins), dtype=torch.float64, device=dev)
        best_cnt = torch.empty((J, self.nbins), dtype=torch.int32, device=dev)
        if J:
            _lib.call("pdd_fold_search", _lib.ptr(prof), _lib.ptr(cnt), _lib.ptr(sumsq), J,
                      self.npart, self.nbins, self.A, self.B, _lib.ptr(chi2), _lib.ptr(best),
                      _lib.ptr(best_chi2), _lib.ptr(best_prof), _lib.ptr(best_cnt),
                      _lib.stream_ptr())
        return chi2, best, best_chi2, best_prof, best_cnt

    def __call__(self, plane, dms, dt, cands, dm_halfwidth=2):
        """Fold and refine candidates (``SiftedCandidate`` objects with their
        ``row`` set, or ``(row, freq)`` pairs): each is folded at its
        frequency on its own row and ``dm_halfwidth`` rows on each side
        (clipped at the plane's edges), all folds of the call in one
        pdd_fold_rows and one pdd_fold_search; the row with the largest best
        chi-square wins (ties: the candidate's own row).  A candidate that
        carries ``fd != 0`` (one of the acceleration search, whose frequency
        is the mid-observation one) is folded at ``(f - fd n dt / 2, fd)``,
        the frequency at the first sample, and refined from there; a pair
        may be a triple ``(row, freq, fd)``.  Returns a list of
        FoldedCandidate."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        h = int(dm_halfwidth)
        assert h >= 0
        want = []
        for c in cands:
            row, f = (int(c.row), float(c.freq)) if hasattr(c, "freq") else (int(c[0]), float(c[1]))
            fd = float(getattr(c, "fd", 0.0)) if hasattr(c, "freq") else \
                (float(c[2]) if len(c) > 2 else 0.0)
            if fd != 0.0:
                f = f - 0.5 * fd * n * float(dt)
            if row < 0 and hasattr(c, "dm") and D:
                # (a candidate read back from a .accelcands file: the nearest DM trial)
                row = int(np.argmin(np.abs(dms - float(c.dm))))
            if not 0 <= row < D:
                raise ValueError("candidate row %d outside the plane's %d rows" % (row, D))
            want.append((row, f, list(range(max(0, row - h), min(D, row + h + 1))), fd))
        if not want:
            return []
        rows = np.concatenate([w[2] for w in want])
        freqs = np.concatenate([[w[1]] * len(w[2]) for w in want])
        fds = np.concatenate([[w[3]] * len(w[2]) for w in want])
        prof, cnt, sumsq = self.fold(plane, rows, freqs, fds, dt)
        chi2, best, best_chi2, best_prof, best_cnt = self.search(prof, cnt, sumsq)
        best, best_chi2 = best.cpu().numpy(), best_chi2.cpu().numpy()
        T = self.span(n, dt)
        out, j0 = [], 0
        for row, f, rr, fd in want:
            cv = best_chi2[j0:j0 + len(rr)]
            k = rr.index(row)
            for q in range(len(rr)):
                if cv[q] > cv[k]:
                    k = q
            j = j0 + k
            ia, ib = int(best[j, 0]), int(best[j, 1])
            f1, fd1 = trial_to_ffdot(ia, ib, f, fd, self.nbins, T)
            pj, cj = prof[j].cpu().numpy(), cnt[j].cpu().numpy()
            nsamp = int(cj.astype(np.int64).sum())
            avg = float(pj.sum() / nsamp) if nsamp else 0.0
            var = float(sumsq[j].sum().item() / nsamp - avg * avg) if nsamp else 0.0
            out.append(FoldedCandidate(
                dm=float(dms[rr[k]]), row=int(rr[k]), f=f1, fd=fd1, period=1.0 / f1, f_fold=f,
                trial=(ia, ib), chi2=float(cv[k]), dms=dms[rr].copy(),
                rows=np.asarray(rr, dtype=np.int64), chi2_vs_dm=cv.copy(),
                chi2_plane=chi2[j].cpu().numpy(), subints=align(pj, ia, ib),
                subint_counts=align(cj, ia, ib), profile=best_prof[j].cpu().numpy(),
                counts=best_cnt[j].cpu().numpy(), sigma=chi2_sigma(float(cv[k]), self.nbins),
                data_avg=avg, data_var=var, nsamp=nsamp, T=T, dt=float(dt),
                nbins=self.nbins, npart=self.npart))
            j0 += len(rr)
        return out


# ---- .bestprof files (host) ----

_BESTPROF_KEYS = ("Input file", "Candidate", "T_sample", "Data Folded", "Data Avg", "Data StdDev",
                  "Profile Bins", "Profile Avg", "Profile StdDev", "Reduced chi-sqr", "Best DM",
                  "P_topo (ms)", "P'_topo (s/s)")


def mean_profile(fc):
    """The mean-per-sample profile S / C (0 where no sample fell)."""
    S, C = np.asarray(fc.profile, dtype=np.float64), np.asarray(fc.counts, dtype=np.float64)
    return np.divide(S, C, out=np.zeros_like(S), where=C > 0)


def write_bestprof(fc, fn, infile="", candname=""):
    """Write a FoldedCandidate as text in the style of PRESTO's ``.bestprof``:
    ``# Key = value`` header lines, a row of ``#``, then ``bin value`` lines
    with the mean-per-sample profile.  (No barycentring, no errors: the
    period is topocentric and is written without ``+/-``.)"""
    p = mean_profile(fc)
    vals = (infile, candname, "%.17g" % fc.dt, "%d" % fc.nsamp, "%.17g" % fc.data_avg,
            "%.17g" % np.sqrt(max(fc.data_var, 0.0)), "%d" % len(p), "%.17g" % p.mean(),
            "%.17g" % p.std(), "%.17g" % fc.chi2, "%.17g" % fc.dm,
            "%.17g" % (1000.0 * fc.period), "%.17g" % (-fc.fd / (fc.f * fc.f)))
    with open(fn, "w") as f:
        for k, v in zip(_BESTPROF_KEYS, vals):
            f.write("# %-17s=  %s\n" % (k, v))
        f.write("#" * 54 + "\n")
        for b, v in enumerate(p):
            f.write("%4d  %.17g\n" % (b, v))


def read_bestprof(fn):
    """(header dict: key -> text, numbers as float / int; profile float64
    array) of a file written by write_bestprof (or PRESTO's prepfold)."""
    hdr, prof = {}, []
    for line in open(fn):
        s = line.strip()
        if not s or set(s) == {"#"}:
            continue
        if s.startswith("#"):
            for sep in ("=", "<"):
                k, found, v = s[1:].partition(sep)
                if found:
                    break
            k, v = k.strip(), v.strip()
            try:
                hdr[k] = int(v)
            except ValueError:
                try:
                    hdr[k] = float(v.split("+/-")[0])
                except ValueError:
                    hdr[k] = v
            continue
        prof.append(float(s.split()[1]))
    return hdr, np.asarray(prof, dtype=np.float64)
