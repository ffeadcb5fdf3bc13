"""NumPy / Python restatement of the fold and its refinement search
(include/pdd.h, pdd_fold_rows and pdd_fold_search): uint64 wrap-around phases,
the integer shift formula, and the summation orders the header states
(ascending part for S, ascending bin for the chi-square; element-wise NumPy
operations across bins or trials keep each element's own order)."""
from fractions import Fraction

import numpy as np

M64 = 1 << 64


def phase_steps(f, fd, dt, phi0=0.0):
    """(P0, step, accel) by exact rational arithmetic on the float arguments."""
    f, fd, dt, phi0 = Fraction(f), Fraction(fd), Fraction(dt), Fraction(phi0)
    step = round(f * dt * M64) % M64
    accel = round(fd * dt * dt * M64) % M64
    return (round(phi0 * M64) + step // 2) % M64, step, accel


def phases(P0, step, accel, n):
    """P_i = P0 + i step + (i (i - 1) / 2) accel (mod 2^64), i < n."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        tri = (i * (i - np.uint64(1))) >> np.uint64(1)  # (i = 0: 0 * (2^64 - 1) = 0)
        return np.uint64(P0) + i * np.uint64(step) + tri * np.uint64(accel)


def bins_of(P, nbins):
    return (((P >> np.uint64(32)) * np.uint64(nbins)) >> np.uint64(32)).astype(np.int64)


def bins_python(P0, step, accel, n, nbins):
    """The same with Python integers (a check of the uint64 arithmetic)."""
    return [((((P0 + i * step + (i * (i - 1) // 2) * accel) % M64) >> 32) * nbins) >> 32
            for i in range(n)]


def fold_rows(plane, jobs, npart, nbins):
    """plane: [D, n]; jobs: [(row, P0, step, accel)].  (prof float64
    [J, npart, nbins], cnt int32 [J, npart, nbins], sumsq float64 [J, npart])."""
    plane = np.asarray(plane)
    D, n = plane.shape
    L = n // npart
    J = len(jobs)
    prof = np.zeros((J, npart, nbins), dtype=np.float64)
    cnt = np.zeros((J, npart, nbins), dtype=np.int32)
    sumsq = np.zeros((J, npart), dtype=np.float64)
    for j, (row, P0, step, accel) in enumerate(jobs):
        assert 0 <= row < D
        x = plane[row, :npart * L].astype(np.float64)
        b = bins_of(phases(P0, step, accel, npart * L), nbins)
        for p in range(npart):
            xs, bs = x[p * L:(p + 1) * L], b[p * L:(p + 1) * L]
            prof[j, p] = np.bincount(bs, weights=xs, minlength=nbins)
            cnt[j, p] = np.bincount(bs, minlength=nbins)
            sumsq[j, p] = np.sum(xs * xs)
    return prof, cnt, sumsq


def shift(ia, ib, p, N):
    """floor((ia m N + 2 ib m m + N N) / (2 N N)), m = 2 p + 1 - N."""
    m = 2 * p + 1 - N
    return (ia * m * N + 2 * ib * m * m + N * N) // (2 * N * N)


def stats(prof, cnt, sumsq):
    """(mu, var, Ntot) of one job in the header's order."""
    npart, nbins = prof.shape
    psum = np.zeros(npart, dtype=np.float64)
    for b in range(nbins):
        psum += prof[:, b]
    tot = q = 0.0
    for p in range(npart):
        tot += psum[p]
        q += sumsq[p]
    N = int(cnt.astype(np.int64).sum())
    if N == 0:
        return 0.0, 0.0, 0
    mu = tot / N
    return mu, q / N - mu * mu, N


def summed(prof, cnt, ia, ib):
    """S, C of one job for trial (ia, ib): parts added in ascending p."""
    npart, nbins = prof.shape
    S = np.zeros(nbins, dtype=np.float64)
    C = np.zeros(nbins, dtype=np.int64)
    for p in range(npart):
        s = shift(ia, ib, p, npart)
        S += np.roll(prof[p], -s)   # S[b] += prof[p, (b + s) mod nbins]
        C += np.roll(cnt[p], -s)
    return S, C


def better(a, b):
    """a, b = (chi2, ia, ib): a before b in the order (chi2 descending, |ib|,
    |ia|, ib, ia ascending)."""
    if a[0] > b[0]:
        return True
    if not a[0] == b[0]:
        return False
    return (abs(a[2]), abs(a[1]), a[2], a[1]) < (abs(b[2]), abs(b[1]), b[2], b[1])


def search(prof, cnt, sumsq, A, B):
    """One job.  (chi2 [2A+1, 2B+1], (ia, ib), best chi2, S, C of the best)."""
    npart, nbins = prof.shape
    mu, var, _ = stats(prof, cnt, sumsq)
    na, nb = 2 * A + 1, 2 * B + 1
    S = np.zeros((na * nb, nbins), dtype=np.float64)
    C = np.zeros((na * nb, nbins), dtype=np.int64)
    for t in range(na * nb):
        S[t], C[t] = summed(prof, cnt, t // nb - A, t % nb - B)
    chi2 = np.zeros(na * nb, dtype=np.float64)
    if var > 0.0:
        c = C.astype(np.float64)
        d = S - c * mu
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(C > 0, (d * d) / (c * var), 0.0)
        for b in range(nbins):
            chi2 += term[:, b]
        chi2 = chi2 / float(nbins - 1)
    best = None
    for t in range(na * nb):
        o = (chi2[t], t // nb - A, t % nb - B)
        if best is None or better(o, best):
            best = o
    Sb, Cb = summed(prof, cnt, best[1], best[2])
    return chi2.reshape(na, nb), (best[1], best[2]), best[0], Sb, Cb.astype(np.int32)


_CASE = {}


def search_case():
    """The offset pulse train both test files search (built once): a train of
    known (f0, fd0) folded at (f, fd) that lies (7.3, -4.9) trial steps
    away, npart = 16, nbins = 32, A = B = 32."""
    if not _CASE:
        n, dt, npart, nbins, A = 1 << 15, 64e-6, 16, 32, 32
        T = npart * (n // npart) * dt
        f0, fd_fold, ia0, ib0 = 23.4567, 0.02, 7.3, -4.9
        # (a pulse that drifts by +ia0, +ib0 bins in the fold is slower than it)
        fd0 = fd_fold - 8.0 * ib0 / (nbins * T * T)
        f = f0 + (ia0 - 4.0 * ib0) / (nbins * T)
        x = pulse_train(n, dt, f0, fd0, seed=3)
        prof, cnt, sumsq = fold_rows(x[None, :], [(0,) + phase_steps(f, fd_fold, dt)], npart, nbins)
        chi2, best, bchi2, S, C = search(prof[0], cnt[0], sumsq[0], A, A)
        _CASE.update(n=n, dt=dt, npart=npart, nbins=nbins, A=A, B=A, T=T, f0=f0, fd0=fd0, f=f,
                     fd=fd_fold, x=x, prof=prof, cnt=cnt, sumsq=sumsq, chi2=chi2, best=best,
                     best_chi2=bchi2, S=S, C=C)
        for v in _CASE.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _CASE


def pulse_train(n, dt, f0, fd0, width=0.04, amp=40.0, base=100.0, noise=4.0, seed=0):
    """An integer-valued row: pulses of fractional width `width` at phase
    f0 t + fd0 t t / 2 (t at the sample centres) on rounded Gaussian noise."""
    t = (np.arange(n) + 0.5) * dt
    ph = (f0 * t + 0.5 * fd0 * t * t) % 1.0
    x = base + np.random.default_rng(seed).normal(0.0, noise, n)
    x = x + amp * np.exp(-0.5 * ((ph - 0.5) / width) ** 2)
    return np.round(x).astype(np.float32)
