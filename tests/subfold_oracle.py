"""Brute-force NumPy restatement of the subband fold and its DM refinement
(include/pdd.h, pdd_subfold and pdd_subfold_dm): every channel is dedispersed
on its own, binned with the phases of tests/fold_oracle.py and summed into
its subband; the refinement runs in the header's order, operation by
operation (element-wise NumPy across bins keeps each element's own order)."""
import numpy as np

import fold_oracle as fo
from oracle import spectra_oracle as orc

_K = 0.000241


def delays_of(dm, freqs, dt):
    """b[c] of one DM (reference: the highest channel) and bmax."""
    b = np.asarray(orc.sweep_table([float(dm)], freqs, dt)[0], dtype=np.int64)
    assert dm >= 0 and b.min() >= 0
    return b, int(b.max())


def geometry(N, bmax, npart):
    """(n_out, L, folded samples npart L)."""
    n_out = int(N) - int(bmax)
    L = n_out // npart
    return n_out, L, npart * L


def subfold(x, freqs, dt, jobs, npart, nsub, nbins):
    """x: the whole file [N][C] (time-major); jobs: [(dm, f, fd, phi0)].
    (cube float64 [J, npart, nsub, nbins], cnt int32 [J, npart, nbins],
    chansum, chansq float64 [J, C])."""
    x = np.asarray(x)
    N, C = x.shape
    assert C % nsub == 0
    cps = C // nsub
    J = len(jobs)
    cube = np.zeros((J, npart, nsub, nbins), dtype=np.float64)
    cnt = np.zeros((J, npart, nbins), dtype=np.int32)
    chansum = np.zeros((J, C), dtype=np.float64)
    chansq = np.zeros((J, C), dtype=np.float64)
    for j, (dm, f, fd, phi0) in enumerate(jobs):
        b, bmax = delays_of(dm, freqs, dt)
        _, L, nf = geometry(N, bmax, npart)
        assert L >= 1
        bins = fo.bins_of(fo.phases(*fo.phase_steps(f, fd, dt, phi0), nf), nbins)
        for p in range(npart):
            cnt[j, p] = np.bincount(bins[p * L:(p + 1) * L], minlength=nbins)
        for c in range(C):
            y = x[b[c]:b[c] + nf, c].astype(np.float64)
            chansum[j, c] = np.sum(y)
            chansq[j, c] = np.sum(y * y)
            for p in range(npart):
                cube[j, p, c // cps] += np.bincount(bins[p * L:(p + 1) * L],
                                                    weights=y[p * L:(p + 1) * L], minlength=nbins)
    return cube, cnt, chansum, chansq


def subband_u(freqs, nsub):
    """u_s: delay per unit DM of the subband centres relative to the highest channel."""
    freqs = np.asarray(freqs, dtype=np.float64)
    cps = len(freqs) // nsub
    hi = freqs[np.arange(nsub) * cps]
    lo = freqs[(1 + np.arange(nsub)) * cps - 1]
    ctr = 0.5 * (hi + lo)
    fmax = np.max(freqs)
    return 1.0 / (_K * ctr * ctr) - 1.0 / (_K * fmax * fmax)


def default_ladder(dm, f, freqs, nsub, nbins, ndm=None):
    ndm = nbins + 1 if ndm is None else ndm
    u = subband_u(freqs, nsub)
    ddm = 1.0 / (nbins * f * np.max(np.abs(u)))
    return dm + (np.arange(ndm) - ndm // 2) * ddm


def ladder_shifts(dm, f, dms, freqs, nsub, nbins):
    """r[k][s] = floor((dms[k] - DM) u_s f nbins + 0.5) mod nbins."""
    u = subband_u(freqs, nsub)
    dms = np.asarray(dms, dtype=np.float64)
    r = np.floor((dms[:, None] - dm) * u[None, :] * f * nbins + 0.5)
    return (r.astype(np.int64) % nbins).astype(np.int32)


def better(a, b, mid):
    """a, b = (chi2, k): a before b in the order (chi2 descending, |k - mid|
    ascending, k ascending)."""
    if a[0] > b[0]:
        return True
    if not a[0] == b[0]:
        return False
    return (abs(a[1] - mid), a[1]) < (abs(b[1] - mid), b[1])


def refine(cube, cnt, chansum, chansq, ntot, trial, r):
    """One job.  cube [npart, nsub, nbins], cnt [npart, nbins], chansum /
    chansq [C], r int [ndm, nsub].  Returns a dict of the header's outputs."""
    npart, nsub, nbins = cube.shape
    C = len(chansum)
    cps = C // nsub
    ndm = len(r)
    sub = np.zeros((nsub, nbins), dtype=np.float64)
    Cb = np.zeros(nbins, dtype=np.int64)
    for p in range(npart):
        s_p = fo.shift(trial[0], trial[1], p, npart)
        sub += np.roll(cube[p], -s_p, axis=1)      # sub[s, b] += cube[p, s, (b + s_p) mod nbins]
        Cb += np.roll(cnt[p].astype(np.int64), -s_p)
    subints = np.zeros((npart, nbins), dtype=np.float64)
    for s in range(nsub):
        subints += cube[:, s, :]
    mu = np.zeros(nsub, dtype=np.float64)
    var = np.zeros(nsub, dtype=np.float64)
    if ntot > 0:
        nt = float(ntot)
        mc = np.asarray(chansum, dtype=np.float64) / nt
        vc = np.asarray(chansq, dtype=np.float64) / nt - mc * mc
        for q in range(cps):                        # ascending c within every subband
            mu += mc.reshape(nsub, cps)[:, q]
            var += vc.reshape(nsub, cps)[:, q]
    chi2 = np.zeros(ndm, dtype=np.float64)
    S_all = np.zeros((ndm, nbins), dtype=np.float64)
    C_all = np.zeros((ndm, nbins), dtype=np.int64)
    for k in range(ndm):
        S = np.zeros(nbins, dtype=np.float64)
        E = np.zeros(nbins, dtype=np.float64)
        V = np.zeros(nbins, dtype=np.float64)
        for s in range(nsub):
            rr = int(r[k][s]) % nbins
            c = np.roll(Cb, -rr)
            S += np.roll(sub[s], -rr)               # S[b] += sub[s, (b + r) mod nbins]
            E += mu[s] * c.astype(np.float64)
            V += var[s] * c.astype(np.float64)
            C_all[k] += c
        d = S - E
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(V > 0.0, (d * d) / V, 0.0)
        acc = 0.0
        for b in range(nbins):
            acc += term[b]
        chi2[k] = acc / float(nbins - 1)
        S_all[k] = S
    best = None
    for k in range(ndm):
        o = (chi2[k], k)
        if best is None or better(o, best, ndm // 2):
            best = o
    kb = best[1]
    return dict(chi2=chi2, best=kb, best_chi2=chi2[kb], best_prof=S_all[kb], best_cnt=C_all[kb],
                sub=sub, subints=subints, mu=mu, var=var)
