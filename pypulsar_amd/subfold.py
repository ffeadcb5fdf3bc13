"""Folding of periodicity candidates from the raw file into (sub-integration,
subband, phase) cubes, and the refinement of their DM on the cube: the
phase-versus-frequency image that tells a dispersed, broadband pulsar from
interference (prepfold's subband panel), a DM ladder finer than the search
grid, and a fold at the file's own time resolution.  Everything comes from
the raw block in file order, many candidates per launch
(pypulsar_amd/csrc/pdd_subfold.hip).  The definition is this project's
(include/pdd.h; restated by brute force in
tests/subfold_oracle.py).

All times are RAW file samples and ``dt`` is the raw sample time.  A job is
(DM, f at raw sample 0, fd, phi0):

* ``b[c] = delays.sweep_table([DM], freqs, dt)[0][c]`` (reference: the
  highest channel, every entry >= 0), ``bmax = max b``; ``n_out = N - bmax``,
  ``L = n_out // npart``; the dedispersed samples ``i < npart L`` are folded;
* phase and bin of sample ``i`` are those of ``fold.phase_steps`` /
  pdd_fold_rows, shared by every channel;
* subband ``s`` = channels ``s C/nsub .. (s+1) C/nsub - 1`` in file order;
* ``cube[p][s][bin(i)] += sum_{c in s} x[i + b[c]][c]``, ``cnt[p][bin(i)] += 1``,
  ``chansum[c]`` / ``chansq[c]``: sums and sums of squares per channel.

8-bit input folds to the exact integers, whatever the split into blocks;
float32 input to float64 sums in no fixed order.  The zero-DM filter is NOT
applied: as in the cut-outs the data is used as recorded.

Limits (refused, never clamped): 2 <= nbins <= 256, 1 <= npart <= 128,
npart nbins <= 8192, nsub nbins <= 8192, 1 <= ndm <= 1024, nsub divides C,
DM >= 0, table entries fit int32.  No CPU fallback.
"""
import ctypes

import numpy as np

from . import delays
from .fold import MAX_BINS, MAX_CELLS, MAX_PART, chi2_sigma, phase_steps

MAX_DM = 1024
_KEYS = ("sub", "subints", "subint_counts", "profile", "counts", "chi2_vs_dm", "dms", "chansum",
         "chansq", "sub_freqs")
_SCALARS = ("dm_fold", "dm", "ddm", "best", "chi2", "sigma", "f", "fd", "T", "dt", "nsamp")


def check_sizes(C, npart, nsub, nbins, ndm=None):
    if not 2 <= nbins <= MAX_BINS:
        raise ValueError("nbins must be in 2..%d" % MAX_BINS)
    if not 1 <= npart <= MAX_PART:
        raise ValueError("npart must be in 1..%d" % MAX_PART)
    if npart * nbins > MAX_CELLS:
        raise ValueError("npart * nbins must not exceed %d" % MAX_CELLS)
    if nsub < 1 or C % nsub:
        raise ValueError("nsub must divide the %d channels" % C)
    if nsub * nbins > MAX_CELLS:
        raise ValueError("nsub * nbins must not exceed %d" % MAX_CELLS)
    if ndm is not None and not 1 <= ndm <= MAX_DM:
        raise ValueError("ndm must be in 1..%d" % MAX_DM)


def subband_u(freqs, nsub):
    """u_s: the delay (s) per unit DM of the subband centres
    (``delays.subband_layout``) relative to the highest channel."""
    freqs = np.asarray(freqs, dtype=np.float64)
    ctr = delays.subband_layout(freqs, nsub)[2]
    return delays.delay_from_DM(1.0, ctr) - delays.delay_from_DM(1.0, np.max(freqs))


def ladder_step(f, freqs, nsub, nbins):
    """The DM step that moves the subband furthest from the reference by one
    bin: 1 / (nbins f max_s |u_s|)."""
    return 1.0 / (nbins * float(f) * np.max(np.abs(subband_u(freqs, nsub))))


def default_ladder(dm, f, freqs, nsub, nbins, ndm=None):
    """dms[k] = DM + (k - ndm // 2) ddm, ndm = nbins + 1 by default: half a
    turn of the lowest subband each way."""
    ndm = nbins + 1 if ndm is None else int(ndm)
    return float(dm) + (np.arange(ndm) - ndm // 2) * ladder_step(f, freqs, nsub, nbins)


def ladder_shifts(dm, f, dms, freqs, nsub, nbins):
    """int32 [ndm, nsub]: r[k][s] = floor((dms[k] - DM) u_s f nbins + 0.5) mod nbins."""
    u = subband_u(freqs, nsub)
    dms = np.asarray(dms, dtype=np.float64)
    r = np.floor((dms[:, None] - float(dm)) * u[None, :] * float(f) * nbins + 0.5)
    if r.size and not np.all(np.abs(r) < 2.0 ** 62):
        raise OverflowError("ladder shifts do not fit int64")
    return (r.astype(np.int64) % nbins).astype(np.int32)


def candidate_params(cands, N, dt):
    """[(dm, f, fd, trial)] with f at raw sample 0.  A ``FoldedCandidate``
    gives its refined dm, f (already at the first sample) and fd, trial
    (0, 0); a sifted candidate (``freq`` and ``fd`` mid-observation) is
    converted as ``Folder.__call__`` does, ``f = freq - fd N dt / 2``; a
    tuple is (dm, f, fd) or (dm, f), f at raw sample 0."""
    from .fold import FoldedCandidate
    out = []
    for c in cands:
        if isinstance(c, FoldedCandidate):
            out.append((float(c.dm), float(c.f), float(c.fd), (0, 0)))
        elif hasattr(c, "freq"):
            f, fd = float(c.freq), float(getattr(c, "fd", 0.0))
            if fd != 0.0:
                f = f - 0.5 * fd * int(N) * float(dt)
            out.append((float(c.dm), f, fd, (0, 0)))
        else:
            out.append((float(c[0]), float(c[1]), float(c[2]) if len(c) > 2 else 0.0, (0, 0)))
    return out


class Jobs(object):
    """The geometry of J jobs on a file of ``N`` samples: ``dm``, ``f``,
    ``fd``, ``phi0`` [J]; ``table`` int32 [J, C] (b of every job), ``bmax``,
    ``L``, ``nfold`` (= npart L) [J]; ``words`` int64 [J, 3] = (P0, step,
    accel)."""

    def __init__(self, freqs, dt, npart, N, dm, f, fd=0.0, phi0=0.0):
        self.freqs, self.dt = np.asarray(freqs, dtype=np.float64), float(dt)
        self.npart, self.N = int(npart), int(N)
        self.dm = np.atleast_1d(np.asarray(dm, dtype=np.float64))
        self.f, self.fd, self.phi0 = (np.broadcast_to(np.asarray(v, dtype=np.float64),
                                                      self.dm.shape).copy() for v in (f, fd, phi0))
        if len(self.dm) and not np.all(self.dm >= 0):
            raise ValueError("a negative DM cannot be folded (delays relative to the top channel)")
        t = delays.sweep_table(self.dm, self.freqs, self.dt)
        if t.size and t.min() < 0:
            raise ValueError("negative delay in the table")
        self.table = delays.to_int32(t)
        self.bmax = self.table.max(axis=1).astype(np.int64) if len(self.dm) else \
            np.zeros(0, dtype=np.int64)
        self.L = (self.N - self.bmax) // self.npart
        if len(self.dm) and self.L.min() < 1:
            raise ValueError("%d samples less the delays cannot be cut into %d parts" % (
                self.N, self.npart))
        self.nfold = self.L * self.npart
        w = np.empty((len(self.dm), 3), dtype=np.uint64)
        for j in range(len(self.dm)):
            for q, v in enumerate(phase_steps(self.f[j], self.fd[j], self.dt, self.phi0[j])):
                w[j, q] = np.uint64(v)
        self.words = w.view(np.int64)

    def __len__(self):
        return len(self.dm)

    @property
    def tile_span(self):
        """The largest delay range within an aligned group of 64 channels of
        any job (``tile_span`` of pdd_subfold: sizes the kernel's staging)."""
        C = self.table.shape[1]
        return max([int(np.ptp(self.table[:, c:c + 64], axis=1).max())
                    for c in range(0, C, 64)] if len(self.dm) else [0])

    @property
    def T(self):
        """Seconds folded per job."""
        return self.nfold * self.dt


def plan_blocks(nfold, bmax, max_rows):
    """Blocks of at most ``max_rows`` file rows that fold jobs of ``nfold[j]``
    dedispersed samples with largest delays ``bmax[j]``: [(a, b, i0, i1)],
    rows [a, b) and per job the samples [i0[j], i1[j]) folded from them.  The
    rows cover [0, max(nfold + bmax)), consecutive blocks overlap by
    max(bmax) rows, every sample is folded by exactly one block."""
    nfold = np.atleast_1d(np.asarray(nfold, dtype=np.int64))
    bmax = np.atleast_1d(np.asarray(bmax, dtype=np.int64))
    if not len(nfold):
        return []
    end, over = int((nfold + bmax).max()), int(bmax.max())
    if int(max_rows) <= over:
        raise ValueError("blocks of %d rows cannot hold delays of %d rows" % (max_rows, over))
    out, a = [], 0
    while True:
        b = min(end, a + int(max_rows))
        last = b == end
        i0 = np.minimum(a, nfold)
        i1 = nfold.copy() if last else np.minimum(b - over, nfold)
        out.append((a, b, i0, i1))
        if last:
            return out
        a = b - over


class SubbandFold(object):
    """One candidate folded into subbands (all arrays on the host).

    ``dm_fold``: the DM it was folded at; ``dm``: the best DM of the ladder
    ``dms`` (step ``ddm``), ``best`` its index, ``chi2_vs_dm`` the reduced
    chi-square of every entry, ``chi2`` / ``sigma`` of the best; ``f``,
    ``fd`` (at raw sample 0), ``T`` the folded span (s); ``sub`` [nsub,
    nbins]: the phase-versus-frequency image at the fold DM (parts collapsed
    by the trial's shifts), ``sub_freqs`` its subband centres (MHz);
    ``subints`` [npart, nbins] (all subbands, parts not shifted),
    ``subint_counts``; ``profile`` / ``counts`` [nbins]: the summed profile
    at the best DM and the (sample, subband) pairs behind each bin;
    ``chansum`` / ``chansq`` [C]; ``nsamp``: folded samples; ``dt``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "SubbandFold(DM %.2f -> %.2f +- %.2f, P=%.9g s, chi2=%.2f, sigma=%.1f)" % (
            self.dm_fold, self.dm, self.ddm, 1.0 / self.f, self.chi2, self.sigma)


class SubbandFolder(object):
    """``SubbandFolder(freqs, dt, npart, nsub, nbins, ndm)``: ``fold`` adds
    one block of the file to the cubes of many jobs, ``refine`` runs the DM
    ladder on finished cubes, ``__call__(block, cands)`` does both for a file
    held in one block.  All device work is queued on torch's current stream."""

    def __init__(self, freqs, dt, npart=32, nsub=32, nbins=64, ndm=None):
        self.freqs, self.dt = np.asarray(freqs, dtype=np.float64), float(dt)
        self.npart, self.nsub, self.nbins = int(npart), int(nsub), int(nbins)
        self.ndm = self.nbins + 1 if ndm is None else int(ndm)
        check_sizes(len(self.freqs), self.npart, self.nsub, self.nbins, self.ndm)

    def plan(self, N, dm, f, fd=0.0, phi0=0.0):
        return Jobs(self.freqs, self.dt, self.npart, N, dm, f, fd, phi0)

    def _jobs(self, jobs, N):
        if isinstance(jobs, Jobs):
            assert jobs.N == int(N) and jobs.npart == self.npart and len(jobs.freqs) == len(self.freqs)
            return jobs
        cols = [[float(j[q]) if len(j) > q else 0.0 for j in jobs] for q in range(4)]
        return self.plan(N, *cols)

    def empty(self, J, device="cuda"):
        """Zeroed outputs (cube, cnt, chansum, chansq) of J jobs."""
        import torch
        from . import _lib
        _lib.require_gpu()
        C = len(self.freqs)
        out = (torch.empty((J, self.npart, self.nsub, self.nbins), dtype=torch.float64, device=device),
               torch.empty((J, self.npart, self.nbins), dtype=torch.int32, device=device),
               torch.empty((J, C), dtype=torch.float64, device=device),
               torch.empty((J, C), dtype=torch.float64, device=device))
        if J:
            _lib.call("pdd_subfold_zero", *[_lib.ptr(t) for t in out], J, C, self.npart, self.nsub,
                      self.nbins, _lib.stream_ptr())
        return out

    def fold(self, block, t_first, N, jobs, out=None, span=None):
        """Add to ``out`` (None: fresh zeroed outputs) what ``block`` -- device
        [n, C] uint8 or float32, time-major, rows may be strided, first row =
        raw sample ``t_first`` of a file of ``N`` samples -- holds of every
        job (a ``Jobs`` or (dm, f, fd, phi0) tuples).  ``span`` = (i0, i1),
        scalars or one per job: the dedispersed samples folded by this call
        (default: all the block covers, ``[t_first, t_first + n - bmax)`` cut
        to the folded range -- right for one block or blocks that do not
        overlap; overlapping blocks take their spans from ``plan_blocks``).
        A span the block does not cover raises ValueError; nothing is
        launched then.  Returns ``out``; does not synchronise."""
        import torch
        from . import _lib
        _lib.require_gpu()
        codes = {torch.uint8: _lib.U8, torch.float32: _lib.F32}
        C = len(self.freqs)
        if block.dtype not in codes:
            raise TypeError("SubbandFolder: 8-bit or float32 blocks only, got %s" % block.dtype)
        assert block.is_cuda and block.dim() == 2 and block.shape[1] == C
        assert block.shape[0] == 0 or block.stride(1) == 1 or C == 1
        jobs = self._jobs(jobs, N)
        J, n, t_first = len(jobs), int(block.shape[0]), int(t_first)
        if out is None:
            out = self.empty(J, block.device)
        cube, cnt, chansum, chansq = out
        assert tuple(cube.shape) == (J, self.npart, self.nsub, self.nbins) and cube.is_contiguous()
        assert tuple(cnt.shape) == (J, self.npart, self.nbins) and cnt.is_contiguous()
        assert tuple(chansum.shape) == tuple(chansq.shape) == (J, C)
        assert cube.dtype == chansum.dtype == chansq.dtype == torch.float64
        assert cnt.dtype == torch.int32 and chansum.is_contiguous() and chansq.is_contiguous()
        if J == 0:
            return out
        if not 0 < n < 2 ** 31 or t_first < 0 or t_first + n > jobs.N:
            raise ValueError("a block of %d rows at sample %d does not lie in the file's %d" % (
                n, t_first, jobs.N))
        if span is None:
            i0 = np.minimum(t_first, jobs.nfold)
            i1 = np.clip(t_first + n - jobs.bmax, i0, jobs.nfold)
        else:
            i0, i1 = (np.broadcast_to(np.asarray(v, dtype=np.int64), (J,)).copy() for v in span)
        live = i0 < i1
        if np.any(i0 < 0) or np.any(i1 < i0) or np.any(i1 > jobs.nfold) or \
                np.any(live & ((i0 < t_first) | (i1 - 1 + jobs.bmax >= t_first + n))):
            raise ValueError("the block [%d, %d) does not cover the span of every job "
                             "(samples i0 .. i1 - 1 + bmax)" % (t_first, t_first + n))
        jb = np.zeros((J, 8), dtype=np.int64)
        jb[:, :3] = jobs.words
        jb[:, 3], jb[:, 4], jb[:, 5] = jobs.L, i0, i1
        jb[:, 6], jb[:, 7] = np.arange(J), jobs.bmax
        ld = block.stride(0) if n > 1 else C
        table, jd = torch.from_numpy(jobs.table).to(block.device), torch.from_numpy(jb).to(block.device)
        _lib.call("pdd_subfold", _lib.ptr(block), codes[block.dtype], n, C, ld, t_first,
                  jb.ctypes.data_as(ctypes.c_void_p), _lib.ptr(jd), J, _lib.ptr(table), J,
                  self.npart, self.nsub, self.nbins, _lib.ptr(cube), _lib.ptr(cnt),
                  _lib.ptr(chansum), _lib.ptr(chansq), jobs.tile_span, _lib.stream_ptr())
        return out

    def ladders(self, jobs, dms=None):
        """(dms float64 [J, ndm], r int32 [J, ndm, nsub]) of the jobs:
        ``dms`` None: the default ladder of ``self.ndm`` entries per job."""
        J = len(jobs)
        if dms is None:
            dms = np.stack([default_ladder(jobs.dm[j], jobs.f[j], self.freqs, self.nsub, self.nbins,
                                           self.ndm) for j in range(J)]) if J else \
                np.zeros((0, self.ndm))
        dms = np.asarray(dms, dtype=np.float64)
        if dms.ndim == 1:
            dms = np.broadcast_to(dms, (J, len(dms)))
        if dms.shape[0] != J or not 1 <= dms.shape[1] <= MAX_DM:
            raise ValueError("a ladder of 1..%d entries per job expected" % MAX_DM)
        r = np.zeros((J, dms.shape[1], self.nsub), dtype=np.int32)
        for j in range(J):
            r[j] = ladder_shifts(jobs.dm[j], jobs.f[j], dms[j], self.freqs, self.nsub, self.nbins)
        return np.ascontiguousarray(dms), r

    def refine(self, cube, cnt, chansum, chansq, jobs, trials=None, dms=None):
        """The DM ladder on finished cubes.  ``trials``: (ia, ib) per job
        (default (0, 0)); ``dms``: [J, ndm] or [ndm] (default: the default
        ladder).  Returns a dict: device tensors chi2 [J, ndm], best [J],
        best_chi2 [J], best_prof [J, nbins], best_cnt int64 [J, nbins], sub
        [J, nsub, nbins], subints [J, npart, nbins], and the host arrays dms
        [J, ndm], r [J, ndm, nsub]; does not synchronise."""
        import torch
        from . import _lib
        _lib.require_gpu()
        J, C, dev = len(jobs), len(self.freqs), cube.device
        assert tuple(cube.shape) == (J, self.npart, self.nsub, self.nbins) and cube.is_contiguous()
        assert tuple(cnt.shape) == (J, self.npart, self.nbins) and cnt.is_contiguous()
        assert cube.dtype == torch.float64 and cnt.dtype == torch.int32
        for t in (chansum, chansq):
            assert tuple(t.shape) == (J, C) and t.dtype == torch.float64 and t.is_contiguous()
        dms, r = self.ladders(jobs, dms)
        ndm = dms.shape[1]
        tr = np.zeros((J, 2), dtype=np.int32)
        if trials is not None:
            tr[:] = np.asarray(trials, dtype=np.int64).reshape(J, 2)
        f64 = dict(dtype=torch.float64, device=dev)
        res = dict(chi2=torch.empty((J, ndm), **f64),
                   best=torch.empty((J,), dtype=torch.int32, device=dev),
                   best_chi2=torch.empty((J,), **f64), best_prof=torch.empty((J, self.nbins), **f64),
                   best_cnt=torch.empty((J, self.nbins), dtype=torch.int64, device=dev),
                   sub=torch.empty((J, self.nsub, self.nbins), **f64),
                   subints=torch.empty((J, self.npart, self.nbins), **f64), dms=dms, r=r)
        if J:
            ntot = torch.from_numpy(np.ascontiguousarray(jobs.nfold, dtype=np.int64)).to(dev)
            trd, rd = torch.from_numpy(tr).to(dev), torch.from_numpy(r).to(dev)
            _lib.call("pdd_subfold_dm", _lib.ptr(cube), _lib.ptr(cnt), _lib.ptr(chansum),
                      _lib.ptr(chansq), _lib.ptr(ntot), _lib.ptr(trd), _lib.ptr(rd), J, C,
                      self.npart, self.nsub, self.nbins, ndm, _lib.ptr(res["chi2"]),
                      _lib.ptr(res["best"]), _lib.ptr(res["best_chi2"]), _lib.ptr(res["best_prof"]),
                      _lib.ptr(res["best_cnt"]), _lib.ptr(res["sub"]), _lib.ptr(res["subints"]),
                      _lib.stream_ptr())
        return res

    def results(self, out, res, jobs):
        """The SubbandFolds of folded (``out``) and refined (``res``) jobs."""
        cnt, chansum, chansq = (t.cpu().numpy() for t in out[1:])
        host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
        ctr = delays.subband_layout(self.freqs, self.nsub)[2]
        folds = []
        for j in range(len(jobs)):
            k = int(host["best"][j])
            dms = host["dms"][j]
            ddm = float(dms[1] - dms[0]) if len(dms) > 1 else 0.0
            chi2 = float(host["best_chi2"][j])
            folds.append(SubbandFold(
                dm_fold=float(jobs.dm[j]), dm=float(dms[k]), ddm=ddm, best=k, dms=dms.copy(),
                chi2_vs_dm=host["chi2"][j].copy(), chi2=chi2, sigma=chi2_sigma(chi2, self.nbins),
                f=float(jobs.f[j]), fd=float(jobs.fd[j]), T=float(jobs.T[j]), dt=self.dt,
                nsamp=int(jobs.nfold[j]), sub=host["sub"][j].copy(), sub_freqs=ctr.copy(),
                subints=host["subints"][j].copy(), subint_counts=cnt[j].copy(),
                profile=host["best_prof"][j].copy(), counts=host["best_cnt"][j].copy(),
                chansum=chansum[j].copy(), chansq=chansq[j].copy()))
        return folds

    def __call__(self, block, cands, dms=None):
        """Fold and refine candidates (see ``candidate_params``) on a whole
        file held in ``block`` -> list of SubbandFold."""
        N = int(block.shape[0])
        par = candidate_params(cands, N, self.dt)
        if not par:
            return []
        jobs = self.plan(N, [p[0] for p in par], [p[1] for p in par], [p[2] for p in par])
        out = self.fold(block, 0, N, jobs)
        res = self.refine(*out, jobs, trials=[p[3] for p in par], dms=dms)
        return self.results(out, res, jobs)


def subfold_from_file(fb, cands, rfimask=None, load_bytes=256 << 20, npart=32, nsub=32, nbins=64,
                      ndm=None, dms=None):
    """Fold and refine candidates from the open ``filterbank`` ``fb`` (8 or
    32 bits), read in overlapping blocks of at most ``load_bytes``; every job
    runs on every block.  ``rfimask``: its cells are replaced
    (``RFIMask.apply``, the mask's own fill values) in each block first.  The
    zero-DM filter is not applied.  Returns a list of SubbandFold."""
    import torch
    dtype = np.dtype(fb.dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise ValueError("subband folds: 8-bit or float32 filterbanks only")
    sf = SubbandFolder(fb.freqs, fb.tsamp, npart, nsub, nbins, ndm)
    N, C = int(fb.number_of_samples), len(sf.freqs)
    par = candidate_params(cands, N, sf.dt)
    if not par:
        return []
    jobs = sf.plan(N, [p[0] for p in par], [p[1] for p in par], [p[2] for p in par])
    max_rows = max(1, int(load_bytes) // (C * dtype.itemsize))
    out = None
    for a, b, i0, i1 in plan_blocks(jobs.nfold, jobs.bmax, max_rows):
        host = np.empty((b - a, C), dtype=dtype)
        got = fb.read_block_into(a, host)
        if got != b - a:
            raise IOError("short read: %d of %d rows at sample %d" % (got, b - a, a))
        block = torch.from_numpy(host).cuda()
        if rfimask is not None:
            rfimask.apply(block, a)
        out = sf.fold(block, a, N, jobs, out=out, span=(i0, i1))
    res = sf.refine(*out, jobs, trials=[p[3] for p in par], dms=dms)
    return sf.results(out, res, jobs)


def write_subfold(fn, sf):
    """``.npz`` (no pickle) of a SubbandFold: the arrays sub, subints,
    subint_counts, profile, counts, chi2_vs_dm, dms, chansum, chansq,
    sub_freqs and the scalars dm_fold, dm, ddm, best, chi2, sigma, f, fd, T,
    dt, nsamp."""
    cols = {k: np.asarray(getattr(sf, k)) for k in _KEYS}
    for k in _SCALARS:
        cols[k] = np.int64(getattr(sf, k)) if k in ("best", "nsamp") else np.float64(getattr(sf, k))
    with open(fn, "wb") as fh:
        np.savez(fh, **cols)


def read_subfold(fn):
    """Inverse of write_subfold."""
    with np.load(fn, allow_pickle=False) as z:
        kw = {k: z[k] for k in _KEYS}
        for k in _SCALARS:
            kw[k] = int(z[k]) if k in ("best", "nsamp") else float(z[k])
    return SubbandFold(**kw)
