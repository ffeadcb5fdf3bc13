"""Fast-folding (FFA) search of DM-time planes: a phase-coherent fold over a
grid of trial periods, scored with a matched boxcar -- the time-domain
periodic search for slow, narrow pulses that the harmonic sums of
``periodicity`` and ``accel`` lose (whitening eats the lowest bins, at most 32
harmonics are summed).

Per DM row and step ``(f, b_lo, b_hi)`` of the plan (kernels in
pypulsar_amd/csrc/pdd_ffa.hip, the arithmetic in include/pdd.h, restated in
tests/ffa_oracle.py):

* the row is downsampled by ``f`` (sums of ``f`` samples) and detrended with
  the line between the means of consecutive chunks of ``L`` samples
  (pdd_ffa_downsample, pdd_ffa_detrend), which also gives its ``sigma``;
* for every base period ``p0`` of ``b_lo .. b_hi - 1`` bins the ``M = n_ds //
  p0`` rows of ``p0`` bins, zero padded to ``Mp`` rows, go through the radix-2
  fast-folding butterfly (pdd_ffa_pass: ``log2(Mp)`` stages in LDS, in one
  launch or, through a workspace, a few); trial ``s < Mp - 1`` is the fold at
  ``(p0 + s / (Mp - 1)) f dt``;
* every profile is scored in LDS with circular boxcars of ``widths`` bins up
  to ``ducy_max``; only the best S/N and its width index reach memory;
* local maxima of a row's periodogram above ``snr_threshold`` are the
  candidates (pdd_ffa_search).

Records (``FFA_CAND_DTYPE``) carry the fields ``periodicity.sift``,
``write_accelcands`` and ``fold.Folder`` read; ``r = n dt / period`` is float64
(slow pulsars sit at a handful of Fourier bins).  A trial step is ``1 / p0`` of
a Fourier bin, so ``sift(rtol_bins=1.5)`` groups a peak's neighbours and the
harmonics ``m P``.  No CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

DEFAULT_WIDTHS = (1, 2, 3, 4, 6, 9, 13, 19, 28, 42)
MAX_WIDTHS = 16
MAX_PROBLEMS = 65535     # problems (row, base period) of one pdd_ffa_pass launch

FFA_CAND_DTYPE = np.dtype([("DM", "f8"), ("row", "i4"), ("r", "f8"), ("freq", "f8"),
                           ("period", "f8"), ("numharm", "i4"), ("power", "f4"), ("sigma", "f8"),
                           ("width", "i4"), ("nbins", "i4"), ("ds", "i4"), ("duty", "f8")])


def ffa_plan(n, dt, period_min, period_max, bins_min=250, bins_max=500):
    """Steps ``(f, b_lo, b_hi)`` that tile ``[period_min, period_max)``: the
    step searches base periods ``b_lo .. b_hi - 1`` bins on the series
    downsampled by ``f``, chosen so that a period has ``bins_min .. bins_max``
    bins.  ValueError where the series is too short for a period (a fold
    needs two rows)."""
    n, bins_min, bins_max = int(n), int(bins_min), int(bins_max)
    dt, period_min, period_max = float(dt), float(period_min), float(period_max)
    if not (8 <= bins_min and 2 * bins_min <= bins_max <= 1024):
        raise ValueError("ffa_plan: need 8 <= bins_min and 2 bins_min <= bins_max <= 1024")
    if not (period_min >= bins_min * dt and period_max > period_min):
        raise ValueError("ffa_plan: need bins_min * dt <= period_min < period_max")
    steps, P = [], period_min
    while P < period_max:
        f = max(1, int(math.floor(P / (bins_min * dt))))
        dts = f * dt
        b_lo = int(math.floor(P / dts))
        b_hi = min(bins_max, int(math.ceil(period_max / dts)))
        if b_hi <= b_lo:
            break  # (rounding at the very end of the range)
        if n // f < 2 * b_hi:
            raise ValueError("ffa_plan: a series of %d samples is too short for a period of "
                             "%g s (two rows of %d bins at downsampling %d)"
                             % (n, b_hi * dts, b_hi, f))
        steps.append((f, b_lo, b_hi))
        P = b_hi * dts
    return steps


def plan_info(n_ds, p0):
    """(M, K, kpass, npass) of base period ``p0`` on ``n_ds`` samples: ``M``
    rows, ``Mp = 2^K``, the butterfly in ``npass`` launches of ``kpass``
    stages (the last one the rest).  Host only."""
    info = (ctypes.c_int64 * 4)()
    call("pdd_ffa_plan_info", int(n_ds), int(p0), ctypes.cast(info, ctypes.c_void_p))
    return tuple(int(v) for v in info)


class FFASearch(object):
    """``FFASearch(period_min, period_max)(plane, dms, dt)`` -> candidates.

    ``plane``: [D, n] float32 device tensor (a sweep plane, any row stride);
    ``dms``: the D trial DMs of its rows; ``dt``: its sample time.  ``detrend``:
    the length in seconds of the chunks whose means make the baseline (at
    least ``2 bins_max`` samples); default ``4 period_max``, long enough
    that a chunk's mean averages over several pulses, short enough to follow
    receiver drifts of tens of seconds.  All device work is queued on torch's
    current stream."""

    WORKSPACE_BYTES = 2 << 30  # bound of a launch's intermediate rows, and of a row batch
    PERIOD_SPAN = 64           # base periods of one launch

    def __init__(self, period_min, period_max, bins_min=250, bins_max=500, snr_threshold=8.0,
                 widths=DEFAULT_WIDTHS, ducy_max=0.2, detrend=None, max_cands=1 << 20):
        _lib.require_gpu()
        self.period_min, self.period_max = float(period_min), float(period_max)
        self.bins_min, self.bins_max = int(bins_min), int(bins_max)
        self.snr_threshold = float(snr_threshold)
        w = np.ascontiguousarray(np.asarray(widths, dtype=np.int32))
        assert w.ndim == 1 and 1 <= len(w) <= MAX_WIDTHS, "1..%d widths" % MAX_WIDTHS
        assert np.all(w >= 1) and np.all(np.diff(w) > 0), "widths must ascend from >= 1"
        self.widths = w
        self.ducy_max = float(ducy_max)
        assert self.ducy_max > 0.0
        self.detrend = 4.0 * self.period_max if detrend is None else float(detrend)
        assert self.detrend > 0.0
        self.max_cands = int(max_cands)
        self.workspace_bytes = self.WORKSPACE_BYTES
        # a list here (scripts/bench_ffa.py) collects (name, start, end) device
        # events of every launch
        self.events = None

    def _call(self, key, name, *args):
        if self.events is None:
            return call(name, *args)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(name, *args)
        b.record()
        self.events.append((key, a, b))

    # ---- host ----

    def plan(self, n, dt):
        return ffa_plan(n, dt, self.period_min, self.period_max, self.bins_min, self.bins_max)

    def chunk_len(self, f, dt):
        """L: downsampled samples of a detrending chunk."""
        return max(2 * self.bins_max, int(math.ceil(self.detrend / (f * float(dt)))))

    plan_info = staticmethod(plan_info)

    def trials(self, n, dt, plan=None):
        """The host trial table of a row's axis: (period, p0, s, f, M) arrays,
        steps and base periods in ascending period, s = 0 .. Mp - 2."""
        plan = self.plan(n, dt) if plan is None else plan
        per, p0s, ss, fs, Ms = [], [], [], [], []
        for f, b_lo, b_hi in plan:
            n_ds, dts = n // f, f * float(dt)
            for p0 in range(b_lo, b_hi):
                M = n_ds // p0
                Mp = max(2, 1 << int(M - 1).bit_length())
                s = np.arange(Mp - 1)
                per.append((p0 + s / float(Mp - 1)) * dts)
                p0s.append(np.full(Mp - 1, p0))
                ss.append(s)
                fs.append(np.full(Mp - 1, f))
                Ms.append(np.full(Mp - 1, M))
        cat = lambda v, t: np.concatenate(v).astype(t) if v else np.empty(0, t)  # noqa: E731
        return (cat(per, np.float64), cat(p0s, np.int64), cat(ss, np.int64), cat(fs, np.int64),
                cat(Ms, np.int64))

    # ---- device stages ----

    @staticmethod
    def _check_plane(plane):
        assert plane.is_cuda and plane.dtype == torch.float32 and plane.dim() == 2
        assert plane.shape[0] == 0 or plane.stride(1) == 1

    def prep(self, plane, f, L=None, dt=None):
        """[D, n] plane rows -> (y' [D, n // f] float32, sigma [D] float64):
        downsampled by ``f`` and detrended over chunks of ``L`` downsampled
        samples (default: from ``detrend`` and ``dt``)."""
        self._check_plane(plane)
        D, n = plane.shape
        f = int(f)
        assert 1 <= f <= n
        if L is None:
            assert dt is not None, "prep needs L or dt"
            L = self.chunk_len(f, dt)
        L = int(L)
        n_ds = n // f
        nchunk = max(1, n_ds // L)
        dev = plane.device
        y = torch.empty((D, n_ds), dtype=torch.float32, device=dev)
        sigma = torch.empty(D, dtype=torch.float64, device=dev)
        for r0 in range(0, D, MAX_PROBLEMS):
            rows = plane[r0:r0 + MAX_PROBLEMS]
            d = rows.shape[0]
            mean = torch.empty((d, nchunk), dtype=torch.float64, device=dev)
            part = torch.empty((d, nchunk, 2), dtype=torch.float64, device=dev)
            self._call("downsample", "pdd_ffa_downsample", ptr(rows), d, n, rows.stride(0), f, L,
                       ptr(y[r0:r0 + d]), ptr(mean), stream_ptr())
            self._call("detrend", "pdd_ffa_detrend", ptr(y[r0:r0 + d]), d, n_ds, L, ptr(mean),
                       ptr(part), ptr(sigma[r0:r0 + d]), stream_ptr())
        return y, sigma

    def transform(self, yprime, p0):
        """Test hook: the [D, Mp, p0] float32 profiles of base period ``p0`` of
        the prepared rows ``yprime`` [D, n_ds] (any row stride)."""
        self._check_plane(yprime)
        D, n_ds = yprime.shape
        M, K, _, npass = plan_info(n_ds, p0)
        Mp = 1 << K
        prof = torch.empty((D, Mp, p0), dtype=torch.float32, device=yprime.device)
        if D:
            self._passes(yprime, int(p0), 1, npass, Mp * int(p0), prof=prof)
        return prof

    def _passes(self, y, p_lo, np_, npass, slot, sigma=None, toff=None, snr=None, widx=None,
                ntrial=0, prof=None):
        """All passes of the problems (rows of y) x (np_ base periods from
        p_lo), at most MAX_PROBLEMS."""
        D, n_ds = y.shape
        assert D * np_ <= MAX_PROBLEMS
        nbuf = 0 if npass <= 1 else (1 if npass == 2 else 2)
        ws = [torch.empty(D * np_ * slot, dtype=torch.float32, device=y.device)
              for _ in range(nbuf)]
        for p in range(npass):
            self._call("pass%d" % p, "pdd_ffa_pass", ptr(y), D, n_ds, y.stride(0), p_lo, np_, p,
                       ptr(ws[(p - 1) % nbuf]) if p > 0 else None,
                       ptr(ws[p % nbuf]) if nbuf and p < npass - 1 else None, slot,
                       ptr(sigma), ptr(toff), self.widths.ctypes.data_as(ctypes.c_void_p),
                       len(self.widths), self.ducy_max, ptr(snr), ptr(widx), int(ntrial),
                       ptr(prof), stream_ptr())

    def periodogram(self, plane, dt, workspace_bytes=None):
        """(snr [D, ntrial] float32, width index [D, ntrial] uint8, trial
        table) of the plane's rows; the table is ``trials(n, dt)``.  The
        (row, base period) problems of a step run in launches whose
        intermediate rows stay within ``workspace_bytes`` (default: the
        instance's ``workspace_bytes``, from WORKSPACE_BYTES); the batching
        changes no bit."""
        self._check_plane(plane)
        D, n = plane.shape
        plan = self.plan(n, dt)
        table = self.trials(n, dt, plan)
        ntrial = len(table[0])
        bound = int(self.workspace_bytes if workspace_bytes is None else workspace_bytes)
        dev = plane.device
        snr = torch.empty((D, ntrial), dtype=torch.float32, device=dev)
        widx = torch.empty((D, ntrial), dtype=torch.uint8, device=dev)
        if D == 0:
            return snr, widx, table
        t0 = 0
        for f, b_lo, b_hi in plan:
            y, sigma = self.prep(plane, f, dt=dt)
            n_ds = y.shape[1]
            infos = [plan_info(n_ds, p0) for p0 in range(b_lo, b_hi)]
            ntr = np.asarray([(1 << K) - 1 for _, K, _, _ in infos], dtype=np.int64)
            toff_h = t0 + np.concatenate([[0], np.cumsum(ntr)[:-1]])
            toff = torch.from_numpy(toff_h).to(dev)
            # problems of one launch: by the workspace; at most PERIOD_SPAN base periods
            # (a launch declares the LDS of its longest profile), as many rows as fit
            slot_all = max((1 << K) * p0 for p0, (_, K, _, _) in zip(range(b_lo, b_hi), infos))
            npass_all = max(i[3] for i in infos)
            per_problem = 4 * slot_all * (0 if npass_all <= 1 else (1 if npass_all == 2 else 2))
            nprob = MAX_PROBLEMS if per_problem == 0 else \
                max(1, min(MAX_PROBLEMS, bound // per_problem))
            nb = b_hi - b_lo
            pstep = max(1, min(nb, nprob, self.PERIOD_SPAN))
            rstep = max(1, nprob // pstep)
            for r0 in range(0, D, rstep):
                for q0 in range(0, nb, pstep):
                    q1 = min(nb, q0 + pstep)
                    sub = infos[q0:q1]
                    slot = max((1 << K) * p0 for p0, (_, K, _, _) in
                               zip(range(b_lo + q0, b_lo + q1), sub))
                    self._passes(y[r0:r0 + rstep], b_lo + q0, q1 - q0, max(i[3] for i in sub),
                                 slot, sigma=sigma[r0:r0 + rstep], toff=toff[q0:q1],
                                 snr=snr[r0:r0 + rstep], widx=widx[r0:r0 + rstep], ntrial=ntrial)
            t0 += int(ntr.sum())
            del y, sigma
        assert t0 == ntrial
        return snr, widx, table

    def raw(self, snr, width):
        """Device-side candidate search of a periodogram; returns (cands int32
        [max_cands, 4] = row, trial, width index, snr bits; count tensor)
        without synchronising."""
        assert snr.is_cuda and snr.dtype == torch.float32 and snr.dim() == 2
        assert width.is_cuda and width.dtype == torch.uint8 and width.shape == snr.shape
        assert snr.shape[0] == 0 or (snr.stride(1) == 1 and width.stride() == snr.stride())
        D, nt = snr.shape
        cands = torch.empty((self.max_cands, 4), dtype=torch.int32, device=snr.device)
        count = torch.zeros(1, dtype=torch.int64, device=snr.device)
        if D and nt:
            self._call("search", "pdd_ffa_search", ptr(snr), ptr(width), D, nt, snr.stride(0),
                       ctypes.c_float(self.snr_threshold), ptr(cands), self.max_cands,
                       ptr(count), stream_ptr())
        return cands, count

    def collect(self, cands, count, dms, table, n, dt, row0=0):
        """Device (cands, count) -> sorted FFA_CAND_DTYPE records
        (synchronises)."""
        k = int(count.item())
        if k > self.max_cands:
            raise RuntimeError("FFA search: %d candidates exceed max_cands=%d "
                               "(raise the threshold or max_cands)" % (k, self.max_cands))
        return to_records(cands[:k].cpu().numpy(), dms, table, self.widths, n, dt, row0)

    def row_batch(self, n, ntrial):
        """Rows per batch that keep the prepared rows (4 bytes per sample) and
        the periodogram (5 bytes per trial) within the workspace bound."""
        return max(1, int(self.workspace_bytes) // (4 * int(n) + 5 * int(ntrial) + 1))

    def __call__(self, plane, dms, dt, row_batch=None):
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        if D == 0:
            return np.empty(0, dtype=FFA_CAND_DTYPE)
        ntrial = len(self.trials(n, dt)[0])
        step = self.row_batch(n, ntrial) if row_batch is None else int(row_batch)
        assert step >= 1
        parts = []
        for r0 in range(0, D, step):
            snr, widx, table = self.periodogram(plane[r0:r0 + step], dt)
            c, k = self.raw(snr, widx)
            parts.append(self.collect(c, k, dms, table, n, dt, row0=r0))
            del snr, widx, c, k
        return merge(parts)


def to_records(c, dms, table, widths, n, dt, row0=0):
    """int32 [k, 4] (row, trial, width index, snr bits) -> FFA_CAND_DTYPE
    records sorted by (row, period)."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 4)
    period, p0, _, f, _ = table
    out = np.empty(len(c), dtype=FFA_CAND_DTYPE)
    if not len(c):
        return out
    k = c[:, 1]
    out["row"] = c[:, 0] + int(row0)
    out["DM"] = np.asarray(dms, dtype=np.float64)[out["row"]]
    out["period"] = period[k]
    out["freq"] = 1.0 / out["period"]
    out["r"] = int(n) * float(dt) / out["period"]
    out["numharm"] = 1
    out["power"] = c[:, 3].view(np.float32)
    out["sigma"] = out["power"].astype(np.float64)
    out["width"] = np.asarray(widths)[c[:, 2]]
    out["nbins"] = p0[k]
    out["ds"] = f[k]
    out["duty"] = out["width"] / out["nbins"].astype(np.float64)
    return np.sort(out, order=("row", "period"))


def merge(parts):
    """Concatenate candidate arrays of several row batches, sorted by (row,
    period)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=FFA_CAND_DTYPE)
    return np.sort(np.concatenate(parts), order=("row", "period"))
