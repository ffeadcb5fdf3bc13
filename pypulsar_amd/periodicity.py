"""Periodicity search of DM-time planes: whitened power spectra, harmonic
sums, candidates, sifting across DMs and ``.accelcands`` output.

Beside ``SinglePulseSearch`` the second consumer of the sweep's plane: every
rank searches the rows it swept and only candidates (16 B each) leave the GPU.
Per DM row (kernels in pypulsar_amd/csrc/pdd_period.hip, restated in
tests/period_oracle.py):

* the row's float64 mean is removed and the row zero padded to ``nfft``
  (pdd_ps_prep), then transformed by rocFFT (``torch.fft.rfft``); the first
  ``nn = nfft // 2`` bins are used (no Nyquist bin, as in PRESTO's packed
  ``.fft`` layout);
* the spectrum is whitened as by ``PrestoFFT.deredden``
  (formats/prestofft.py:151-195, PRESTO's running median over blocks of
  ``int(initialbuflen * ln(offset))`` bins): pdd_ps_block_medians +
  pdd_ps_normalise give powers with unit mean under noise;
* ``PrestoFFT.harmonic_sum`` (:98-113), ``S_H[k] = sum_{h=1..H} P[h k]`` for
  ``k < nn // H``, is searched for all ``harms`` at once (pdd_ps_search): bin
  ``k >= rlo`` is a candidate of stage ``H`` when ``S_H[k]`` reaches the
  stage's threshold and is a local maximum (``> S_H[k-1]``, ``>= S_H[k+1]``).

Departures from the reference / PRESTO: rows are zero padded after mean
removal (PRESTO pads with the mean); where the whitening level is <= 0 (a
dead row) the normalised power is 0 (the reference gives inf / NaN).

Significance: after whitening ``2 S_H ~ chi2(2 H)``; ``sigma`` is the
equivalent Gaussian deviate of that single-trial probability.  No CPU
fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

DEFAULT_HARMS = (1, 2, 4, 8, 16)
MAX_BLOCK = 256        # longest whitening block (kPsMaxBlock in pdd_period.hip)
WORKSPACE_BYTES = 4 << 30  # default bound of __call__'s per-batch workspace

CAND_DTYPE = np.dtype([("DM", "f8"), ("row", "i4"), ("r", "i8"), ("freq", "f8"),
                       ("period", "f8"), ("numharm", "i4"), ("power", "f4"), ("sigma", "f8")])


def deredden_table(nn, initialbuflen=6, maxbuflen=200):
    """(offs, lens) int32: the blocks whose medians ``PrestoFFT.deredden``
    takes on a spectrum of ``nn`` bins, by the reference's own control flow
    (formats/prestofft.py:157-191) -- including its quirk that the first cap
    tests ``newoffset > maxbuflen`` and the later ones ``newbuflen >
    maxbuflen``.  Block j < B - 1 is corrected with the line between the
    medians of blocks j and j + 1; bins from offs[B-1] on take the last value
    of block B - 2."""
    nn, initialbuflen, maxbuflen = int(nn), int(initialbuflen), int(maxbuflen)
    assert 1 <= initialbuflen <= maxbuflen <= MAX_BLOCK, \
        "block lengths must be in 1..%d" % MAX_BLOCK
    offs, lens = [1], [initialbuflen]
    newoffset = 1 + initialbuflen
    newbuflen = int(initialbuflen * np.log(newoffset))
    if newoffset > maxbuflen:
        newbuflen = maxbuflen
    while newoffset + newbuflen < nn:
        offs.append(newoffset)
        lens.append(newbuflen)
        newoffset += newbuflen
        newbuflen = int(initialbuflen * np.log(newoffset))
        if newbuflen > maxbuflen:
            newbuflen = maxbuflen
    # (the reference would use an unbound `scaleval` without a corrected block)
    assert len(offs) >= 2, "spectrum of %d bins too short to whiten" % nn
    assert min(lens) >= 1 and max(lens) <= MAX_BLOCK
    return np.asarray(offs, dtype=np.int32), np.asarray(lens, dtype=np.int32)


# ---- significance (host, float64) ----

def _log_chi2_sf(S, H):
    """ln P(chi2(2H) > 2S) = -S + ln sum_{j<H} S^j / j!  (exact for the even
    number of degrees of freedom; no underflow)."""
    from scipy.special import gammaln, logsumexp
    S = np.asarray(S, dtype=np.float64)
    j = np.arange(int(H), dtype=np.float64)
    with np.errstate(divide="ignore"):
        logS = np.log(np.maximum(S, 0.0))
    with np.errstate(invalid="ignore"):  # (0 * -inf at S == 0, j == 0: replaced)
        terms = np.where(j == 0, 0.0, j * logS[..., None]) - gammaln(j + 1.0)
    return -np.maximum(S, 0.0) + logsumexp(terms, axis=-1)


_LOG_DIRECT = -650.0  # above this ln p, exp(ln p) is a normal float64


def _sigma_of_logp(logp):
    """x with ln norm.sf(x) = logp.  Direct through norm.isf where p is
    representable; below that Newton's iteration on ln norm.sf (concave,
    started right of the root: monotone convergence)."""
    from scipy.special import log_ndtr
    from scipy.stats import norm
    logp = np.atleast_1d(np.asarray(logp, dtype=np.float64))
    out = np.empty_like(logp)
    direct = logp > _LOG_DIRECT
    out[direct] = norm.isf(np.exp(logp[direct]))
    if not np.all(direct):
        lp = logp[~direct]
        x = np.sqrt(-2.0 * lp)
        for _ in range(12):
            ls = log_ndtr(-x)
            x = x + (ls - lp) / np.exp(norm.logpdf(x) - ls)
        out[~direct] = x
    return out


def sigma(S, H):
    """Equivalent Gaussian sigma of a harmonic sum ``S`` of ``H`` whitened
    powers: ``norm.isf(chi2.sf(2 S, 2 H))`` for a single trial, finite and
    monotonic up to S = 1e6 (log-space where the probability underflows)."""
    from scipy.special import gammainc
    from scipy.stats import norm
    S = np.asarray(S, dtype=np.float64)
    logp = np.atleast_1d(_log_chi2_sf(S, H))
    r = _sigma_of_logp(logp)
    # (p > 1/2: from the lower tail, which the upper one no longer resolves)
    low = logp > math.log(0.5)
    r[low] = norm.ppf(gammainc(float(H), np.atleast_1d(S)[low]))
    r = r.reshape(S.shape)
    return float(r) if r.ndim == 0 else r


def threshold_power(sig, H):
    """The inverse of ``sigma``: the summed power S with sigma(S, H) == sig."""
    from scipy.optimize import brentq
    from scipy.stats import norm
    logp = float(norm.logsf(float(sig)))
    if logp >= 0.0:
        return 0.0
    f = lambda s: float(_log_chi2_sf(s, H)) - logp  # noqa: E731  (decreasing in s)
    hi = max(1.0, -logp)  # ln Q(H, S) >= -S: f(-logp) >= 0
    while f(hi) > 0.0:
        hi *= 2.0
    return brentq(f, 0.0, hi, xtol=1e-13, rtol=1e-14)


# ---- device search ----

def _harms(harms):
    h = np.ascontiguousarray(np.asarray(harms, dtype=np.int32))
    assert h.ndim == 1 and 1 <= len(h) <= 8, "1..8 harmonic stages"
    assert np.all(h >= 1) and np.all(h <= 32), "harmonic counts must be in 1..32"
    assert np.all(np.diff(h) > 0), "harms must ascend"
    return h


class PeriodicitySearch(object):
    """``PeriodicitySearch(sigma_threshold=6.0)(plane, dms, dt)`` -> candidates.

    ``plane``: [D, n] float32 device tensor (a sweep plane, any row stride);
    ``dms``: the D trial DMs of its rows; ``dt``: its sample time.  ``flo``:
    lowest searched frequency (Hz).  All device work is queued on torch's
    current stream (the FFT is torch's)."""

    def __init__(self, sigma_threshold=6.0, harms=DEFAULT_HARMS, initialbuflen=6, maxbuflen=200,
                 flo=1.0, max_cands=1 << 20):
        _lib.require_gpu()
        self.sigma_threshold = float(sigma_threshold)
        self.harms = _harms(harms)
        self.initialbuflen, self.maxbuflen = int(initialbuflen), int(maxbuflen)
        assert self.maxbuflen <= MAX_BLOCK
        self.flo = float(flo)
        self.max_cands = int(max_cands)
        # float32 thresholds: the comparison the kernel (and the oracle) makes
        self.thr = np.asarray([threshold_power(self.sigma_threshold, int(h)) for h in self.harms],
                              dtype=np.float32)
        self._tables = {}

    def _table(self, nn, device):
        """Device (offs, lens) of a spectrum of nn bins, cached per (nn,
        initialbuflen, maxbuflen) and per stream: the buffers are created and
        filled on the stream whose kernels read them."""
        st = torch.cuda.current_stream(device)
        key = (int(nn), self.initialbuflen, self.maxbuflen, str(device), st.cuda_stream)
        t = self._tables.get(key)
        if t is None:
            offs, lens = deredden_table(nn, self.initialbuflen, self.maxbuflen)
            t = (torch.from_numpy(offs).to(device), torch.from_numpy(lens).to(device))
            self._tables[key] = t
        return t

    @staticmethod
    def default_nfft(n):
        return 1 << max(1, int(n - 1).bit_length())

    def prep(self, plane, nfft=None):
        """[D, n] plane rows -> [D, nfft] float32: each row minus its float64
        mean, zero padded (``nfft`` even, default the next power of two >=
        n)."""
        assert plane.is_cuda and plane.dtype == torch.float32 and plane.dim() == 2
        assert plane.stride(1) == 1
        D, n = plane.shape
        nfft = self.default_nfft(n) if nfft is None else int(nfft)
        assert nfft % 2 == 0 and nfft >= n >= 1, "nfft must be even and >= n"
        padded = torch.empty((D, nfft), dtype=torch.float32, device=plane.device)
        if D:
            call("pdd_ps_prep", ptr(plane), D, n, plane.stride(0), nfft, ptr(padded),
                 stream_ptr())
        return padded

    def spectrum(self, plane, nfft=None):
        """[D, nfft // 2 + 1] complex64 spectra of the prepared rows (rocFFT
        through torch); the search uses the first nfft // 2 bins."""
        return torch.fft.rfft(self.prep(plane, nfft), dim=1)

    def _spec_args(self, spec):
        assert spec.is_cuda and spec.dtype == torch.complex64 and spec.dim() == 2
        assert spec.stride(1) == 1
        return torch.view_as_real(spec), spec.shape[0], spec.stride(0)

    def medians(self, spec, nn=None):
        """Whitening levels [D, B] (block medians / ln 2) of the first ``nn``
        bins (default: all but the last, the Nyquist bin) of ``spec``."""
        f, D, ld = self._spec_args(spec)
        nn = spec.shape[1] - 1 if nn is None else int(nn)
        assert 1 <= nn <= spec.shape[1]
        offs, lens = self._table(nn, spec.device)
        B = offs.numel()
        med = torch.empty((D, B), dtype=torch.float32, device=spec.device)
        if D:
            call("pdd_ps_block_medians", ptr(f), D, nn, ld, ptr(offs), ptr(lens), B, ptr(med),
                 stream_ptr())
        return med

    def normalise(self, spec, want_spectrum=False, nn=None):
        """Whitened powers [D, nn] float32 of ``spec`` ([D, >= nn] complex64;
        ``nn`` defaults to all bins but the last, the Nyquist bin).  With
        ``want_spectrum`` also the whitened complex spectrum [D, nn] (the
        reference's ``deredden`` return value): (powers, spectrum)."""
        f, D, ld = self._spec_args(spec)
        nn = spec.shape[1] - 1 if nn is None else int(nn)
        med = self.medians(spec, nn)
        offs, lens = self._table(nn, spec.device)
        powers = torch.empty((D, nn), dtype=torch.float32, device=spec.device)
        out = torch.empty((D, nn), dtype=torch.complex64, device=spec.device) \
            if want_spectrum else None
        if D:
            call("pdd_ps_normalise", ptr(f), D, nn, ld, ptr(offs), ptr(lens), offs.numel(),
                 ptr(med), ptr(powers), ptr(torch.view_as_real(out)) if want_spectrum else None,
                 stream_ptr())
        return (powers, out) if want_spectrum else powers

    def harmonic_sum(self, powers, nharm):
        """[D, nn // nharm] sums of the first ``nharm`` harmonics."""
        assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 2
        assert powers.stride(1) == 1
        D, nn = powers.shape
        out = torch.empty((D, nn // int(nharm)), dtype=torch.float32, device=powers.device)
        if D and out.shape[1]:
            call("pdd_ps_harmsum", ptr(powers), D, nn, powers.stride(0), int(nharm), ptr(out),
                 stream_ptr())
        return out

    def rlo(self, nfft, dt):
        return max(1, int(math.ceil(self.flo * nfft * dt)))

    def raw(self, powers, nfft, dt):
        """Device-side search of whitened powers [D, nn]; returns (cands int32
        [max_cands, 4] = row, bin, harmonics, power bits; count tensor)
        without synchronising."""
        assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 2
        assert powers.stride(1) == 1
        D, nn = powers.shape
        cands = torch.empty((self.max_cands, 4), dtype=torch.int32, device=powers.device)
        count = torch.zeros(1, dtype=torch.int64, device=powers.device)
        if D and nn:
            call("pdd_ps_search", ptr(powers), D, nn, powers.stride(0),
                 self.harms.ctypes.data_as(ctypes.c_void_p), len(self.harms),
                 self.thr.ctypes.data_as(ctypes.c_void_p), self.rlo(nfft, dt), ptr(cands),
                 self.max_cands, ptr(count), stream_ptr())
        return cands, count

    def collect(self, cands, count, dms, nfft, dt, row0=0):
        """Device (cands, count) -> sorted candidate records (synchronises)."""
        k = int(count.item())
        if k > self.max_cands:
            raise RuntimeError("periodicity search: %d candidates exceed max_cands=%d "
                               "(raise the threshold or max_cands)" % (k, self.max_cands))
        return to_records(cands[:k].cpu().numpy(), dms, nfft, dt, row0)

    def row_batch(self, nfft):
        """Rows per batch that keep the workspace (padded rows + spectrum +
        powers, 4 + 4 + 2 bytes per padded sample, and as much again for the
        FFT's own work area) within WORKSPACE_BYTES."""
        return max(1, WORKSPACE_BYTES // (20 * int(nfft)))

    def __call__(self, plane, dms, dt, row_batch=None, nfft=None, zap=None, tap=None):
        """``zap``: a ``pypulsar_amd.zap.Zaplist`` whose bins are set to the
        whitened mean level in every row before the search (None: nothing is
        zapped).  ``tap``: a callable ``tap(powers, row0, nfft)``
        that is handed every batch's whitened (and zapped) powers [rows, nfft // 2]
        before they are released -- how ``pypulsar_amd.sideband`` searches the same
        powers without a second prep, FFT and whitening."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        nfft = self.default_nfft(n) if nfft is None else int(nfft)
        step = self.row_batch(nfft) if row_batch is None else int(row_batch)
        assert step >= 1
        if zap is not None:
            from . import zap as _zap
            zbins = _zap.device_bins(zap.bins(nfft, dt, nfft // 2), nfft // 2, plane.device)
        parts = []
        for r0 in range(0, D, step):
            rows = plane[r0:r0 + step]
            spec = self.spectrum(rows, nfft)
            powers = self.normalise(spec)
            del spec
            if zap is not None:
                _zap.apply(powers, zbins)
            if tap is not None:
                tap(powers, r0, nfft)
            c, k = self.raw(powers, nfft, dt)
            parts.append(self.collect(c, k, dms, nfft, dt, row0=r0))
            del powers, c, k
        return merge(parts)


def to_records(c, dms, nfft, dt, row0=0):
    """int32 [k, 4] (row, bin, harmonics, power bits) -> sorted CAND_DTYPE
    records; ``row0`` is the plane row of the searched batch's row 0."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 4)
    out = np.empty(len(c), dtype=CAND_DTYPE)
    out["row"] = c[:, 0] + int(row0)
    out["DM"] = np.asarray(dms, dtype=np.float64)[out["row"]] if len(c) else []
    out["r"] = c[:, 1]
    out["freq"] = out["r"] / (float(nfft) * dt)
    out["period"] = 1.0 / out["freq"] if len(c) else []
    out["numharm"] = c[:, 2]
    out["power"] = c[:, 3].view(np.float32)
    sig = np.empty(len(c), dtype=np.float64)
    for h in np.unique(out["numharm"]):
        m = out["numharm"] == h
        sig[m] = sigma(out["power"][m].astype(np.float64), int(h))
    out["sigma"] = sig
    return np.sort(out, order=("row", "numharm", "r"))


def merge(parts):
    """Concatenate candidate arrays of several row batches / ranks, sorted by
    (row, numharm, r)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=CAND_DTYPE)
    return np.sort(np.concatenate(parts), order=("row", "numharm", "r"))


# ---- sifting and .accelcands files (host) ----

class SiftedCandidate(object):
    """A candidate with its DM hits (the fields of a ``.accelcands`` entry).
    ``hits``: [(DM, sigma)] sorted by DM, the candidate's own DM included.
    ``z``: the drift in Fourier bins over the observation and ``fd`` the
    frequency derivative (Hz / s) of a candidate of the acceleration search
    (pypulsar_amd.accel), whose ``period`` is the mid-observation one; both 0
    otherwise.  ``w``: the jerk in Fourier bins over the observation and
    ``fdd`` the frequency's second derivative (Hz / s^2) of a candidate of the
    jerk search (pypulsar_amd.jerk), whose ``z`` and ``fd`` are the means over
    the observation; both 0 otherwise."""

    def __init__(self, dm, r, period, numharm, power, sigma, row=-1, accelfile=None, candnum=None,
                 z=0.0, fd=0.0, w=0.0, fdd=0.0):
        self.dm, self.r, self.period = float(dm), float(r), float(period)
        self.z, self.fd = float(z), float(fd)
        self.w, self.fdd = float(w), float(fdd)
        self.numharm, self.power, self.sigma = int(numharm), float(power), float(sigma)
        self.row = int(row)
        self.accelfile, self.candnum = accelfile, candnum
        self.hits = []

    @property
    def freq(self):
        return 1.0 / self.period

    def __repr__(self):
        return "SiftedCandidate(DM=%.2f, r=%.2f, P=%.6g s, numharm=%d, sigma=%.2f, %d hits)" % (
            self.dm, self.r, self.period, self.numharm, self.sigma, len(self.hits))


def sift(cands, rtol_bins=1.5, max_ratio=16):
    """Group candidate records across DMs and harmonics.  In order of
    descending sigma, a candidate is absorbed into the first stronger one
    whose ``r`` it matches within ``rtol_bins``, or of whose ``r`` it is --
    or which is of its ``r`` -- an integer multiple m <= max_ratio within
    ``rtol_bins``.  An absorbed candidate at another DM becomes a DM hit;
    each DM keeps its best sigma.  Records of the acceleration search (with a
    ``zbins`` field, the drift in bins of ``r``) match within ``rtol_bins +
    0.5 |zbins_a - m zbins_b|``: the Fresnel sidelobes of one signal lie
    within half the z difference in r.  Records of the jerk search (with a
    ``wbins`` field, the jerk in bins of ``r``) widen that by ``|wbins_a - m
    wbins_b| / 12``: the instantaneous frequency of a signal leaves its mean
    by at most a twelfth of its jerk (reasoned the same way, not measured).
    Returns SiftedCandidates by descending sigma."""
    order = np.argsort(-cands["sigma"], kind="stable")
    kept, kept_r = [], np.empty(0)
    has_z = cands.dtype.names is not None and "zbins" in cands.dtype.names
    has_w = cands.dtype.names is not None and "wbins" in cands.dtype.names
    kept_z, kept_w = np.empty(0), np.empty(0)
    m = np.arange(1, int(max_ratio) + 1, dtype=np.float64)
    for i in order:
        c = cands[i]
        r = float(c["r"])
        j = -1
        if len(kept):
            big, small = np.maximum(kept_r, r), np.minimum(kept_r, r)
            tol = rtol_bins
            if has_z:
                zb = float(c["zbins"])
                zbig, zsmall = np.where(kept_r >= r, kept_z, zb), np.where(kept_r >= r, zb, kept_z)
                tol = rtol_bins + 0.5 * np.abs(zbig[:, None] - m[None, :] * zsmall[:, None])
            if has_w:
                wb = float(c["wbins"])
                wbig, wsmall = np.where(kept_r >= r, kept_w, wb), np.where(kept_r >= r, wb, kept_w)
                tol = tol + np.abs(wbig[:, None] - m[None, :] * wsmall[:, None]) / 12.0
            rel = np.any(np.abs(big[:, None] - m[None, :] * small[:, None]) <= tol, axis=1)
            hit = np.flatnonzero(rel)
            if len(hit):
                j = int(hit[0])
        if j < 0:
            s = SiftedCandidate(c["DM"], r, c["period"], c["numharm"], c["power"], c["sigma"],
                                row=c["row"])
            if has_z:
                s.z, s.fd = float(c["z"]), float(c["fd"])
                kept_z = np.append(kept_z, float(c["zbins"]))
            if has_w:
                s.w, s.fdd = float(c["w"]), float(c["fdd"])
                kept_w = np.append(kept_w, float(c["wbins"]))
            s._hits = {float(c["DM"]): float(c["sigma"])}
            kept.append(s)
            kept_r = np.append(kept_r, r)
        else:
            # (descending sigma: the first entry of a DM is its best)
            kept[j]._hits.setdefault(float(c["DM"]), float(c["sigma"]))
    for s in kept:
        s.hits = sorted(s._hits.items())
        del s._hits
    return kept


ACCELCANDS_HEADER = ("#" + "file:candnum".center(66) + "DM".center(9) + "SNR".center(8) +
                     "sigma".center(8) + "numharm".center(9) + "ipow".center(9) +
                     "cpow".center(9) + "P(ms)".center(14) + "r".center(12) + "z".center(8) +
                     "numhits".center(9) + "\n")


def write_accelcands(sifted, fn, basename="pulsar_search", zmax=0, wmax=0):
    """Write SiftedCandidates in the ``.accelcands`` layout of
    formats/accelcands.py (``Candidate.__str__`` / ``DMHit.__str__``), by
    descending sigma, hits by ascending DM.  This search has no coherent
    power or S/N: ``ipow`` and ``cpow`` are both the summed power, ``SNR`` is
    the sigma (also for the hits); ``z`` is the candidate's (0 unless it comes
    from the acceleration search).  Candidates without a name are called
    ``<basename>_DM<dm>_ACCEL_<zmax>:<n>`` (``zmax``: the searched range, 0
    for the periodicity search), with ``_JERK_<wmax>`` appended when ``wmax``
    > 0 (the jerk search; the layout has no column for ``w``)."""
    jerk = "_JERK_%d" % int(wmax) if int(wmax) > 0 else ""
    cl = sorted(sifted, key=lambda c: -c.sigma)
    with open(fn, "w") as f:
        f.write(ACCELCANDS_HEADER)
        for n, c in enumerate(cl):
            name = c.accelfile if c.accelfile is not None \
                else "%s_DM%.2f_ACCEL_%d%s" % (basename, c.dm, int(zmax), jerk)
            cand = "%s:%d" % (name, c.candnum if c.candnum is not None else n + 1)
            f.write("%-65s   %7.2f  %6.2f  %6.2f  %s   %7.1f  %7.1f  %12.6f  %10.2f  %8.2f  (%d)\n"
                    % (cand, c.dm, c.sigma, c.sigma, "%2d".center(7) % c.numharm, c.power,
                       c.power, c.period * 1000.0, c.r, getattr(c, "z", 0.0) + 0.0, len(c.hits)))
            for dm, sg in sorted(c.hits):
                f.write("  DM=%6.2f SNR=%5.2f Sigma=%5.2f" % (dm, sg, sg) +
                        "   " + int(sg / 3.0) * "*" + "\n")


def read_accelcands(fn):
    """Inverse of write_accelcands (to the precision of the text): a list of
    SiftedCandidates with ``accelfile`` and ``candnum`` set."""
    out = []
    for line in open(fn):
        if not line.partition("#")[0].strip():
            continue
        if line.lstrip().startswith("DM="):
            while "= " in line:  # ("DM=  5.00": the value follows its padding)
                line = line.replace("= ", "=")
            kv = dict(t.split("=") for t in line.replace("*", " ").split())
            out[-1].hits.append((float(kv["DM"]), float(kv["Sigma"] if "Sigma" in kv
                                                          else kv["SNR"])))
            continue
        head, _, rest = line.rpartition("(")
        t = head.split()
        name, _, num = t[0].rpartition(":")
        dm, _snr, sg, numharm, ipow, _cpow, pms, r, z = t[1:10]
        c = SiftedCandidate(dm, r, float(pms) / 1000.0, numharm, ipow, sg, accelfile=name,
                            candnum=int(num), z=z)
        c._numhits = int(rest.split(")")[0])
        out.append(c)
    for c in out:
        assert len(c.hits) == c._numhits, "%s: hit count mismatch" % fn
        del c._numhits
    return out
