"""Fourier-domain zapping of periodic interference ("birdies"): a finder on
the rows of a DM-time plane, PRESTO ``.zaplist`` files, and the zap itself.

A mains line, a radar rotation or a cryo-pump line is in (nearly) every DM
row of the plane and so in every row's candidate list; a celestial signal
peaks in a few neighbouring rows.  An order statistic across rows -- by
default the median -- of the whitened power spectra therefore keeps the
birdie and discards the pulsar.  The reference's ``bin/autozap.py`` takes the
same statistic across the spectra of different beams; here the rows of the
plane are the many spectra (kernels in pypulsar_amd/csrc/pdd_zap.hip,
restated in tests/zap_oracle.py):

* ``BirdieFinder.find`` whitens ``rows`` evenly spaced rows with the
  search's own ``PeriodicitySearch`` (prep, FFT, ``deredden``), takes the
  ``rank``-th smallest power of every bin (pdd_zap_percentile), flags the bins
  above a threshold of known false-alarm probability and returns a
  ``Zaplist``;
* ``PeriodicitySearch`` and ``AccelSearch`` called with ``zap=<Zaplist>``
  set the whitened powers (and spectrum) of the listed bins to the whitened
  mean level, 1 (pdd_zap_apply), between the whitening and the search.

Definitions.  ``rank(R) = max(1, ceil(percent / 100 * R))``: the order
statistic that at least ``percent`` % of the R rows do not exceed.  It equals
``scipy.stats.scoreatpercentile`` (autozap.calc_percentile) whenever
``percent / 100 * (R - 1)`` is an integer -- the median of an odd number of
rows is one such case -- and is chosen over linear interpolation because its
noise distribution is known in closed form: whitened noise powers are Exp(1),
the j-th of R order statistics exceeds x with probability ``I_{exp(-x)}(R - j
+ 1, j)`` (regularised incomplete beta function), so the threshold of a
per-bin false-alarm probability ``norm.sf(nsig)`` is ``-ln betaincinv(R - j +
1, j, norm.sf(nsig))``.  No baseline is fitted: autozap's median filter,
fitted sigma and log-log detrend (gen_mask / hone_mask) exist because its
spectra are not whitened; these are.  The rate holds where the rows are
independent: at frequencies below about one over the spread of the
dedispersion delays between the rows they carry the same noise, and at the
bins of a signal that is in a good part (but less than ``100 - percent`` %)
of the rows the statistic is that of the remaining ones; both raise it
(DESIGN.md §6i).

The fill is the whitened mean level, not zero (PRESTO fills with the local
mean too): a pulsar whose harmonic falls on a zapped bin keeps the expected
noise contribution in its harmonic sum, and the fill alone reaches no
threshold.  The zap acts after whitening; the block medians still see the
birdie.

``.zaplist`` files.  The text layout is that of the reference's
``autozap.write_zaplist`` (pinned by tests/golden/golden_zaplist.txt).  The
meaning of the second column as the FULL width in Hz and the floor / ceil bin
rule of ``Zaplist.bins`` follow PRESTO's ``zapbirds``; PRESTO is not
available to this project, so that part is parity unpinned.  (The reference's
own width column is half of a span that ends two bins past the last flagged
one; that arithmetic is not reproduced.)  No CPU fallback for the device
parts.
"""
import math

import numpy as np

MAX_ROWS = 64           # most rows of a percentile (kZapMaxRows in pdd_zap.hip)
BIN_EPS = 1e-6          # slack of the floor / ceil bin rule (in bins)

ZAPLIST_HEADER = ("# This file was created automatically with pypulsar_amd.zap\n"
                  "# Lines beginning with '#' are comments\n"
                  "# Lines beginning with 'B' are barycentric freqs (i.e. PSR freqs)\n"
                  "#                 Freq                 Width\n"
                  "# --------------------  --------------------\n")


def merge_intervals(iv):
    """[k, 2] inclusive integer intervals -> sorted int32 [m, 2] with
    overlapping and touching ones merged."""
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
    iv = iv[np.argsort(iv[:, 0], kind="stable")]
    out = []
    for lo, hi in iv:
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], int(hi))
        else:
            out.append([int(lo), int(hi)])
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


class Zaplist(object):
    """Centre frequencies and FULL widths (Hz, float64) of the intervals to
    zap, sorted by frequency."""

    def __init__(self, freqs=(), widths=()):
        f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
        w = np.atleast_1d(np.asarray(widths, dtype=np.float64))
        assert f.ndim == 1 and f.shape == w.shape, "one width per frequency"
        assert np.all(w >= 0.0), "widths must be >= 0"
        o = np.argsort(f, kind="stable")
        self.freqs, self.widths = f[o], w[o]

    def __len__(self):
        return len(self.freqs)

    def __repr__(self):
        return "Zaplist(%d intervals)" % len(self)

    def bins(self, nfft, dt, nn=None):
        """int32 [nz, 2]: the inclusive bin intervals ``[floor((f - w / 2) T +
        1e-6), ceil((f + w / 2) T - 1e-6)]`` of a spectrum of ``nfft`` samples
        of ``dt`` (T = nfft dt), clipped to [1, nn - 1] (``nn`` defaults to
        nfft // 2), empty ones dropped, overlapping or touching ones merged."""
        nn = int(nfft) // 2 if nn is None else int(nn)
        T = float(nfft) * float(dt)
        lo = np.floor((self.freqs - 0.5 * self.widths) * T + BIN_EPS)
        hi = np.ceil((self.freqs + 0.5 * self.widths) * T - BIN_EPS)
        lo, hi = np.maximum(lo, 1.0), np.minimum(hi, float(nn - 1))
        keep = lo <= hi
        return merge_intervals(np.stack((lo[keep], hi[keep]), axis=1))

    @classmethod
    def from_bins(cls, bins, nfft, dt):
        """The inverse of ``bins``: ``f = (lo + hi) / (2 T)``, ``w = (hi - lo)
        / T``; ``from_bins(b, nfft, dt).bins(nfft, dt)`` is ``b`` exactly
        (that is what the 1e-6 of the bin rule is for)."""
        b = np.asarray(bins, dtype=np.float64).reshape(-1, 2)
        T = float(nfft) * float(dt)
        return cls((b[:, 0] + b[:, 1]) / (2.0 * T), (b[:, 1] - b[:, 0]) / T)

    def merged(self, other):
        """Both lists' entries in one (``bins`` merges what overlaps)."""
        return Zaplist(np.concatenate((self.freqs, other.freqs)),
                       np.concatenate((self.widths, other.widths)))


def read_zaplist(fn, baryv=0.0):
    """Read a PRESTO ``.zaplist``: ``#`` lines are comments, every other line
    holds a frequency and a full width in Hz.  A line that starts with ``B``
    gives a barycentric frequency: it and its width are multiplied by ``(1 +
    baryv)`` (``baryv``: the observatory's velocity towards the source in
    units of c; it is accepted, not computed)."""
    freqs, widths = [], []
    with open(fn) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            scale = 1.0
            if s[0] in "Bb":
                s, scale = s[1:], 1.0 + float(baryv)
            t = s.split()
            freqs.append(float(t[0]) * scale)
            widths.append(float(t[1]) * scale)
    return Zaplist(freqs, widths)


def write_zaplist(fn, zl):
    """Write a ``Zaplist`` in the layout of the reference's
    ``autozap.write_zaplist``: the comment header, then one ``"  %20.15g
    %20.15g\\n"`` line (frequency, full width) per entry."""
    with open(fn, "w") as f:
        f.write(ZAPLIST_HEADER)
        for fr, w in zip(zl.freqs, zl.widths):
            f.write("  %20.15g  %20.15g\n" % (fr, w))


def device_bins(bins, nn, device):
    """Check host intervals (sorted, disjoint, within [1, nn - 1]) and upload
    them: the int32 [nz, 2] device tensor ``apply`` takes."""
    import torch
    b = np.ascontiguousarray(np.asarray(bins, dtype=np.int32).reshape(-1, 2))
    if len(b):
        assert np.all(b[:, 0] <= b[:, 1]), "zap intervals must have lo <= hi"
        assert b[0, 0] >= 1 and b[-1, 1] <= int(nn) - 1, "zap intervals must lie in [1, nn - 1]"
        assert np.all(b[1:, 0] > b[:-1, 1]), "zap intervals must be sorted and disjoint"
    return torch.from_numpy(b).to(device)


def apply(powers, bins, spectrum=None):
    """Set the bins of the inclusive intervals ``bins`` ([nz, 2]; a host
    array, or the device tensor of ``device_bins``) to 1 in every row of the
    whitened ``powers`` ([D, nn] float32 device tensor, any row stride) and,
    where given, to ``(1 + 1j) / sqrt(2)`` in the whitened ``spectrum`` ([D,
    >= nn] complex64), in place (pdd_zap_apply).  Nothing else is written."""
    import torch
    from ._lib import call, ptr, stream_ptr
    assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 2
    assert powers.stride(1) == 1
    D, nn = powers.shape
    if not torch.is_tensor(bins):
        bins = device_bins(bins, nn, powers.device)
    assert bins.is_cuda and bins.dtype == torch.int32 and bins.dim() == 2 and bins.shape[1] == 2
    assert bins.is_contiguous()
    sp, lds = None, 0
    if spectrum is not None:
        assert spectrum.is_cuda and spectrum.dtype == torch.complex64 and spectrum.dim() == 2
        assert spectrum.stride(1) == 1 and spectrum.shape[0] == D and spectrum.shape[1] >= nn
        sp, lds = torch.view_as_real(spectrum), spectrum.stride(0)
    nz = bins.shape[0]
    if D and nz:
        call("pdd_zap_apply", ptr(powers), powers.stride(0), ptr(sp), lds, D, nn, ptr(bins), nz,
             stream_ptr())
    return powers


class BirdieFinder(object):
    """``BirdieFinder(rows=33, percent=50.0, nsig=5.0, grow=1).find(ps, plane,
    dt)`` -> ``Zaplist`` of the bins whose ``percent``-th percentile across
    ``rows`` evenly spaced plane rows stands out of whitened noise at a
    per-bin false-alarm probability of ``norm.sf(nsig)`` (expected false zaps
    a spectrum: ``nn norm.sf(nsig)``, 0.15 at nsig = 5 and nn = 2^19); every
    run of flagged bins is grown by ``grow`` bins on each side."""

    def __init__(self, rows=33, percent=50.0, nsig=5.0, grow=1):
        self.rows, self.percent = int(rows), float(percent)
        self.nsig, self.grow = float(nsig), int(grow)
        assert 1 <= self.rows <= MAX_ROWS, "rows must be in 1..%d" % MAX_ROWS
        assert 0.0 < self.percent <= 100.0, "percent must be in (0, 100]"
        assert self.grow >= 0

    def select_rows(self, D):
        """The plane rows used: ``min(rows, D)`` evenly spaced ones."""
        D = int(D)
        assert D >= 1
        return np.unique(np.round(np.linspace(0, D - 1, min(self.rows, D)))).astype(np.int64)

    def rank(self, R):
        """``max(1, ceil(percent / 100 * R))`` (1-based): the order statistic
        that at least ``percent`` % of R rows do not exceed."""
        return max(1, int(math.ceil(self.percent * int(R) / 100.0)))

    def threshold(self, R):
        """The power that the ``rank(R)``-th of R independent Exp(1) values
        exceeds with probability ``norm.sf(nsig)``."""
        from scipy.special import betaincinv
        from scipy.stats import norm
        R = int(R)
        j = self.rank(R)
        return float(-np.log(betaincinv(float(R - j + 1), float(j), norm.sf(self.nsig))))

    def percentile(self, powers, rank):
        """Device [R, nn] float32 (any row stride) -> device [nn]: the
        ``rank``-th smallest (1-based) value of every column, by exact
        selection (pdd_zap_percentile; 1 <= rank <= R <= 64)."""
        import torch
        from ._lib import call, ptr, stream_ptr
        assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 2
        assert powers.stride(1) == 1 and powers.shape[1] >= 1
        R, nn = powers.shape
        out = torch.empty(nn, dtype=torch.float32, device=powers.device)
        call("pdd_zap_percentile", ptr(powers), R, nn, powers.stride(0), int(rank), ptr(out),
             stream_ptr())
        return out

    def flag(self, pct, R, rlo):
        """Host percentile spectrum [nn] of R rows -> int32 [m, 2] intervals:
        the runs of bins ``k >= rlo`` with ``pct[k] > threshold(R)`` (compared
        in float64), grown by ``grow`` on each side within [1, nn - 1] and
        merged."""
        pct = np.asarray(pct, dtype=np.float64)
        nn = len(pct)
        hot = pct > self.threshold(R)
        hot[:max(1, int(rlo))] = False
        k = np.flatnonzero(hot)
        iv = np.stack((np.maximum(k - self.grow, 1), np.minimum(k + self.grow, nn - 1)), axis=1)
        return merge_intervals(iv)

    def find(self, ps, plane, dt, nfft=None, return_spectrum=False):
        """``Zaplist`` of the birdies of ``plane`` ([D, n] float32 device
        tensor), whitened by the ``PeriodicitySearch`` ``ps`` at FFT length
        ``nfft`` (default: ``ps``'s own); bins below ``ps.rlo`` are not
        flagged.  One copy of nn floats leaves the device.  With
        ``return_spectrum`` also the percentile spectrum (host float32 [nn]):
        (zaplist, spectrum)."""
        import torch
        D, n = plane.shape
        nfft = ps.default_nfft(n) if nfft is None else int(nfft)
        sel = self.select_rows(D)
        rows = plane.index_select(0, torch.from_numpy(sel).to(plane.device))
        powers = ps.normalise(ps.spectrum(rows, nfft))
        R = len(sel)
        pct = self.percentile(powers, self.rank(R)).cpu().numpy()
        zl = Zaplist.from_bins(self.flag(pct, R, ps.rlo(nfft, dt)), nfft, dt)
        return (zl, pct) if return_spectrum else zl
