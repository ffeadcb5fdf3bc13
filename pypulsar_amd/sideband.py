"""Sideband search of DM-time planes: pulsars in binaries whose orbit is
shorter than the observation (Ransom, Cordes & Eikenberry 2003; PRESTO's
``search_bin``).

The periodicity, acceleration and jerk searches assume that the frequency
drifts smoothly over the observation.  With ``Porb < T`` the signal is phase
modulated instead: its power is spread over a comb of about ``2 beta``
sidebands around the spin frequency (``beta = 2 pi f x`` the modulation index),
``T / Porb`` bins apart, none of which needs to reach the threshold.  A short
FFT of a stretch of the *power spectrum* turns a comb of spacing ``s`` bins into
a peak at mini-bin ``L / s``.  Per DM row and mini-FFT length ``L`` (kernel
in pypulsar_amd/csrc/pdd_sideband.hip, restated in tests/sideband_oracle.py;
DESIGN.md §6q), on the whitened powers ``PeriodicitySearch.normalise`` gives:

* segments of ``L`` bins start every ``L >> shift`` bins from ``rlo``;
* each segment, clipped at ``clip``, is transformed and normalised by its DC
  term to the half-bin grid ``q = 0..L-1`` (``q / 2`` the mini-bin): ``M[2k] =
  L |A_k|^2 / A_0^2`` and the interbin ``M[2k+1] = (pi^2 / 16) L |A_k -
  A_{k+1}|^2 / A_0^2``;
* ``S_H[q] = sum_{h=1..H} M[h q]`` is searched for every stage ``H`` of
  ``harms``: ``q`` of ``[qlo, L // H)`` is a candidate when ``S_H[q]`` reaches
  the stage's threshold and is a local maximum.

A candidate at ``q`` in a segment ``[lo, lo + L)`` has the orbital period
``Porb = q nfft dt / (2 L)`` and a spin frequency inside ``[lo, lo + L) / (nfft
dt)``.  Thresholds and significance are those of the periodicity search
(``2 S_H ~ chi2(2 H)``, single trial).  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import periodicity as _per
from ._lib import call, ptr, stream_ptr

DEFAULT_HARMS = (1, 2, 4)
MIN_LOG2, MAX_LOG2 = 5, 14   # mini-FFT lengths 32..16384 (kSbMinLog2, kSbMaxLog2)
MAX_HARM = 8                 # largest harmonic count of a stage (kSbMaxHarm)
MAX_STAGES = 4               # most stages (kSbMaxStages)

CAND_DTYPE = np.dtype([("DM", "f8"), ("row", "i4"), ("L", "i4"), ("lo", "i8"), ("q", "i4"),
                       ("numharm", "i4"), ("power", "f4"), ("sigma", "f8"), ("freq", "f8"),
                       ("freq_lo", "f8"), ("freq_hi", "f8"), ("porb", "f8")])
SIFTED_DTYPE = np.dtype(CAND_DTYPE.descr + [("nhits", "i4"), ("ndms", "i4")])
_ORDER = ("row", "L", "lo", "numharm", "q")
# the columns of a .bincands line, in order
BINCAND_DTYPE = np.dtype([("sigma", "f8"), ("DM", "f8"), ("freq", "f8"), ("freq_lo", "f8"),
                          ("freq_hi", "f8"), ("porb", "f8"), ("L", "i4"), ("q", "i4"),
                          ("numharm", "i4"), ("power", "f4"), ("nhits", "i4"), ("ndms", "i4")])


def twiddle_table(L):
    """float32 [L // 2, 2]: (cos, sin)(2 pi j / L), j < L / 2, computed in
    float64 and rounded once."""
    a = 2.0 * np.pi * np.arange(int(L) // 2, dtype=np.float64) / float(L)
    return np.ascontiguousarray(np.stack((np.cos(a), np.sin(a)), axis=-1).astype(np.float32))


def nseg(nn, rlo, L, shift=2):
    """Segments of length ``L`` in bins ``[rlo, nn)``, ``L >> shift`` apart."""
    nn, rlo, L = int(nn), int(rlo), int(L)
    return 0 if nn - rlo < L else (nn - rlo - L) // (L >> int(shift)) + 1


def _harms(harms):
    h = np.ascontiguousarray(np.asarray(harms, dtype=np.int32))
    assert h.ndim == 1 and 1 <= len(h) <= MAX_STAGES, "1..%d harmonic stages" % MAX_STAGES
    assert np.all(h >= 1) and np.all(h <= MAX_HARM), "harmonic counts must be in 1..%d" % MAX_HARM
    assert np.all(np.diff(h) > 0), "harms must ascend"
    return h


def _log2(v, what):
    v = int(v)
    e = v.bit_length() - 1
    assert v == 1 << e and MIN_LOG2 <= e <= MAX_LOG2, \
        "%s must be a power of two in %d..%d" % (what, 1 << MIN_LOG2, 1 << MAX_LOG2)
    return e


class SidebandSearch(object):
    """``SidebandSearch(sigma_threshold=6.0)(plane, dms, dt)`` -> candidates
    (CAND_DTYPE records).

    ``plane``, ``dms``, ``dt`` as for ``PeriodicitySearch``; ``minfft`` ..
    ``maxfft``: the ladder of mini-FFT lengths (powers of two in 32..16384);
    ``shift``: segments start ``L >> shift`` bins apart (0..3); ``harms``: the
    stages (each 1..8, at most 4); ``clip``: powers are clipped there before
    the mini FFT ("auto": the single-bin threshold of ``sigma_threshold`` --
    bins above it are candidates of the plain search anyway, and a lone strong
    line left in gives a flat mini spectrum full of spurious maxima; 0: no
    clip); ``qlo``: lowest searched half-bin.  ``ps``: the
    ``PeriodicitySearch`` whose prep, FFT and whitening are used (default: one
    made with ``initialbuflen``, ``maxbuflen`` and ``flo``).  All device work is
    queued on torch's current stream."""

    def __init__(self, sigma_threshold=6.0, minfft=32, maxfft=16384, shift=2, harms=DEFAULT_HARMS,
                 clip="auto", qlo=4, flo=1.0, max_cands=1 << 20, initialbuflen=6, maxbuflen=200,
                 ps=None):
        _lib.require_gpu()
        self.sigma_threshold = float(sigma_threshold)
        e0, e1 = _log2(minfft, "minfft"), _log2(maxfft, "maxfft")
        assert e0 <= e1, "minfft must not exceed maxfft"
        self.log2s = tuple(range(e0, e1 + 1))
        self.shift = int(shift)
        assert 0 <= self.shift <= 3, "shift must be in 0..3"
        self.harms = _harms(harms)
        self.qlo = int(qlo)
        assert 1 <= self.qlo <= (1 << e0) // 8, "qlo must be in 1..minfft / 8"
        self.max_cands = int(max_cands)
        self.ps = ps if ps is not None else _per.PeriodicitySearch(
            sigma_threshold, (1,), initialbuflen, maxbuflen, flo, max_cands)
        self.flo = float(flo) if ps is None else float(ps.flo)
        # float32 thresholds: the comparison the kernel (and the oracle) makes
        self.thr = np.asarray([_per.threshold_power(self.sigma_threshold, int(h))
                               for h in self.harms], dtype=np.float32)
        self.clip = float(_per.threshold_power(self.sigma_threshold, 1)) if clip == "auto" \
            else float(clip)
        assert self.clip >= 0.0, "clip must be >= 0 (0: none)"
        self._tables = {}

    def _table(self, L, device):
        """Device twiddles of length ``L``, cached per stream as
        ``PeriodicitySearch._table``."""
        st = torch.cuda.current_stream(device)
        key = (int(L), str(device), st.cuda_stream)
        t = self._tables.get(key)
        if t is None:
            t = torch.from_numpy(twiddle_table(L)).to(device)
            self._tables[key] = t
        return t

    def rlo(self, nfft, dt):
        return self.ps.rlo(nfft, dt)

    def _search(self, powers, rlo, e, mini, cands, max_cands, count):
        call("pdd_sb_search", ptr(powers), powers.shape[0], powers.shape[1], powers.stride(0),
             int(rlo), int(e), self.shift, ctypes.c_float(self.clip),
             self.harms.ctypes.data_as(ctypes.c_void_p), len(self.harms),
             self.thr.ctypes.data_as(ctypes.c_void_p), self.qlo,
             ptr(self._table(1 << e, powers.device)), ptr(mini), ptr(cands), int(max_cands),
             ptr(count), stream_ptr())

    @staticmethod
    def _check(powers):
        assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 2
        assert powers.stride(1) == 1

    def raw(self, powers, nfft, dt):
        """Device-side search of whitened powers [D, nn] over the whole
        ladder; returns (cands int32 [max_cands, 6] = row, log2 L, lo, q,
        harmonics, power bits; count tensor) without synchronising."""
        self._check(powers)
        D, nn = powers.shape
        cands = torch.empty((self.max_cands, 6), dtype=torch.int32, device=powers.device)
        count = torch.zeros(1, dtype=torch.int64, device=powers.device)
        rlo = self.rlo(nfft, dt)
        for e in self.log2s:
            if D and nseg(nn, rlo, 1 << e, self.shift):
                self._search(powers, rlo, e, None, cands, self.max_cands, count)
        return cands, count

    def mini(self, powers, nfft, dt, L):
        """The normalised mini spectra [D, nseg, L] float32 of length ``L``
        (for tests and inspection; no candidates are kept)."""
        self._check(powers)
        e = _log2(L, "L")
        D, nn = powers.shape
        rlo = self.rlo(nfft, dt)
        out = torch.empty((D, nseg(nn, rlo, L, self.shift), int(L)), dtype=torch.float32,
                          device=powers.device)
        count = torch.zeros(1, dtype=torch.int64, device=powers.device)
        if out.numel():
            self._search(powers, rlo, e, out, None, 0, count)
        return out

    def collect(self, cands, count, dms, nfft, dt, row0=0):
        """Device (cands, count) -> sorted candidate records (synchronises)."""
        k = int(count.item())
        if k > self.max_cands:
            raise RuntimeError("sideband search: %d candidates exceed max_cands=%d "
                               "(raise the threshold or max_cands)" % (k, self.max_cands))
        return to_records(cands[:k].cpu().numpy(), dms, nfft, dt, row0)

    def tap(self, dms, dt, parts):
        """A ``tap`` for the ``__call__`` of the periodicity, acceleration or
        jerk search: every batch of whitened powers they make is searched
        here too and its records appended to the list ``parts``
        (``merge(parts)`` afterwards)."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))

        def search(powers, row0, nfft):
            c, k = self.raw(powers, nfft, dt)
            parts.append(self.collect(c, k, dms, nfft, dt, row0=row0))
        return search

    def __call__(self, plane, dms, dt, row_batch=None, nfft=None, zap=None):
        """``zap``: a ``pypulsar_amd.zap.Zaplist`` whose bins are set to the
        whitened mean level in every row before the search (None: nothing is
        zapped)."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        nfft = self.ps.default_nfft(n) if nfft is None else int(nfft)
        step = self.ps.row_batch(nfft) if row_batch is None else int(row_batch)
        assert step >= 1
        if zap is not None:
            from . import zap as _zap
            zbins = _zap.device_bins(zap.bins(nfft, dt, nfft // 2), nfft // 2, plane.device)
        parts = []
        for r0 in range(0, D, step):
            spec = self.ps.spectrum(plane[r0:r0 + step], nfft)
            powers = self.ps.normalise(spec)
            del spec
            if zap is not None:
                _zap.apply(powers, zbins)
            c, k = self.raw(powers, nfft, dt)
            parts.append(self.collect(c, k, dms, nfft, dt, row0=r0))
            del powers, c, k
        return merge(parts)


def to_records(c, dms, nfft, dt, row0=0):
    """int32 [k, 6] (row, log2 L, lo, q, harmonics, power bits) -> sorted
    CAND_DTYPE records: ``porb = q nfft dt / (2 L)``; ``freq_lo``, ``freq_hi``
    and ``freq`` the edges ``lo``, ``lo + L`` and the centre of the segment in
    Hz; ``row0`` is the plane row of the searched batch's row 0."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 6)
    out = np.empty(len(c), dtype=CAND_DTYPE)
    T = float(nfft) * float(dt)
    out["row"] = c[:, 0] + int(row0)
    out["DM"] = np.asarray(dms, dtype=np.float64)[out["row"]] if len(c) else []
    out["L"] = 1 << c[:, 1].astype(np.int64)
    out["lo"] = c[:, 2]
    out["q"] = c[:, 3]
    out["numharm"] = c[:, 4]
    out["power"] = c[:, 5].view(np.float32)
    L = out["L"].astype(np.float64)
    out["freq_lo"] = out["lo"] / T
    out["freq_hi"] = (out["lo"] + L) / T
    out["freq"] = (out["lo"] + 0.5 * L) / T
    out["porb"] = out["q"] * T / (2.0 * L) if len(c) else []
    sig = np.empty(len(c), dtype=np.float64)
    for h in np.unique(out["numharm"]):
        m = out["numharm"] == h
        sig[m] = _per.sigma(out["power"][m].astype(np.float64), int(h))
    out["sigma"] = sig
    return np.sort(out, order=_ORDER)


def merge(parts):
    """Concatenate candidate arrays of several row batches, sorted by (row, L,
    lo, numharm, q)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=CAND_DTYPE)
    return np.sort(np.concatenate(parts), order=_ORDER)


# ---- sifting and .bincands files (host) ----

def sift(cands, min_dms=1, max_ratio=4):
    """Group candidate records across rows, lengths, segments and stages.  Two
    are the same signal when their bin ranges ``[lo, lo + L)`` overlap and their
    ``porb`` agree within one half-bin step of the shorter segment, ``nfft dt /
    (2 min(L1, L2))`` -- directly, or after one of them is multiplied by an
    integer 2..``max_ratio`` (a harmonic of the comb).  In order of descending
    sigma a candidate is absorbed into the first stronger one it matches; the
    kept ones gain ``nhits`` (members, itself included) and ``ndms`` (their
    distinct rows); those seen in fewer than ``min_dms`` rows are dropped.
    Returns SIFTED_DTYPE records by descending sigma."""
    cands = np.asarray(cands)
    order = np.argsort(-cands["sigma"], kind="stable")
    kept, rows = [], []
    k_lo, k_hi, k_porb, k_step = (np.empty(0) for _ in range(4))
    m = np.arange(1, int(max_ratio) + 1, dtype=np.float64)
    for i in order:
        c = cands[i]
        lo, L, porb = float(c["lo"]), float(c["L"]), float(c["porb"])
        own = porb / float(c["q"])  # porb = q T / (2 L): one half-bin step of its segment
        j = -1
        if kept:
            # (the shorter segment's step is the larger; a part in 1e9 for rounding)
            step = np.maximum(k_step, own)[:, None] * (1.0 + 1e-9)
            overlap = (k_lo < lo + L) & (lo < k_hi)
            a = k_porb[:, None]
            near = np.any((np.abs(a - m[None, :] * porb) <= step) |
                          (np.abs(m[None, :] * a - porb) <= step), axis=1)
            hit = np.flatnonzero(overlap & near)
            if len(hit):
                j = int(hit[0])
        if j < 0:
            kept.append(i)
            rows.append([int(c["row"])])
            k_lo = np.append(k_lo, lo)
            k_hi = np.append(k_hi, lo + L)
            k_porb = np.append(k_porb, porb)
            k_step = np.append(k_step, own)
        else:
            rows[j].append(int(c["row"]))
    out = np.empty(len(kept), dtype=SIFTED_DTYPE)
    for name in CAND_DTYPE.names:
        out[name] = cands[name][kept] if len(kept) else []
    out["nhits"] = [len(r) for r in rows]
    out["ndms"] = [len(set(r)) for r in rows]
    return out[out["ndms"] >= int(min_dms)]


BINCANDS_HEADER = "# " + " ".join(BINCAND_DTYPE.names) + "   (freq in Hz, porb in s)\n"


def write_bincands(sifted, fn):
    """Write sifted candidates as ``<base>.bincands``: one line each, by
    descending sigma, of sigma, DM, centre frequency (Hz), the frequency range
    (Hz), porb (s), L, q, numharm, power, nhits, ndms -- every number in its
    shortest exact form, so ``read_bincands`` returns what was written."""
    s = np.asarray(sifted)
    s = s[np.argsort(-s["sigma"], kind="stable")]
    with open(fn, "w") as f:
        f.write(BINCANDS_HEADER)
        for c in s:
            f.write(" ".join(repr(c[n].item()) if BINCAND_DTYPE[n].kind == "f" and
                             BINCAND_DTYPE[n].itemsize == 8 else str(c[n])
                             for n in BINCAND_DTYPE.names) + "\n")


def read_bincands(fn):
    """Inverse of write_bincands: BINCAND_DTYPE records."""
    rows = []
    for line in open(fn):
        t = line.partition("#")[0].split()
        if t:
            assert len(t) == len(BINCAND_DTYPE.names), "%s: bad line %r" % (fn, line)
            rows.append(tuple(t))
    out = np.empty(len(rows), dtype=BINCAND_DTYPE)
    for i, n in enumerate(BINCAND_DTYPE.names):
        out[n] = [np.dtype(BINCAND_DTYPE[n]).type(r[i]) for r in rows] if rows else []
    return out


def write_bincands_npz(sifted, fn):
    """``<base>_bincands.npz``: the columns of the ``.bincands`` file, by
    descending sigma."""
    s = np.asarray(sifted)
    s = s[np.argsort(-s["sigma"], kind="stable")]
    np.savez(fn, **{n: np.asarray(s[n], dtype=BINCAND_DTYPE[n]) for n in BINCAND_DTYPE.names})
