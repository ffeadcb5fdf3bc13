"""Acceleration search of DM-time planes in the Fourier domain: the (frequency,
frequency-derivative) plane of every DM row, its harmonic stages and
candidates.

A pulsar in a binary drifts in frequency during the observation; a drift of
``z`` Fourier bins (of 1/T) spreads its power over about ``|z|`` bins and the
z = 0 search of ``pypulsar_amd.periodicity`` loses it.  Here the whitened
complex spectrum that search already produces is correlated with the
responses of drifting signals (kernels in pypulsar_amd/csrc/pdd_accel.hip,
restated in tests/accel_oracle.py):

* a signal of mid-observation frequency ``r`` (bins) and drift ``z`` has the
  coefficients ``W(k - r; z)`` with ``W(x; z) = int_0^1 exp(2 pi i [-x v + z
  (v^2 - v) / 2]) dv`` (``z_response``); z = 0 gives ``exp(-i pi x) sinc(x)``,
  the kernel of ``PrestoFFT.interpolate`` (formats/prestofft.py:76-96) with
  its sinc corrected;
* ``template_bank`` holds the conjugate responses on the grid ``z_j = (j -
  J0) dz`` at whole and half bins, cut at ``hw_j = ceil((|z_j| / 2 + 16) /
  eta)`` bins and scaled to keep the noise mean of the power at 1 on a zero
  padded spectrum (``eta = n / nfft``);
* ``pdd_acc_correlate`` gives the powers ``P[d][j][i]`` at half-bin positions
  ``r = i / 2``; ``pdd_acc_search`` sums harmonics on the TOP harmonic's grid
  and reports the local maxima of every stage above its threshold.

A candidate of stage ``H`` at cell ``(jc, i)`` has the fundamental ``r = i /
(2 H)`` and ``z = jc dz / H``.  Thresholds and significance are those of the
periodicity search (``2 S_H ~ chi2(2 H)``).  No CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import periodicity as _per
from ._lib import call, ptr, stream_ptr

DEFAULT_HARMS = (1, 2, 4, 8)
MAX_HARM = 16          # largest harmonic count of a stage (kAccMaxHarm in pdd_accel.hip)
MAX_HALF_WIDTH = 512   # largest tap half-width (kAccMaxM)
MAX_NZ = 255           # most z trials (kAccMaxNz)
C_LIGHT = 299792458.0  # m / s

ACCEL_CAND_DTYPE = np.dtype([("DM", "f8"), ("row", "i4"), ("r", "f8"), ("freq", "f8"),
                             ("period", "f8"), ("numharm", "i4"), ("power", "f4"),
                             ("sigma", "f8"), ("z", "f8"), ("zbins", "f8"), ("fd", "f8"),
                             ("accel", "f8")])
_ORDER = ("row", "numharm", "r", "z")


def z_response(x, z):
    """``W(x; z)`` (complex128): the Fourier coefficient, ``x`` bins of 1/T
    above its mid-observation frequency, of a unit signal that drifts ``z``
    bins over the observation.  z = 0: ``exp(-i pi x) sinc(x)``.  z > 0: the
    phase is ``pi z (v - q)^2 - pi z q^2`` with ``q = (x + z / 2) / z``, so
    with ``u = sqrt(2 z) (v - q)`` the integral is ``exp(-i pi z q^2) / sqrt(2
    z)`` times ``C(u) + i S(u)`` between ``u(0)`` and ``u(1)`` (Fresnel
    integrals); z < 0: ``conj(W(-x; -z))``."""
    from scipy.special import fresnel
    x = np.asarray(x, dtype=np.float64)
    z = float(z)
    if z == 0.0:
        return np.exp(-1j * np.pi * x) * np.sinc(x)
    if z < 0.0:
        return np.conj(z_response(-x, -z))
    a = math.sqrt(2.0 * z)
    q = (x + 0.5 * z) / z
    s1, c1 = fresnel(a * (1.0 - q))
    s0, c0 = fresnel(-a * q)
    return np.exp(-1j * np.pi * z * q * q) * ((c1 - c0) + 1j * (s1 - s0)) / a


def z_grid(zmax, dz=2):
    """(z values float64 [nz], J0) of the grid ``z_j = (j - J0) dz``, ``J0 =
    zmax // dz``, ``nz = 2 J0 + 1``."""
    zmax, dz = int(zmax), int(dz)
    if dz < 1 or zmax < 0:
        raise ValueError("zmax must be >= 0 and dz >= 1")
    J0 = zmax // dz
    if 2 * J0 + 1 > MAX_NZ:
        raise ValueError("zmax / dz gives %d z trials, more than %d" % (2 * J0 + 1, MAX_NZ))
    return (np.arange(2 * J0 + 1, dtype=np.float64) - J0) * dz, J0


def template_bank(n, nfft, zmax, dz=2):
    """(taps float32 [nz, 2, 2 M + 1, 2], hw int32 [nz], M) for rows of ``n``
    samples padded to ``nfft``: ``taps[j, phi, M + e] = (re, im)`` of
    ``conj(W(eta (e - phi / 2); z_j))`` for ``|e| <= hw_j``, 0 beyond, every
    (j, phi) set scaled so that ``sum |t|^2 = eta`` (neighbouring bins of a
    zero padded spectrum are correlated: this keeps the noise mean of the
    correlated power at 1).  Computed in float64, rounded once."""
    n, nfft = int(n), int(nfft)
    if not 1 <= n <= nfft:
        raise ValueError("need 1 <= n <= nfft")
    eta = float(n) / float(nfft)
    zs, _ = z_grid(zmax, dz)
    hw = np.asarray([int(math.ceil((abs(z) / 2.0 + 16.0) / eta)) for z in zs], dtype=np.int32)
    M = int(hw.max())
    if M > MAX_HALF_WIDTH:
        raise ValueError("tap half-width %d exceeds %d (zmax too large for n / nfft = %.3g)"
                         % (M, MAX_HALF_WIDTH, eta))
    t = np.zeros((len(zs), 2, 2 * M + 1), dtype=np.complex128)
    for j, z in enumerate(zs):
        e = np.arange(-int(hw[j]), int(hw[j]) + 1, dtype=np.float64)
        for phi in (0, 1):
            w = np.conj(z_response(eta * (e - 0.5 * phi), z))
            w *= math.sqrt(eta / float(np.sum(w.real * w.real + w.imag * w.imag)))
            t[j, phi, M - hw[j]:M + hw[j] + 1] = w
    taps = np.ascontiguousarray(np.stack((t.real, t.imag), axis=-1).astype(np.float32))
    return taps, hw, M


def _harms(harms):
    h = np.ascontiguousarray(np.asarray(harms, dtype=np.int32))
    assert h.ndim == 1 and 1 <= len(h) <= 8, "1..8 harmonic stages"
    assert np.all(h >= 1) and np.all(h <= MAX_HARM), "harmonic counts must be in 1..%d" % MAX_HARM
    assert np.all(np.diff(h) > 0), "harms must ascend"
    return h


class AccelSearch(object):
    """``AccelSearch(sigma_threshold=6.0, zmax=50)(plane, dms, dt)`` ->
    candidates (ACCEL_CAND_DTYPE records).

    ``plane``, ``dms``, ``dt`` as for ``PeriodicitySearch``; ``zmax``: largest
    searched drift in bins of 1/T (``z = fd T^2``), on a grid of ``dz``;
    ``harms``: the harmonic stages (each 1..16).  ``ps``: the
    ``PeriodicitySearch`` whose prep, FFT and whitening are used (it is
    neither copied nor changed; default: one made with ``initialbuflen``,
    ``maxbuflen`` and ``flo``).  All device work is queued on torch's current
    stream."""

    def __init__(self, sigma_threshold=6.0, zmax=50, dz=2, harms=DEFAULT_HARMS, flo=1.0,
                 max_cands=1 << 20, initialbuflen=6, maxbuflen=200, ps=None):
        _lib.require_gpu()
        self.sigma_threshold = float(sigma_threshold)
        self.zmax, self.dz = int(zmax), int(dz)
        self.zs, self.J0 = z_grid(self.zmax, self.dz)
        self.nz = len(self.zs)
        self.harms = _harms(harms)
        self.max_cands = int(max_cands)
        self.ps = ps if ps is not None else _per.PeriodicitySearch(
            sigma_threshold, (1,), initialbuflen, maxbuflen, flo, max_cands)
        self.flo = float(flo) if ps is None else float(ps.flo)
        # float32 thresholds: the comparison the kernel (and the oracle) makes
        self.thr = np.asarray([_per.threshold_power(self.sigma_threshold, int(h))
                               for h in self.harms], dtype=np.float32)
        self._banks = {}

    def _bank(self, n, nfft, device):
        """Device taps, host half-widths and M, cached per (nfft, n, zmax, dz)
        and per stream, as ``PeriodicitySearch._table``."""
        st = torch.cuda.current_stream(device)
        key = (int(nfft), int(n), self.zmax, self.dz, str(device), st.cuda_stream)
        b = self._banks.get(key)
        if b is None:
            taps, hw, M = template_bank(n, nfft, self.zmax, self.dz)
            b = (torch.from_numpy(taps).to(device), hw, M)
            self._banks[key] = b
        return b

    def rlo(self, nfft, dt):
        return self.ps.rlo(nfft, dt)

    def correlate(self, spec, n=None):
        """Whitened complex spectrum [D, nn] (``PeriodicitySearch.normalise(...,
        want_spectrum=True)``; any row stride) of rows of ``n`` samples padded
        to ``2 nn`` (default: no padding) -> powers [D, nz, 2 nn] float32."""
        assert spec.is_cuda and spec.dtype == torch.complex64 and spec.dim() == 2
        assert spec.stride(1) == 1
        D, nn = spec.shape
        nfft = 2 * nn
        n = nfft if n is None else int(n)
        taps, hw, M = self._bank(n, nfft, spec.device)
        powers = torch.empty((D, self.nz, 2 * nn), dtype=torch.float32, device=spec.device)
        if D:
            call("pdd_acc_correlate", ptr(torch.view_as_real(spec)), D, nn, spec.stride(0),
                 ptr(taps), hw.ctypes.data_as(ctypes.c_void_p), self.nz, M, ptr(powers),
                 stream_ptr())
        return powers

    def raw(self, powers, nfft, dt):
        """Device-side search of powers [D, nz, ni]; returns (cands int32
        [max_cands, 6] = row, i, jc, harmonics, power bits, 0; count tensor)
        without synchronising."""
        assert powers.is_cuda and powers.dtype == torch.float32 and powers.dim() == 3
        assert powers.is_contiguous() and powers.shape[1] == self.nz
        D, nz, ni = powers.shape
        cands = torch.empty((self.max_cands, 6), dtype=torch.int32, device=powers.device)
        count = torch.zeros(1, dtype=torch.int64, device=powers.device)
        if D and ni:
            call("pdd_acc_search", ptr(powers), D, nz, ni,
                 self.harms.ctypes.data_as(ctypes.c_void_p), len(self.harms),
                 self.thr.ctypes.data_as(ctypes.c_void_p), self.rlo(nfft, dt), ptr(cands),
                 self.max_cands, ptr(count), stream_ptr())
        return cands, count

    def collect(self, cands, count, dms, n, nfft, dt, row0=0):
        """Device (cands, count) -> sorted candidate records (synchronises)."""
        k = int(count.item())
        if k > self.max_cands:
            raise RuntimeError("acceleration search: %d candidates exceed max_cands=%d "
                               "(raise the threshold or max_cands)" % (k, self.max_cands))
        return to_records(cands[:k].cpu().numpy(), dms, n, nfft, dt, self.dz, row0)

    def row_batch(self, nfft):
        """Rows per batch that keep the workspace -- the periodicity search's
        20 bytes per padded sample, the whitened spectrum (4) and the powers
        volume (4 nz) -- within the periodicity search's WORKSPACE_BYTES."""
        return max(1, _per.WORKSPACE_BYTES // ((24 + 4 * self.nz) * int(nfft)))

    def __call__(self, plane, dms, dt, row_batch=None, nfft=None, zap=None, tap=None):
        """``zap``: a ``pypulsar_amd.zap.Zaplist`` whose bins of the whitened
        spectrum are set to the whitened mean level in every row before the
        correlation (None: nothing is zapped).  ``tap``: as for
        ``PeriodicitySearch``."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        nfft = self.ps.default_nfft(n) if nfft is None else int(nfft)
        step = self.row_batch(nfft) if row_batch is None else int(row_batch)
        assert step >= 1
        if zap is not None:
            from . import zap as _zap
            zbins = _zap.device_bins(zap.bins(nfft, dt, nfft // 2), nfft // 2, plane.device)
        parts = []
        for r0 in range(0, D, step):
            spec = self.ps.spectrum(plane[r0:r0 + step], nfft)
            wpow, white = self.ps.normalise(spec, want_spectrum=True)
            del spec
            if zap is not None:
                _zap.apply(wpow, zbins, white)
            if tap is not None:
                tap(wpow, r0, nfft)
            del wpow
            powers = self.correlate(white, n)
            c, k = self.raw(powers, nfft, dt)
            parts.append(self.collect(c, k, dms, n, nfft, dt, row0=r0))
            del white, powers, c, k
        return merge(parts)


def to_records(c, dms, n, nfft, dt, dz=2, row0=0):
    """int32 [k, 6] (row, i, jc, harmonics, power bits, 0) -> sorted
    ACCEL_CAND_DTYPE records: the fundamental's ``r = i / (2 H)`` (bins of the
    padded spectrum) and ``z = jc dz / H`` (bins of 1/T, T = n dt);
    ``zbins = z nfft / n`` the drift in bins of the padded spectrum; ``freq =
    r / (nfft dt)`` the mid-observation frequency; ``fd = z / T^2``; ``accel
    = fd c / freq`` (m / s^2)."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 6)
    out = np.empty(len(c), dtype=ACCEL_CAND_DTYPE)
    H = c[:, 3].astype(np.float64)
    T = float(n) * float(dt)
    out["row"] = c[:, 0] + int(row0)
    out["DM"] = np.asarray(dms, dtype=np.float64)[out["row"]] if len(c) else []
    out["r"] = c[:, 1] / (2.0 * H)
    out["freq"] = out["r"] / (float(nfft) * dt)
    out["period"] = 1.0 / out["freq"] if len(c) else []
    out["numharm"] = c[:, 3]
    out["power"] = c[:, 4].view(np.float32)
    out["z"] = c[:, 2] * float(dz) / H + 0.0
    out["zbins"] = out["z"] * float(nfft) / float(n)
    out["fd"] = out["z"] / (T * T)
    out["accel"] = out["fd"] * C_LIGHT / out["freq"] if len(c) else []
    sig = np.empty(len(c), dtype=np.float64)
    for h in np.unique(out["numharm"]):
        m = out["numharm"] == h
        sig[m] = _per.sigma(out["power"][m].astype(np.float64), int(h))
    out["sigma"] = sig
    return np.sort(out, order=_ORDER)


def merge(parts):
    """Concatenate candidate arrays of several row batches, sorted by (row,
    numharm, r, z)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=ACCEL_CAND_DTYPE)
    return np.sort(np.concatenate(parts), order=_ORDER)
