"""Jerk search of DM-time planes in the Fourier domain: the (frequency,
frequency-derivative, second derivative) volume of every DM row, its harmonic
stages and candidates.

The acceleration search (``pypulsar_amd.accel``) assumes a constant frequency
derivative.  In a tight binary observed for a good part of its orbit the
line-of-sight acceleration changes: the frequency's second derivative moves
the signal by ``w = fdd T^3`` bins of 1/T, and the z-only templates lose it.
Here every DM row is correlated with templates on a grid of ``(z, w)``
(PRESTO's ``accelsearch -wmax``; kernels in pypulsar_amd/csrc/pdd_accel.hip
and pdd_jerk.hip, restated in tests/jerk_oracle.py):

* a unit signal of mid-observation frequency ``r`` (bins), mean drift ``z``
  and jerk ``w`` (both in bins of 1/T over the observation) has the
  coefficients ``W(k - r; z, w)`` with ``W(x; z, w) = int_0^1 exp(2 pi i [-x v
  + z (v^2 - v) / 2 + w (v^3 / 6 - v^2 / 4 + v / 12)]) dv`` (``w_response``):
  the cubic keeps ``r`` and ``z`` the MEAN frequency and drift (PRESTO's ``r0
  = r - z / 2 + w / 12``, ``z0 = z - w / 2``); ``W(x; z, 0)`` is
  ``accel.z_response``.  No closed form for w != 0: Gauss-Legendre quadrature
  in float64;
* ``template_bank`` holds the conjugate responses on the grid ``z_j = (j -
  J0) dz``, ``w_l = (l - L0) dw`` at whole and half bins, cut at ``hw_lj =
  ceil((|z_j| / 2 + |w_l| / 12 + 16) / eta)`` bins (the instantaneous
  frequency leaves ``r`` by at most ``|z| / 2 + |w| / 12``) and scaled as the
  acceleration search's; the slab ``w = 0`` IS ``accel.template_bank``;
* ``pdd_acc_correlate``, once per ``w`` slab, fills the volume ``P[l][d][j][i]``;
  ``pdd_jerk_search`` sums harmonics on the TOP harmonic's grid in both
  template axes and reports the local maxima (26 neighbours) of every stage
  above its threshold.

A candidate of stage ``H`` at cell ``(lc, jc, i)`` has the fundamental ``r = i
/ (2 H)``, ``z = jc dz / H`` and ``w = lc dw / H``.  Thresholds and
significance are those of the periodicity search.  No CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import accel as _acc
from . import periodicity as _per
from ._lib import call, ptr, stream_ptr

DEFAULT_HARMS = _acc.DEFAULT_HARMS
MAX_NW = 63                        # most w trials (kJrkMaxNw in pdd_jerk.hip)
DEFAULT_WORKSPACE_BYTES = 32 << 30  # default bound of __call__'s per-batch workspace
QUAD_NODES, QUAD_PANELS = 48, 128  # Gauss-Legendre nodes a panel, panels of [0, 1]

JERK_CAND_DTYPE = np.dtype(_acc.ACCEL_CAND_DTYPE.descr + [("w", "f8"), ("wbins", "f8"),
                                                          ("fdd", "f8"), ("jerk", "f8")])
_ORDER = ("row", "numharm", "r", "z", "w")


def _quadrature(nodes=QUAD_NODES, panels=QUAD_PANELS):
    """(v, weights) of the composite Gauss-Legendre rule on [0, 1]."""
    x, g = np.polynomial.legendre.leggauss(int(nodes))
    a = np.arange(int(panels), dtype=np.float64) / panels
    v = (a[:, None] + (x[None, :] + 1.0) / (2.0 * panels)).ravel()
    return v, np.tile(g / (2.0 * panels), int(panels))


def _template_phase(v, z, w):
    """The phase (cycles) of the template (z, w) at v, without the -x v term."""
    return 0.5 * z * (v * v - v) + w * (v * v * v / 6.0 - 0.25 * v * v + v / 12.0)


def _responses(x, zw, chunk=1024):
    """``W(x_e; z_t, w_t)`` complex128 [T, E] for positions ``x`` [E] and
    templates ``zw`` [T, 2] as ONE matrix product over the quadrature nodes:
    the node-by-position matrix ``exp(-2 pi i x_e v_m)`` is shared by every
    template (built ``chunk`` nodes at a time)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    zw = np.asarray(zw, dtype=np.float64).reshape(-1, 2)
    v, g = _quadrature()
    out = np.zeros((len(zw), len(x)), dtype=np.complex128)
    for m0 in range(0, len(v), chunk):
        vm, gm = v[m0:m0 + chunk], g[m0:m0 + chunk]
        G = gm[None, :] * np.exp(2j * np.pi * _template_phase(vm[None, :], zw[:, 0:1], zw[:, 1:2]))
        out += G @ np.exp(-2j * np.pi * vm[:, None] * x[None, :])
    return out


def w_response(x, z, w):
    """``W(x; z, w)`` (complex128): the Fourier coefficient, ``x`` bins of 1/T
    above its mid-observation frequency, of a unit signal of mean drift ``z``
    and jerk ``w`` (bins of 1/T).  w = 0: ``accel.z_response`` (closed form);
    otherwise composite Gauss-Legendre quadrature, 48 nodes on each of 128
    panels (5e-15 from the closed form at w = 0).
    ``W(x; -z, -w) = conj(W(-x; z, w))``; ``W(x; z, -w) = exp(-2 pi i x) W(-x;
    z, w)``."""
    x = np.asarray(x, dtype=np.float64)
    if float(w) == 0.0:
        return _acc.z_response(x, z)
    return _responses(x.ravel(), [(float(z), float(w))])[0].reshape(x.shape)


def w_grid(wmax, dw=20):
    """(w values float64 [nw], L0) of the grid ``w_l = (l - L0) dw``, ``L0 =
    wmax // dw``, ``nw = 2 L0 + 1``."""
    wmax, dw = int(wmax), int(dw)
    if dw < 1 or wmax < 0:
        raise ValueError("wmax must be >= 0 and dw >= 1")
    L0 = wmax // dw
    if 2 * L0 + 1 > MAX_NW:
        raise ValueError("wmax / dw gives %d w trials, more than %d" % (2 * L0 + 1, MAX_NW))
    return (np.arange(2 * L0 + 1, dtype=np.float64) - L0) * dw, L0


def half_widths(zs, ws, eta):
    """int32 [nw, nz]: ``ceil((|z_j| / 2 + |w_l| / 12 + 16) / eta)``."""
    return np.asarray([[int(math.ceil((abs(z) / 2.0 + abs(w) / 12.0 + 16.0) / eta)) for z in zs]
                       for w in ws], dtype=np.int32)


def template_bank(n, nfft, zmax, dz=2, wmax=0, dw=20):
    """(taps float32 [nw, nz, 2, 2 M + 1, 2], hw int32 [nw, nz], M) for rows of
    ``n`` samples padded to ``nfft``: ``taps[l, j, phi, M + e] = (re, im)`` of
    ``conj(W(eta (e - phi / 2); z_j, w_l))`` for ``|e| <= hw_lj``, 0 beyond out
    to the common ``M = max hw``, every (l, j, phi) set scaled so that ``sum
    |t|^2 = eta`` (as ``accel.template_bank``).  Computed in float64, rounded
    once.  The slab ``w_l = 0`` is ``accel.template_bank``'s, bit for bit."""
    n, nfft = int(n), int(nfft)
    if not 1 <= n <= nfft:
        raise ValueError("need 1 <= n <= nfft")
    eta = float(n) / float(nfft)
    zs, _ = _acc.z_grid(zmax, dz)
    ws, L0 = w_grid(wmax, dw)
    hw = half_widths(zs, ws, eta)
    M = int(hw.max())
    if M > _acc.MAX_HALF_WIDTH:
        raise ValueError("tap half-width %d exceeds %d (zmax or wmax too large for n / nfft = "
                         "%.3g)" % (M, _acc.MAX_HALF_WIDTH, eta))
    nw, nz = len(ws), len(zs)
    taps = np.zeros((nw, nz, 2, 2 * M + 1, 2), dtype=np.float32)
    t0, hw0, M0 = _acc.template_bank(n, nfft, zmax, dz)
    assert np.array_equal(hw0, hw[L0])
    taps[L0, :, :, M - M0:M + M0 + 1] = t0
    if nw > 1:
        e = np.arange(-M, M + 1, dtype=np.float64)
        x = eta * np.concatenate((e, e - 0.5))  # phi = 0, then phi = 1
        ls = [l for l in range(nw) if l != L0]
        zw = [(z, ws[l]) for l in ls for z in zs]
        R = np.conj(_responses(x, zw)).reshape(len(ls), nz, 2, 2 * M + 1)
        for a, l in enumerate(ls):
            for j in range(nz):
                h = int(hw[l, j])
                for phi in (0, 1):
                    t = R[a, j, phi, M - h:M + h + 1].copy()
                    t *= math.sqrt(eta / float(np.sum(t.real * t.real + t.imag * t.imag)))
                    taps[l, j, phi, M - h:M + h + 1, 0] = t.real
                    taps[l, j, phi, M - h:M + h + 1, 1] = t.imag
    return taps, hw, M


class JerkSearch(object):
    """``JerkSearch(sigma_threshold=6.0, zmax=50, wmax=100)(plane, dms, dt)`` ->
    candidates (JERK_CAND_DTYPE records).

    As ``accel.AccelSearch`` with a jerk axis: ``wmax``: the largest searched
    ``w = fdd T^3`` in bins of 1/T, on a grid of ``dw``.  ``wmax = 0`` gives
    the acceleration search's records with ``w = 0``.  ``workspace_bytes``
    bounds a row batch: the whole volume of a row, ``4 nw nz nfft`` bytes,
    must be resident (plus three stage slabs of ``4 nz nfft`` and the
    periodicity search's 24 bytes per padded sample).  All device work is
    queued on torch's current stream."""

    def __init__(self, sigma_threshold=6.0, zmax=50, wmax=100, dz=2, dw=20, harms=DEFAULT_HARMS,
                 flo=1.0, max_cands=1 << 20, initialbuflen=6, maxbuflen=200, ps=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        _lib.require_gpu()
        self.sigma_threshold = float(sigma_threshold)
        self.zmax, self.dz = int(zmax), int(dz)
        self.wmax, self.dw = int(wmax), int(dw)
        self.zs, self.J0 = _acc.z_grid(self.zmax, self.dz)
        self.ws, self.L0 = w_grid(self.wmax, self.dw)
        self.nz, self.nw = len(self.zs), len(self.ws)
        self.harms = _acc._harms(harms)
        self.max_cands = int(max_cands)
        self.workspace_bytes = int(workspace_bytes)
        self.ps = ps if ps is not None else _per.PeriodicitySearch(
            sigma_threshold, (1,), initialbuflen, maxbuflen, flo, max_cands)
        self.flo = float(flo) if ps is None else float(ps.flo)
        self.thr = np.asarray([_per.threshold_power(self.sigma_threshold, int(h))
                               for h in self.harms], dtype=np.float32)
        self._banks = {}

    def _bank(self, n, nfft, device):
        """Device taps, host half-widths and M, cached per (nfft, n, zmax, dz,
        wmax, dw), device and stream."""
        st = torch.cuda.current_stream(device)
        key = (int(nfft), int(n), self.zmax, self.dz, self.wmax, self.dw, str(device),
               st.cuda_stream)
        b = self._banks.get(key)
        if b is None:
            taps, hw, M = template_bank(n, nfft, self.zmax, self.dz, self.wmax, self.dw)
            b = (torch.from_numpy(taps).to(device), np.ascontiguousarray(hw), M)
            self._banks[key] = b
        return b

    def rlo(self, nfft, dt):
        return self.ps.rlo(nfft, dt)

    def correlate(self, spec, n=None):
        """Whitened complex spectrum [D, nn] (any row stride) of rows of ``n``
        samples padded to ``2 nn`` -> the volume [nw, D, nz, 2 nn] float32:
        one ``pdd_acc_correlate`` per w slab."""
        assert spec.is_cuda and spec.dtype == torch.complex64 and spec.dim() == 2
        assert spec.stride(1) == 1
        D, nn = spec.shape
        nfft = 2 * nn
        n = nfft if n is None else int(n)
        taps, hw, M = self._bank(n, nfft, spec.device)
        vol = torch.empty((self.nw, D, self.nz, 2 * nn), dtype=torch.float32, device=spec.device)
        if D:
            f = torch.view_as_real(spec)
            for l in range(self.nw):
                call("pdd_acc_correlate", ptr(f), D, nn, spec.stride(0), ptr(taps[l]),
                     hw[l].ctypes.data_as(ctypes.c_void_p), self.nz, M, ptr(vol[l]), stream_ptr())
        return vol

    def raw(self, vol, nfft, dt):
        """Device-side search of a volume [nw, D, nz, ni]; returns (cands int32
        [max_cands, 8] = row, i, jc, lc, harmonics, power bits, 0, 0; count
        tensor) without synchronising."""
        assert vol.is_cuda and vol.dtype == torch.float32 and vol.dim() == 4
        assert vol.is_contiguous() and vol.shape[0] == self.nw and vol.shape[2] == self.nz
        nw, D, nz, ni = vol.shape
        cands = torch.empty((self.max_cands, 8), dtype=torch.int32, device=vol.device)
        count = torch.zeros(1, dtype=torch.int64, device=vol.device)
        if D and ni:
            scratch = torch.empty(3 * D * nz * ni, dtype=torch.float32, device=vol.device)
            call("pdd_jerk_search", ptr(vol), D, nw, nz, ni,
                 self.harms.ctypes.data_as(ctypes.c_void_p), len(self.harms),
                 self.thr.ctypes.data_as(ctypes.c_void_p), self.rlo(nfft, dt), ptr(scratch),
                 scratch.numel(), ptr(cands), self.max_cands, ptr(count), stream_ptr())
            # (the launches are queued on the current stream, which the caching
            # allocator keeps the freed scratch on)
        return cands, count

    def collect(self, cands, count, dms, n, nfft, dt, row0=0):
        """Device (cands, count) -> sorted candidate records (synchronises)."""
        k = int(count.item())
        if k > self.max_cands:
            raise RuntimeError("jerk search: %d candidates exceed max_cands=%d "
                               "(raise the threshold or max_cands)" % (k, self.max_cands))
        return to_records(cands[:k].cpu().numpy(), dms, n, nfft, dt, self.dz, self.dw, row0)

    def row_bytes(self, nfft):
        """Workspace bytes of one row: the periodicity search's 20 bytes per
        padded sample, the whitened spectrum (4), the volume (4 nw nz) and the
        three stage slabs (12 nz)."""
        return (24 + 4 * self.nz * (self.nw + 3)) * int(nfft)

    def row_batch(self, nfft):
        """Rows per batch that keep the workspace within ``workspace_bytes``;
        ValueError when one row does not fit."""
        per = self.row_bytes(nfft)
        if per > self.workspace_bytes:
            raise ValueError(
                "jerk search: one row needs %d bytes (the volume alone 4 nw nz nfft = 4 x %d x %d "
                "x %d = %d), more than workspace_bytes = %d: reduce nfft, zmax (nz) or wmax (nw), "
                "or raise workspace_bytes" % (per, self.nw, self.nz, int(nfft),
                                              4 * self.nw * self.nz * int(nfft),
                                              self.workspace_bytes))
        return self.workspace_bytes // per

    def __call__(self, plane, dms, dt, row_batch=None, nfft=None, zap=None, tap=None):
        """``zap``, ``tap``: as for ``AccelSearch``."""
        dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
        D, n = plane.shape
        assert len(dms) == D, "one DM per plane row"
        nfft = self.ps.default_nfft(n) if nfft is None else int(nfft)
        step = self.row_batch(nfft)
        if row_batch is not None:
            step = int(row_batch)
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
            vol = self.correlate(white, n)
            c, k = self.raw(vol, nfft, dt)
            parts.append(self.collect(c, k, dms, n, nfft, dt, row0=r0))
            del white, vol, c, k
        return merge(parts)


def to_records(c, dms, n, nfft, dt, dz=2, dw=20, row0=0):
    """int32 [k, 8] (row, i, jc, lc, harmonics, power bits, 0, 0) -> sorted
    JERK_CAND_DTYPE records: the fields of ``accel.to_records`` (the same
    arithmetic) and the fundamental's ``w = lc dw / H`` (bins of 1/T, T = n
    dt), ``wbins = w nfft / n`` (bins of the padded spectrum), ``fdd = w /
    T^3`` and ``jerk = fdd c / freq`` (m / s^3)."""
    c = np.asarray(c, dtype=np.int32).reshape(-1, 8)
    out = np.empty(len(c), dtype=JERK_CAND_DTYPE)
    H = c[:, 4].astype(np.float64)
    T = float(n) * float(dt)
    out["row"] = c[:, 0] + int(row0)
    out["DM"] = np.asarray(dms, dtype=np.float64)[out["row"]] if len(c) else []
    out["r"] = c[:, 1] / (2.0 * H)
    out["freq"] = out["r"] / (float(nfft) * dt)
    out["period"] = 1.0 / out["freq"] if len(c) else []
    out["numharm"] = c[:, 4]
    out["power"] = c[:, 5].view(np.float32)
    out["z"] = c[:, 2] * float(dz) / H + 0.0
    out["zbins"] = out["z"] * float(nfft) / float(n)
    out["fd"] = out["z"] / (T * T)
    out["accel"] = out["fd"] * _acc.C_LIGHT / out["freq"] if len(c) else []
    out["w"] = c[:, 3] * float(dw) / H + 0.0
    out["wbins"] = out["w"] * float(nfft) / float(n)
    out["fdd"] = out["w"] / (T * T * T)
    out["jerk"] = out["fdd"] * _acc.C_LIGHT / out["freq"] if len(c) else []
    sig = np.empty(len(c), dtype=np.float64)
    for h in np.unique(out["numharm"]):
        m = out["numharm"] == h
        sig[m] = _per.sigma(out["power"][m].astype(np.float64), int(h))
    out["sigma"] = sig
    return np.sort(out, order=_ORDER)


def merge(parts):
    """Concatenate candidate arrays of several row batches, sorted by (row,
    numharm, r, z, w)."""
    parts = [p for p in parts if p is not None and len(p)]
    if not parts:
        return np.empty(0, dtype=JERK_CAND_DTYPE)
    return np.sort(np.concatenate(parts), order=_ORDER)
