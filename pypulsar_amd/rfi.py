"""RFI excision before dedispersion: rfifind-style statistics of the raw
block on the device, the host-side mask decision, PRESTO ``.mask`` output and
the in-place replacement of masked cells in the streaming path.

The reference reads ``.mask`` files (bin/waterfaller.py:28-48 through PRESTO's
rfifind module, restated in formats/rfifind.py) but cannot make one; PRESTO's
own clipping rule is not available, so the rule below is this project's
(DESIGN.md §6g), restated independently in tests/rfi_oracle.py.

The time-major block x[t][c] is cut into intervals of ``ptsperint`` samples.
Per (interval, channel) cell, over its N = ptsperint samples:

* ``avg``: the mean; ``std``: the population standard deviation -- for 8-bit
  data from exact integer sums (bit-reproducible), for float32 from float64
  sums;
* ``pow``: ``max_{k=1..N/2} |rfft(x - avg)[k]|^2 / (N var)``, 0 where var == 0:
  the largest normalised Fourier power (mean 1 for white noise).

``decide`` (float64 NumPy on the nint x C arrays; not hot) flags cells:

1. ``bad = pow > pthr or std == 0`` with ``pthr = -ln(1 - (1 - Q(freq_sig))^(1/nb))``,
   nb = N // 2: the power a ``freq_sig`` sigma event among nb exponential bins
   reaches (Q: the one-sided normal tail);
2. per channel, over the intervals not ``bad``: median and 1.4826 MAD of
   ``avg`` and of ``std``; a cell whose avg or std deviates from the median
   by more than ``time_sig`` scatters is flagged;
3. per channel m_c = median over its unflagged intervals of ``std``, compared
   with the median and 1.4826 MAD of m over channels c - chan_window .. c +
   chan_window (clipped at the band edges; undefined m left out): the whole
   channel is flagged beyond ``chan_sig`` scatters, or when m_c is undefined;
4. channels flagged in more than ``chantrigfrac`` of the intervals are
   zapped everywhere;
5. intervals flagged in more than ``inttrigfrac`` of the channels are zapped
   entirely.

Channel numbers are the columns of the raw block (file order), as
bin/waterfaller.py applies a mask.  No CPU fallback for the device steps.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .formats import rfifind as _fmt

WORKSPACE_BYTES = 1 << 30  # default bound of stats()'s per-batch rows + spectrum
MAD_SCALE = 1.4826
_CODES = {torch.uint8: _lib.U8, torch.float32: _lib.F32}
_TILE = {torch.uint8: 128, torch.float32: 32}  # channels per k_rfi_prep workgroup


def power_threshold(freq_sig, ptsperint):
    """-ln(1 - (1 - Q(freq_sig))^(1 / nb)), nb = ptsperint // 2."""
    nb = ptsperint // 2
    q = 0.5 * math.erfc(freq_sig / math.sqrt(2.0))
    return -math.log(-math.expm1(math.log1p(-q) / nb))


def _median_scatter(v):
    med = np.median(v)
    return med, MAD_SCALE * np.median(np.abs(v - med))


def decide(avg, std, pow, ptsperint, time_sig=10.0, freq_sig=4.0, chan_sig=6.0, chan_window=16,
           chantrigfrac=0.7, inttrigfrac=0.3):
    """bool [nint, C] mask (True = zapped) from the cell statistics; the rule
    of the module docstring, in float64."""
    avg = np.asarray(avg, dtype=np.float64)
    std = np.asarray(std, dtype=np.float64)
    pow = np.asarray(pow, dtype=np.float64)
    nint, C = avg.shape
    if nint == 0:
        return np.zeros((0, C), dtype=bool)
    bad = (pow > power_threshold(freq_sig, ptsperint)) | (std == 0)
    flag = bad.copy()
    for c in range(C):
        ok = ~bad[:, c]
        if not ok.any():
            continue
        for v in (avg[:, c], std[:, c]):
            med, scat = _median_scatter(v[ok])
            flag[:, c] |= np.abs(v - med) > time_sig * scat
    m = np.full(C, np.nan)
    for c in range(C):
        ok = ~flag[:, c]
        if ok.any():
            m[c] = np.median(std[ok, c])
    for c in range(C):
        w = m[max(0, c - chan_window):min(C, c + chan_window + 1)]
        w = w[~np.isnan(w)]
        if np.isnan(m[c]):
            flag[:, c] = True
            continue
        med, scat = _median_scatter(w)
        if abs(m[c] - med) > chan_sig * scat:
            flag[:, c] = True
    flag[:, flag.sum(axis=0) > chantrigfrac * nint] = True
    flag[flag.sum(axis=1) > inttrigfrac * C, :] = True
    return flag


def channel_fill(avg, mask):
    """Per-channel replacement value: the median over the unflagged intervals
    of ``avg``; the band median of those where a channel has none."""
    avg = np.asarray(avg, dtype=np.float64)
    C = avg.shape[1]
    fill = np.full(C, np.nan)
    for c in range(C):
        ok = ~mask[:, c]
        if ok.any():
            fill[c] = np.median(avg[ok, c])
    good = fill[~np.isnan(fill)]
    fill[np.isnan(fill)] = np.median(good) if good.size else 0.0
    return fill


class RFIMask(object):
    """A decided mask: bool ``mask`` [nint, C] (True = zapped), ``ptsperint``,
    the per-channel ``fill`` and the ``.mask`` header fields."""

    def __init__(self, mask, ptsperint, fill, time_sig=10.0, freq_sig=4.0, mjd=0.0, dtint=None,
                 lofreq=1250.0, df=1.0, tsamp=1.0):
        self.mask = np.ascontiguousarray(mask, dtype=bool)
        assert self.mask.ndim == 2
        self.nint, self.nchan = self.mask.shape
        self.ptsperint = int(ptsperint)
        self.fill = np.asarray(fill, dtype=np.float64).reshape(self.nchan).copy()
        self.time_sig, self.freq_sig, self.mjd = float(time_sig), float(freq_sig), float(mjd)
        self.dtint = float(self.ptsperint * tsamp if dtint is None else dtint)
        self.lofreq, self.df = float(lofreq), float(df)
        self._dev = {}

    @property
    def masked_fraction(self):
        return float(self.mask.mean()) if self.mask.size else 0.0

    def zap_chans(self):
        """Channels zapped in every interval."""
        return np.flatnonzero(self.mask.all(axis=0)) if self.nint else np.zeros(0, dtype=np.intp)

    def zap_ints(self):
        """Intervals zapped in every channel."""
        return np.flatnonzero(self.mask.all(axis=1))

    def write(self, fn):
        _fmt.write_mask(fn, self.nchan, self.ptsperint,
                        [np.flatnonzero(row) for row in self.mask],
                        zap_chans=[int(c) for c in self.zap_chans()],
                        zap_ints=[int(i) for i in self.zap_ints()],
                        time_sig=self.time_sig, freq_sig=self.freq_sig, mjd=self.mjd,
                        dtint=self.dtint, lofreq=self.lofreq, df=self.df)

    @classmethod
    def from_file(cls, fn, fill=None):
        """The mask of a ``.mask`` file.  The format stores no replacement
        values: pass ``fill`` ([C]) or set them later (``set_fill``,
        ``fill_from_block``); the default is 0."""
        r = _fmt.rfifind(fn)
        mask = np.zeros((r.nint, r.nchan), dtype=bool)
        for i, z in enumerate(r.mask_zap_chans_per_int):
            mask[i, np.asarray(z, dtype=np.intp)] = True
        return cls(mask, r.ptsperint, np.zeros(r.nchan) if fill is None else fill,
                   time_sig=r.time_sig, freq_sig=r.freq_sig, mjd=r.MJD, dtint=r.dtint,
                   lofreq=r.lofreq, df=r.df)

    def set_fill(self, fill):
        self.fill = np.asarray(fill, dtype=np.float64).reshape(self.nchan).copy()
        self._dev = {k: v for k, v in self._dev.items() if k[0] == "bitmap"}

    def fill_from_block(self, block, t0=0):
        """Replacement values from a device block [n, C] that starts at
        sample ``t0`` (a multiple of ptsperint): the median of the unflagged
        intervals' means (the block's channel means if it holds no interval)."""
        assert t0 % self.ptsperint == 0
        avg, _, _ = RFIFind(self.ptsperint).stats(block, power=False)
        if avg.shape[0] == 0:
            self.set_fill(block.double().mean(dim=0).cpu().numpy())
            return
        i0 = t0 // self.ptsperint
        sub = np.ones(avg.shape, dtype=bool)
        k = max(0, min(avg.shape[0], self.nint - i0))
        sub[:k] = self.mask[i0:i0 + k]
        sub[k:] = False
        self.set_fill(channel_fill(avg.cpu().numpy(), sub))

    def to_device(self, device="cuda"):
        """Packed bitmap int32 [nint, ceil(C / 32)]: bit c % 32 of word c // 32."""
        key = ("bitmap", str(device))
        if key not in self._dev:
            W = -(-self.nchan // 32)
            bits = np.zeros((self.nint, W * 32), dtype=np.uint8)
            bits[:, :self.nchan] = self.mask
            packed = np.packbits(bits, axis=1, bitorder="little")
            words = np.ascontiguousarray(packed).view("<u4").astype(np.uint32)
            self._dev[key] = torch.from_numpy(words.view(np.int32).reshape(self.nint, W)).to(device)
        return self._dev[key]

    def fill_device(self, dtype, device="cuda"):
        """``fill`` in the data's type on the device (rounded for 8 bits)."""
        key = ("fill", str(device), dtype)
        if key not in self._dev:
            if dtype == torch.uint8:
                f = np.clip(np.rint(self.fill), 0, 255).astype(np.uint8)
            else:
                f = self.fill.astype(np.float32)
            self._dev[key] = torch.from_numpy(f).to(device)
        return self._dev[key]

    def apply(self, block, t0=0, stream=None):
        """Replace, in place, the masked samples of the time-major device
        block [n, C] (8-bit or float32) whose first row is sample ``t0``."""
        if block.dtype not in _CODES:
            raise TypeError("RFIMask.apply: 8-bit or float32 blocks only, got %s" % block.dtype)
        assert block.is_cuda and block.dim() == 2 and block.shape[1] == self.nchan
        assert block.stride(1) == 1 or block.shape[1] == 1
        n = block.shape[0]
        if n == 0 or self.nint == 0:
            return block
        call("pdd_rfi_apply", ptr(block), _CODES[block.dtype], n, self.nchan, block.stride(0),
             int(t0), self.ptsperint, ptr(self.to_device(block.device)), self.nint,
             ptr(self.fill_device(block.dtype, block.device)), stream_ptr(stream))
        return block


class RFIFind(object):
    """``RFIFind(ptsperint).find(chunks)`` -> RFIMask.  ``stats(block)`` gives
    the device statistics of one block, ``accumulate(chunks)`` those of a
    whole stream (host float64), ``decide`` the mask."""

    def __init__(self, ptsperint, time_sig=10.0, freq_sig=4.0, chan_sig=6.0, chan_window=16,
                 chantrigfrac=0.7, inttrigfrac=0.3, workspace_bytes=WORKSPACE_BYTES):
        self.ptsperint = int(ptsperint)
        if self.ptsperint < 16:
            raise ValueError("ptsperint must be >= 16")
        self.time_sig, self.freq_sig, self.chan_sig = float(time_sig), float(freq_sig), float(chan_sig)
        self.chan_window = int(chan_window)
        self.chantrigfrac, self.inttrigfrac = float(chantrigfrac), float(inttrigfrac)
        self.workspace_bytes = int(workspace_bytes)

    def chan_batch(self, nint, C, dtype):
        """Channels per batch that keep the workspace (float rows + complex
        spectrum, ~8 bytes a sample) within ``workspace_bytes``: whole
        k_rfi_prep tiles, at least one."""
        P = self.ptsperint
        per_chan = nint * (4 * P + 8 * (P // 2 + 1) + 8)
        tile = _TILE[dtype]
        g = self.workspace_bytes // max(per_chan, 1) // tile * tile
        return int(min(C, max(tile, g)))

    def stats(self, block, power=True, stream=None):
        """Device float64 (avg, std, pow), [nint, C] each, of the whole
        intervals of the time-major device block [T, C] (8-bit or float32, any
        row stride); nint = T // ptsperint, the ragged tail is ignored.
        ``power=False`` skips the Fourier step (pow is None)."""
        _lib.require_gpu()
        if block.dtype not in _CODES:
            raise TypeError("RFIFind.stats: 8-bit or float32 blocks only, got %s" % block.dtype)
        assert block.is_cuda and block.dim() == 2 and (block.stride(1) == 1 or block.shape[1] == 1)
        T, C = block.shape
        P = self.ptsperint
        nint = T // P
        dev = block.device
        avg = torch.empty((nint, C), dtype=torch.float64, device=dev)
        std = torch.empty_like(avg)
        pw = torch.empty_like(avg) if power else None
        if nint == 0 or C == 0:
            return avg, std, pw
        G = self.chan_batch(nint, C, block.dtype)
        rows = torch.empty((min(G, C) * nint, P), dtype=torch.float32, device=dev)
        nvar = torch.empty(min(G, C) * nint, dtype=torch.float64, device=dev)
        # (torch.fft.rfft runs on torch's current stream)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            for c0 in range(0, C, G):
                nc = min(G, C - c0)
                call("pdd_rfi_stats_prep", ptr(block), _CODES[block.dtype], nint, C,
                     block.stride(0), P, c0, nc, ptr(rows), ptr(avg), ptr(std), ptr(nvar),
                     stream_ptr(stream))
                if not power:
                    continue
                spec = torch.fft.rfft(rows[:nc * nint], dim=1)
                sr = torch.view_as_real(spec)
                assert sr.is_contiguous()
                call("pdd_rfi_stats_power", ptr(sr), nc * nint, P, ptr(nvar), nint, C, c0, ptr(pw),
                     stream_ptr(stream))
                del spec, sr
        return avg, std, pw

    def accumulate(self, chunks):
        """Whole-stream statistics: host float64 (avg, std, pow), [nint, C]
        each, of the concatenated chunks ([n, C], pinned host or device; every
        chunk at most as long as the first).  Chunks are copied on a copy
        stream into two rotating device buffers, guarded by events, while the
        previous chunk's statistics run; the samples past a chunk's last whole
        interval are carried into the next chunk's buffer."""
        _lib.require_gpu()
        P = self.ptsperint
        off = -(-(P - 1) // 16) * 16  # rows kept free in front of a chunk for the carry
        cur = torch.cuda.current_stream()
        dev = torch.device("cuda", torch.cuda.current_device())
        copy_stream = torch.cuda.Stream(device=dev)
        bufs, h2d, free = None, None, None
        carry, prev = 0, None  # rows carried over, the buffer they end in
        out = []
        C = None
        for i, chunk in enumerate(chunks):
            n = chunk.shape[0]
            if bufs is None:
                C, nmax = chunk.shape[1], n
                bufs = [torch.empty((off + nmax, C), dtype=chunk.dtype, device=dev)
                        for _ in range(2)]
                h2d = [torch.cuda.Event() for _ in range(2)]
                free = [torch.cuda.Event() for _ in range(2)]
                for e in free:
                    e.record(cur)
            assert chunk.shape[1] == C and n <= nmax, "chunks must not grow"
            b = i % 2
            buf = bufs[b]
            if i >= 2:
                # at most two copies in flight: a pinned chunk may be refilled
                # by the caller once two later chunks have been handed in
                h2d[b].synchronize()
            copy_stream.wait_event(free[b])
            with torch.cuda.stream(copy_stream):
                buf[off:off + n].copy_(chunk, non_blocking=True)
            h2d[b].record(copy_stream)
            if carry:
                pbuf, pend = prev
                buf[off - carry:off].copy_(pbuf[pend - carry:pend])
            if prev is not None:
                free[1 - b].record(cur)  # (the other buffer: its carry has been taken)
            cur.wait_event(h2d[b])
            total = carry + n
            if total >= P:
                out.append(self.stats(buf[off - carry:off + n]))
            carry = total % P
            prev = (buf, off + n)
        if prev is not None:
            torch.cuda.synchronize(dev)
        if not out:
            e = np.zeros((0, C or 0), dtype=np.float64)
            return e, e.copy(), e.copy()
        return tuple(torch.cat([o[k] for o in out]).cpu().numpy() for k in range(3))

    def decide(self, avg, std, pow):
        return decide(avg, std, pow, self.ptsperint, self.time_sig, self.freq_sig, self.chan_sig,
                      self.chan_window, self.chantrigfrac, self.inttrigfrac)

    def find(self, chunks, **header):
        """Statistics of the stream, the decision and the fill: an RFIMask
        (``header``: mjd, tsamp or dtint, lofreq, df)."""
        avg, std, pw = self.accumulate(chunks)
        return self.mask_from_stats(avg, std, pw, **header)

    def mask_from_stats(self, avg, std, pow, **header):
        if torch.is_tensor(avg):
            avg, std, pow = (a.cpu().numpy() for a in (avg, std, pow))
        mask = self.decide(avg, std, pow)
        return RFIMask(mask, self.ptsperint, channel_fill(avg, mask), time_sig=self.time_sig,
                       freq_sig=self.freq_sig, **header)


def mask_from_file(fn, fb, nmax=1 << 18):
    """The RFIMask of ``.mask`` file ``fn`` for filterbank object ``fb``: the
    replacement values (not part of the format) come from the file's first
    <= nmax spectra (RFIMask.fill_from_block)."""
    mask = RFIMask.from_file(fn)
    if mask.nchan != fb.nchans:
        raise ValueError("%s: %d channels, the data have %d" % (fn, mask.nchan, fb.nchans))
    n = min(int(fb.number_of_samples), max(int(nmax), mask.ptsperint))
    host = np.empty((n, fb.nchans), dtype=np.dtype(fb.dtype))
    n = fb.read_block_into(0, host)
    head = torch.from_numpy(host[:n])
    if head.dtype not in _CODES:
        raise ValueError("8-bit or float32 data only")
    mask.fill_from_block(head.cuda(), 0)
    return mask


def file_header(fb):
    """The ``.mask`` header fields of a filterbank file object."""
    hdr = fb.header
    foff = float(hdr.get("foff", 1.0))
    freqs = np.asarray(fb.freqs, dtype=np.float64)
    return dict(mjd=float(hdr.get("tstart", 0.0)), tsamp=float(fb.tsamp),
                lofreq=float(freqs.min()), df=abs(foff))
