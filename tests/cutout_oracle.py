"""Brute-force restatement of the candidate cut-outs (pypulsar_amd/cutout.py,
DESIGN.md §6k) in NumPy int64 / float64 on oracle.spectra_oracle's delay
arithmetic.

All times are RAW file samples; ds is the search's downsampling factor.  For a
candidate (DM, Sample, Downfact), image sizes nbin, nsub, ndm, half-range h:

  W      = Downfact * ds
  f      = clamp(W // 2, 1, fmax)            (or given)
  centre = Sample * ds + W // 2
  t0     = centre - (nbin // 2) * f          (may be negative)
  dms[j] = DM + (j - ndm // 2) * (2 h / ndm), h = max(DM, dm_min_half) by default
  FT[s, b]  = sum_{c in subband s} sum_{k<f} X[c, t0 + b f + k + bins(DM)[c]]
  DMT[j, b] = sum_{all c}          sum_{k<f} X[c, t0 + b f + k + bins(dms[j])[c]]

bins(dm) = dedisperse_bins(dm, 0, freqs, dt) (reference frequency: the highest
channel); a subband is C / nsub consecutive channels in file order; a sample
outside the block contributes padvals[c] (None: 0).
"""
import numpy as np

from oracle import spectra_oracle as orc


def geometry(dm, sample, downfact, ds, nbin, ndm, h=None, dm_min_half=10.0, fmax=1024):
    """(f, t0, dms) of one candidate."""
    W = int(downfact) * int(ds)
    f = min(max(W // 2, 1), fmax)
    centre = int(sample) * int(ds) + W // 2
    t0 = centre - (nbin // 2) * f
    if h is None:
        h = max(float(dm), dm_min_half)
    dms = np.array([dm + (j - ndm // 2) * (2.0 * h / ndm) for j in range(ndm)])
    return f, t0, dms


def channel_boxes(x_tc, bins, t0, f, nbin, padvals=None):
    """[C, nbin]: per channel sum_{k<f} X[c, t0 + b f + k + bins[c]] of the
    time-major block x_tc [n, C]; (in-range sums as int64 for integer data,
    float64 pad term) -> returned as the pair (inside, pad)."""
    x = np.asarray(x_tc)
    n, C = x.shape
    wide = x.astype(np.int64 if x.dtype.kind in "ui" else np.float64)
    inside = np.zeros((C, nbin), dtype=wide.dtype)
    pad = np.zeros((C, nbin), dtype=np.float64)
    for c in range(C):
        p = t0 + int(bins[c]) + np.arange(nbin * f, dtype=np.int64)
        ok = (p >= 0) & (p < n)
        v = np.where(ok, wide[np.clip(p, 0, max(n - 1, 0)), c] if n else 0, 0)
        inside[c] = v.reshape(nbin, f).sum(axis=1)
        if padvals is not None:
            pad[c] = (~ok).reshape(nbin, f).sum(axis=1) * float(padvals[c])
    return inside, pad


def ft_image(x_tc, freqs, dt, t0, f, dm, nbin, nsub, padvals=None):
    """(inside [nsub, nbin], pad [nsub, nbin]): the image is inside + pad."""
    C = len(freqs)
    assert C % nsub == 0
    bins = orc.dedisperse_bins(dm, 0.0, freqs, dt)
    a, p = channel_boxes(x_tc, bins, t0, f, nbin, padvals)
    cps = C // nsub
    return a.reshape(nsub, cps, nbin).sum(axis=1), p.reshape(nsub, cps, nbin).sum(axis=1)


def dmt_image(x_tc, freqs, dt, t0, f, dms, nbin, padvals=None):
    """(inside [ndm, nbin], pad [ndm, nbin])."""
    ins, pads = [], []
    for dm in dms:
        a, p = channel_boxes(x_tc, orc.dedisperse_bins(dm, 0.0, freqs, dt), t0, f, nbin, padvals)
        ins.append(a.sum(axis=0))
        pads.append(p.sum(axis=0))
    return np.array(ins), np.array(pads)


def expected(inside, pad):
    """What the device returns for 8-bit data: float32(exact integer sum) +
    the pad term; for float data the float64 value."""
    if inside.dtype.kind == "i":
        return inside.astype(np.float32).astype(np.float64) + pad
    return inside + pad


def chain_ft(x_tc, freqs, dt, t0, f, dm, nbin):
    """The frequency-time image with nsub = C through the oracle's Spectra
    chain: dedisperse (pad 0), slice [t0, t0 + nbin f), downsample(f).
    t0 >= 0 and t0 + nbin f <= n."""
    data = np.asarray(x_tc, dtype=np.float64).T
    dd, _ = orc.dedisperse(data, freqs, dt, dm, padval=0)
    out, _ = orc.downsample(dd[:, t0:t0 + nbin * f], dt, f)
    return out
