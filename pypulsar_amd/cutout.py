"""Cut-outs of single-pulse candidates: per candidate the dedispersed
frequency-time image and the DM-time image ("bow tie") that a person or a
classifier looks at (FETCH's input pair; the frequency-time image is what the
reference's bin/waterfaller.py draws for one hand-picked event).  Both come
from the raw block of the file in file order, many candidates per launch
(pypulsar_amd/csrc/pdd_cutout.hip).  The definition is this project's
(restated by brute force in tests/cutout_oracle.py).

All times are RAW file samples; ``ds`` is the search's downsampling factor.
For a candidate (DM, Sample, Downfact), image sizes nbin, nsub, ndm and a DM
half-range h:

* ``W = Downfact * ds``; ``f = clamp(W // 2, 1, fmax)`` samples per image bin
  (or the ``factor`` given);
* ``centre = Sample * ds + W // 2``; ``t0 = centre - (nbin // 2) * f`` (may
  be negative);
* ``dms[j] = DM + (j - ndm // 2) * (2 h / ndm)``, ``h = max(DM, dm_min_half)``
  by default: row ndm // 2 is the candidate's own DM, the ladder runs from
  about 0 to 2 DM; trial DMs below 0 are allowed;
* ``bins(dm)[c] = delays.dedisperse_bins(dm, freqs, dt)`` at the raw dt,
  reference frequency = the highest channel (``delays.sweep_table``);
* ``FT[s, b] = sum_{c in subband s} sum_{k<f} x[c, t0 + b f + k + bins(DM)[c]]``,
  a subband = C / nsub consecutive channels in file order: every channel is
  dedispersed at full resolution, then groups are summed (NOT waterfaller's
  subband-then-dedisperse order with its two roundings);
* ``DMT[j, b] = sum_{all c} sum_{k<f} x[c, t0 + b f + k + bins(dms[j])[c]]``;
* a sample outside the loaded block contributes ``padvals[c]`` (None: 0).

8-bit input: float32(exact integer sum of the in-range samples) + the float32
pad term.  float32 input: float32 sums in a fixed order.  The zero-DM filter
is NOT applied: a cut-out shows the data as recorded, broadband interference
included.

Limits (refused, never clamped): 1 <= nbin, ndm <= 1024, 1 <= f <= 1024,
C f 255 < 2^31, table entries fit int32, nsub divides C, and per job
nbin f + (largest - smallest delay of its ladder) <= 2^22.  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib, delays
from ._lib import call, ptr, stream_ptr

MAX_IMAGE, MAX_FACTOR, MAX_SPAN = 1024, 1024, 1 << 22
_CODES = {torch.uint8: _lib.U8, torch.float32: _lib.F32}


def _check_sizes(C, nbin, nsub, ndm):
    if not 1 <= nbin <= MAX_IMAGE or not 1 <= ndm <= MAX_IMAGE:
        raise ValueError("nbin and ndm must be in 1..%d" % MAX_IMAGE)
    if nsub < 1 or C % nsub:
        raise ValueError("nsub must divide the %d channels" % C)


class Jobs(object):
    """What ``plan_jobs`` returns, one entry per candidate: ``f`` (samples
    per bin), ``t0`` (raw sample of the image's first bin), ``dms``
    [J, ndm], ``bmin`` / ``bmax`` (smallest / largest delay of the ladder),
    ``lo`` / ``hi`` (the raw samples [lo, hi) the two images read; not cut at
    the file's ends), and ``tables()``."""

    def __init__(self, freqs, dt, nbin, nsub, ndm, f, t0, dms, bmin, bmax):
        self.freqs, self.dt = np.asarray(freqs, dtype=np.float64), float(dt)
        self.nbin, self.nsub, self.ndm = int(nbin), int(nsub), int(ndm)
        self.f, self.t0, self.dms, self.bmin, self.bmax = f, t0, dms, bmin, bmax

    def __len__(self):
        return len(self.f)

    @property
    def lo(self):
        return self.t0 + self.bmin

    @property
    def hi(self):
        return self.t0 + self.nbin * self.f + self.bmax

    @property
    def span(self):
        """Per job the positions of its per-channel box sums (``span`` of
        pdd_cutout_dmt): M f, M = ceil(((nbin - 1) f + bmax - bmin + 1) / f)."""
        return -(-((self.nbin - 1) * self.f + self.bmax - self.bmin + 1) // self.f) * self.f

    def tables(self, i0=0, i1=None):
        """int32 [k, ndm, C] delay tables of jobs i0 .. i1 - 1; row ndm // 2
        of a job is the table of its own DM (the frequency-time image's)."""
        d = self.dms[i0:i1]
        t = delays.sweep_table(d.reshape(-1), self.freqs, self.dt)
        return delays.to_int32(t).reshape(d.shape[0], self.ndm, len(self.freqs))

    def subset(self, idx):
        idx = np.asarray(idx, dtype=np.intp)
        return Jobs(self.freqs, self.dt, self.nbin, self.nsub, self.ndm, self.f[idx], self.t0[idx],
                    self.dms[idx], self.bmin[idx], self.bmax[idx])


def plan_jobs(records, ds, freqs, dt, nbin=256, nsub=256, ndm=256, dm_half=None, dm_min_half=10.0,
              factor=None, fmax=MAX_FACTOR):
    """The cut-out geometry of every record (``search.CAND_DTYPE`` or
    ``spgroup.GROUP_DTYPE``: the fields DM, Sample, Downfact) -> ``Jobs``.
    Pure NumPy.  ``dm_half``: the ladder's half-range h for all (default
    per candidate max(DM, dm_min_half)); ``factor``: f for all (default
    clamp(W // 2, 1, fmax))."""
    freqs = np.asarray(freqs, dtype=np.float64)
    C, ds = len(freqs), int(ds)
    nbin, nsub, ndm = int(nbin), int(nsub), int(ndm)
    _check_sizes(C, nbin, nsub, ndm)
    if ds < 1 or not 1 <= int(fmax) <= MAX_FACTOR:
        raise ValueError("ds must be >= 1 and fmax in 1..%d" % MAX_FACTOR)
    dm = np.asarray(records["DM"], dtype=np.float64).reshape(-1)
    samp = np.asarray(records["Sample"], dtype=np.int64).reshape(-1)
    W = np.asarray(records["Downfact"], dtype=np.int64).reshape(-1) * ds
    if len(W) and W.min() < 1:
        raise ValueError("Downfact must be >= 1")
    if factor is None:
        f = np.clip(W // 2, 1, int(fmax))
    else:
        f = np.broadcast_to(np.asarray(factor, dtype=np.int64), W.shape).copy()
    if len(f) and (f.min() < 1 or f.max() > MAX_FACTOR):
        raise ValueError("factor must be in 1..%d" % MAX_FACTOR)
    if len(f) and C * int(f.max()) * 255 >= 2 ** 31:
        raise ValueError("C * f * 255 must be below 2^31 (C %d, f %d)" % (C, f.max()))
    t0 = samp * ds + W // 2 - (nbin // 2) * f
    if dm_half is None:
        h = np.maximum(dm, float(dm_min_half))
    else:
        h = np.broadcast_to(np.asarray(dm_half, dtype=np.float64), dm.shape)
    if len(h) and not np.all(h > 0):
        raise ValueError("the DM half-range must be positive")
    dms = dm[:, None] + (np.arange(ndm) - ndm // 2)[None, :] * (2.0 * h / ndm)[:, None]
    # a channel's delay grows with the trial DM: the ladder's ends bound it
    ends = delays.to_int32(delays.sweep_table(
        np.concatenate([dms[:, 0], dms[:, -1]]) if len(dm) else np.zeros(0), freqs, dt))
    bmin = ends.min(axis=1).reshape(2, -1).min(axis=0).astype(np.int64)
    bmax = ends.max(axis=1).reshape(2, -1).max(axis=0).astype(np.int64)
    jobs = Jobs(freqs, dt, nbin, nsub, ndm, f, t0, dms, bmin, bmax)
    if len(f) and jobs.span.max() > MAX_SPAN:
        raise ValueError("nbin * f + the ladder's delay range must be <= 2^22 samples")
    return jobs


class Cutouts(object):
    """``Cutouts(freqs, dt, nbin, nsub, ndm)(block, t_first, jobs)`` ->
    device float32 tensors (ft [J, nsub, nbin], dmt [J, ndm, nbin]).

    Jobs go to the device in batches whose delay tables fit ``table_bytes``;
    ``work_bytes`` bounds the box-sum scratch of the DM-time image (one job's
    need at least).  The results do not depend on either."""

    def __init__(self, freqs, dt, nbin=256, nsub=256, ndm=256, table_bytes=256 << 20,
                 work_bytes=1 << 30):
        _lib.require_gpu()
        self.freqs, self.dt = np.asarray(freqs, dtype=np.float64), float(dt)
        self.nbin, self.nsub, self.ndm = int(nbin), int(nsub), int(ndm)
        _check_sizes(len(self.freqs), self.nbin, self.nsub, self.ndm)
        self.table_bytes, self.work_bytes = int(table_bytes), int(work_bytes)

    def plan(self, records, ds, **kw):
        return plan_jobs(records, ds, self.freqs, self.dt, self.nbin, self.nsub, self.ndm, **kw)

    def __call__(self, block, t_first, jobs, padvals=None, stream=None):
        """``block``: device [n, C] uint8 or float32, time-major (the file's
        order; rows may be strided), whose first row is raw sample
        ``t_first``.  ``padvals``: device float32 [C] or None (0)."""
        C, nbin, nsub, ndm = len(self.freqs), self.nbin, self.nsub, self.ndm
        if block.dtype not in _CODES:
            raise TypeError("Cutouts: 8-bit or float32 blocks only, got %s" % block.dtype)
        assert block.is_cuda and block.dim() == 2 and block.shape[1] == C
        assert block.shape[0] == 0 or block.stride(1) == 1 or C == 1
        assert (jobs.nbin, jobs.nsub, jobs.ndm) == (nbin, nsub, ndm) and len(jobs.freqs) == C
        if padvals is not None:
            assert padvals.is_cuda and padvals.dtype == torch.float32 and padvals.shape == (C,) \
                and padvals.is_contiguous()
        J, dev = len(jobs), block.device
        n = block.shape[0]
        ld = block.stride(0) if n > 1 else C
        ft = torch.empty((J, nsub, nbin), dtype=torch.float32, device=dev)
        dmt = torch.empty((J, ndm, nbin), dtype=torch.float32, device=dev)
        if J == 0:
            return ft, dmt
        if C * int(jobs.f.max()) * 255 >= 2 ** 31 or jobs.f.min() < 1 or jobs.f.max() > MAX_FACTOR:
            raise ValueError("f must be in 1..%d with C * f * 255 below 2^31" % MAX_FACTOR)
        if jobs.span.max() > MAX_SPAN:
            raise ValueError("nbin * f + the ladder's delay range must be <= 2^22 samples")
        code = _CODES[block.dtype]
        per = max(1, self.table_bytes // (ndm * C * 4))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            for i0 in range(0, J, per):
                i1 = min(J, i0 + per)
                k = i1 - i0
                table = torch.from_numpy(jobs.tables(i0, i1).reshape(k * ndm, C)).to(dev)
                jb = np.zeros((k, 5), dtype=np.int64)
                jb[:, 0], jb[:, 1] = jobs.t0[i0:i1] - int(t_first), jobs.f[i0:i1]
                jb[:, 2] = np.arange(k) * ndm
                jb[:, 3], jb[:, 4] = jobs.bmin[i0:i1], jobs.bmax[i0:i1]
                jft = jb.copy()
                jft[:, 2] += ndm // 2
                fmax, span = int(jobs.f[i0:i1].max()), int(jobs.span[i0:i1].max())
                es = 2 if (code == _lib.U8 and fmax * 255 <= 65535) else 4
                one = span * C * es
                work = torch.empty(min(k * one, max(self.work_bytes // one, 1) * one),
                                   dtype=torch.uint8, device=dev)
                djb, djft = torch.from_numpy(jb).to(dev), torch.from_numpy(jft).to(dev)
                call("pdd_cutout_ft", ptr(block), code, n, C, ld, ptr(djft), k, ptr(table),
                     k * ndm, ptr(padvals), nbin, nsub, fmax, ptr(ft[i0:i1]), stream_ptr(stream))
                call("pdd_cutout_dmt", ptr(block), code, n, C, ld, ptr(djb), k, ptr(table),
                     k * ndm, ptr(padvals), nbin, ndm, fmax, span, ptr(work), work.numel(),
                     ptr(dmt[i0:i1]), stream_ptr(stream))
                # (the batch's tensors are freed to torch's pool in stream order)
        return ft, dmt


def group_loads(lo, hi, nsamp, max_rows):
    """Loads [a, b) of the file that cover the windows [lo_i, hi_i) cut to
    [0, nsamp): windows are taken in order of lo and share a load while it
    stays within ``max_rows`` rows (a single larger window gets its own).
    Returns [(a, b, indices)]; a window entirely outside the file joins a
    load of zero or more rows."""
    lo = np.clip(np.asarray(lo, dtype=np.int64), 0, nsamp)
    hi = np.clip(np.asarray(hi, dtype=np.int64), 0, nsamp)
    loads = []
    for i in np.argsort(lo, kind="stable"):
        if loads and max(loads[-1][1], hi[i]) - loads[-1][0] <= max_rows:
            loads[-1][1] = max(loads[-1][1], int(hi[i]))
            loads[-1][2].append(int(i))
        else:
            loads.append([int(lo[i]), int(max(hi[i], lo[i])), [int(i)]])
    return [(a, b, idx) for a, b, idx in loads]


def cutouts_from_file(fb, records, ds, rfimask=None, nbin=256, nsub=256, ndm=256,
                      load_bytes=256 << 20, **plan_kw):
    """Both images of every record from the open ``filterbank`` ``fb`` (8 or
    32 bits).  Each window of the file is read once; candidates whose windows
    fit one load of ``load_bytes`` share it.  ``rfimask``: its cells are
    replaced (``RFIMask.apply``, the mask's own fill values) before the
    images are made.  Past the file's ends the channel means of the loaded
    window stand in.  Returns (ft, dmt, jobs): host float32 arrays."""
    dtype = np.dtype(fb.dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise ValueError("cut-outs: 8-bit or float32 filterbanks only")
    cut = Cutouts(fb.freqs, fb.tsamp, nbin, nsub, ndm)
    jobs = cut.plan(records, ds, **plan_kw)
    C, nsamp = len(cut.freqs), int(fb.number_of_samples)
    ft = np.empty((len(jobs), nsub, nbin), dtype=np.float32)
    dmt = np.empty((len(jobs), ndm, nbin), dtype=np.float32)
    max_rows = max(1, int(load_bytes) // (C * dtype.itemsize))
    for a, b, idx in group_loads(jobs.lo, jobs.hi, nsamp, max_rows):
        host = np.empty((b - a, C), dtype=dtype)
        got = fb.read_block_into(a, host) if b > a else 0
        block = torch.from_numpy(host[:got]).cuda()
        if rfimask is not None and got:
            rfimask.apply(block, a)
        pad = block.double().mean(dim=0).float() if got else None
        f, d = cut(block, a, jobs.subset(idx), padvals=pad)
        ft[idx], dmt[idx] = f.cpu().numpy(), d.cpu().numpy()
    return ft, dmt, jobs


def write_cutouts(fn, ft, dmt, records, jobs):
    """``.npz``: ft [J, nsub, nbin], dmt [J, ndm, nbin], the records' columns
    (as ``rec_<name>``), factor, t0 (raw samples), dms [J, ndm], sub_freqs
    (subband centres, MHz), dt (raw, s), nbin, nsub, ndm."""
    records = np.asarray(records)
    cols = {"rec_" + name: np.asarray(records[name]) for name in records.dtype.names}
    _, _, ctr = delays.subband_layout(jobs.freqs, jobs.nsub)
    with open(fn, "wb") as fh:
        np.savez(fh, ft=np.asarray(ft, dtype=np.float32), dmt=np.asarray(dmt, dtype=np.float32),
                 factor=jobs.f, t0=jobs.t0, dms=jobs.dms, sub_freqs=ctr, dt=np.float64(jobs.dt),
                 nbin=np.int64(jobs.nbin), nsub=np.int64(jobs.nsub), ndm=np.int64(jobs.ndm),
                 **cols)


def read_cutouts(fn):
    """Inverse of write_cutouts: a dict of its arrays, with the records'
    columns gathered into the structured array ``records``."""
    with np.load(fn, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files if not k.startswith("rec_")}
        names = [k[4:] for k in z.files if k.startswith("rec_")]
        rec = np.empty(len(out["ft"]), dtype=[(nm, z["rec_" + nm].dtype) for nm in names])
        for nm in names:
            rec[nm] = z["rec_" + nm]
    out["records"] = rec
    for k in ("nbin", "nsub", "ndm"):
        out[k] = int(out[k])
    out["dt"] = float(out["dt"])
    return out
