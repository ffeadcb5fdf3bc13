"""Grouping of single-pulse candidates across DM row, time and width.

The single-pulse search (pypulsar_amd/search.py) emits one candidate per (DM
row, window of 1024 starts), so one bright burst comes out as one line per
neighbouring DM trial of its bow tie and one interference spike as a whole
column of rows.  This module decides which lines are the same event: a
friends-of-friends pass on the device (pypulsar_amd/csrc/pdd_spgroup.hip;
heimdall's candidate clustering and PRESTO's rrattrap do this step).  The
reference has nothing here, so the definition is this project's (DESIGN.md
§6j; restated by brute force in tests/spgroup_oracle.py):

* a candidate (row r, start s, width w, S/N) has the extent [s, s + w);
* a, b are **linked** when ``|r_a - r_b| <= row_tol`` and
  ``max(s_a, s_b) - min(s_a + w_a, s_b + w_b) <= time_tol``;
* a **group** is a connected component of the links;
* canonical order: ascending (s // 1024, r, s, w, S/N bits as int32); the
  **label** of a candidate is the canonical index of the first member of its
  group -- independent of the input order and of scheduling;
* a group's summary: member count, best member (highest S/N as floats, the
  smallest canonical index on a tie), row range, min start, max end.

Limits: 0 <= row_tol <= 16, 0 <= time_tol <= 1023, 1 <= w <= 1025, s >= 0,
s + w + time_tol < 2^31.  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .search import CAND_DTYPE, WINDOW

MAX_ROW_TOL, MAX_TIME_TOL, MAX_WIDTH = 16, 1023, 1025

GROUP_DTYPE = np.dtype(CAND_DTYPE.descr + [
    ("Members", "i4"), ("DMlo", "f8"), ("DMhi", "f8"), ("rowlo", "i4"), ("rowhi", "i4"),
    ("SampleLo", "i8"), ("SampleHi", "i8"), ("Tbegin", "f8"), ("Tend", "f8")])


def record_rows(records, dms=None):
    """Plane row of every record: the ``row`` field, or with ``dms`` the
    index of the record's DM in ``dms`` (exact match; for lists gathered from
    several ranks, whose ``row`` fields are rank-local)."""
    if dms is None:
        return np.asarray(records["row"], dtype=np.int64)
    dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
    idx = np.argsort(dms, kind="stable")
    dm = np.asarray(records["DM"], dtype=np.float64)
    pos = np.clip(np.searchsorted(dms[idx], dm), 0, max(len(dms) - 1, 0))
    if len(dm) and (len(dms) == 0 or np.any(dms[idx][pos] != dm)):
        raise ValueError("a candidate's DM is not one of dms")
    return idx[pos].astype(np.int64) if len(dm) else np.empty(0, dtype=np.int64)


def time_axis(records):
    """(starttime, dt) of the records' own Time = starttime + Sample dt, from
    the two records furthest apart (dt is NaN when all share one Sample and
    that Sample is 0: then nothing tells it)."""
    s = np.asarray(records["Sample"], dtype=np.int64)
    t = np.asarray(records["Time"], dtype=np.float64)
    a, b = int(np.argmin(s)), int(np.argmax(s))
    if s[b] != s[a]:
        dt = (t[b] - t[a]) / float(s[b] - s[a])
        return t[a] - s[a] * dt, dt
    return 0.0, (t[a] / s[a] if s[a] else float("nan"))


def canonical_order(cands, nrows):
    """Device int64 [k]: canonical index -> input index of a device int32
    [k, 4] candidate tensor, by two stable sorts on the current stream
    (plumbing): the minor keys (start within its window, width, snr bits as
    int32) packed into one int64, then the cell key."""
    c = cands.to(torch.int64)
    minor = ((c[:, 1] & (WINDOW - 1)) << 43) | (c[:, 2] << 32) | (c[:, 3] + (1 << 31))
    o1 = torch.sort(minor, stable=True)[1]
    cell = (c[:, 1] // WINDOW) * int(nrows) + c[:, 0]
    return o1[torch.sort(cell[o1], stable=True)[1]]


class SinglePulseGrouper(object):
    """``SinglePulseGrouper(row_tol=2, time_tol=3)(records)`` ->
    (group_of, groups)."""

    def __init__(self, row_tol=2, time_tol=3):
        _lib.require_gpu()
        self.row_tol, self.time_tol = int(row_tol), int(time_tol)
        if not 0 <= self.row_tol <= MAX_ROW_TOL:
            raise ValueError("row_tol must be in 0..%d" % MAX_ROW_TOL)
        if not 0 <= self.time_tol <= MAX_TIME_TOL:
            raise ValueError("time_tol must be in 0..%d" % MAX_TIME_TOL)

    def raw(self, cands, nrows, stream=None):
        """Device-side grouping of a device int32 [k, 4] tensor {row, start,
        width, snr bits} in any order (e.g. ``SinglePulseSearch.raw(...)[0][:k]``),
        ``nrows`` > every row.  Returns device tensors (order int64 [k]:
        canonical index -> input index; label int32 [k]; groups int32 [k, 8]:
        at a label {members, best, row_lo, row_hi, start_lo, end_hi, snr bits
        of best, 0}, zeros elsewhere), label and best in canonical indices,
        without synchronising."""
        assert cands.is_cuda and cands.dtype == torch.int32 and cands.dim() == 2 \
            and cands.shape[1] == 4
        k, dev = cands.shape[0], cands.device
        assert k < (1 << 31) and 1 <= int(nrows) <= (1 << 31)
        if k == 0:
            return (torch.empty(0, dtype=torch.int64, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty((0, 8), dtype=torch.int32, device=dev))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            order = canonical_order(cands, nrows)
            cs = cands[order].contiguous()
            label = torch.empty(k, dtype=torch.int32, device=dev)
            groups = torch.empty((k, 8), dtype=torch.int32, device=dev)
            call("pdd_spg_label", ptr(cs), k, int(nrows), self.row_tol, self.time_tol, ptr(label),
                 stream_ptr(stream))
            call("pdd_spg_summarise", ptr(cs), ptr(label), k, ptr(groups), stream_ptr(stream))
        return order, label, groups

    def __call__(self, records, dms=None):
        """``records``: a ``search.CAND_DTYPE`` array in any order.  Returns
        (group_of, groups): ``group_of[i]`` is the index into ``groups`` of
        record i; ``groups`` is a ``GROUP_DTYPE`` array ordered by label: the
        columns of the best member, then Members, the DM / row / sample /
        time ranges (SampleHi, Tend: exclusive end)."""
        records = np.asarray(records)
        k = len(records)
        if k == 0:
            return np.empty(0, dtype=np.int64), np.empty(0, dtype=GROUP_DTYPE)
        rows = record_rows(records, dms)
        samp = np.asarray(records["Sample"], dtype=np.int64)
        wid = np.asarray(records["Downfact"], dtype=np.int64)
        if rows.min() < 0:
            raise ValueError("negative row (a list read from a file has none: pass dms)")
        if wid.min() < 1 or wid.max() > MAX_WIDTH:
            raise ValueError("widths must be in 1..%d" % MAX_WIDTH)
        base = (int(samp.min()) // WINDOW) * WINDOW
        if int((samp - base + wid).max()) + self.time_tol >= (1 << 31):
            raise ValueError("the candidates span more than 2^31 samples")
        c = np.empty((k, 4), dtype=np.int32)
        c[:, 0], c[:, 1], c[:, 2] = rows, samp - base, wid
        c[:, 3] = np.ascontiguousarray(records["Sigma"], dtype=np.float32).view(np.int32)
        order, label, grp = self.raw(torch.from_numpy(c).cuda(), int(rows.max()) + 1)
        order, label, grp = order.cpu().numpy(), label.cpu().numpy(), grp.cpu().numpy()
        roots = np.flatnonzero(grp[:, 0] > 0)
        group_of = np.empty(k, dtype=np.int64)
        group_of[order] = np.searchsorted(roots, label)
        g = grp[roots]
        best = order[g[:, 1]]
        out = np.empty(len(roots), dtype=GROUP_DTYPE)
        for name in CAND_DTYPE.names:
            out[name] = records[name][best]
        out["Members"] = g[:, 0]
        out["rowlo"], out["rowhi"] = g[:, 2], g[:, 3]
        # the DM of a row: that of any record in it
        urows, first = np.unique(rows, return_index=True)
        dm = np.asarray(records["DM"], dtype=np.float64)[first]
        out["DMlo"] = dm[np.searchsorted(urows, g[:, 2])]
        out["DMhi"] = dm[np.searchsorted(urows, g[:, 3])]
        out["SampleLo"] = g[:, 4].astype(np.int64) + base
        out["SampleHi"] = g[:, 5].astype(np.int64) + base
        t0, dt = time_axis(records)
        out["Tbegin"] = t0 + out["SampleLo"] * dt
        out["Tend"] = t0 + out["SampleHi"] * dt
        return group_of, out


def select(groups, min_members=1, min_dm=None, min_sigma=None):
    """Host-side filter: drops a group with fewer than ``min_members``
    members, with its best member below ``min_dm`` (interference peaks at DM
    0) or weaker than ``min_sigma``."""
    keep = groups["Members"] >= min_members
    if min_dm is not None:
        keep &= groups["DM"] >= min_dm
    if min_sigma is not None:
        keep &= groups["Sigma"] >= min_sigma
    return groups[keep]


def write_groups(groups, fn):
    """Text: the ``.singlepulse`` columns and formats of the best member,
    then Members DMlo DMhi Tbegin Tend."""
    with open(fn, "w") as f:
        f.write("# DM      Sigma      Time (s)     Sample    Downfact  Members    DMlo    DMhi"
                "        Tbegin          Tend\n")
        for g in groups:
            f.write("%7.2f %7.2f %13.6f %10d     %3d %8d %7.2f %7.2f %13.6f %13.6f\n"
                    % (g["DM"], g["Sigma"], g["Time"], g["Sample"], g["Downfact"], g["Members"],
                       g["DMlo"], g["DMhi"], g["Tbegin"], g["Tend"]))


def read_groups(fn):
    """Inverse of write_groups (to the digits written); what the text does
    not hold is -1: row, rowlo, rowhi, SampleLo, SampleHi."""
    rows = [l.split() for l in open(fn) if l.strip() and not l.startswith("#")]
    out = np.empty(len(rows), dtype=GROUP_DTYPE)
    for i, r in enumerate(rows):
        out[i] = (float(r[0]), float(r[1]), float(r[2]), int(r[3]), int(r[4]), -1, int(r[5]),
                  float(r[6]), float(r[7]), -1, -1, -1, -1, float(r[8]), float(r[9]))
    return out
