"""The host side of the single-pulse candidate grouping
(pypulsar_amd/spgroup.py) without a GPU: the brute-force oracle
(tests/spgroup_oracle.py) on hand-built cases, the group files, the filter,
the DM -> row mapping, and the argument checks of the two ABI calls, which
come before any HIP call."""
import ctypes

import numpy as np
import pytest

import spgroup_oracle as so


def _groups(n):
    from pypulsar_amd.spgroup import GROUP_DTYPE
    g = np.zeros(n, dtype=GROUP_DTYPE)
    g["DM"] = 10.0 * np.arange(n)
    g["Sigma"] = 6.0 + np.arange(n)
    g["Sample"] = 1000 + 4096 * np.arange(n)
    g["Time"] = g["Sample"] * 1e-3
    g["Downfact"] = 1 + np.arange(n)
    g["row"] = np.arange(n)
    g["Members"] = 1 + 3 * np.arange(n)
    g["DMlo"], g["DMhi"] = g["DM"] - 1.25, g["DM"] + 2.5
    g["rowlo"], g["rowhi"] = g["row"], g["row"] + 2
    g["SampleLo"], g["SampleHi"] = g["Sample"] - 3, g["Sample"] + 40
    g["Tbegin"], g["Tend"] = g["SampleLo"] * 1e-3, g["SampleHi"] * 1e-3
    return g


# ---- the oracle on hand-built cases ----

def test_oracle_reach_two_pair():
    # extents [0, 1025) and [2048, 2049): the gap is 1023 samples, two windows apart
    c = so.cands([5, 5], [0, 2048], [1025, 1], [8.0, 7.0])
    order, lab, grp = so.group(c, row_tol=0, time_tol=1023)
    assert list(order) == [0, 1] and list(lab) == [0, 0]
    assert list(grp[0]) == [2, 0, 5, 5, 0, 2049, c[0, 3], 0] and not grp[1].any()
    order, lab, grp = so.group(c, row_tol=0, time_tol=1022)
    assert list(lab) == [0, 1]
    assert list(grp[0]) == [1, 0, 5, 5, 0, 1025, c[0, 3], 0]
    assert list(grp[1]) == [1, 1, 5, 5, 2048, 2049, c[1, 3], 0]


def test_oracle_links_and_canonical_order():
    # given out of order: canonical order is (window, row, start, width, snr)
    c = so.cands([3, 1, 2, 9], [1030, 10, 12, 11], [2, 4, 1, 1], [6.0, 9.0, 7.0, 6.5])
    order, lab, grp = so.group(c, row_tol=1, time_tol=0)
    assert list(order) == [1, 2, 3, 0]
    # rows 1 and 2 overlap in time; row 9 is far in rows, window 1 far in time
    assert list(lab) == [0, 0, 2, 3]
    assert list(grp[0]) == [2, 0, 1, 2, 10, 14, c[1, 3], 0]
    # touching extents link at time_tol 0, a gap of one sample does not
    t = so.cands([0, 0, 0], [0, 4, 9], [4, 4, 1], [6, 6, 6])
    assert list(so.group(t, 0, 0)[1]) == [0, 0, 2]
    assert list(so.group(t, 0, 1)[1]) == [0, 0, 0]
    # a chain: the ends are grouped through the middle
    ch = so.cands([0, 2, 4], [0, 0, 0], [1, 1, 1], [6, 6, 6])
    assert list(so.group(ch, 2, 0)[1]) == [0, 0, 0]
    assert list(so.group(ch, 1, 0)[1]) == [0, 1, 2]


def test_oracle_snr_tie_and_empty():
    c = so.cands([0, 1, 2], [5, 5, 5], [1, 1, 1], [7.0, 9.0, 9.0])
    _, lab, grp = so.group(c, 1, 0)
    assert list(lab) == [0, 0, 0]
    assert grp[0, 0] == 3 and grp[0, 1] == 1  # the smaller canonical index of the tie
    order, lab, grp = so.group(np.empty((0, 4), dtype=np.int32))
    assert len(order) == len(lab) == 0 and grp.shape == (0, 8)


def test_oracle_partition_is_order_free():
    c = so.bow_ties(3, rows=24, windows=6, events=4)
    p0 = so.partition(*so.group(c)[:2])
    perm = np.random.default_rng(0).permutation(len(c))
    o, lab, _ = so.group(c[perm])
    assert set(frozenset(int(perm[i]) for i in s) for s in so.partition(o, lab)) == p0


# ---- files, filter, rows ----

def test_groups_round_trip(tmp_path):
    from pypulsar_amd.search import write_singlepulse
    from pypulsar_amd.spgroup import read_groups, write_groups
    g = _groups(5)
    fn, fs = str(tmp_path / "a.spgroups"), str(tmp_path / "a.singlepulse")
    write_groups(g, fn)
    write_singlepulse(g, fs)
    lines, sp = open(fn).read().splitlines(), open(fs).read().splitlines()
    assert lines[0].startswith("#") and len(lines) == 6
    # the first five columns: exactly the .singlepulse layout of the best member
    assert lines[0].startswith(sp[0])
    for a, b in zip(lines[1:], sp[1:]):
        assert a.startswith(b) and len(a.split()) == 10
    back = read_groups(fn)
    for name in ("DM", "Sigma", "Sample", "Downfact", "Members", "DMlo", "DMhi"):
        np.testing.assert_array_equal(back[name], g[name])
    for name in ("Time", "Tbegin", "Tend"):
        np.testing.assert_allclose(back[name], g[name], rtol=0, atol=5e-7)
    assert np.all(back["row"] == -1)
    write_groups(g[:0], fn)
    assert len(read_groups(fn)) == 0


def test_select():
    from pypulsar_amd.spgroup import select
    g = _groups(5)  # DM 0, 10, ..; Sigma 6, 7, ..; Members 1, 4, 7, ..
    assert len(select(g)) == 5
    assert list(select(g, min_members=4)["row"]) == [1, 2, 3, 4]
    assert list(select(g, min_dm=5.0)["row"]) == [1, 2, 3, 4]
    assert list(select(g, min_dm=10.0)["row"]) == [1, 2, 3, 4]
    assert list(select(g, min_sigma=8.5)["row"]) == [3, 4]
    assert list(select(g, min_members=5, min_dm=25.0, min_sigma=6.0)["row"]) == [3, 4]
    assert len(select(g, min_members=100)) == 0


def test_rows_from_dms():
    from pypulsar_amd.search import CAND_DTYPE
    from pypulsar_amd.spgroup import record_rows
    dms = np.linspace(0.0, 30.0, 7)
    rec = np.zeros(4, dtype=CAND_DTYPE)
    rec["DM"] = dms[[6, 0, 3, 3]]
    rec["row"] = [2, 0, 1, 1]  # rank-local rows: not used with dms
    assert list(record_rows(rec, dms)) == [6, 0, 3, 3]
    assert list(record_rows(rec)) == [2, 0, 1, 1]
    assert list(record_rows(rec, dms[::-1])) == [0, 6, 3, 3]
    rec["DM"][2] = 15.01
    with pytest.raises(ValueError):
        record_rows(rec, dms)
    rec["DM"][2] = 99.0
    with pytest.raises(ValueError):
        record_rows(rec, dms)
    assert len(record_rows(rec[:0], dms)) == 0


def test_time_axis():
    from pypulsar_amd.search import CAND_DTYPE
    from pypulsar_amd.spgroup import time_axis
    rec = np.zeros(3, dtype=CAND_DTYPE)
    rec["Sample"] = [4096, 1024, 2048]
    rec["Time"] = 100.0 + rec["Sample"] * 0.25
    t0, dt = time_axis(rec)
    assert t0 == 100.0 and dt == 0.25


# ---- the C ABI without a GPU ----

def test_exports():
    from pypulsar_amd import _lib
    for name in ("pdd_spg_label", "pdd_spg_summarise"):
        assert name in _lib.EXPORTS and name in _lib._SIGS


def test_argument_checks_without_gpu():
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()
    buf = (ctypes.c_int32 * 64)()  # host memory: never dereferenced by a refused call
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.pdd_spg_label(None, 4, 8, 2, 3, p, None) < 0
    assert b"null pointer" in h.pdd_last_error()
    assert h.pdd_spg_label(p, 4, 8, 2, 3, None, None) < 0
    assert b"null pointer" in h.pdd_last_error()
    assert h.pdd_spg_label(p, 4, 8, 17, 3, p, None) < 0
    assert b"row_tol" in h.pdd_last_error()
    assert h.pdd_spg_label(p, 4, 8, -1, 3, p, None) < 0
    assert h.pdd_spg_label(p, 4, 8, 2, 1024, p, None) < 0
    assert b"time_tol" in h.pdd_last_error()
    assert h.pdd_spg_label(p, -1, 8, 2, 3, p, None) < 0
    assert h.pdd_spg_label(p, 1 << 31, 8, 2, 3, p, None) < 0
    assert h.pdd_spg_label(p, 4, 0, 2, 3, p, None) < 0
    assert h.pdd_spg_summarise(None, p, 4, p, None) < 0
    assert b"null pointer" in h.pdd_last_error()
    assert h.pdd_spg_summarise(p, p, 4, None, None) < 0
    assert h.pdd_spg_summarise(p, p, -1, p, None) < 0
    # k == 0 launches nothing
    assert h.pdd_spg_label(None, 0, 8, 2, 3, None, None) == 0
    assert h.pdd_spg_summarise(None, None, 0, None, None) == 0
