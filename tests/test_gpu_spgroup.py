"""Grouping of single-pulse candidates on the GPU (pypulsar_amd/spgroup.py,
csrc/pdd_spgroup.hip) against the brute-force oracle (tests/spgroup_oracle.py):
exact equality of every label and of every summary field, for any input
order."""
import functools
import os

import numpy as np
import pytest

import spgroup_oracle as so

pytestmark = pytest.mark.gpu
DT = 1e-3


@functools.lru_cache(maxsize=None)
def _ties():
    c = so.bow_ties(1)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _noise():
    c = so.noise(7)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(which, row_tol, time_tol):
    c = {"ties": _ties, "noise": _noise, "cell": lambda: so.per_cell(5)}[which]()
    order, lab, grp = so.group(c, row_tol, time_tol)
    for a in (order, lab, grp):
        a.setflags(write=False)
    return c, order, lab, grp


def _raw(c, row_tol, time_tol, nrows):
    import torch
    from pypulsar_amd.spgroup import SinglePulseGrouper
    order, lab, grp = SinglePulseGrouper(row_tol, time_tol).raw(
        torch.from_numpy(np.array(c, dtype=np.int32, order="C")).cuda(), nrows)
    torch.cuda.synchronize()
    return order.cpu().numpy(), lab.cpu().numpy(), grp.cpu().numpy()


def _same(c, got, want):
    (order, lab, grp), (order_w, lab_w, grp_w) = got, want
    assert order.dtype == np.int64 and lab.dtype == np.int32 and grp.dtype == np.int32
    assert sorted(order) == list(range(len(c)))
    np.testing.assert_array_equal(c[order], c[order_w])  # the canonical list
    np.testing.assert_array_equal(lab, lab_w)
    np.testing.assert_array_equal(grp, grp_w)


def _records(c, dms, t0=0):
    """CAND_DTYPE records of a candidate list, in the list's order."""
    from pypulsar_amd.search import CAND_DTYPE
    rec = np.empty(len(c), dtype=CAND_DTYPE)
    rec["row"], rec["DM"] = c[:, 0], np.asarray(dms)[c[:, 0]]
    rec["Sigma"] = c[:, 3].view(np.float32)
    rec["Sample"] = c[:, 1].astype(np.int64) + t0
    rec["Time"] = rec["Sample"] * DT
    rec["Downfact"] = c[:, 2]
    return rec


def _check_records(rec, group_of, groups, c, want):
    """(group_of, groups) of __call__ on records made from list c against
    the oracle's (order, label, groups) of c."""
    order_w, lab_w, grp_w = want
    roots = np.flatnonzero(grp_w[:, 0])
    gof = np.empty(len(c), dtype=np.int64)
    gof[order_w] = np.searchsorted(roots, lab_w)
    np.testing.assert_array_equal(group_of, gof)
    g = grp_w[roots]
    assert len(groups) == len(roots)
    best = order_w[g[:, 1]]
    for name in ("DM", "Sigma", "Time", "Sample", "Downfact", "row"):
        np.testing.assert_array_equal(groups[name], rec[name][best])
    t0 = int(rec["Sample"][0]) - int(c[0, 1])
    np.testing.assert_array_equal(groups["Members"], g[:, 0])
    np.testing.assert_array_equal(groups["rowlo"], g[:, 2])
    np.testing.assert_array_equal(groups["rowhi"], g[:, 3])
    np.testing.assert_array_equal(groups["SampleLo"], g[:, 4].astype(np.int64) + t0)
    np.testing.assert_array_equal(groups["SampleHi"], g[:, 5].astype(np.int64) + t0)


# ---- 1. bow ties plus noise ----

@pytest.mark.parametrize("row_tol,time_tol", [(2, 3), (1, 3), (2, 0), (3, 8)])
def test_bow_ties(gpu, row_tol, time_tol):
    c, order_w, lab_w, grp_w = _want("ties", row_tol, time_tol)
    members = grp_w[:, 0][grp_w[:, 0] > 0]
    print("k %d groups %d largest %d groups>=10: %d"
          % (len(c), len(members), members.max(), np.sum(members >= 10)))
    # the input is not degenerate (asserted on the oracle's output)
    assert len(members) >= 100 and members.max() >= 25 and np.sum(members >= 10) >= 10
    _same(c, _raw(c, row_tol, time_tol, 64), (order_w, lab_w, grp_w))


@pytest.mark.parametrize("row_tol,time_tol", [(0, 0), (16, 1023)])
def test_noise_extreme_tolerances(gpu, row_tol, time_tol):
    c, order_w, lab_w, grp_w = _want("noise", row_tol, time_tol)
    members = grp_w[:, 0][grp_w[:, 0] > 0]
    print("k %d groups %d largest %d" % (len(c), len(members), members.max()))
    assert len(c) >= 100 and len(members) >= 10
    if row_tol:  # thin enough not to merge into one group, dense enough to merge
        assert members.max() >= 3
    _same(c, _raw(c, row_tol, time_tol, 64), (order_w, lab_w, grp_w))


# ---- 2. depth: chains and a star (the oracle is the statement itself) ----

def _chain(n, w):
    snr = 6.0 + ((np.arange(n) * 7919) % 1000) / 100.0
    return so.cands(np.zeros(n), 1024 * np.arange(n), np.full(n, w), snr)


def test_chain_one_group(gpu):
    n = 6000
    c = _chain(n, 1024)  # each touches only the next
    order, lab, grp = _raw(c, 0, 0, 1)
    np.testing.assert_array_equal(order, np.arange(n))
    np.testing.assert_array_equal(lab, np.zeros(n, dtype=np.int32))
    best = int(np.argmax(c[:, 3].view(np.float32)))  # (the first of the largest)
    assert list(grp[0]) == [n, best, 0, 0, 0, 1024 * n, c[best, 3], 0]
    assert not grp[1:].any()


def test_chain_no_group(gpu):
    n = 6000
    c = _chain(n, 1023)  # one sample short of the next
    order, lab, grp = _raw(c, 0, 0, 1)
    np.testing.assert_array_equal(lab, np.arange(n, dtype=np.int32))
    want = np.zeros((n, 8), dtype=np.int32)
    want[:, 0], want[:, 1], want[:, 4] = 1, np.arange(n), c[:, 1]
    want[:, 5], want[:, 6] = c[:, 1] + 1023, c[:, 3]
    np.testing.assert_array_equal(grp, want)


@pytest.mark.parametrize("row_tol", [16, 15])
def test_star(gpu, row_tol):
    # window i: a short candidate in row 0 (canonical index 2 i) inside the
    # extent of a wide one in row 16 (index 2 i + 1) that touches the next
    n = 3000
    i = np.arange(n)
    c = np.concatenate([so.cands(np.zeros(n), 1024 * i + 500, np.ones(n), np.full(n, 6.5)),
                        so.cands(np.full(n, 16), 1024 * i, np.full(n, 1024), np.full(n, 8.0))])
    order, lab, grp = _raw(c, row_tol, 0, 17)
    cs = c[order]
    assert np.all(cs[0::2, 0] == 0) and np.all(cs[1::2, 0] == 16)
    if row_tol == 16:  # one group through the wide ones
        np.testing.assert_array_equal(lab, np.zeros(2 * n, dtype=np.int32))
        assert list(grp[0]) == [2 * n, 1, 0, 16, 0, 1024 * n, cs[1, 3], 0]
        assert not grp[1:].any()
    else:  # the short ones alone, the wide ones one group
        np.testing.assert_array_equal(lab[0::2], 2 * i)
        np.testing.assert_array_equal(lab[1::2], np.ones(n, dtype=np.int32))
        assert list(grp[1]) == [n, 1, 16, 16, 0, 1024 * n, cs[1, 3], 0]
        np.testing.assert_array_equal(grp[0::2, 0], np.ones(n))
        assert not grp[3::2].any()


# ---- 3. the reach-2 pair ----

@pytest.mark.parametrize("time_tol,linked", [(1023, True), (1022, False)])
def test_reach_two_pair(gpu, time_tol, linked):
    c = so.cands([5, 5], [0, 2048], [1025, 1], [8.0, 7.0])
    got = _raw(c, 0, time_tol, 6)
    assert list(got[1]) == ([0, 0] if linked else [0, 1])
    _same(c, got, so.group(c, 0, time_tol))
    # and with other windows' candidates between the two in the list
    c = np.concatenate([c, so.cands([0, 1, 4, 5], [1030, 1500, 1024, 5000], [1, 1, 1, 1],
                                    [6, 6, 6, 6])])
    got = _raw(c, 0, time_tol, 6)
    want = so.group(c, 0, time_tol)
    far = int(np.flatnonzero(c[want[0], 1] == 2048)[0])
    assert far == 4 and (want[1][far] == 0) == linked
    _same(c, got, want)


# ---- 4. several candidates per cell ----

@pytest.mark.parametrize("row_tol,time_tol", [(2, 3), (1, 100)])
def test_several_per_cell(gpu, row_tol, time_tol):
    c, order_w, lab_w, grp_w = _want("cell", row_tol, time_tol)
    cells = (c[:, 1] // 1024) * 32 + c[:, 0]
    assert len(c) >= 300 and np.all(np.unique(cells, return_counts=True)[1] == 3)
    members = grp_w[:, 0][grp_w[:, 0] > 0]
    assert 1 < len(members) < len(c)
    _same(c, _raw(c, row_tol, time_tol, 32), (order_w, lab_w, grp_w))


# ---- 5. order and determinism ----

def test_order_and_determinism(gpu):
    from pypulsar_amd.spgroup import SinglePulseGrouper
    c, order_w, lab_w, grp_w = _want("ties", 2, 3)
    dms = np.linspace(0.0, 63.0, 64)
    grouper = SinglePulseGrouper()
    first = None
    for seed in (0, 1, 2):
        perm = np.random.default_rng(seed).permutation(len(c))
        cp = c[perm]
        order, lab, grp = _raw(cp, 2, 3, 64)
        # (one candidate a cell: the canonical list itself is order free)
        np.testing.assert_array_equal(cp[order], c[order_w])
        np.testing.assert_array_equal(lab, lab_w)
        np.testing.assert_array_equal(grp, grp_w)
        rec = _records(cp, dms)
        group_of, groups = grouper(rec)
        _check_records(rec, group_of, groups, cp, so.group(cp, 2, 3))
        back = np.empty(len(c), dtype=np.int64)
        back[perm] = group_of  # group of every candidate of the unshuffled list
        if first is None:
            first = (back, groups)
        np.testing.assert_array_equal(back, first[0])
        assert groups.tobytes() == first[1].tobytes()
    a, b = _raw(c, 2, 3, 64), _raw(c, 2, 3, 64)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- 6. edge sizes ----

def test_empty_and_single(gpu):
    import torch
    from pypulsar_amd.search import CAND_DTYPE
    from pypulsar_amd.spgroup import GROUP_DTYPE, SinglePulseGrouper
    g = SinglePulseGrouper()
    order, lab, grp = g.raw(torch.empty((0, 4), dtype=torch.int32, device="cuda"), 8)
    assert order.shape == (0,) and lab.shape == (0,) and grp.shape == (0, 8)
    group_of, groups = g(np.empty(0, dtype=CAND_DTYPE))
    assert len(group_of) == 0 and len(groups) == 0 and groups.dtype == GROUP_DTYPE
    c = so.cands([3], [5000], [9], [7.5])
    order, lab, grp = _raw(c, 2, 3, 4)
    assert list(order) == [0] and list(lab) == [0]
    assert list(grp[0]) == [1, 0, 3, 3, 5000, 5009, c[0, 3], 0]


def test_row_clamp(gpu):
    # rows 0 and nrows - 1 with the widest row tolerance: the ranges of rows
    # r - 16 .. r + 16 are cut at the plane's edges
    nrows = 20
    rows = [0, 0, 19, 19, 3, 16, 0, 19]
    starts = [10, 1034, 12, 1030, 11, 13, 3000, 3001]
    c = so.cands(rows, starts, [4] * 8, 6.0 + np.arange(8))
    for row_tol in (16, 3, 0):
        _same(c, _raw(c, row_tol, 1023, nrows), so.group(c, row_tol, 1023))
    assert list(so.group(c, 16, 1023)[1]) == [0] * 6 + [6, 7]


def test_sample_offsets_beyond_int32(gpu):
    from pypulsar_amd.spgroup import SinglePulseGrouper
    c, order_w, lab_w, grp_w = _want("cell", 2, 3)
    dms = np.linspace(0.0, 31.0, 32)
    t0 = 5 * (1 << 31) + 777  # (no multiple of 1024: the windows move)
    rec = _records(c, dms, t0)
    group_of, groups = SinglePulseGrouper()(rec)
    off = (t0 // 1024) * 1024
    cw = c.copy()
    cw[:, 1] += t0 - off
    _check_records(rec, group_of, groups, cw, so.group(cw, 2, 3))
    assert groups["SampleLo"].min() > (1 << 31)
    np.testing.assert_allclose(groups["Tbegin"], groups["SampleLo"] * DT, rtol=1e-12)
    np.testing.assert_allclose(groups["Tend"], groups["SampleHi"] * DT, rtol=1e-12)
    # a span that does not fit int32 is refused
    rec2 = rec.copy()
    rec2["Sample"][0] += 1 << 31
    with pytest.raises(ValueError):
        SinglePulseGrouper()(rec2)
    # rows through dms= (as after gather_candidates, whose rows are rank-local)
    rec3 = rec.copy()
    rec3["row"] = -1
    g3 = SinglePulseGrouper()(rec3, dms=dms)
    np.testing.assert_array_equal(g3[0], group_of)
    np.testing.assert_array_equal(g3[1]["rowlo"], groups["rowlo"])
    rec3["DM"][5] += 0.01
    with pytest.raises(ValueError):
        SinglePulseGrouper()(rec3, dms=dms)


# ---- 7. end to end on a plane ----

def burst_plane():
    """[32, 8192] noise; a burst at sample 3000 whose amplitude falls and
    width grows with |row - 16|; a single-sample spike at 6000 in all rows,
    strongest in row 0."""
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (32, 8192)).astype(np.float32)
    for r in range(32):
        dr = abs(r - 16)
        w = 2 + 2 * dr
        snr = 36.0 / (1.0 + dr / 3.0)
        x[r, 3000 - w // 2:3000 - w // 2 + w] += np.float32(snr / np.sqrt(w))
        x[r, 6000] += np.float32(16.0 if r == 0 else 11.0)
    return x


def test_plane_end_to_end(gpu):
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    from pypulsar_amd.spgroup import SinglePulseGrouper, select
    dms = np.linspace(0.0, 62.0, 32)
    rec = SinglePulseSearch(threshold=7)(torch.from_numpy(burst_plane()).cuda(), dms, DT)
    assert 40 <= len(rec) <= 200
    group_of, groups = SinglePulseGrouper()(rec)
    c = so.cands(rec["row"], rec["Sample"], rec["Downfact"], rec["Sigma"])
    _check_records(rec, group_of, groups, c, so.group(c, 2, 3))
    burst = groups[np.argmax(groups["Sigma"])]
    assert burst["row"] == 16 and burst["Members"] >= 10
    assert burst["SampleLo"] <= 3000 < burst["SampleHi"]
    assert burst["DMlo"] == dms[burst["rowlo"]] and burst["DMhi"] == dms[burst["rowhi"]]
    assert burst["Tbegin"] == pytest.approx(burst["SampleLo"] * DT, abs=1e-9)
    assert burst["Tend"] == pytest.approx(burst["SampleHi"] * DT, abs=1e-9)
    # every member of the burst's group is near it
    mem = rec[group_of == int(np.argmax(groups["Sigma"]))]
    assert len(mem) == burst["Members"] and np.all(np.abs(mem["Sample"] - 3000) < 64)
    spike = groups[(groups["SampleLo"] <= 6000) & (groups["SampleHi"] > 6000)]
    assert len(spike) == 1 and spike[0]["row"] == 0 and spike[0]["Members"] == 32
    kept = select(groups, min_dm=dms[1])
    assert len(kept) == len(groups) - 1 and not np.any(kept["row"] == 0)
    assert np.any((kept["row"] == 16) & (kept["Sample"] == burst["Sample"]))


# ---- 8. the CLI ----

def test_frb_search_group_cli(gpu, tmp_path, capsys):
    """The burst file of test_frb_search_cli: --group writes .spgroups and
    leaves the .singlepulse file as it is without it."""
    from conftest import u8_data
    from pypulsar_amd.bin import frb_search as fs
    from pypulsar_amd.delays import delay_from_DM
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.spgroup import read_groups
    C, N, block, dt = 128, 3 * 8192, 8192, 64e-6
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, 8, dt, 1550.0 + foff / 2, foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    freqs = 1550.0 + foff / 2 + foff * np.arange(C)
    x = u8_data(C, N, 31).astype(np.int32).T.copy()  # [N, C] file order
    bins = np.round((delay_from_DM(40.0, freqs) - delay_from_DM(40.0, freqs.max())) / dt)
    t_arr = 9000
    for ch in range(C):
        x[t_arr + int(bins[ch]):t_arr + int(bins[ch]) + 8, ch] += 30
    fn = str(tmp_path / "burst.fil")
    fbm.write_filterbank(fn, params, hdr, np.clip(x, 0, 255).astype(np.uint8))
    args = ["--lodm", "0", "--hidm", "80", "--numdms", "81", "--downsamp", "2", "--block",
            str(block), "-t", "8"]
    plain, grouped = str(tmp_path / "plain.singlepulse"), str(tmp_path / "grouped.singlepulse")
    assert fs.main(args + ["-o", plain, fn]) == 0
    assert not os.path.exists(str(tmp_path / "plain.spgroups"))
    assert fs.main(args + ["--group", "--min-members", "3", "-o", grouped, fn]) == 0
    assert open(plain, "rb").read() == open(grouped, "rb").read()
    assert "groups" in capsys.readouterr().out
    groups = read_groups(str(tmp_path / "grouped.spgroups"))
    assert len(groups) >= 1 and np.all(groups["Members"] >= 3)
    best = groups[np.argmax(groups["Sigma"])]
    assert abs(best["DM"] - 40.0) <= 2.0
    assert abs(best["Time"] - t_arr * dt) <= 16 * dt
    assert best["DMlo"] <= best["DM"] <= best["DMhi"]
    assert best["Tbegin"] <= best["Time"] < best["Tend"]
