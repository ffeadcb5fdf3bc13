"""Host side of the candidate cut-outs (pypulsar_amd/cutout.py): the job
geometry of plan_jobs against its restatement (tests/cutout_oracle.py), the
oracle's own invariants, the .npz round trip and the limit checks.  No GPU."""
import numpy as np
import pytest

import cutout_oracle as co
from conftest import band, u8_data
from oracle import spectra_oracle as orc

DT = 64e-6


def _records(dm, sample, downfact):
    from pypulsar_amd.search import CAND_DTYPE
    dm = np.atleast_1d(np.asarray(dm, dtype=np.float64))
    rec = np.zeros(len(dm), dtype=CAND_DTYPE)
    rec["DM"], rec["Sample"], rec["Downfact"] = dm, sample, downfact
    rec["Sigma"] = 8.0 + np.arange(len(dm))
    rec["Time"] = rec["Sample"] * DT
    rec["row"] = -1
    return rec


@pytest.mark.parametrize("descending", [True, False])
def test_plan_jobs_arithmetic(descending):
    from pypulsar_amd.cutout import plan_jobs
    from pypulsar_amd.delays import dedisperse_bins
    freqs = band(64, descending)
    ds, nbin, nsub, ndm, nfile = 2, 32, 16, 16, 50000
    # odd and even W (ds 2: W = 2, 6, 8; ds 1 below), sample 0 and the file's last
    rec = _records([60.0, 5.0, 0.0, 33.3], [1000, 0, nfile // ds - 1, 777], [1, 3, 4, 150])
    jobs = plan_jobs(rec, ds, freqs, DT, nbin, nsub, ndm)
    assert len(jobs) == 4
    tabs = jobs.tables()
    assert tabs.dtype == np.int32 and tabs.shape == (4, ndm, 64)
    for i, r in enumerate(rec):
        f, t0, dms = co.geometry(r["DM"], r["Sample"], r["Downfact"], ds, nbin, ndm)
        assert (jobs.f[i], jobs.t0[i]) == (f, t0)
        np.testing.assert_array_equal(jobs.dms[i], dms)
        assert jobs.dms[i, ndm // 2] == r["DM"]
        np.testing.assert_array_equal(tabs[i, ndm // 2], dedisperse_bins(r["DM"], freqs, DT))
        for j in range(ndm):
            np.testing.assert_array_equal(tabs[i, j], orc.dedisperse_bins(dms[j], 0.0, freqs, DT))
        # the window: every sample either image reads, nothing more
        assert jobs.bmin[i] == tabs[i].min() and jobs.bmax[i] == tabs[i].max()
        assert jobs.lo[i] == t0 + tabs[i].min()
        assert jobs.hi[i] == t0 + nbin * f + tabs[i].max()
    # W = 2, 6, 8, 300 -> f = 1, 3, 4, 150
    assert list(jobs.f) == [1, 3, 4, 150]
    assert jobs.t0[1] == 0 * ds + 3 - 16 * 3 and jobs.t0[1] < 0       # sample 0: negative
    assert jobs.hi[2] > nfile                                          # runs past the end
    assert jobs.dms[1].min() < 0 and jobs.bmin[1] < 0                  # DM 5, h = 10
    # odd W at ds 1
    j1 = plan_jobs(_records([10.0, 10.0], [500, 500], [3, 2]), 1, freqs, DT, nbin, nsub, ndm)
    assert list(j1.f) == [1, 1] and list(j1.t0) == [500 + 1 - 16, 500 + 1 - 16]
    # f and h given; fmax clamps
    j2 = plan_jobs(rec, ds, freqs, DT, nbin, nsub, ndm, factor=5, dm_half=20.0, fmax=100)
    assert list(j2.f) == [5] * 4
    np.testing.assert_allclose(j2.dms[0, 1] - j2.dms[0, 0], 40.0 / ndm)
    j3 = plan_jobs(rec, ds, freqs, DT, nbin, nsub, ndm, fmax=100)
    assert list(j3.f) == [1, 3, 4, 100]
    assert len(plan_jobs(rec[:0], ds, freqs, DT, nbin, nsub, ndm)) == 0
    sub = jobs.subset([2, 0])
    assert list(sub.t0) == [jobs.t0[2], jobs.t0[0]] and sub.tables().shape == (2, ndm, 64)


def test_group_loads():
    from pypulsar_amd.cutout import group_loads
    lo = np.array([900, -50, 100, 5000, 99990, 200000])
    hi = np.array([1500, 300, 800, 9000, 100100, 200100])
    loads = group_loads(lo, hi, 100000, 2000)
    assert [(a, b) for a, b, _ in loads] == [(0, 1500), (5000, 9000), (99990, 100000)]
    assert [sorted(i) for _, _, i in loads] == [[0, 1, 2], [3], [4, 5]]
    assert sorted(i for _, _, idx in loads for i in idx) == list(range(6))


@pytest.mark.parametrize("descending", [True, False])
def test_oracle_invariants(descending):
    C, n, nbin, ndm, f, dm = 64, 6000, 32, 16, 3, 60.0
    freqs = band(C, descending)
    x = u8_data(C, n, 5).T.copy()
    _, t0, dms = co.geometry(dm, 700, 3, 2, nbin, ndm)
    assert t0 >= 0
    ft, _ = co.ft_image(x, freqs, DT, t0, f, dm, nbin, C)
    np.testing.assert_array_equal(ft, co.chain_ft(x, freqs, DT, t0, f, dm, nbin))
    dmt, _ = co.dmt_image(x, freqs, DT, t0, f, dms, nbin)
    np.testing.assert_array_equal(dmt[ndm // 2], ft.sum(axis=0))
    ft16, _ = co.ft_image(x, freqs, DT, t0, f, dm, nbin, 16)
    np.testing.assert_array_equal(ft16, ft.reshape(16, 4, nbin).sum(axis=1))
    # an injected pulse of width W on a plane sample peaks in the middle
    ds, downfact, sample = 2, 3, 1200
    W = downfact * ds
    bins = orc.dedisperse_bins(dm, 0.0, freqs, DT)
    y = np.zeros((n, C), dtype=np.int64)
    for c in range(C):
        y[sample * ds + bins[c]:sample * ds + bins[c] + W, c] = 10
    fj, tj, dmsj = co.geometry(dm, sample, downfact, ds, nbin, ndm)
    ftp, _ = co.ft_image(y, freqs, DT, tj, fj, dm, nbin, 16)
    assert set(np.argmax(ftp, axis=1)) <= {nbin // 2 - 1, nbin // 2}
    dmtp, _ = co.dmt_image(y, freqs, DT, tj, fj, dmsj, nbin)
    assert np.unravel_index(np.argmax(dmtp), dmtp.shape)[0] == ndm // 2
    # pad: a window past both ends counts the missing samples
    pv = np.arange(C) + 0.5
    a, p = co.ft_image(x, freqs, DT, -10, f, 0.0, nbin, 1, pv)
    assert p[0, 0] == 3 * pv.sum() and p[0, 3] == 1 * pv.sum() and p[0, 4] == 0


def test_npz_round_trip(tmp_path):
    from pypulsar_amd.cutout import plan_jobs, read_cutouts, write_cutouts
    from pypulsar_amd.delays import subband_layout
    freqs = band(64)
    rec = _records([60.0, 5.0], [1000, 20], [2, 3])
    jobs = plan_jobs(rec, 2, freqs, DT, 32, 16, 8)
    rng = np.random.default_rng(0)
    ft = rng.normal(size=(2, 16, 32)).astype(np.float32)
    dmt = rng.normal(size=(2, 8, 32)).astype(np.float32)
    fn = str(tmp_path / "c.npz")
    write_cutouts(fn, ft, dmt, rec, jobs)
    z = read_cutouts(fn)
    np.testing.assert_array_equal(z["ft"], ft)
    np.testing.assert_array_equal(z["dmt"], dmt)
    for name in rec.dtype.names:
        np.testing.assert_array_equal(z["records"][name], rec[name])
    np.testing.assert_array_equal(z["factor"], jobs.f)
    np.testing.assert_array_equal(z["t0"], jobs.t0)
    np.testing.assert_array_equal(z["dms"], jobs.dms)
    np.testing.assert_array_equal(z["sub_freqs"], subband_layout(freqs, 16)[2])
    assert (z["dt"], z["nbin"], z["nsub"], z["ndm"]) == (DT, 32, 16, 8)


def test_limits_raise():
    from pypulsar_amd.cutout import plan_jobs
    freqs = band(64)
    rec = _records([60.0], [1000], [2])
    for kw in (dict(nbin=0), dict(nbin=1025), dict(ndm=0), dict(ndm=1025), dict(nsub=7),
               dict(nsub=0), dict(factor=0), dict(factor=1025), dict(fmax=2000),
               dict(dm_half=0.0)):
        args = dict(nbin=32, nsub=16, ndm=16)
        args.update(kw)
        with pytest.raises(ValueError):
            plan_jobs(rec, 2, freqs, DT, **args)
    with pytest.raises(ValueError):
        plan_jobs(_records([60.0], [1000], [0]), 2, freqs, DT, 32, 16, 16)
    # C f 255 >= 2^31
    wide = band(16384)
    plan_jobs(rec, 2, wide, DT, 32, 16, 16, factor=512)
    with pytest.raises(ValueError):
        plan_jobs(rec, 2, wide, DT, 32, 16, 16, factor=1024)
    # table entries beyond int32
    with pytest.raises(OverflowError):
        plan_jobs(_records([1e9], [1000], [2]), 2, freqs, 1e-9, 32, 16, 16)
    # nbin f + the ladder's delay range beyond 2^22
    with pytest.raises(ValueError):
        plan_jobs(_records([3000.0], [1000], [2]), 2, freqs, 1e-6, 1024, 16, 16, factor=1024)
    # f = 1024 at C = 64 sits at the limit
    assert plan_jobs(rec, 2, freqs, DT, 32, 16, 16, factor=1024).f[0] == 1024


def test_abi_refuses_without_gpu():
    """The limits are checked before any HIP call."""
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()
    def ft(dtype=_lib.U8, C=64, nbin=32, nsub=16, fmax=8):
        return h.pdd_cutout_ft(None, dtype, 16, C, C, None, 1, None, 1, None, nbin, nsub, fmax,
                               None, None)

    def dmt(C=64, nbin=32, ndm=16, fmax=8, span=4096, nsub=None):
        return h.pdd_cutout_dmt(None, _lib.U8, 16, C, C, None, 1, None, 16, None, nbin, ndm, fmax,
                                span, None, 0, None, None)

    assert ft() == -1 and b"null pointer" in h.pdd_last_error()
    for bad in (dict(nbin=0), dict(nbin=1025), dict(nsub=7), dict(fmax=0), dict(fmax=1025),
                dict(dtype=_lib.U16)):
        assert ft(**bad) == -1 and b"null pointer" not in h.pdd_last_error(), bad
    for fn in (ft, dmt):
        assert fn(C=16384, nsub=1, fmax=512) == -1 and b"null pointer" in h.pdd_last_error()
        assert fn(C=16384, nsub=1, fmax=1024) == -1 and b"2^31" in h.pdd_last_error()
    for bad in (dict(ndm=0), dict(ndm=1025), dict(span=0), dict(span=(1 << 22) + 1)):
        assert dmt(**bad) == -1 and b"null pointer" not in h.pdd_last_error(), bad
