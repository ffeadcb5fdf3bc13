"""Candidate cut-outs on the GPU (pypulsar_amd/cutout.py, csrc/pdd_cutout.hip)
against the brute-force oracle (tests/cutout_oracle.py).

8-bit input with no pad values: exact equality with float32(integer sum).
float32 input, or 8-bit input with non-zero pad values: |got - ref| <=
1e-5 max|ref| (the project's parity bar)."""
import functools
import os

import numpy as np
import pytest

import cutout_oracle as co
from conftest import band, u8_data

pytestmark = pytest.mark.gpu
DT = 64e-6
N, NBIN, NDM = 4096, 32, 16


@functools.lru_cache(maxsize=None)
def _block(C, kind):
    """Host block [N, C + 5] (ld > C; the spare columns hold what must never
    be read as data: 255 / 1e6)."""
    if kind == "u8":
        x = np.full((N, C + 5), 255, dtype=np.uint8)
        x[:, :C] = u8_data(C, N, 3).T
    else:
        x = np.full((N, C + 5), 1e6, dtype=np.float32)
        x[:, :C] = np.random.default_rng(4).normal(0.0, 3.0, (N, C)).astype(np.float32)
    x.setflags(write=False)
    return x


def _jobs(freqs, dm, t0, f, nsub, h=None, nbin=NBIN, ndm=NDM):
    """Jobs with the given DMs, first samples and factors."""
    from pypulsar_amd.cutout import plan_jobs
    from pypulsar_amd.search import CAND_DTYPE
    dm = np.atleast_1d(np.asarray(dm, dtype=np.float64))
    rec = np.zeros(len(dm), dtype=CAND_DTYPE)
    rec["DM"], rec["Downfact"] = dm, 1
    jobs = plan_jobs(rec, 1, freqs, DT, nbin, nsub, ndm, factor=np.asarray(f), dm_half=h)
    jobs.t0[:] = t0
    return jobs


def _run(x, freqs, jobs, padvals=None, **kw):
    import torch
    from pypulsar_amd.cutout import Cutouts
    C = len(freqs)
    dev = torch.from_numpy(np.array(x)).cuda()[:, :C]
    assert dev.stride(0) > C or x.shape[1] == C
    pv = None if padvals is None else torch.from_numpy(np.asarray(padvals, np.float32)).cuda()
    ft, dmt = Cutouts(freqs, DT, jobs.nbin, jobs.nsub, jobs.ndm, **kw)(dev, 0, jobs, padvals=pv)
    torch.cuda.synchronize()
    assert ft.dtype == torch.float32 and dmt.dtype == torch.float32
    return ft.cpu().numpy(), dmt.cpu().numpy()


def _ref(x, freqs, jobs, i, padvals=None):
    """Oracle images of job i: ((ft inside, pad), (dmt inside, pad))."""
    xs = np.asarray(x)[:, :len(freqs)]
    a = co.ft_image(xs, freqs, DT, int(jobs.t0[i]), int(jobs.f[i]), jobs.dms[i, jobs.ndm // 2],
                    jobs.nbin, jobs.nsub, padvals)
    b = co.dmt_image(xs, freqs, DT, int(jobs.t0[i]), int(jobs.f[i]), jobs.dms[i], jobs.nbin,
                     padvals)
    return a, b


def _check(x, freqs, jobs, got, padvals=None, exact=True):
    ft, dmt = got
    assert ft.shape == (len(jobs), jobs.nsub, jobs.nbin)
    assert dmt.shape == (len(jobs), jobs.ndm, jobs.nbin)
    for i in range(len(jobs)):
        for name, g, (ins, pad) in zip(("ft", "dmt"), (ft[i], dmt[i]),
                                       _ref(x, freqs, jobs, i, padvals)):
            want = co.expected(ins, pad)
            if exact:
                assert ins.dtype.kind == "i" and not pad.any()
                np.testing.assert_array_equal(g, ins.astype(np.float32), err_msg="%s job %d"
                                              % (name, i))
            else:
                scale = np.max(np.abs(want))
                err = np.max(np.abs(g.astype(np.float64) - want))
                print("%s job %d: err %.3g of max %.3g" % (name, i, err, scale))
                assert err <= 1e-5 * scale, (name, i, err, scale)


# six jobs: f in {1, 3, 8} x DM in {0, 60}, windows inside the block
SIX = dict(dm=[0.0, 60.0, 0.0, 60.0, 0.0, 60.0], t0=[700, 900, 650, 872, 400, 800],
           f=[1, 1, 3, 3, 8, 8])


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("C", [64, 48])
def test_u8_exact(gpu, C, descending):
    freqs, x = band(C, descending), _block(C, "u8")
    for nsub in (C, 16, 1):
        jobs = _jobs(freqs, nsub=nsub, **SIX)
        assert jobs.lo.min() >= 0 and jobs.hi.max() <= N
        got = _run(x, freqs, jobs)
        _check(x, freqs, jobs, got)
        # the candidate's own row of the DM-time image is the frequency-time image summed
        np.testing.assert_array_equal(got[1][:, NDM // 2], got[0].astype(np.float64).sum(axis=1))


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("C", [64, 48])
def test_f32(gpu, C, descending):
    freqs, x = band(C, descending), _block(C, "f32")
    for nsub in (C, 16, 1):
        jobs = _jobs(freqs, nsub=nsub, **SIX)
        _check(x, freqs, jobs, _run(x, freqs, jobs), exact=False)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_padding(gpu, kind):
    C = 48
    freqs, x = band(C), _block(C, kind)
    # t0 = -10; past row n; wholly after the block; wholly before it
    jobs = _jobs(freqs, dm=[60.0, 60.0, 0.0, 60.0, 60.0], t0=[-10, N - 100, -10, N + 5000, -100000],
                 f=[3, 8, 1, 3, 8], nsub=16)
    assert jobs.lo[0] < 0 < jobs.hi[0] and jobs.lo[1] < N < jobs.hi[1]
    got0 = _run(x, freqs, jobs)
    _check(x, freqs, jobs, got0, exact=(kind == "u8"))
    for g in got0:  # pad NULL: nothing outside the block
        assert not g[3].any() and not g[4].any()
    pv = (np.arange(C) * 0.25 + 100.5).astype(np.float32)
    got = _run(x, freqs, jobs, padvals=pv)
    _check(x, freqs, jobs, got, padvals=pv, exact=False)
    # the pure pad image
    for i in (3, 4):
        f = float(jobs.f[i])
        np.testing.assert_allclose(got[0][i], np.broadcast_to(
            f * pv.reshape(16, 3).sum(axis=1, dtype=np.float64)[:, None], (16, NBIN)), rtol=1e-5)
        np.testing.assert_allclose(got[1][i], f * pv.sum(dtype=np.float64), rtol=1e-5)


def test_trial_dms_below_zero(gpu):
    C = 64
    for descending in (True, False):
        freqs, x = band(C, descending), _block(C, "u8")
        jobs = _jobs(freqs, dm=[5.0, 5.0], t0=[1500, 1400], f=[1, 3], nsub=16, h=20.0)
        assert jobs.dms.min() < -14 and jobs.bmin.min() < 0 and jobs.lo.min() >= 0
        _check(x, freqs, jobs, _run(x, freqs, jobs))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_batching_same_bits(gpu, kind):
    C = 48
    freqs, x = band(C), _block(C, kind)
    pv = (np.arange(C) * 0.5 + 90.0).astype(np.float32)
    jobs = _jobs(freqs, dm=[0.0, 60.0, 30.0, 60.0, 5.0, 45.5, 60.0],
                 t0=[700, 900, -10, 872, 400, N - 150, 100], f=[1, 8, 3, 3, 8, 1, 2], nsub=16)
    whole = _run(x, freqs, jobs, padvals=pv)
    _check(x, freqs, jobs, whole, padvals=pv, exact=False)
    ones = [_run(x, freqs, jobs.subset([i]), padvals=pv) for i in range(len(jobs))]
    pairs = _run(x, freqs, jobs, padvals=pv, table_bytes=2 * NDM * C * 4)  # batches of 2
    single = _run(x, freqs, jobs, padvals=pv, work_bytes=1)  # one job per pair of launches
    for k in (0, 1):
        assert np.concatenate([o[k] for o in ones]).tobytes() == whole[k].tobytes()
        assert pairs[k].tobytes() == whole[k].tobytes()
        assert single[k].tobytes() == whole[k].tobytes()


def test_factor_limit(gpu):
    import torch
    from pypulsar_amd.cutout import Cutouts
    C = 64
    freqs, x = band(C), _block(C, "u8")
    # f = 1024 at C = 64: the limit (32-bit box sums); most of the window is outside the block
    jobs = _jobs(freqs, dm=[60.0, 60.0], t0=[-3000, 500], f=[1024, 300], nsub=16, nbin=8, ndm=4)
    _check(x, freqs, jobs, _run(x, freqs, jobs))
    # C f 255 >= 2^31 is refused
    wide = band(16384)
    jw = _jobs(wide, dm=[10.0], t0=[0], f=[512], nsub=1, nbin=4, ndm=2)
    jw.f[:] = 1024
    with pytest.raises(ValueError):
        Cutouts(wide, DT, 4, 1, 2)(torch.zeros((4, 16384), dtype=torch.uint8, device="cuda"), 0, jw)


def test_oracle_chain(gpu):
    C = 64
    for descending in (True, False):
        freqs, x = band(C, descending), _block(C, "u8")
        jobs = _jobs(freqs, dm=[60.0, 0.0], t0=[872, 10], f=[3, 8], nsub=C)
        ft, _ = _run(x, freqs, jobs)
        for i in range(2):
            want = co.chain_ft(x[:, :C], freqs, DT, int(jobs.t0[i]), int(jobs.f[i]),
                               float(jobs.dms[i, NDM // 2]), NBIN)
            np.testing.assert_array_equal(ft[i], want)


def test_broken_job_is_nan_not_a_read(gpu):
    """A job whose stated delay bounds do not hold reads nothing outside its
    box sums: the image is NaN, the other jobs are untouched."""
    C = 48
    freqs, x = band(C), _block(C, "u8")
    jobs = _jobs(freqs, dm=[60.0, 60.0], t0=[900, 900], f=[3, 3], nsub=16)
    good = _run(x, freqs, jobs)
    jobs.bmax[1] -= 7
    ft, dmt = _run(x, freqs, jobs)
    assert np.isnan(dmt[1]).any() and not np.isnan(dmt[0]).any()
    np.testing.assert_array_equal(dmt[0], good[1][0])
    np.testing.assert_array_equal(ft, good[0])


def test_frb_search_cutouts_cli(gpu, tmp_path, capsys):
    """The burst file of test_frb_search_group_cli: --cutouts 1 writes the
    .npz, leaves the text outputs as they are, and shows the burst in the
    middle of both images."""
    from pypulsar_amd.bin import frb_search as fs
    from pypulsar_amd.cutout import read_cutouts
    from pypulsar_amd.delays import delay_from_DM
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C, n, block, dt = 128, 3 * 8192, 8192, 64e-6
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, 8, dt, 1550.0 + foff / 2, foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    freqs = 1550.0 + foff / 2 + foff * np.arange(C)
    x = u8_data(C, n, 31).astype(np.int32).T.copy()  # [n, C] file order
    bins = np.round((delay_from_DM(40.0, freqs) - delay_from_DM(40.0, freqs.max())) / dt)
    t_arr = 9000
    for ch in range(C):
        x[t_arr + int(bins[ch]):t_arr + int(bins[ch]) + 8, ch] += 30
    data = np.clip(x, 0, 255).astype(np.uint8)
    fn = str(tmp_path / "burst.fil")
    fbm.write_filterbank(fn, params, hdr, data)
    args = ["--lodm", "0", "--hidm", "80", "--numdms", "81", "--downsamp", "2", "--block",
            str(block), "-t", "8", "--min-members", "3"]
    grouped, cut = str(tmp_path / "grouped.singlepulse"), str(tmp_path / "cut.singlepulse")
    assert fs.main(args + ["--group", "-o", grouped, fn]) == 0
    assert not os.path.exists(str(tmp_path / "grouped_cutouts.npz"))
    nbin, nsub, ndm = 64, 32, 32
    assert fs.main(args + ["--cutouts", "1", "--cutout-bins", str(nbin), "--cutout-subbands",
                           str(nsub), "--cutout-dms", str(ndm), "-o", cut, fn]) == 0
    assert "cut-outs" in capsys.readouterr().out
    assert open(grouped, "rb").read() == open(cut, "rb").read()
    assert open(str(tmp_path / "grouped.spgroups"), "rb").read() == \
        open(str(tmp_path / "cut.spgroups"), "rb").read()
    z = read_cutouts(str(tmp_path / "cut_cutouts.npz"))
    assert z["ft"].shape == (1, nsub, nbin) and z["dmt"].shape == (1, ndm, nbin)
    assert (z["nbin"], z["nsub"], z["ndm"], z["dt"]) == (nbin, nsub, ndm, dt)
    rec = z["records"][0]
    assert abs(rec["DM"] - 40.0) <= 2.0
    assert z["dms"][0, ndm // 2] == rec["DM"]
    assert abs(int(np.argmax(z["ft"][0].sum(axis=0))) - nbin // 2) <= 1
    row = np.unravel_index(np.argmax(z["dmt"][0]), z["dmt"][0].shape)[0]
    assert abs(int(row) - ndm // 2) <= 1
    # the stored image is the oracle's of the file's bytes (the window lies inside the file)
    t0, f = int(z["t0"][0]), int(z["factor"][0])
    ins, pad = co.ft_image(data, freqs, dt, t0, f, float(rec["DM"]), nbin, nsub)
    np.testing.assert_array_equal(z["ft"][0], ins.astype(np.float32))
    ins, pad = co.dmt_image(data, freqs, dt, t0, f, z["dms"][0], nbin)
    np.testing.assert_array_equal(z["dmt"][0], ins.astype(np.float32))
