"""The fold and its refinement search on the GPU (pdd_fold_rows,
pdd_fold_search through pypulsar_amd.fold.Folder) against the NumPy oracle
(tests/fold_oracle.py), and end to end behind the sweep and the periodicity
search.  Bars: integer-valued rows fold bit-exactly; everything else holds to
conftest.rel_err <= 1e-5, the project's float bar."""
import os

import numpy as np
import pytest

import fold_oracle as fo
from conftest import band, rel_err
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = 64e-6
BAR = 1e-5
D, N, LD, NPART, NBINS = 5, 5003, 5120, 7, 50
# (row, f, fd, phi0): row 2 twice, row 3 unused;
#   a period of 20 samples (< nbins: 30 bins stay empty),
#   a period of 2000 samples (> the 714 of a part: most bins of a part empty),
#   accelerations of either sign worth about 2000 turns over the row,
#   a start phase just below 1
JOBS = ((0, 1.0 / (20 * DT), 0.0, 0.0), (2, 1.0 / (2000 * DT), 0.0, 0.25),
        (2, 91.3, 4.0e4, 0.0), (4, 5.1, -4.0e4, 0.3), (1, 777.7, 0.0, 0.9999999))


def _int_rows(seed, D=D, n=N):
    rng = np.random.default_rng(seed)
    return np.round(524288.0 + rng.normal(0.0, 1024.0, (D, n))).astype(np.float32)


def _strided(x, ld):
    import torch
    big = torch.full((x.shape[0], ld), 7.0e5, dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = torch.from_numpy(np.array(x)).cuda()
    return big[:, :x.shape[1]]


def _jobs(jobs=JOBS):
    return [(r,) + fo.phase_steps(f, fd, DT, phi0) for r, f, fd, phi0 in jobs]


def _fold(folder, view, jobs=JOBS):
    rows, f, fd, phi0 = (np.asarray(v) for v in zip(*jobs))
    return [t.cpu().numpy() for t in folder.fold(view, rows, f, fd, DT, phi0)]


@pytest.fixture(scope="module")
def int_case():
    x = _int_rows(31)
    ref = fo.fold_rows(x, _jobs(), NPART, NBINS)
    x.setflags(write=False)
    return x, ref


def test_fold_integer_rows_exact(gpu, int_case):
    from pypulsar_amd.fold import Folder
    x, (prof, cnt, sumsq) = int_case
    view = _strided(x, LD)
    assert view.stride(0) == LD
    gp, gc, gs = _fold(Folder(NPART, NBINS), view)
    assert gp.dtype == np.float64 and gc.dtype == np.int32 and gp.shape == (5, NPART, NBINS)
    assert np.all(cnt.sum(axis=2) == N // NPART)        # (the remainder is dropped)
    assert np.count_nonzero(cnt[0].sum(axis=0)) == 20   # period < nbins: empty bins
    assert np.count_nonzero(cnt[1, 0]) < NBINS // 2     # period > part: mostly empty
    np.testing.assert_array_equal(gc, cnt)
    np.testing.assert_array_equal(gp, prof)
    e = rel_err(gs, sumsq)
    print("fold int: sumsq rel err %.3g" % e)
    assert e <= BAR
    # jobs of the same row at other phases do not disturb each other; a second
    # run gives the same bits
    gp2, gc2, _ = _fold(Folder(NPART, NBINS), view)
    np.testing.assert_array_equal(gp2, gp)
    np.testing.assert_array_equal(gc2, gc)


def test_fold_gaussian_rows(gpu):
    from pypulsar_amd.fold import Folder
    x = np.random.default_rng(32).normal(3.0, 10.0, (D, N)).astype(np.float32)
    prof, cnt, sumsq = fo.fold_rows(x, _jobs(), NPART, NBINS)
    gp, gc, gs = _fold(Folder(NPART, NBINS), _strided(x, LD))
    np.testing.assert_array_equal(gc, cnt)
    ep, es = rel_err(gp, prof), rel_err(gs, sumsq)
    print("fold float: prof rel err %.3g, sumsq rel err %.3g" % (ep, es))
    assert ep <= BAR and es <= BAR


@pytest.mark.parametrize("npart,nbins,n", [(7, 2, N), (32, 256, N), (128, 64, N), (1, 50, 40001)])
def test_fold_extremes(gpu, npart, nbins, n):
    # (n = 40001 in one part: three workgroup slices of several tiles each)
    import torch
    from pypulsar_amd.fold import Folder
    x = _int_rows(33, 3, n)
    jobs = ((1, 1.0 / (37.3 * DT), 0.0, 0.0), (2, 333.3, -2.0e3, 0.7))
    prof, cnt, sumsq = fo.fold_rows(x, _jobs(jobs), npart, nbins)
    gp, gc, gs = _fold(Folder(npart, nbins), torch.from_numpy(x).cuda(), jobs)
    np.testing.assert_array_equal(gc, cnt)
    np.testing.assert_array_equal(gp, prof)
    assert rel_err(gs, sumsq) <= BAR


def test_fold_no_jobs_and_bad_row(gpu):
    import torch
    from pypulsar_amd._lib import PddError
    from pypulsar_amd.fold import Folder
    xd = torch.from_numpy(_int_rows(34, 3, 1000)).cuda()
    f = Folder(4, 16)
    prof, cnt, sumsq = f.fold(xd, [], 10.0, 0.0, DT)
    assert prof.shape == (0, 4, 16) and cnt.shape == (0, 4, 16) and sumsq.shape == (0, 4)
    chi2, best, bc, bp, bn = f.search(prof, cnt, sumsq)
    assert chi2.shape == (0, 33, 33) and best.shape == (0, 2) and bp.shape == (0, 16)
    for rows in ([0, 3], [-1]):
        with pytest.raises(PddError, match="outside"):
            f.fold(xd, rows, 10.0, 0.0, DT)
    torch.cuda.synchronize()


def _search(folder, prof, cnt, sumsq):
    import torch
    out = folder.search(*(torch.from_numpy(np.array(v)).cuda() for v in (prof, cnt, sumsq)))
    return [t.cpu().numpy() for t in out]


def _check_search(got, prof, cnt, sumsq, A, B, what):
    chi2, best, bc, bp, bn = got
    for j in range(len(prof)):
        want, wbest, wbc, wS, wC = fo.search(prof[j], cnt[j], sumsq[j], A, B)
        assert chi2[j].shape == want.shape == (2 * A + 1, 2 * B + 1)
        e = rel_err(chi2[j], want)
        print("%s job %d: chi2 plane rel err %.3g (max |diff| %.3g), best %s chi2 %.6g" % (
            what, j, e, np.max(np.abs(chi2[j] - want)), wbest, wbc))
        assert e <= BAR
        assert (int(best[j, 0]), int(best[j, 1])) == wbest
        assert rel_err(bc[j], wbc) <= BAR and bc[j] == chi2[j][wbest[0] + A, wbest[1] + B]
        np.testing.assert_array_equal(bn[j], wC)
        np.testing.assert_array_equal(bp[j], wS)


def test_search_offset_pulse_train(gpu):
    from pypulsar_amd.fold import Folder
    c = fo.search_case()
    f = Folder(c["npart"], c["nbins"], c["A"], c["B"])
    got = _search(f, c["prof"], c["cnt"], c["sumsq"])
    e = rel_err(got[0][0], c["chi2"])
    print("search: chi2 plane rel err %.3g, max |diff| %.3g" % (
        e, np.max(np.abs(got[0][0] - c["chi2"]))))
    assert e <= BAR
    assert (int(got[1][0, 0]), int(got[1][0, 1])) == c["best"]
    np.testing.assert_array_equal(got[3][0], c["S"])
    np.testing.assert_array_equal(got[4][0], c["C"])
    # the device's own fold of the same row gives the same search
    import torch
    prof, cnt, sumsq = f.fold(torch.from_numpy(c["x"].copy()).cuda()[None, :], [0], c["f"],
                              c["fd"], c["dt"])
    np.testing.assert_array_equal(prof.cpu().numpy(), c["prof"])
    chi2, best = f.search(prof, cnt, sumsq)[:2]
    assert rel_err(chi2.cpu().numpy()[0], c["chi2"]) <= BAR
    assert tuple(int(v) for v in best.cpu().numpy()[0]) == c["best"]


def test_search_single_trial_and_single_part(gpu, int_case):
    from pypulsar_amd.fold import Folder
    c = fo.search_case()
    _check_search(_search(Folder(c["npart"], c["nbins"], 0, 0), c["prof"], c["cnt"], c["sumsq"]),
                  c["prof"], c["cnt"], c["sumsq"], 0, 0, "A=B=0")
    # one part: every shift is 0, every trial the same chi-square, best (0, 0)
    x, _ = int_case
    prof, cnt, sumsq = fo.fold_rows(x, _jobs(JOBS[:3]), 1, NBINS)
    got = _search(Folder(1, NBINS, 3, 2), prof, cnt, sumsq)
    _check_search(got, prof, cnt, sumsq, 3, 2, "npart=1")
    assert np.all(got[1] == 0)
    for j in range(3):
        assert np.all(got[0][j] == got[0][j, 0, 0])


def test_search_empty_bins_and_constant_row(gpu, int_case):
    from pypulsar_amd.fold import Folder
    x, (prof, cnt, sumsq) = int_case
    # job 0 has 30 bins without a sample (C[b] == 0 in every trial of B = 0,
    # A = 0 and in many others); job 1 has parts that are mostly empty
    assert np.count_nonzero(cnt[0].sum(axis=0) == 0) == 30
    got = _search(Folder(NPART, NBINS, 5, 5), prof, cnt, sumsq)
    _check_search(got, prof, cnt, sumsq, 5, 5, "empty bins")
    assert np.all(np.isfinite(got[0]))
    # a constant row: var == 0, chi-square 0, best trial (0, 0)
    const = np.full((1, N), 37.0, dtype=np.float32)
    cp, cc, cs = fo.fold_rows(const, _jobs(((0, 300.0, 0.0, 0.0),)), NPART, NBINS)
    got = _search(Folder(NPART, NBINS, 4, 3), cp, cc, cs)
    assert np.all(got[0] == 0.0) and np.all(got[1] == 0) and got[2][0] == 0.0
    np.testing.assert_array_equal(got[3][0], cp[0].sum(axis=0))


def test_large_configuration_search(gpu):
    # 8192 staged cells (the LDS limit), 4 bins per lane, parts beyond 64
    from pypulsar_amd.fold import Folder
    x = _int_rows(35, 1, 40001)
    x[0, ::977] += 9000.0
    for npart, nbins in ((32, 256), (128, 64)):
        prof, cnt, sumsq = fo.fold_rows(x, _jobs(((0, 1.0 / (977.4 * DT), 0.0, 0.1),)), npart, nbins)
        got = _search(Folder(npart, nbins, 3, 2), prof, cnt, sumsq)
        _check_search(got, prof, cnt, sumsq, 3, 2, "npart=%d nbins=%d" % (npart, nbins))


def test_non_default_stream(gpu, int_case):
    import torch
    from pypulsar_amd.fold import Folder
    x, (prof, cnt, sumsq) = int_case
    f = Folder(NPART, NBINS, 5, 5)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view = _strided(x, LD)
        rows, fr, fd, phi0 = (np.asarray(v) for v in zip(*JOBS))
        gp, gc, gs = f.fold(view, rows, fr, fd, DT, phi0)
        out = f.search(gp, gc, gs)
    s.synchronize()
    np.testing.assert_array_equal(gp.cpu().numpy(), prof)
    np.testing.assert_array_equal(gc.cpu().numpy(), cnt)
    _check_search([t.cpu().numpy() for t in out], prof, cnt, sumsq, 5, 5, "stream")


E2E_DMS = np.linspace(52.0, 67.0, 16)   # 1 pc/cc steps; the injected DM 60 is row 8
E2E_PERIOD = 16384 / 265.2              # samples: 0.2 Fourier bins off a bin centre


@pytest.fixture(scope="module")
def pulsar_data():
    C, n, width = 64, 1 << 14, 2
    freqs = band(C)
    rng = np.random.default_rng(22)
    x = rng.normal(128.0, 16.0, (C, n))
    delays = orc.sweep_table([60.0], freqs, DT)[0]
    turns = np.arange(int(n / E2E_PERIOD) + 1)
    for c in range(C):
        for w in range(width):
            t = np.round(7 + turns * E2E_PERIOD).astype(np.int64) + w + int(delays[c])
            x[c, t[t < n]] += 12.0
    return freqs, np.clip(np.round(x), 0, 255).astype(np.uint8)


def test_end_to_end(gpu, pulsar_data, tmp_path):
    import torch
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.fold import Folder, read_bestprof, write_bestprof
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.periodicity import PeriodicitySearch, sift
    from pypulsar_amd.sweep import DMSweep
    freqs, x = pulsar_data
    sw = DMSweep(E2E_DMS, freqs, DT, dtype="f32")
    plane = sw(torch.from_numpy(x).cuda().float())
    n = plane.shape[1]
    assert plane.shape[0] == 16 and 8192 < n < 16384
    s = sift(PeriodicitySearch()(plane, E2E_DMS, DT, nfft=16384))
    top = s[0]
    assert abs(top.row - 8) <= 1 and abs(top.r - 265.2) <= 1.0, top
    folder = Folder(npart=8, nbins=32)
    fc = folder(plane, E2E_DMS, DT, [top])[0]
    sw.close()
    print(fc, fc.trial, fc.chi2_vs_dm)
    T = folder.span(n, DT)
    p_inj = E2E_PERIOD * DT
    assert abs(fc.row - 8) <= 1 and fc.dm == E2E_DMS[fc.row]
    # one trial step in frequency is 1 / (nbins T)
    assert abs(1.0 / fc.period - 1.0 / p_inj) <= 1.0 / (32 * T)
    assert fc.rows.tolist() == list(range(top.row - 2, top.row + 3))
    assert abs(int(fc.rows[np.argmax(fc.chi2_vs_dm)]) - 8) <= 1
    assert fc.chi2 == fc.chi2_vs_dm.max() == fc.chi2_plane.max() and fc.chi2 > 10.0
    assert fc.sigma > 8.0 and np.isfinite(fc.sigma)
    assert fc.subints.shape == (8, 32) and fc.chi2_plane.shape == (65, 65)
    np.testing.assert_array_equal(fc.subints.sum(axis=0), fc.profile)
    np.testing.assert_array_equal(fc.subint_counts.sum(axis=0), fc.counts)
    assert fc.counts.sum() == fc.nsamp == 8 * (n // 8)
    # (row, freq) pairs are candidates too
    fc2 = folder(plane, E2E_DMS, DT, [(top.row, top.freq)])[0]
    assert (fc2.row, fc2.trial, fc2.chi2) == (fc.row, fc.trial, fc.chi2)
    # a candidate without a row (read back from a file) folds at the nearest DM trial
    from pypulsar_amd.periodicity import SiftedCandidate
    norow = SiftedCandidate(top.dm, top.r, top.period, top.numharm, top.power, top.sigma)
    fc3 = folder(plane, E2E_DMS, DT, [norow])[0]
    assert norow.row == -1 and (fc3.row, fc3.trial, fc3.chi2) == (fc.row, fc.trial, fc.chi2)
    fn = str(tmp_path / "top.bestprof")
    write_bestprof(fc, fn, infile="psr.fil", candname="top")
    hdr, prof = read_bestprof(fn)
    assert hdr["Best DM"] == fc.dm and hdr["P_topo (ms)"] == 1000.0 * fc.period
    assert hdr["Reduced chi-sqr"] == fc.chi2 and hdr["Data Folded"] == fc.nsamp
    np.testing.assert_array_equal(prof, fc.profile / fc.counts)

    # the command line: without --fold only the .accelcands file, with
    # --fold 3 the same file and a .bestprof / .npz pair per candidate
    C = x.shape[0]
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), float(freqs[1] - freqs[0]),
                                      src_raj=123456.789, src_dej=-123456.5)
    os.mkdir(str(tmp_path / "a"))
    os.mkdir(str(tmp_path / "b"))
    for d in "ab":
        fbm.write_filterbank(str(tmp_path / d / "psr.fil"), params, hdr, x.T.copy())
    args = ["--lodm", "52", "--hidm", "67", "--numdms", "16", "--nfft", "16384"]
    assert pulsar_search.main(args + [str(tmp_path / "a" / "psr.fil")]) == 0
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["psr.accelcands", "psr.fil"]
    assert pulsar_search.main(args + ["--fold", "3", "--fold-nbins", "32", "--fold-npart", "8",
                                      str(tmp_path / "b" / "psr.fil")]) == 0
    k = min(3, len(s))
    want = ["psr.accelcands", "psr.fil"] + ["psr_cand%d.%s" % (i, e) for i in range(1, k + 1)
                                            for e in ("bestprof", "npz")]
    assert sorted(os.listdir(str(tmp_path / "b"))) == sorted(want)
    assert open(str(tmp_path / "a" / "psr.accelcands")).read() == \
        open(str(tmp_path / "b" / "psr.accelcands")).read()
    hdr1, prof1 = read_bestprof(str(tmp_path / "b" / "psr_cand1.bestprof"))
    assert hdr1["Best DM"] == fc.dm and hdr1["Reduced chi-sqr"] == fc.chi2
    np.testing.assert_array_equal(prof1, prof)
    z = np.load(str(tmp_path / "b" / "psr_cand1.npz"))
    np.testing.assert_array_equal(z["subints"], fc.subints)
    np.testing.assert_array_equal(z["chi2_plane"], fc.chi2_plane)
    np.testing.assert_array_equal(z["chi2_vs_dm"], fc.chi2_vs_dm)
