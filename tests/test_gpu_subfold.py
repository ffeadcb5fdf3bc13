"""The subband fold and its DM refinement on the GPU (pdd_subfold,
pdd_subfold_dm through pypulsar_amd.subfold) against the brute-force oracle
(tests/subfold_oracle.py).  Bars: 8-bit input folds bit-exactly, whatever the
split into blocks; everything else holds to conftest.rel_err <= 1e-5, the
project's float bar."""
import os

import numpy as np
import pytest

import subfold_oracle as so
from conftest import band, rel_err
from test_gpu_fold import JOBS

pytestmark = pytest.mark.gpu
DT = 64e-6
BAR = 1e-5
N, LD, NPART, NSUB, NBINS = 5003, 80, 7, 8, 50
# band(64) at 64 us: about 14.5 rows of delay per unit DM -- bmax of a few rows and of hundreds
DMS = (0.3, 30.0, 30.0, 0.3, 12.0)
SF_JOBS = tuple((dm, f, fd, phi0) for dm, (_, f, fd, phi0) in zip(DMS, JOBS))
_REF = {}


def _u8(C, n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(96, 30, size=(n, C))), 0, 255).astype(np.uint8)


def _view(x, ld, odd=False):
    """x [n, C] inside rows of ld elements of a device buffer filled with
    other values; ``odd``: the view starts one element into the allocation."""
    import torch
    n, C = x.shape
    fill = 201 if x.dtype == np.uint8 else 7.0e5
    flat = torch.full((n * ld + 1,), fill, dtype=torch.from_numpy(x[:1]).dtype, device="cuda")
    v = flat[1 if odd else 0:][:n * ld].view(n, ld)[:, :C]
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return v


def _ref(key, x, freqs, jobs, npart, nsub, nbins):
    """The oracle's fold of a case, computed once."""
    if key not in _REF:
        out = so.subfold(x, freqs, DT, list(jobs), npart, nsub, nbins)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _fold(folder, view, n, jobs, **kw):
    return [t.cpu().numpy() for t in folder.fold(view, 0, n, list(jobs), **kw)]


def _same(got, want):
    for g, w, name in zip(got, want, ("cube", "cnt", "chansum", "chansq")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


CASES = {
    # name: (C, n, ld, npart, nsub, nbins, descending, odd view)
    "base": (64, N, LD, NPART, NSUB, NBINS, True, False),
    "c70": (70, N, LD, NPART, 7, NBINS, True, False),         # 10 channels a subband, C % 4 != 0
    "nsub_is_c": (64, N, LD, NPART, 64, NBINS, True, False),
    "nsub_1": (64, N, LD, NPART, 1, NBINS, True, False),
    "c1": (1, N, 3, NPART, 1, NBINS, True, False),
    "ascending": (64, N, LD, NPART, NSUB, NBINS, False, False),
    "two_slices": (16, 40000, 16, NPART, 4, NBINS, True, False),  # parts of 5714 > 4096 samples
    "odd_offset": (64, N, LD, NPART, NSUB, NBINS, True, True),
    "four_a_lane": (260, 2003, 263, 3, 5, NBINS, True, False),  # 4 channels a lane, a partial tile
    "max_bins": (64, N, LD, 32, 32, 256, True, False),          # more than 64 KiB of LDS
}


def _case(name):
    C, n, ld, npart, nsub, nbins, desc, odd = CASES[name]
    freqs = band(C, desc)
    x = _u8(C, n, 40 + C)
    return x, freqs, _ref((name if name != "odd_offset" else "base"), x, freqs, SF_JOBS, npart,
                          nsub, nbins)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_u8_exact(gpu, name):
    from pypulsar_amd.subfold import SubbandFolder
    C, n, ld, npart, nsub, nbins, desc, odd = CASES[name]
    x, freqs, ref = _case(name)
    view = _view(x, ld, odd)
    assert view.stride(0) == ld and view.data_ptr() % 2 == (1 if odd else 0)
    folder = SubbandFolder(freqs, DT, npart, nsub, nbins)
    jobs = folder.plan(n, *zip(*SF_JOBS))
    if C == 64:
        assert jobs.bmax.min() < 10 and jobs.bmax.max() > 300
    got = _fold(folder, view, n, SF_JOBS)
    assert got[0].shape == (5, npart, nsub, nbins) and got[0].dtype == np.float64
    assert np.all(ref[1].sum(axis=2) == jobs.L[:, None])       # (the remainder is dropped)
    _same(got, ref)


def test_block_splitting_and_job_sets(gpu):
    from pypulsar_amd.subfold import SubbandFolder, plan_blocks
    x, freqs, ref = _case("base")
    view = _view(x, LD)
    folder = SubbandFolder(freqs, DT, NPART, NSUB, NBINS)
    jobs = folder.plan(N, *zip(*SF_JOBS))
    over = int(jobs.bmax.max())
    # three calls with seams at arbitrary rows, consecutive blocks overlapping by bmax
    out = None
    for a, b in ((0, 1777), (1777, 3210), (3210, N)):
        rows = view[a:min(N, b + over)]
        span = (np.minimum(a, jobs.nfold), np.minimum(b, jobs.nfold))
        out = folder.fold(rows, a, N, jobs, out=out, span=span)
    _same([t.cpu().numpy() for t in out], ref)
    # the planner's blocks
    out, blocks = None, plan_blocks(jobs.nfold, jobs.bmax, 1300)
    assert len(blocks) > 3
    for a, b, i0, i1 in blocks:
        out = folder.fold(view[a:b], a, N, jobs, out=out, span=(i0, i1))
    _same([t.cpu().numpy() for t in out], ref)
    # jobs of different DMs in one call equal the jobs run one by one
    for j in (0, 1, 4):
        one = _fold(folder, view, N, SF_JOBS[j:j + 1])
        _same(one, [r[j:j + 1] for r in ref])


@pytest.mark.parametrize("kind", ["gauss", "plane"])
def test_fold_float32(gpu, kind):
    from pypulsar_amd.subfold import SubbandFolder
    rng = np.random.default_rng(51)
    if kind == "gauss":
        x = rng.normal(0.0, 1.0, (N, 64)).astype(np.float32)
    else:  # plane-like: integers near 2^19, exact in float32 and in the float64 sums
        x = np.round(524288.0 + rng.normal(0.0, 1024.0, (N, 64))).astype(np.float32)
    freqs = band(64)
    ref = so.subfold(x, freqs, DT, list(SF_JOBS), NPART, NSUB, NBINS)
    got = _fold(SubbandFolder(freqs, DT, NPART, NSUB, NBINS), _view(x, LD), N, SF_JOBS)
    np.testing.assert_array_equal(got[1], ref[1])
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print("subfold f32 %s: rel err cube %.3g, chansum %.3g, chansq %.3g" % (
        kind, errs[0], errs[2], errs[3]))
    assert max(errs) <= BAR
    if kind == "plane":
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[2], ref[2])


def test_against_sweep_and_fold_on_device(gpu):
    import torch
    from pypulsar_amd.fold import Folder
    from pypulsar_amd.subfold import SubbandFolder
    from pypulsar_amd.sweep import DMSweep
    x, freqs, _ = _case("base")
    xd = torch.from_numpy(x).cuda()
    for dm in (0.3, 30.0):
        jobs = [(dm,) + j[1:] for j in SF_JOBS]
        cube, cnt = SubbandFolder(freqs, DT, NPART, NSUB, NBINS).fold(xd, 0, N, jobs)[:2]
        sw = DMSweep([dm], freqs, DT, dtype="u8")
        plane = sw(xd.t().contiguous())
        sw.close()
        assert plane.shape == (1, N - int(so.delays_of(dm, freqs, DT)[1]))
        _, f, fd, phi0 = (np.asarray(v) for v in zip(*jobs))
        prof, pc, _ = Folder(NPART, NBINS).fold(plane, [0] * len(jobs), f, fd, DT, phi0)
        np.testing.assert_array_equal(cube.sum(dim=2).cpu().numpy(), prof.cpu().numpy())
        np.testing.assert_array_equal(cnt.cpu().numpy(), pc.cpu().numpy())


# ---- the DM refinement ----

def _refine(folder, jobs, ref, trials, dms):
    import torch
    dev = [torch.from_numpy(np.array(a)).cuda() for a in ref]
    res = folder.refine(*dev, jobs, trials=trials, dms=dms)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _check_refine(got, ref, jobs, trials, what):
    worst = 0.0
    for j in range(len(jobs)):
        want = so.refine(ref[0][j], ref[1][j], ref[2][j], ref[3][j], int(jobs.nfold[j]),
                         trials[j], got["r"][j])
        errs = [rel_err(got[k][j], want[k]) for k in ("chi2", "sub", "best_prof", "subints")]
        worst = max(worst, max(errs))
        assert max(errs) <= BAR, (what, j, errs)
        np.testing.assert_array_equal(got["best_cnt"][j], want["best_cnt"])
        top = np.sort(want["chi2"])[::-1]
        if len(top) < 2 or top[0] - top[1] > BAR * max(top[0], 1e-30):
            assert int(got["best"][j]) == want["best"], (what, j)
        assert got["best_chi2"][j] == got["chi2"][j][int(got["best"][j])]
    print("subfold_dm %s: worst rel err of chi2 / sub / best_prof / subints %.3g" % (what, worst))
    return worst


@pytest.mark.parametrize("ndm", [1, 51, 1024])
def test_refine_against_oracle(gpu, ndm):
    from pypulsar_amd.subfold import SubbandFolder
    x, freqs, ref = _case("base")
    folder = SubbandFolder(freqs, DT, NPART, NSUB, NBINS, ndm=ndm)
    jobs = folder.plan(N, *zip(*SF_JOBS))
    if ndm == 1:
        dms = np.asarray(DMS)[:, None] + 0.7
    elif ndm == 51:
        dms = None                                        # the default ladder, nbins + 1
    else:
        dms = np.asarray(DMS)[:, None] + np.linspace(-20.0, 20.0, ndm)[None, :]
    for trials in ([(0, 0)] * 5, [(3, -2), (-7, 5), (0, 1), (64, 0), (-300, 300)]):
        got = _refine(folder, jobs, ref, trials, dms)
        assert got["chi2"].shape == (5, ndm) and got["r"].shape == (5, ndm, NSUB)
        _check_refine(got, ref, jobs, trials, "ndm %d trials %s" % (ndm, trials[0]))
        if trials[0] == (0, 0):
            np.testing.assert_array_equal(got["sub"], ref[0].sum(axis=1))
        np.testing.assert_array_equal(got["subints"], ref[0].sum(axis=2))


def test_refine_dead_subband_constant_job_and_ties(gpu):
    from pypulsar_amd.subfold import SubbandFolder
    freqs = band(64)
    x = _u8(64, N, 61)
    x[:, 24:32] = 7                                       # subband 3 is dead: var_s == 0
    folder = SubbandFolder(freqs, DT, NPART, NSUB, NBINS, ndm=5)
    jobs = folder.plan(N, [30.0, 12.0], [91.3, 333.3])
    sel = [(30.0, 91.3, 0.0, 0.0), (12.0, 333.3, 0.0, 0.0)]
    ref = so.subfold(x, freqs, DT, sel, NPART, NSUB, NBINS)
    # exact ties: equal ladder entries give equal shifts and equal chi-squares
    d = np.array([[31.0, 33.0, 29.5, 33.0, 31.0], [12.5, 12.5, 12.5, 12.5, 12.5]])
    got = _refine(folder, jobs, ref, [(0, 0)] * 2, d)
    _check_refine(got, ref, jobs, [(0, 0)] * 2, "dead subband, ties")
    want = so.refine(ref[0][0], ref[1][0], ref[2][0], ref[3][0], int(jobs.nfold[0]), (0, 0),
                     got["r"][0])
    assert want["var"][3] == 0.0 and np.all(want["var"][[0, 1, 2, 4, 5, 6, 7]] > 0)
    c = got["chi2"]
    assert c[0, 0] == c[0, 4] and c[0, 1] == c[0, 3] and np.all(c[1] == c[1, 0])
    for j in range(2):                                    # the total order on the device's own values
        best = None
        for k in range(5):
            if best is None or so.better((c[j, k], k), best, 2):
                best = (c[j, k], k)
        assert int(got["best"][j]) == best[1]
    assert int(got["best"][1]) == 2                       # all equal: the centre
    assert int(got["best"][0]) in (0, 1, 2)               # of a tied pair the earlier entry
    # an all-constant job: chi2 == 0 everywhere, best = ndm // 2
    const = np.full((N, 64), 37, dtype=np.uint8)
    cref = so.subfold(const, freqs, DT, sel[:1], NPART, NSUB, NBINS)
    one = folder.plan(N, [30.0], [91.3])
    got = _refine(folder, one, cref, [(2, 1)], None)
    assert np.all(got["chi2"] == 0.0) and int(got["best"][0]) == 2 and got["best_chi2"][0] == 0.0
    _check_refine(got, cref, one, [(2, 1)], "constant")


def test_violations_raise_before_launch(gpu):
    import ctypes
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.subfold import SubbandFolder
    freqs = band(64)
    for kw in (dict(nbins=257), dict(npart=129), dict(nsub=7), dict(nsub=64, nbins=256),
               dict(ndm=1025)):
        with pytest.raises(ValueError):
            SubbandFolder(freqs, DT, **kw)
    folder = SubbandFolder(freqs, DT, NPART, NSUB, NBINS)
    xd = torch.from_numpy(_u8(64, N, 62)).cuda()
    jobs = folder.plan(N, [30.0], [91.3])
    out = folder.empty(1)
    nf, bmax = int(jobs.nfold[0]), int(jobs.bmax[0])
    for block, t_first, span in ((xd[:2000], 0, (0, 2000 - bmax + 1)),   # one row short
                                 (xd[100:], 100, (99, nf)),              # starts before the block
                                 (xd, 0, (0, nf + 1)),                   # beyond the folded range
                                 (xd[:nf + bmax - 1], 0, (0, nf))):           # one row short
        with pytest.raises(ValueError):
            folder.fold(block, t_first, N, jobs, out=out, span=span)
    with pytest.raises(TypeError):
        folder.fold(xd.to(torch.int16), 0, N, jobs, out=out)
    # the library refuses on its own host copy too
    jb = np.array([[0, 1 << 40, 0, jobs.L[0], 0, nf, 0, bmax]], dtype=np.int64)
    jd, tab = torch.from_numpy(jb).cuda(), torch.from_numpy(jobs.table).cuda()
    with pytest.raises(_lib.PddError, match="does not cover"):
        _lib.call("pdd_subfold", _lib.ptr(xd), _lib.U8, nf + bmax - 1, 64, 64, 0,
                  jb.ctypes.data_as(ctypes.c_void_p), _lib.ptr(jd), 1, _lib.ptr(tab), 1, NPART,
                  NSUB, NBINS, *[_lib.ptr(t) for t in out], -1, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(float(t.double().abs().sum()) == 0.0 for t in out)         # nothing was launched
    # no jobs: nothing to do
    e = folder.fold(xd, 0, N, [])
    assert e[0].shape == (0, NPART, NSUB, NBINS)


# ---- recovery of an injected, dispersed pulsar ----

def _pulsar():
    C, n, dt, period, dm = 64, 1 << 15, 256e-6, 50.03e-3, 60.0
    freqs = band(C, True, 1400.0, 1500.0)
    rng = np.random.default_rng(71)
    x = rng.normal(96.0, 12.0, (n, C))
    delay = (1.0 / (0.000241 * freqs * freqs) - 1.0 / (0.000241 * freqs.max() ** 2)) * dm
    t = (np.arange(n) + 0.5) * dt
    ph = ((t[:, None] - delay[None, :]) / period) % 1.0
    x += 30.0 * np.exp(-0.5 * ((ph - 0.5) / 0.02) ** 2)
    return freqs, dt, period, np.clip(np.round(x), 0, 255).astype(np.uint8)


def test_recovery(gpu):
    import torch
    from pypulsar_amd.subfold import SubbandFolder, ladder_step
    freqs, dt, period, x = _pulsar()
    n, npart, nsub, nbins = x.shape[0], 8, 8, 64
    f = 1.0 / period
    job = [(55.0, f, 0.0, 0.0)]
    ref = so.subfold(x, freqs, dt, job, npart, nsub, nbins)
    dms = so.default_ladder(55.0, f, freqs, nsub, nbins)
    step = dms[1] - dms[0]
    r = so.ladder_shifts(55.0, f, dms, freqs, nsub, nbins)
    nf = so.geometry(n, so.delays_of(55.0, freqs, dt)[1], npart)[2]
    want = so.refine(ref[0][0], ref[1][0], ref[2][0], ref[3][0], nf, (0, 0), r)
    kb = want["best"]
    print("recovery: ladder step %.3f, oracle best DM %.2f, chi2 %.1f against %.1f at the centre" % (
        step, dms[kb], want["chi2"][kb], want["chi2"][nbins // 2]))
    assert abs(dms[kb] - 60.0) <= step and want["chi2"][kb] > want["chi2"][nbins // 2]
    assert abs(step - ladder_step(f, freqs, nsub, nbins)) <= 1e-12 * step
    folder = SubbandFolder(freqs, dt, npart, nsub, nbins)
    xd = torch.from_numpy(x).cuda()
    got = folder(xd, job)[0]
    np.testing.assert_array_equal(got.dms, dms)
    assert got.best == kb and got.dm == dms[kb] and got.dm_fold == 55.0
    e = rel_err(got.chi2_vs_dm, want["chi2"])
    print("recovery: device chi2 rel err %.3g" % e)
    assert e <= BAR and got.chi2 == got.chi2_vs_dm[kb]
    np.testing.assert_array_equal(got.sub, want["sub"])
    np.testing.assert_array_equal(got.profile, want["best_prof"])
    np.testing.assert_array_equal(got.subint_counts, ref[1][0])
    assert got.sigma > 20.0 and np.isfinite(got.sigma) and got.nsamp == nf
    assert got.sub_freqs.shape == (nsub,) and got.T == nf * dt
    # folded at the true DM the subbands line up
    at60 = folder(xd, [(60.0, f, 0.0, 0.0)])[0]
    peaks = np.argmax(at60.sub, axis=1)
    d = (peaks - peaks[0] + nbins // 2) % nbins - nbins // 2
    assert np.all(np.abs(d) <= 1), peaks


# ---- the command line ----

def test_cli_fold_subbands(gpu, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.subfold import _KEYS, _SCALARS, read_subfold
    freqs, x = _period_data()
    C = x.shape[0]
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), float(freqs[1] - freqs[0]),
                                      src_raj=123456.789, src_dej=-123456.5)
    args = ["--lodm", "52.5", "--hidm", "67.5", "--numdms", "16", "--nfft", "32768", "--fold", "1"]
    fil = str(tmp_path / "psr.fil")
    fbm.write_filterbank(fil, params, hdr, x.T.copy())
    # without the option, then with it in the same place: the same files, byte for byte, and one more
    assert pulsar_search.main(args + [fil]) == 0
    before = {n: open(str(tmp_path / n), "rb").read() for n in os.listdir(str(tmp_path))}
    assert sorted(before) == ["psr.accelcands", "psr.fil", "psr_cand1.bestprof", "psr_cand1.npz"]
    assert pulsar_search.main(args + ["--fold-subbands", "8", fil]) == 0
    assert sorted(os.listdir(str(tmp_path))) == sorted(list(before) + ["psr_cand1_subbands.npz"])
    for name in ("psr.accelcands", "psr_cand1.bestprof"):
        assert open(str(tmp_path / name), "rb").read() == before[name], name
    fn = str(tmp_path / "psr_cand1_subbands.npz")
    with np.load(fn, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(_KEYS + _SCALARS)
    sf = read_subfold(fn)
    assert sf.sub.shape == (8, 64) and sf.subints.shape == (32, 64) and sf.profile.shape == (64,)
    assert sf.chi2_vs_dm.shape == sf.dms.shape == (65,) and sf.sub_freqs.shape == (8,)
    assert sf.chansum.shape == (C,) and sf.subint_counts.shape == (32, 64)
    assert sf.dms[32] == sf.dm_fold and abs(sf.dm_fold - 60.0) <= 2.0
    assert sf.chi2 == sf.chi2_vs_dm.max() and sf.chi2 > 10.0 and sf.sigma > 8.0
    assert sf.subint_counts.sum() == sf.nsamp
    with pytest.raises(SystemExit):
        pulsar_search.main(["--fold-subbands", "8", fil])                 # needs --fold K


def _period_data():
    """The psr.fil recipe of tests/test_gpu_period.py (its fixture's body)."""
    from oracle import spectra_oracle as orc
    C, n, period, width = 64, 1 << 15, 64, 2
    freqs = band(C)
    rng = np.random.default_rng(21)
    x = rng.normal(128.0, 16.0, (C, n))
    delays = orc.sweep_table([60.0], freqs, DT)[0]
    for c in range(C):
        for w in range(width):
            t = np.arange(7 + w + int(delays[c]), n, period)
            x[c, t] += 12.0
    return freqs, np.clip(np.round(x), 0, 255).astype(np.uint8)
