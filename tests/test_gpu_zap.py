"""The birdie zapper on the GPU: pdd_zap_percentile and pdd_zap_apply bit
for bit against NumPy, ``BirdieFinder.find`` against tests/zap_oracle.py on
the GPU's own whitened powers, and the zap end to end in the periodicity
search, the acceleration search and ``pulsar_search.py``."""
import numpy as np
import pytest

import period_oracle as po
import zap_oracle as zo
from conftest import band
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = zo.DT
A_E2E = 500.0   # birdie amplitude of the end-to-end planes (checked in `e2e` below)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ---- pdd_zap_percentile ----

def _columns(R, nn, seed):
    """[R, nn] float32: the left half quantised to 1/4 (exact ties), a
    duplicated row and an all-zero row where R allows."""
    rng = np.random.default_rng(seed)
    P = rng.exponential(1.0, (R, nn)).astype(np.float32)
    P[:, :nn // 2] = np.round(P[:, :nn // 2] * 4.0) / 4.0
    if R >= 2:
        P[1] = P[0]
    if R >= 3:
        P[2] = 0.0
    return P


@pytest.mark.parametrize("nn", [19, 257, 2051])
@pytest.mark.parametrize("R", [1, 2, 9, 33, 64])
def test_percentile_exact(gpu, R, nn):
    import torch
    from pypulsar_amd.zap import BirdieFinder
    bf = BirdieFinder()
    P = _columns(R, nn, 100 * R + nn)
    buf = torch.full((R, nn + 13), float("nan"), dtype=torch.float32, device=gpu)
    view = buf[:, :nn]
    view.copy_(torch.from_numpy(P))
    assert view.stride(0) == nn + 13
    srt = np.sort(P, axis=0)
    for rank in sorted({1, (R + 1) // 2, R}):
        got = bf.percentile(view, rank).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (nn,)
        np.testing.assert_array_equal(_bits(got), _bits(srt[rank - 1]))
        again = bf.percentile(view, rank).cpu().numpy()
        np.testing.assert_array_equal(_bits(again), _bits(got))
    if R % 2:
        med = bf.percentile(view, (R + 1) // 2).cpu().numpy()
        np.testing.assert_array_equal(med, np.percentile(P, 50, axis=0).astype(np.float32))
        assert bf.rank(R) == (R + 1) // 2
    # the input (and the filler beside it) is only read
    back = buf.cpu().numpy()
    np.testing.assert_array_equal(_bits(back[:, :nn]), _bits(P))
    assert np.all(np.isnan(back[:, nn:]))


def test_percentile_refuses_bad_arguments(gpu):
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.zap import BirdieFinder
    bf = BirdieFinder()
    nn = 19
    err = (RuntimeError, AssertionError)
    with pytest.raises(err):
        bf.percentile(torch.zeros((0, nn), dtype=torch.float32, device=gpu), 1)
    with pytest.raises(err):
        bf.percentile(torch.zeros((65, nn), dtype=torch.float32, device=gpu), 1)
    x = torch.zeros((9, nn), dtype=torch.float32, device=gpu)
    for rank in (0, 10):
        with pytest.raises(err):
            bf.percentile(x, rank)
    with pytest.raises(err):
        bf.percentile(x.double(), 1)
    with pytest.raises(err):
        bf.percentile(x.t(), 1)
    # the C entry point reports them and writes nothing
    h = _lib.lib()
    big = torch.zeros((65, nn), dtype=torch.float32, device=gpu)
    out = torch.full((nn,), -7.0, dtype=torch.float32, device=gpu)
    for R, rank, ld in ((0, 1, nn), (65, 1, nn), (9, 10, nn), (9, 0, nn), (9, 1, nn - 1)):
        st = h.pdd_zap_percentile(_lib.ptr(big), R, nn, ld, rank, _lib.ptr(out), _lib.stream_ptr())
        assert st < 0 and b"pdd_zap_percentile" in h.pdd_last_error(), (R, rank, ld)
    assert h.pdd_zap_percentile(None, 9, nn, nn, 1, _lib.ptr(out), _lib.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)


# ---- pdd_zap_apply ----

APPLY_BINS = np.asarray([[1, 1], [7, 9], [300, 1900], [2050, 2050]], dtype=np.int32)


@pytest.mark.parametrize("with_spec", [False, True])
def test_apply_exact(gpu, with_spec):
    import torch
    from pypulsar_amd import zap
    D, nn, ld = 3, 2051, 2051 + 5
    rng = np.random.default_rng(7)
    P = rng.exponential(1.0, (D, ld)).astype(np.float32)
    P[:, nn:] = np.nan
    S = (rng.normal(0, 1, (D, ld)) + 1j * rng.normal(0, 1, (D, ld))).astype(np.complex64)
    pd, sd = torch.from_numpy(P).to(gpu), torch.from_numpy(S).to(gpu)
    pv, sv = pd[:, :nn], sd[:, :nn]
    hit = np.zeros(ld, dtype=bool)
    for lo, hi in APPLY_BINS:
        hit[lo:hi + 1] = True
    assert hit.sum() == 1 + 3 + 1601 + 1 and not hit[0]

    # no intervals: nothing changes
    zap.apply(pv, np.zeros((0, 2), dtype=np.int32), sv if with_spec else None)
    np.testing.assert_array_equal(_bits(pd.cpu().numpy()), _bits(P))
    np.testing.assert_array_equal(sd.cpu().numpy().view(np.int32), S.view(np.int32))

    ret = zap.apply(pv, APPLY_BINS, sv if with_spec else None)
    assert ret is pv
    got = pd.cpu().numpy()
    assert np.all(_bits(got[:, hit]) == _bits(np.float32(1.0)))
    np.testing.assert_array_equal(_bits(got[:, ~hit]), _bits(P[:, ~hit]))
    gs = sd.cpu().numpy()
    if with_spec:
        fill = np.asarray([0.70710677, 0.70710677], dtype=np.float32).view(np.int32)
        z = np.ascontiguousarray(gs[:, hit]).view(np.int32).reshape(D, -1, 2)
        assert np.all(z == fill)
        np.testing.assert_array_equal(np.ascontiguousarray(gs[:, ~hit]).view(np.int32),
                                      np.ascontiguousarray(S[:, ~hit]).view(np.int32))
        # the oracle's fill is the same
        qp, qs = zo.fill(P[:, :nn], APPLY_BINS, S[:, :nn])
        np.testing.assert_array_equal(_bits(got[:, :nn]), _bits(qp))
        np.testing.assert_array_equal(np.ascontiguousarray(gs[:, :nn]).view(np.int32),
                                      qs.view(np.int32))
    else:
        np.testing.assert_array_equal(gs.view(np.int32), S.view(np.int32))
    # the device tensor of device_bins is taken as it is; D = 0 is a no-op
    zb = zap.device_bins(APPLY_BINS, nn, gpu)
    zap.apply(pv, zb)
    np.testing.assert_array_equal(_bits(pd.cpu().numpy()), _bits(got))
    zap.apply(pv[:0], zb)


def test_apply_refuses_bad_intervals(gpu):
    import torch
    from pypulsar_amd import zap
    p = torch.ones((2, 64), dtype=torch.float32, device=gpu)
    for bad in ([[0, 3]], [[5, 64]], [[9, 8]], [[5, 9], [9, 12]], [[20, 22], [3, 4]]):
        with pytest.raises(AssertionError):
            zap.apply(p, np.asarray(bad, dtype=np.int32))
    with pytest.raises(AssertionError):
        zap.apply(p.double(), APPLY_BINS[:1])
    assert np.all(p.cpu().numpy() == 1.0)


# ---- BirdieFinder.find ----

@pytest.mark.parametrize("D,n,nfft", zo.SHAPES + ((9, 4096, 5000),))
def test_find_vs_oracle(gpu, D, n, nfft):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    from pypulsar_amd.zap import BirdieFinder, Zaplist
    plane = torch.from_numpy(zo.synthetic_plane(D, n, 4096, A=150.0)).to(gpu)
    ps = PeriodicitySearch(6.0)
    for nsig, grow in ((5.0, 1), (4.0, 0)):
        bf = BirdieFinder(nsig=nsig, grow=grow)
        zl, pct = bf.find(ps, plane, DT, nfft=nfft, return_spectrum=True)
        assert isinstance(zl, Zaplist) and pct.dtype == np.float32 and pct.shape == (nfft // 2,)
        sel = bf.select_rows(D)
        P = ps.normalise(ps.spectrum(plane[torch.from_numpy(sel).to(gpu)], nfft)).cpu().numpy()
        R = len(sel)
        assert R == D
        np.testing.assert_array_equal(_bits(pct), _bits(zo.order_statistic(P, zo.rank(R))))
        want = zo.flag(pct, R, ps.rlo(nfft, DT), 50.0, nsig, grow)
        got = zl.bins(nfft, DT)
        np.testing.assert_array_equal(got, want)
        flagged = set(k for lo, hi in got for k in range(lo, hi + 1))
        b = int(round(zo.BIRDIE_BIN * nfft / 4096.0))
        assert b in flagged
        if nfft == 4096:
            assert flagged <= set(range(b - 1 - grow, b + 2 + grow)), flagged
        assert bf.find(ps, plane, DT, nfft=nfft).bins(nfft, DT).tolist() == got.tolist()


# ---- the searches ----

@pytest.fixture(scope="module", params=zo.SHAPES, ids=lambda s: "D%d_n%d" % s[:2])
def e2e(gpu, request):
    """(shape, device plane, DMs) with a birdie that the oracle sees, in every
    row, at twice the single-harmonic threshold of a 6 sigma search or more."""
    import torch
    D, n, nfft = request.param
    host = zo.synthetic_plane(D, n, nfft, A=A_E2E)
    P = zo.whiten(host, nfft)
    assert P[:, zo.BIRDIE_BIN].min() >= 2.0 * po.threshold_power(6.0, 1), P[:, zo.BIRDIE_BIN].min()
    return request.param, torch.from_numpy(host).to(gpu), np.arange(D, dtype=np.float64)


def _record_set(c):
    return set(zip(c["row"].tolist(), c["r"].tolist(), c["numharm"].tolist(),
                   _bits(c["power"]).tolist()))


def test_periodicity_zap(e2e):
    from pypulsar_amd.periodicity import PeriodicitySearch
    from pypulsar_amd.zap import BirdieFinder
    (D, n, nfft), plane, dms = e2e
    ps = PeriodicitySearch(6.0)
    plain = ps(plane, dms, DT, nfft=nfft)
    np.testing.assert_array_equal(ps(plane, dms, DT, nfft=nfft, zap=None), plain)
    h1 = plain[plain["numharm"] == 1]
    for d in range(D):
        assert np.any((h1["row"] == d) & (h1["r"] == zo.BIRDIE_BIN)), d

    zl = BirdieFinder().find(ps, plane, DT, nfft=nfft)
    bins = zl.bins(nfft, DT)
    assert any(lo <= zo.BIRDIE_BIN <= hi for lo, hi in bins)
    got = ps(plane, dms, DT, nfft=nfft, zap=zl)
    g1 = got[got["numharm"] == 1]
    for lo, hi in bins:
        assert not np.any((g1["r"] >= lo) & (g1["r"] <= hi)), (lo, hi)
    # the pulsar keeps its bits
    psr = lambda c: c[(c["row"] == zo.PULSAR_ROW) & (c["r"] == nfft // 64) &  # noqa: E731
                      (c["numharm"] == 1)]
    assert len(psr(plain)) == 1 and len(psr(got)) == 1
    assert _bits(psr(got)["power"])[0] == _bits(psr(plain)["power"])[0]
    # the whole candidate set: the oracle's search of the GPU's own whitened
    # powers, zapped by the oracle
    P = ps.normalise(ps.spectrum(plane, nfft)).cpu().numpy()
    want = po.candidates(zo.fill(P, bins), ps.harms, ps.thr, ps.rlo(nfft, DT))
    assert _record_set(got) == want
    assert _record_set(plain) == po.candidates(P, ps.harms, ps.thr, ps.rlo(nfft, DT))
    assert _record_set(plain) != want
    # row batches change nothing
    np.testing.assert_array_equal(ps(plane, dms, DT, nfft=nfft, row_batch=4, zap=zl), got)


def test_accel_zap(gpu):
    import torch
    from pypulsar_amd.accel import AccelSearch
    from pypulsar_amd.zap import BirdieFinder
    D, n, nfft = zo.SHAPES[0]
    plane = torch.from_numpy(zo.synthetic_plane(D, n, nfft, A=A_E2E)).to(gpu)
    dms = np.arange(D, dtype=np.float64)
    zmax = 4
    acc = AccelSearch(6.0, zmax=zmax, dz=2)
    plain = acc(plane, dms, DT, nfft=nfft)
    np.testing.assert_array_equal(acc(plane, dms, DT, nfft=nfft, zap=None), plain)
    h1 = plain[plain["numharm"] == 1]
    for d in range(D):
        assert np.any((h1["row"] == d) & (np.abs(h1["r"] - zo.BIRDIE_BIN) <= 0.5)), d
    zl = BirdieFinder().find(acc.ps, plane, DT, nfft=nfft)
    bins = zl.bins(nfft, DT)
    assert bins.tolist() == [[zo.BIRDIE_BIN - 1, zo.BIRDIE_BIN + 1]]
    got = acc(plane, dms, DT, nfft=nfft, zap=zl)
    g1 = got[got["numharm"] == 1]
    for lo, hi in bins:
        assert not np.any((g1["r"] >= lo - zmax / 2.0) & (g1["r"] <= hi + zmax / 2.0)), g1
    for c in (plain, got):
        assert np.any((c["row"] == zo.PULSAR_ROW) & (np.abs(c["r"] - nfft // 64) <= 0.5))
    np.testing.assert_array_equal(acc(plane, dms, DT, nfft=nfft, row_batch=4, zap=zl), got)


# ---- pulsar_search.py ----

CLI_NFFT, CLI_TONE_BIN = 1 << 15, 101
CLI_PERIOD, CLI_DM = 8, 8.0   # the pulsar: period in samples, DM (a trial of 0, 1 .. 15)


@pytest.fixture(scope="module")
def zap_fil(tmp_path_factory):
    """8-bit filterbank: noise, a pulse train of period 8 samples dispersed at
    DM 8 and an undispersed tone (the same in every channel) at Fourier bin
    101 of a 32768-point spectrum.  The period is short and the trials 1 pc/cc
    apart, so that the pulsar is smeared away in all but a few of the 16 DM
    rows; the tone is low enough (48 Hz) to add up across the band at every
    trial."""
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C, N = 64, 1 << 15
    freqs = band(C)
    rng = np.random.default_rng(33)
    x = rng.normal(128.0, 16.0, (C, N))
    delays = orc.sweep_table([CLI_DM], freqs, DT)[0]
    for c in range(C):
        x[c, np.arange(3 + int(delays[c]), N, CLI_PERIOD)] += 0.8
    x += 0.5 * np.sin(2.0 * np.pi * CLI_TONE_BIN * np.arange(N) / CLI_NFFT)[None, :]
    x = np.clip(np.round(x), 0, 255).astype(np.uint8)
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), float(freqs[1] - freqs[0]),
                                      src_raj=123456.789, src_dej=-123456.5)
    fn = str(tmp_path_factory.mktemp("zapcli") / "birdie.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    return fn


def test_cli_autozap_and_zaplist(gpu, zap_fil, tmp_path, capsys):
    import os
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import read_accelcands
    from pypulsar_amd.zap import read_zaplist
    common = ["--lodm", "0", "--hidm", "15", "--numdms", "16", "--nfft", str(CLI_NFFT)]
    near = lambda c: abs(c.r - CLI_TONE_BIN) <= 1.5  # noqa: E731

    plain = str(tmp_path / "plain.accelcands")
    assert pulsar_search.main(common + ["-o", plain, zap_fil]) == 0
    cp = read_accelcands(plain)
    assert any(near(c) for c in cp)
    zfn = os.path.splitext(zap_fil)[0] + ".zaplist"
    assert not os.path.exists(zfn)

    auto = str(tmp_path / "auto.accelcands")
    capsys.readouterr()
    assert pulsar_search.main(common + ["--autozap", "-o", auto, zap_fil]) == 0
    assert "autozap:" in capsys.readouterr().out
    bins = read_zaplist(zfn).bins(CLI_NFFT, DT)
    assert any(lo <= CLI_TONE_BIN <= hi for lo, hi in bins), bins
    ca = read_accelcands(auto)
    for lo, hi in bins:
        assert not any(lo - 0.5 <= c.r <= hi + 0.5 for c in ca), (lo, hi)
    assert not any(near(c) for c in ca)
    # the pulsar is in both lists
    for cl in (cp, ca):
        psr = [c for c in cl if abs(c.period - CLI_PERIOD * DT) <= 0.002 * CLI_PERIOD * DT]
        assert psr and abs(psr[0].dm - CLI_DM) <= 1.0

    # the list just written, given as a file: the same candidates
    listed = str(tmp_path / "listed.accelcands")
    assert pulsar_search.main(common + ["--zaplist", zfn, "-o", listed, zap_fil]) == 0
    strip = lambda fn: [l.split(":", 1)[1] if ":" in l else l for l in open(fn)]  # noqa: E731
    assert strip(listed) == strip(auto)
    assert strip(listed) != strip(plain)
