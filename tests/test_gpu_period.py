"""The periodicity search on the GPU (pdd_ps_prep, torch's rocFFT,
pdd_ps_block_medians, pdd_ps_normalise, pdd_ps_harmsum, pdd_ps_search) against
fixtures made by running the reference (tests/golden/make_golden_period.py)
and the NumPy restatement (tests/period_oracle.py), and end to end behind the
sweep.  FFT lengths used in this file: 4096, 5000 and 32768 only (rocFFT
builds kernels per length on first use)."""
import os

import numpy as np
import pytest

import period_oracle as po
from conftest import GOLDEN, band
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = 64e-6
HARMS = (1, 2, 3, 4, 8, 16)
CASES = ((19, 6, 200), (2048, 6, 200), (2500, 6, 200), (16384, 40, 200))


@pytest.fixture(scope="module")
def gp():
    return np.load(os.path.join(GOLDEN, "golden_period.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def gh():
    return np.load(os.path.join(GOLDEN, "golden_period_hsum.npz"), allow_pickle=False)


def _rows(D, n, seed):
    """Raw sweep rows: near 5e5 with a noise of about 1e3, integers."""
    rng = np.random.default_rng(seed)
    return np.round(524288.0 + rng.normal(0.0, 1024.0, (D, n))).astype(np.float32)


def _strided(x, ld):
    import torch
    big = torch.full((x.shape[0], ld), 7.0e5, dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return big[:, :x.shape[1]]


@pytest.mark.parametrize("n,ld,nfft", [(3000, 3100, 4096), (4096, 4096, 4096)])
def test_prep(gpu, n, ld, nfft):
    from pypulsar_amd.periodicity import PeriodicitySearch
    x = _rows(3, n, 11)
    view = _strided(x, ld)
    assert view.stride(0) == ld
    ps = PeriodicitySearch()
    got = ps.prep(view, nfft).cpu().numpy()
    assert got.shape == (3, nfft) and got.dtype == np.float32
    x64 = x.astype(np.float64)
    ref = (x64 - x64.mean(axis=1, keepdims=True)).astype(np.float32)
    err = np.max(np.abs(got[:, :n].astype(np.float64) - ref)) / np.max(np.abs(ref))
    print("prep: max err / max|ref| = %.3g" % err)
    assert err <= 1e-6
    assert np.all(got[:, n:] == 0.0)
    # deterministic: the same bits on a second run
    again = ps.prep(view, nfft).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32))


@pytest.mark.parametrize("n,nfft", [(3000, 4096), (4700, 5000)])
def test_spectrum(gpu, n, nfft):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    x = _rows(3, n, 12)
    x[1] += (200.0 * np.sin(2 * np.pi * np.arange(n) / 37.0)).astype(np.float32)
    ps = PeriodicitySearch()
    xd = torch.from_numpy(x).cuda()
    prep = ps.prep(xd, nfft).cpu().numpy()
    got = ps.spectrum(xd, nfft).cpu().numpy()
    assert got.shape == (3, nfft // 2 + 1) and got.dtype == np.complex64
    ref = np.fft.rfft(prep.astype(np.float64), axis=1)
    for r in range(3):
        err = np.max(np.abs(got[r] - ref[r])) / np.max(np.abs(ref[r]))
        print("spectrum nfft=%d row %d: max err / max|ref| = %.3g" % (nfft, r, err))
        assert err <= 1e-5


@pytest.mark.parametrize("nn,ibl,mbl", CASES)
def test_normalise_golden(gpu, gp, nn, ibl, mbl):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    spec, dered = gp["nn%d_spec" % nn], gp["nn%d_dered" % nn]
    ps = PeriodicitySearch(initialbuflen=ibl, maxbuflen=mbl)
    sd = torch.from_numpy(spec).cuda()
    powers, out = ps.normalise(sd, want_spectrum=True, nn=nn)
    only = ps.normalise(sd, nn=nn)
    med = ps.medians(sd, nn=nn).cpu().numpy()
    powers, out = powers.cpu().numpy(), out.cpu().numpy()
    np.testing.assert_array_equal(only.cpu().numpy().view(np.int32), powers.view(np.int32))
    assert powers.shape == (3, nn) and out.shape == (3, nn) and out.dtype == np.complex64
    # block levels: np.median / ln 2 of the float32 powers
    offs, lens = gp["nn%d_offs" % nn], gp["nn%d_lens" % nn]
    assert med.shape == (3, len(offs))
    p32 = spec.real * spec.real + spec.imag * spec.imag
    for r in range(3):
        want = po.medians(p32[r], offs, lens)
        e = np.max(np.abs(med[r] - want) / want)
        print("medians nn=%d row %d: max rel err %.3g" % (nn, r, e))
        assert e <= 1e-5
    # powers against |dered_ref|^2 (bin 0 = 1), the spectrum against dered_ref
    d128 = dered.astype(np.complex128)
    pref = np.abs(d128) ** 2
    assert np.all(pref[:, 0] == 1.0) and np.all(powers[:, 0] == 1.0)
    assert np.all(out[:, 0] == 1.0 + 0.0j)
    ep = np.max(np.abs(powers - pref) / pref)
    es = np.max(np.abs(out - d128) / np.abs(d128))
    print("normalise nn=%d: powers max rel err %.3g, spectrum max rel err %.3g" % (nn, ep, es))
    assert ep <= 1e-5
    assert es <= 1e-5


def test_normalise_too_short_and_even_blocks(gpu, gp):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    ps = PeriodicitySearch()
    spec = torch.from_numpy(gp["nn19_spec"]).cuda()
    with pytest.raises(AssertionError):
        ps.normalise(spec[:, :18].contiguous(), nn=18)
    with pytest.raises(AssertionError):
        ps.normalise(spec, nn=18)
    # ties and an even block: the mean of the two middle values, as np.median
    s = np.zeros((1, 40), dtype=np.complex64)
    s.real[0] = np.sqrt(np.asarray([1, 5, 5, 2, 9, 9, 3, 7] * 5, dtype=np.float32))
    sd = torch.from_numpy(s).cuda()
    ps2 = PeriodicitySearch(initialbuflen=6)
    med = ps2.medians(sd, nn=40).cpu().numpy()[0]
    offs, lens = po.table(40, 6, 200)
    p32 = s.real[0] * s.real[0]
    want = po.medians(p32, offs, lens)
    assert np.max(np.abs(med - want) / want) <= 1e-5
    assert 6 in lens and 11 in lens  # an even and an odd block


def test_constant_row(gpu):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    x = _rows(3, 3000, 13)
    x[1] = 524288.0  # a dead row: spectrum 0 -> level 0 -> power 0
    ps = PeriodicitySearch(sigma_threshold=3.0, flo=0.0)
    xd = torch.from_numpy(x).cuda()
    powers = ps.normalise(ps.spectrum(xd, 4096))
    p = powers.cpu().numpy()
    assert np.all(np.isfinite(p))
    assert np.all(p[1, 1:] == 0.0) and p[1, 0] == 1.0
    assert abs(np.mean(p[0, 1:]) - 1.0) < 0.2  # whitened noise: unit mean
    cands = ps(xd, [1.0, 2.0, 3.0], 1e-3, nfft=4096)
    assert len(cands) > 0 and 1 not in set(cands["row"])


def test_harmsum_golden(gpu, gh):
    from pypulsar_amd.periodicity import PeriodicitySearch
    nn = 2500
    powers = gh["nn%d_hsum1" % nn]
    view = _strided(powers, 2600)
    ps = PeriodicitySearch()
    for H in HARMS:
        got = ps.harmonic_sum(view, H).cpu().numpy()
        want = gh["nn%d_hsum%d" % (nn, H)]
        assert got.shape == want.shape == (3, nn // H)
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def _record_set(c, k):
    c = c[:k].cpu().numpy()
    return {(int(a), int(b), int(h), int(s)) for a, b, h, s in c}


@pytest.mark.parametrize("nn,ibl,harms,rlo", [(2500, 6, (1, 2, 4, 8, 16), 1),
                                              (2500, 6, (1, 2, 4, 8, 16), 5),
                                              (16384, 40, (1, 2, 4, 8, 16), 300),
                                              (16384, 40, (2, 3, 5, 14, 32), 3),
                                              (2048, 6, (16,), 1)])
def test_search_vs_oracle(gpu, gp, nn, ibl, harms, rlo):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    nfft = 2 * nn
    dt = (rlo - 0.5) / float(nfft)  # flo = 1 Hz lies between bins rlo - 1 and rlo
    ps = PeriodicitySearch(sigma_threshold=3.5, harms=harms, initialbuflen=ibl)
    assert ps.rlo(nfft, dt) == rlo
    powers = ps.normalise(torch.from_numpy(gp["nn%d_spec" % nn]).cuda(), nn=nn)
    c, k = ps.raw(powers, nfft, dt)
    n = int(k.item())
    got = _record_set(c, n)
    assert len(got) == n  # no duplicates
    ph = powers.cpu().numpy()
    want = po.candidates(ph, harms, ps.thr, rlo)
    assert len(want) > 10
    assert got == want
    # the comb of make_golden_period.make_spectrum: row r at harmonics of
    # k0 = nn // (23 + 7 r), found at its bin for the largest stage
    H = harms[-1]
    for r in range(3):
        k0 = max(2, nn // (23 + 7 * r))
        if rlo <= k0 < nn // H and H <= 16:
            assert any(a == r and b == k0 and h == H for a, b, h, _ in got), (r, k0)
    recs = ps.collect(c, k, [1.0, 2.0, 3.0], nfft, dt)
    assert len(recs) == n and np.all(recs["r"] >= rlo)
    assert np.all(np.diff(recs["row"]) >= 0) and np.all(recs["sigma"] >= 3.5 - 1e-6)
    assert np.allclose(recs["freq"], recs["r"] / (nfft * dt))


def test_search_overflow(gpu, gp):
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    ps = PeriodicitySearch(sigma_threshold=3.0, max_cands=2)
    powers = ps.normalise(torch.from_numpy(gp["nn2048_spec"]).cuda(), nn=2048)
    c, k = ps.raw(powers, 4096, 1.0 / 4096)
    assert int(k.item()) > 2
    with pytest.raises(RuntimeError):
        ps.collect(c, k, [1.0, 2.0, 3.0], 4096, 1.0 / 4096)


# ---- end to end: filterbank -> sweep -> periodicity search -> sift ----

E2E_DMS = np.linspace(52.5, 67.5, 16)  # 1 pc/cc steps around the injected DM 60


@pytest.fixture(scope="module")
def pulsar_data():
    C, N, period, width = 64, 1 << 15, 64, 2
    freqs = band(C)
    rng = np.random.default_rng(21)
    x = rng.normal(128.0, 16.0, (C, N))
    delays = orc.sweep_table([60.0], freqs, DT)[0]
    for c in range(C):
        for w in range(width):
            t = np.arange(7 + w + int(delays[c]), N, period)
            x[c, t] += 12.0
    return freqs, np.clip(np.round(x), 0, 255).astype(np.uint8)


def _check_top(top, step):
    assert abs(top.period - 64 * DT) <= 0.002 * 64 * DT, top
    assert abs(top.dm - 60.0) <= step, top
    assert len(top.hits) >= 3, top


def test_end_to_end(gpu, pulsar_data, tmp_path):
    import torch
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.periodicity import PeriodicitySearch, read_accelcands, sift
    from pypulsar_amd.sweep import DMSweep
    freqs, x = pulsar_data
    step = E2E_DMS[1] - E2E_DMS[0]
    sw = DMSweep(E2E_DMS, freqs, DT, dtype="f32")
    plane = sw(torch.from_numpy(x).cuda().float())
    assert plane.shape[0] == 16 and plane.shape[1] < 32768
    ps = PeriodicitySearch()
    cands = ps(plane, E2E_DMS, DT, nfft=32768)
    # (row batches change nothing)
    batched = ps(plane, E2E_DMS, DT, row_batch=5, nfft=32768)
    np.testing.assert_array_equal(cands, batched)
    sw.close()
    s = sift(cands)
    _check_top(s[0], step)

    # the CLI on the same data writes the same top candidate
    C = x.shape[0]
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path / "psr.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    out = str(tmp_path / "psr.accelcands")
    assert pulsar_search.main(["--lodm", "52.5", "--hidm", "67.5", "--numdms", "16", "--nfft",
                               "32768", "-o", out, fn]) == 0
    back = read_accelcands(out)
    assert len(back) == len(s)
    top, b = s[0], back[0]
    _check_top(b, step)
    assert b.accelfile == "psr_DM%.2f_ACCEL_0" % top.dm and b.candnum == 1
    assert (b.numharm, len(b.hits)) == (top.numharm, len(top.hits))
    assert abs(b.dm - top.dm) <= 0.005 and abs(b.sigma - top.sigma) <= 0.005
    assert abs(b.r - top.r) <= 0.005 and abs(b.period - top.period) <= 0.5e-9
