"""The injector's host model (pypulsar_amd/inject.py), its NumPy restatement
(tests/inject_oracle.py) and the recovery matching (pypulsar_amd/recovery.py).
No GPU."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

import inject_oracle as io
from conftest import band
from oracle import spectra_oracle as orc
from pypulsar_amd import inject as inj
from pypulsar_amd import recovery as rec

DT = 64e-6


def _turns(a):
    """distance of a (turns) from the nearest integer"""
    return abs(a - round(a))


# ---------------------------------------------------------------- phase
def test_phase_coefficients_against_exact_rationals():
    """P0 + i step + U(x x (k2 + x k3)) against the exact rational phase: <=
    1e-9 turns for i < 2^26 with z <= 400 and w <= 600 bins over 2^22 samples."""
    rng = np.random.default_rng(1)
    T = (1 << 22) * DT
    worst = 0.0
    for trial in range(12):
        f = float(rng.uniform(1.0, 700.0))
        fd = float(rng.uniform(-1, 1)) * 400.0 / T ** 2
        fdd = float(rng.uniform(-1, 1)) * 600.0 / T ** 3
        if trial == 0:
            fd, fdd = 400.0 / T ** 2, 600.0 / T ** 3
        phi0 = float(rng.uniform(0, 1))
        delta = float(rng.uniform(0, 0.3))
        P0, step, k2, k3 = inj.phase_coefficients(f, fd, fdd, phi0, DT, delta)
        sig = dict(f=f, fd=fd, fdd=fdd, phi0=phi0)
        i = np.concatenate([[0, 1, (1 << 26) - 1], rng.integers(0, 1 << 26, 60)]).astype(np.int64)
        ph = np.array([[P0, step]], dtype=np.uint64)
        dr = np.array([[k2, k3]])
        got = io.phases(i, ph, dr)[:, 0]
        for ii, g in zip(i, got):
            want = io.exact_phase(sig, DT, delta, int(ii))
            err = _turns(float(Fraction(int(g), 1 << 64) - want))
            worst = max(worst, err)
    print("worst phase error %.3g turns" % worst)
    assert worst <= 1e-9


def test_phase_coefficients_two_derivations_agree():
    sig = dict(f=123.456, fd=-3e-4, fdd=2e-7, phi0=0.3)
    P0, step, k2, k3 = inj.phase_coefficients(sig["f"], sig["fd"], sig["fdd"], sig["phi0"], DT, 0.0123)
    e0, e1, e2, e3 = io.cubic(sig, DT, 0.0123)
    assert P0 == round(e0 * io.M64) % io.M64 and step == round(e1 * io.M64) % io.M64
    assert k2 == float(e2) and k3 == float(e3)


def test_frac_u64_matches_python_ints():
    d = np.array([0.0, 0.5, -0.25, 123.999999999, -1e-30, 7.75, 0.9999999999999999, -3.000001])
    got = io.frac_u64(d)
    for x, g in zip(d, got):
        fr = x - math.floor(x)
        fr = 0.0 if fr >= 1.0 else fr
        assert int(g) == int(Fraction(fr) * (1 << 64))


def test_highest_channel_has_no_lag():
    for desc in (True, False):
        freqs = band(16, descending=desc)
        d = inj.channel_lags(56.7, freqs)
        assert d[np.argmax(freqs)] == 0.0 and np.all(d >= 0)
        assert np.array_equal(d, io.lags(56.7, freqs))


# ---------------------------------------------------------------- tables
def _gl(a, b, n=24):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (a + b), 0.5 * (b - a) * w


def _brute_profile(phi, sigma, s, d, tau):
    """Unit-peak Gaussian (sigma) convolved with unit-area boxes of widths s
    and d and a one-sided unit-area exponential tau, at ``phi`` (any units, not
    periodised): closed form for the first box, quadrature for the rest."""
    from math import erf

    def g1(x):
        if s <= 0:
            return np.exp(-0.5 * (x / sigma) ** 2)
        r = sigma * math.sqrt(2.0)
        e = np.vectorize(erf)
        return sigma * math.sqrt(2 * math.pi) / s * 0.5 * (e((x + s / 2) / r) - e((x - s / 2) / r))

    # box d: composite Gauss-Legendre over [-d/2, d/2]
    xb, wb = _gl(-d / 2, d / 2, 16)
    wb = wb / d

    def g2(x):
        x = np.asarray(x, dtype=np.float64)
        return np.tensordot(g1(x[..., None] - xb), wb, axes=([-1], [0]))

    if tau <= 0:
        return g2(phi)
    # exponential: panels over [0, 40 tau], panel width ~ min(tau, sigma) / 2
    h = min(tau, sigma) / 2
    npan = int(math.ceil(40 * tau / h))
    edges = np.linspace(0.0, 40 * tau, npan + 1)
    us, ws = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        x, w = _gl(a, b, 8)
        us.append(x)
        ws.append(w * np.exp(-x / tau) / tau)
    us, ws = np.concatenate(us), np.concatenate(ws)
    phi = np.asarray(phi, dtype=np.float64)
    return np.tensordot(g2(phi[..., None] - us), ws, axes=([-1], [0]))


@pytest.mark.parametrize("tau", [0.0, 2e-4])
def test_pulsar_tables_against_time_domain(tau):
    C, B = 2, 256
    freqs = band(C, lo=1250.0, hi=1256.0)
    s = inj.PulsarSignal(f=83.3, dm=90.0, amp=2.0, width=0.05, tau=tau, spectral_index=-1.5)
    it = inj.Injector([s], freqs, DT, nbins=B)
    tab = it.jobs[0].tables
    ref = 0.5 * (freqs.max() + freqs.min())
    sigma = 0.05 * inj.FWHM_TO_SIGMA
    worst = 0.0
    for c in range(C):
        A = 2.0 * (freqs[c] / ref) ** -1.5
        sm = abs(90.0 * 3.0 / (0.0001205 * freqs[c] ** 3)) * s.f
        tc = tau * (freqs[c] / ref) ** -4.0 * s.f
        phi = np.arange(B) / B
        want = sum(_brute_profile(phi + w, sigma, sm, DT * s.f, tc) for w in (-1, 0, 1)) * A
        worst = max(worst, float(np.max(np.abs(tab[c] - want)) / want.max()))
        # the mean is A_c x the intrinsic area
        area = sigma * math.sqrt(2 * math.pi)
        assert abs(tab[c].mean() - A * area) <= 1e-12 * A * area
    print("worst table error %.3g of the peak" % worst)
    assert worst <= 1e-6
    jobs, _ = io.build([io.sig_dict(s)], freqs, DT, B)
    # (two transform orders: equal to rounding)
    assert np.max(np.abs(jobs[0]["tab64"] - tab)) <= 1e-13 * tab.max()


def test_tabulated_profile_through_its_dft():
    prof = np.zeros(32)
    prof[3:6] = [1.0, 4.0, 2.0]
    s = inj.PulsarSignal(f=10.0, dm=0.0, amp=3.0, profile=prof)
    it = inj.Injector([s], band(2), 1e-6, nbins=64)
    # dt -> 0, no smear: the table is the band-limited profile, peak scaled to amp
    k = np.fft.rfft(prof / 4.0) / 32
    want = np.fft.irfft(np.concatenate([k, np.zeros(33 - k.size)]) * 64, n=64) * 3.0
    assert np.allclose(it.jobs[0].tables[0], want, atol=1e-6)
    assert abs(it.jobs[0].tables[0].mean() - 3.0 * prof.sum() / 4.0 / 32) < 1e-12


def test_burst_tables_ranges_and_truncation():
    C, B = 3, 256
    freqs = band(C, lo=1250.0, hi=1262.0)
    s = inj.BurstSignal(t=0.05, dm=150.0, amp=1.0, width=1e-3, tau=4e-4)
    it = inj.Injector([s], freqs, DT, nbins=B)
    job = it.jobs[0]
    W, lead = job.window, job.lead
    ref = 0.5 * (freqs.max() + freqs.min())
    sigma = 1e-3 * inj.FWHM_TO_SIGMA
    delta = inj.channel_lags(150.0, freqs)
    worst = 0.0
    for c in range(C):
        sm = abs(150.0 * 4.0 / (0.0001205 * freqs[c] ** 3))
        tc = 4e-4 * (freqs[c] / ref) ** -4.0
        x = np.arange(B) / B * W - lead
        want = _brute_profile(x, sigma, sm, DT, tc)
        peak = want.max()
        worst = max(worst, float(np.max(np.abs(job.tables[c] - want)) / peak))
        # what falls outside the window: below 1e-6 of the mass, and of the peak
        out = np.concatenate([np.linspace(-lead - W, -lead, 400), np.linspace(W - lead, 2 * W - lead, 400)])
        vout = _brute_profile(out, sigma, sm, DT, tc)
        assert vout.max() < 1e-6 * peak
        step = out[1] - out[0]
        mass_out = float(vout.sum()) * step  # (two runs of 400 points of the same spacing)
        assert mass_out < 1e-6 * (sigma * math.sqrt(2 * math.pi))
        # the ranges cover every sample whose value exceeds 1e-6 of the peak
        lo, hi = int(job.lo[c]), int(job.hi[c])
        for i in (lo - 3, lo - 2, lo - 1, hi, hi + 1, hi + 2):
            t = (i + 0.5) * DT - delta[c] - s.t
            assert _brute_profile(np.array([t]), sigma, sm, DT, tc)[0] < 1e-6 * peak
        assert lo < (s.t + delta[c]) / DT < hi
        # inside the range the integer phase does not wrap
        ph = io.phases(np.array([lo, hi - 1]), np.array([[job.P0[c], job.step[c]]], dtype=np.uint64),
                       np.zeros((1, 2)))[:, 0]
        assert int(ph[0]) < 1 << 63 <= int(ph[1])
    print("worst burst table error %.3g of the peak" % worst)
    assert worst <= 1e-6


def test_host_arrays_equal_the_oracle_build():
    C, B = 12, 128
    freqs = band(C, descending=False)
    sigs = [inj.PulsarSignal(f=41.7, dm=30.0, amp=0.4, fd=2e-3, fdd=-1e-4, phi0=0.37, start=100,
                             stop=9000),
            inj.BurstSignal(t=0.11, dm=77.0, amp=5.0, width=6e-4, spectral_index=-2.0, tau=1e-4),
            inj.PulsarSignal(f=3.1, dm=0.0, amp=1.0, width=0.2, ref_freq=1400.0)]
    got = inj.Injector(sigs, freqs, DT, nbins=B).host_arrays()
    _, want = io.build([io.sig_dict(s) for s in sigs], freqs, DT, B)
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # the tables: float32 casts of two float64 transforms that agree to
    # rounding -- within one float32 step of each other
    assert got[3].dtype == want[3].dtype == np.float32 and got[3].shape == want[3].shape
    assert np.all(np.abs(got[3] - want[3]) <= np.spacing(np.abs(want[3]).max()))
    assert inj.Injector(sigs, freqs, DT, nbins=B).tables.shape == (3, C, B)


# ---------------------------------------------------------------- dither and quantisation
def test_dither_is_uniform_and_uncorrelated():
    n, C = 1 << 16, 64
    u = io.dither(12345 + np.arange(n), C, seed=7).astype(np.float64)
    N = u.size
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1 / 12.0 / N)
    assert abs(u.var() - 1 / 12.0) <= 5 * math.sqrt((1 / 80.0 - 1 / 144.0) / N)
    z = (u - 0.5) * math.sqrt(12.0)
    for name, a, b in (("time 1", z[1:], z[:-1]), ("time 2", z[2:], z[:-2]),
                       ("chan 1", z[:, 1:], z[:, :-1]), ("chan 2", z[:, 2:], z[:, :-2]),
                       ("diag", z[1:, 1:], z[:-1, :-1])):
        r = float((a * b).mean())
        print("lag %s: %.3g" % (name, r))
        assert abs(r) <= 5 / math.sqrt(a.size), name
    # another seed, another sequence
    assert not np.array_equal(io.dither(np.arange(64), 8, 1), io.dither(np.arange(64), 8, 2))


def _flat(amp):
    return dict(kind="pulsar", f=10.0, dm=0.0, amp=amp, profile=np.ones(8))


def test_sub_lsb_constant_survives_quantisation():
    n, C = 1 << 14, 32
    x = np.full((n, C), 100, dtype=np.uint8)
    y = io.inject(x, 0, [_flat(0.25)], band(C), DT, B=64, seed=3)
    assert set(np.unique(y)) == {100, 101}
    N = y.size
    assert abs(y.mean() - 100.25) <= 5 * math.sqrt(0.25 * 0.75 / N)
    # without a dither the addition would vanish
    assert np.all(np.rint(x.astype(np.float32) + np.float32(0.25)) == 100)


def test_oracle_whole_equals_pieces_and_clips():
    C, n = 10, 3000
    freqs = band(C)
    sigs = [dict(kind="pulsar", f=97.0, dm=40.0, amp=20.0, fd=1e-2, fdd=1e-3, phi0=0.2),
            dict(kind="burst", t=0.06, dm=60.0, amp=300.0, width=1e-3),
            dict(kind="pulsar", f=5.0, dm=0.0, amp=-200.0, width=0.3, start=500, stop=2500)]
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (n, C)).astype(np.uint8)
    whole = io.inject(x, 777, sigs, freqs, DT, B=256, seed=9)
    assert whole.min() == 0 and whole.max() == 255 and not np.array_equal(whole, x)
    parts = [io.inject(x[a:b], 777 + a, sigs, freqs, DT, B=256, seed=9)
             for a, b in ((0, 1), (1, 1300), (1300, 3000))]
    assert np.array_equal(np.concatenate(parts), whole)
    xf = x.astype(np.float32)
    wf = io.inject(xf, 777, sigs, freqs, DT, B=256)
    pf = np.concatenate([io.inject(xf[a:b], 777 + a, sigs, freqs, DT, B=256)
                         for a, b in ((0, 1700), (1700, 3000))])
    assert np.array_equal(wf, pf)
    # vmax = 3: 2-bit data stay 2-bit
    x2 = rng.integers(0, 4, (n, C)).astype(np.uint8)
    y2 = io.inject(x2, 0, sigs, freqs, DT, B=256, vmax=3)
    assert y2.max() == 3 and y2.min() == 0
    # no job: untouched
    assert np.array_equal(io.inject(x, 0, [], freqs, DT, B=64), x)


# ---------------------------------------------------------------- matched S/N
def test_matched_snr_against_the_dedispersed_oracle_block():
    """matched_snr against the noise-free oracle block dedispersed with
    spectra_oracle.sweep_plane: within 1 % for FWHM >= 8 samples (integer
    delay bins cost about 1 / (24 sigma^2) of the peak)."""
    C, n = 32, 6000
    freqs = band(C)
    sigma_chan = np.linspace(3.0, 5.0, C)
    noise = math.sqrt(float(np.sum(sigma_chan ** 2)))
    b = inj.BurstSignal(t=0.1, dm=50.0, amp=0.7, width=8 * DT, spectral_index=-1.0)
    p = inj.PulsarSignal(f=1.0 / (200 * DT), dm=50.0, amp=0.2, width=0.06)
    for s in (b, p):
        it = inj.Injector([s], freqs, DT, nbins=1024)
        m = it.matched_snr(sigma_chan, n)[0]
        x = io.inject(np.zeros((n, C), dtype=np.float32), 0, [io.sig_dict(s)], freqs, DT, B=1024)
        table = orc.sweep_table([50.0], freqs, DT)
        y = orc.sweep_plane(x.T.astype(np.float64), table)[0]
        if s.kind == "burst":
            got = math.sqrt(float(np.sum(y * y))) / noise
        else:
            y = y[:(len(y) // 200) * 200]
            got = math.sqrt(n * float(np.var(y))) / noise
        print("%s: matched %.4f, dedispersed oracle block %.4f" % (s.kind, m, got))
        assert abs(got / m - 1.0) <= 0.01
        # amp_for_snr is the inverse
        a = inj.amp_for_snr(s, 12.0, freqs, DT, sigma_chan, n)
        s2 = inj.BurstSignal(**{k: v for k, v in s.params().items() if k != "kind"}) \
            if s.kind == "burst" else inj.PulsarSignal(**{k: v for k, v in s.params().items() if k != "kind"})
        s2.amp = a
        assert abs(inj.Injector([s2], freqs, DT).matched_snr(sigma_chan, n)[0] - 12.0) < 1e-9


# ---------------------------------------------------------------- spec and refusals
def test_spec_parsing(tmp_path):
    freqs = band(16)
    spec = [dict(kind="pulsar", f=20.0, dm=10.0, snr=30.0, width=0.04),
            dict(t=0.2, dm=30.0, amp=2.5, width=1e-3)]
    fn = tmp_path / "spec.json"
    fn.write_text(json.dumps(spec))
    it = inj.Injector.from_spec(str(fn), freqs, DT, sigma_chan=4.0, n_samples=1 << 14)
    assert [s.kind for s in it.signals] == ["pulsar", "burst"]
    tr = it.truth()
    assert abs(tr[0]["matched_snr"] - 30.0) < 1e-9 and tr[1]["amp"] == 2.5
    assert tr[1]["sample"] == 0.2 / DT and tr[0]["sample"] == 0.0
    json.dumps(tr)  # the truth is JSON
    it2 = inj.Injector.from_spec(dict(signals=spec[1:], nbins=128, seed=5), freqs, DT)
    assert it2.B == 128 and it2.seed == 5 and it2.truth()[0]["matched_snr"] is None


def test_refusals():
    freqs = band(16)
    bad = [[dict(f=20.0, dm=1.0)],                              # neither amp nor snr
           [dict(f=20.0, dm=1.0, amp=1.0, snr=3.0)],            # both
           [dict(f=20.0, dm=1.0, snr=3.0)],                     # snr without a noise level
           [dict(f=20.0, dm=1.0, amp=1.0, colour="red")],       # unknown field
           [dict(kind="comet", amp=1.0)],
           [dict(t=1.0, dm=1.0, amp=1.0)],                      # a burst needs a width
           dict(nothing=1), [7]]
    for spec in bad:
        with pytest.raises(ValueError):
            inj.Injector.from_spec(spec, freqs, DT)
    with pytest.raises(ValueError):
        inj.Injector([], freqs, DT, nbins=100)
    with pytest.raises(ValueError):
        inj.Injector([], freqs, DT, nbins=8192)
    with pytest.raises(ValueError):
        inj.Injector([inj.BurstSignal(0.1, 1.0, 1.0, 1e-3)] * 65, freqs, DT, nbins=64)
    with pytest.raises(ValueError):
        inj.Injector([], freqs, DT, vmax=256)
    with pytest.raises(ValueError):
        inj.PulsarSignal(f=0.0, dm=1.0, amp=1.0)
    with pytest.raises(ValueError):
        inj.PulsarSignal(f=1.0, dm=1.0, amp=1.0, profile="vonmises")
    with pytest.raises(ValueError):
        inj.BurstSignal(t=0.0, dm=1.0, amp=1.0, width=0.0)
    # snr against a noise level of 0 (the MAD of coarsely quantised data): a
    # ValueError for the command-line tools to report, not a division by zero
    flat = inj.robust_sigma(np.full((512, 16), 2, dtype=np.uint8))
    assert not flat.any()
    for spec in ([dict(f=20.0, dm=1.0, snr=3.0)], [dict(t=0.1, dm=1.0, snr=3.0, width=1e-3)]):
        with pytest.raises(ValueError, match="noise level"):
            inj.Injector.from_spec(spec, freqs, DT, sigma_chan=flat, n_samples=4096)
    with pytest.raises(ValueError, match="noise level"):
        inj.Injector([inj.PulsarSignal(f=20.0, dm=1.0, amp=1.0)], freqs, DT).matched_snr(0.0, 4096)


# ---------------------------------------------------------------- recovery
def _sp(rows):
    from pypulsar_amd.search import CAND_DTYPE
    out = np.zeros(len(rows), dtype=CAND_DTYPE)
    for i, (dm, sig, t, down) in enumerate(rows):
        out[i] = (dm, sig, t, int(t / DT), down, 0)
    return out


def test_match_bursts_hit_miss_and_neighbours():
    freqs = band(64)
    dms = np.linspace(0, 200, 201)
    truth = [dict(kind="burst", t=1.0, dm=100.0, width=1e-3, tau=0.0, matched_snr=15.0),
             dict(kind="burst", t=1.004, dm=100.0, width=1e-3, tau=0.0, matched_snr=10.0),
             dict(kind="burst", t=3.0, dm=50.0, width=1e-3, tau=0.0, matched_snr=12.0),
             dict(kind="pulsar", f=3.0, dm=5.0)]
    cands = _sp([(100.0, 14.0, 1.0002, 8), (101.0, 11.0, 1.0004, 8), (100.0, 9.0, 1.0041, 8),
                 (100.0, 30.0, 2.0, 8), (150.0, 40.0, 1.0, 8)])
    rep = rec.match_bursts(truth, cands, dms, freqs, DT, downsamp=2)
    assert [r["index"] for r in rep] == [0, 1, 2]
    assert rep[0]["found"] and rep[0]["sigma"] == 14.0 and abs(rep[0]["time_offset"] - 2e-4) < 1e-12
    assert abs(rep[0]["ratio"] - 14.0 / 15.0) < 1e-12 and rep[0]["dm_offset"] == 0.0
    # two injections 4 ms apart: each finds its own candidate
    assert rep[1]["found"] and rep[1]["sigma"] == 9.0
    assert not rep[2]["found"] and rep[2]["sigma"] is None
    assert rec.match_bursts(truth, _sp([]), dms, freqs, DT)[0]["found"] is False
    # the DM window: two grid steps, or the DM error that crosses the band in one width
    assert rec.dm_window(1e-3, dms, freqs) == 2.0
    wide = rec.dm_window(0.05, dms, freqs)
    assert abs(wide - 0.05 / (1 / (0.000241 * freqs.min() ** 2) - 1 / (0.000241 * freqs.max() ** 2))) < 1e-9


def test_match_pulsars_harmonics():
    from pypulsar_amd.periodicity import CAND_DTYPE
    freqs = band(64)
    dms = np.linspace(0, 100, 101)
    T = 4.0
    truth = [dict(kind="pulsar", f=50.0, dm=20.0, width=0.05), dict(kind="pulsar", f=7.0, dm=60.0, width=0.05),
             dict(kind="pulsar", f=11.0, dm=80.0, width=0.05)]
    rows = [(20.0, 100.2, 12.0), (20.0, 50.1, 9.0), (60.0, 3.5, 8.0), (80.0, 11.6, 20.0),
            (90.0, 11.0, 50.0)]
    cands = np.zeros(len(rows), dtype=CAND_DTYPE)
    for i, (dm, f, s) in enumerate(rows):
        cands[i]["DM"], cands[i]["freq"], cands[i]["sigma"] = dm, f, s
    rep = rec.match_pulsars(truth, cands, T, dms, freqs, DT)
    assert rep[0]["found"] and rep[0]["harmonic"] == "2*f" and rep[0]["sigma"] == 12.0
    assert abs(rep[0]["freq_offset"] - 0.2) < 1e-9
    assert rep[1]["found"] and rep[1]["harmonic"] == "f/2" and rep[1]["freq_offset"] == 0.0
    assert not rep[2]["found"]  # 0.6 Hz off (window 0.375), and the 11.0 Hz one is 10 DM away
    assert rec.harmonic_relation(50.3, 50.0, T)[0] == "f"
    assert rec.harmonic_relation(50.5, 50.0, T) is None
