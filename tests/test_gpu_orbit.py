"""pdd_orbit_resample / pypulsar_amd.orbit on the device against
tests/orbit_oracle.py: the knots, the bits of both sampling modes on the
device's own knots, the positions against the float64 oracle, the edges, the
search over a bank and the recovery case.

The four orbits of tests/orbit_cases.py and the ``x = 0`` template go in one
launch.  The row is a view inside a buffer that holds 7e5 on both sides, and
``out`` a strided view whose padding must keep its poison: a lane that read
outside the row, or wrote beyond column n, would show."""
import numpy as np
import pytest

import orbit_cases as oc
import orbit_oracle as oo
import period_oracle as po
import sideband_cases as sc

pytestmark = pytest.mark.gpu

POISON = 7e5
FILL = -7.0
ORBITS = np.asarray([oc.ORBITS[k] for k in oc.NAMES] + [oc.IDENTITY], dtype=np.float64)
K_ALL = 4                       # the rule's spacing for the five together (the tight one's)
MODES = {"nearest": oo.NEAREST, "linear": oo.LINEAR}


def device_row(torch, host, lead=13, tail=29):
    """[n] device view of ``host`` inside a buffer poisoned on both sides."""
    host = np.asarray(host, dtype=np.float32)
    buf = torch.full((lead + len(host) + tail,), POISON, dtype=torch.float32, device="cuda")
    view = buf[lead:lead + len(host)]
    view.copy_(torch.from_numpy(host))
    return view


def poisoned_out(torch, T, n, pad=37):
    buf = torch.full((T, n + pad), POISON, dtype=torch.float32, device="cuda")
    return buf, buf[:, :n]


def run(torch, host_row, mode, pad=37, K=None, orbits=ORBITS, want_knots=True, dt=oc.DT):
    """(out [T, n] float32, knots [T, nk] float64 or None) on the host; the
    padding of ``out`` is checked here."""
    from pypulsar_amd.orbit import Resampler
    row = device_row(torch, host_row)
    buf, view = poisoned_out(torch, len(orbits), len(host_row), pad)
    res = Resampler(mode)(row, orbits, dt, fill=FILL, want_knots=want_knots, K=K, out=view)
    torch.cuda.synchronize()
    assert torch.all(buf[:, len(host_row):] == POISON), "wrote beyond column n"
    if want_knots:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy(), None


def restated(host_row, knots, K, mode):
    """The oracle's rows on the given knot tables."""
    return np.stack([oo.sample(host_row, oo.interpolate(k, len(host_row), K), MODES[mode], FILL)
                     for k in knots])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32),
                          np.asarray(b, dtype=np.float32).view(np.int32))


@pytest.fixture(scope="module")
def ramp():
    return np.arange(oc.N, dtype=np.float32)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(11).standard_normal(oc.N).astype(np.float32)


@pytest.fixture(scope="module")
def exact():
    """[5, N] float64 positions by the oracle."""
    return np.stack([oo.positions(o, np.arange(oc.N), oc.DT) for o in ORBITS])


def test_rule_spacing():
    from pypulsar_amd.orbit import knot_spacing
    assert knot_spacing(ORBITS, oc.DT) == K_ALL


def test_knots(gpu, ramp):
    """The dumped knots against the oracle: 1e-6 samples is three orders under
    the interpolation budget; float64 round-off of the phase is about 1e-10
    here."""
    import torch
    _, knots = run(torch, ramp, "nearest")
    assert knots.shape == (5, oo.knot_count(oc.N, K_ALL))
    worst = 0.0
    for o, k in zip(ORBITS, knots):
        worst = max(worst, float(np.max(np.abs(k - oo.knots(o, oc.N, K_ALL, oc.DT)))))
    print("knots: max |device - oracle| = %.2e samples (bar 1e-6)" % worst)
    assert worst <= 1e-6
    assert np.all(knots[:, 0] == 0.0)
    assert np.array_equal(knots[4], K_ALL * np.arange(knots.shape[1], dtype=np.float64))


@pytest.mark.parametrize("pad", [37, 38, 40])       # stores of 1, 2 and 4 floats
@pytest.mark.parametrize("mode", ["nearest", "linear"])
def test_bit_parity(gpu, ramp, noise, mode, pad):
    """Both modes are bit for bit the restatement evaluated on the device's
    own knots; with the ramp, nearest mode shows the index itself."""
    import torch
    for host in (ramp, noise):
        out, knots = run(torch, host, mode, pad=pad)
        assert same_bits(out, restated(host, knots, K_ALL, mode))
    assert same_bits(out[4], noise)                  # x = 0: the row itself


@pytest.mark.parametrize("K", [1, 256])             # one knot a sample; the fewest knots a tile
def test_bit_parity_at_the_extreme_spacings(gpu, noise, K):
    import torch
    for mode in MODES:
        out, knots = run(torch, noise, mode, K=K, pad=40)
        assert knots.shape == (5, oo.knot_count(oc.N, K))
        assert same_bits(out, restated(noise, knots, K, mode))
        assert same_bits(out[4], noise)


def test_against_the_oracle(gpu, ramp, exact):
    """Ramp, linear mode: the output is the position itself.  5e-3 = the 1e-3
    interpolation budget plus three float32 half-ulps at 2^14."""
    import torch
    out, _ = run(torch, ramp, "linear")
    inside = (exact >= 0.0) & (exact <= oc.N - 1)
    err = np.abs(out.astype(np.float64) - exact)[inside]
    print("linear ramp: max |out - p| = %.2e samples (bar 5e-3)" % err.max())
    assert err.max() <= 5e-3
    near, _ = run(torch, ramp, "nearest")
    assert np.max(np.abs(near.astype(np.float64) - exact)[inside]) <= 0.5 + 1e-3


def test_fill(gpu, ramp, noise, exact):
    """Outputs whose position leaves the row take the fill value: 61 at the
    end of the wide orbit, 1 in the tight one, none elsewhere."""
    import torch
    want = [oc.FILL_COUNT[k] for k in oc.NAMES] + [0]
    assert [int(np.sum((p < 0) | (p > oc.N - 1))) for p in exact] == want
    for mode in MODES:
        out, _ = run(torch, ramp, mode)               # (the ramp is >= 0: FILL is not a sample)
        assert [int(np.sum(r == FILL)) for r in out] == want
        assert np.all(out[3, -61:] == FILL)
    assert same_bits(run(torch, noise, "linear")[0][4], noise)


@pytest.mark.parametrize("n", [16421, 2])            # no multiple of the tile or of K; the least
def test_odd_lengths(gpu, n):
    import torch
    host = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    for mode in MODES:
        for pad in (37, 40):
            out, knots = run(torch, host, mode, pad=pad)
            assert knots.shape == (5, oo.knot_count(n, K_ALL))
            assert same_bits(out, restated(host, knots, K_ALL, mode))
            assert same_bits(out[4], host)
    worst = max(float(np.max(np.abs(k - oo.knots(o, n, K_ALL, oc.DT))))
                for o, k in zip(ORBITS, knots))
    assert worst <= 1e-6


def test_launches_agree(gpu, noise):
    """The same bits with and without the knot dump, on a second launch, and
    for the templates split over two launches."""
    import torch
    for mode in MODES:
        a, ka = run(torch, noise, mode, K=K_ALL)
        b, kb = run(torch, noise, mode, K=K_ALL)
        c, _ = run(torch, noise, mode, K=K_ALL, want_knots=False)
        lo, klo = run(torch, noise, mode, K=K_ALL, orbits=ORBITS[:2])
        hi, khi = run(torch, noise, mode, K=K_ALL, orbits=ORBITS[2:])
        assert same_bits(a, b) and same_bits(a, c)
        assert np.array_equal(ka.view(np.int64), kb.view(np.int64))
        assert same_bits(a, np.concatenate((lo, hi)))
        assert np.array_equal(ka.view(np.int64), np.concatenate((klo, khi)).view(np.int64))


def test_defaults_and_refusals(gpu, noise):
    """fill defaults to the row's mean; orbits are validated before upload;
    ``demodulated`` is the one-template nearest resample."""
    import torch
    from pypulsar_amd.orbit import Resampler, demodulated
    row = device_row(torch, noise)
    out = Resampler("nearest")(row, [oc.ORBITS["wide"]], oc.DT)
    assert out.shape == (1, oc.N) and out.is_contiguous()
    tail = out[0, -61:].cpu().numpy()
    assert np.all(tail == tail[0]) and abs(float(tail[0]) - float(noise.mean())) <= 1e-6
    assert torch.equal(demodulated(row, oc.ORBITS["wide"], oc.DT), out[0])
    with pytest.raises(ValueError):
        Resampler("nearest")(row, [(1.0, 0.02, 0.0, 0.0, 0.0)], oc.DT)
    with pytest.raises(ValueError):
        Resampler("cubic")
    assert Resampler("linear")(row, np.empty((0, 5)), oc.DT).shape == (0, oc.N)


# ---- the search over a bank ----

@pytest.fixture(scope="module")
def recovery():
    """(series float32 [8192], bank [45, 5])."""
    return sc.recovery_series(0).astype(np.float32), oc.recovery_bank()


def oracle_recovery(series, bank, sigma=6.0, harms=sc.HARMS):
    """The oracle's candidates over the bank, by descending sigma: (sigma,
    template, bin, H, power)."""
    thr = np.asarray([po.threshold_power(sigma, h) for h in harms], dtype=np.float32)
    fill = np.float32(series.astype(np.float64).mean())
    K = oo.spacing(bank, sc.DT)
    out = []
    for t, orb in enumerate(bank):
        p = sc.whitened_powers(oo.resample(series, orb, sc.DT, K, oo.NEAREST, fill))
        for _, k, H, bits in po.candidates(p[None, :], harms, thr, sc.rlo()):
            power = float(np.asarray([bits], dtype=np.int32).view(np.float32)[0])
            out.append((po.sigma(power, H), t, k, H, power))
    return sorted(out, reverse=True)


def test_search_is_the_periodicity_search_of_the_resampled_rows(gpu, recovery):
    import torch
    from pypulsar_amd.orbit import ORBCAND_DTYPE, OrbitSearch, Resampler, knot_spacing
    from pypulsar_amd.periodicity import CAND_DTYPE, PeriodicitySearch
    series, bank = recovery
    row = device_row(torch, series)
    got = OrbitSearch(3.5, sc.HARMS, "nearest", flo=sc.FLO)(row, 12.5, sc.DT, bank, nfft=sc.N,
                                                            row_batch=16)
    plane = Resampler("nearest")(row, bank, sc.DT, K=knot_spacing(bank, sc.DT))
    want = PeriodicitySearch(3.5, sc.HARMS, flo=sc.FLO)(plane, np.full(len(bank), 12.5), sc.DT,
                                                        nfft=sc.N)
    assert got.dtype == ORBCAND_DTYPE and len(got) == len(want) > len(bank)
    want = np.sort(want, order=("row", "numharm", "r"))
    for name in CAND_DTYPE.names:
        if name != "row":
            assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["template"], want["row"]) and not got["row"].any()
    for k, name in enumerate(("pb", "x", "e", "omega", "t0")):
        assert np.array_equal(got[name], bank[got["template"], k]), name
    # candidates above fhi are dropped on the host
    cut = OrbitSearch(3.5, sc.HARMS, "nearest", flo=sc.FLO, fhi=200.0)(row, 12.5, sc.DT, bank,
                                                                       nfft=sc.N)
    assert np.array_equal(cut, got[got["freq"] <= 200.0]) and 0 < len(cut) < len(got)


def test_recovery(gpu, recovery):
    """A 3 x 5 x 3 bank around the true orbit, off its nodes: the best
    candidate is the oracle's template and bin (bin 2500 at 10.79 sigma on the
    rule's knots, K = 4 -- 10.98 with every position exact: two samples of the
    8192 are taken one later -- and the runner-up at 10.34), its power within
    the bar tests/test_gpu_period.py applies to whitened powers; the plain
    search of the row has nothing above 6 sigma."""
    import torch
    from pypulsar_amd.orbit import OrbitSearch, sift
    from pypulsar_amd.periodicity import PeriodicitySearch
    series, bank = recovery
    ref = oracle_recovery(series, bank)
    row = device_row(torch, series)
    got = OrbitSearch(6.0, sc.HARMS, "nearest", flo=sc.FLO)(row, 0.0, sc.DT, bank, nfft=sc.N)
    top = got[np.argmax(got["sigma"])]
    print("oracle: sigma %.2f template %d bin %d H %d (next %.2f); device: sigma %.2f template "
          "%d bin %d H %d" % (ref[0][:4] + (ref[1][0],) + (top["sigma"], top["template"],
                                                          top["r"], top["numharm"])))
    assert ref[0][2] == 2500 and abs(ref[0][0] - 10.79) <= 0.05 and abs(ref[2][0] - 10.34) <= 0.05
    p = oo.positions(bank[ref[0][1]], np.arange(sc.N), sc.DT)
    every = sc.whitened_powers(oo.sample(series, p, oo.NEAREST, np.float32(series.mean())))
    assert int(np.argmax(every[sc.rlo():])) + sc.rlo() == 2500
    assert abs(po.sigma(float(every[2500]), 1) - 10.98) <= 0.05
    assert (int(top["template"]), int(top["r"]), int(top["numharm"])) == ref[0][1:4]
    assert abs(float(top["power"]) - ref[0][4]) <= 1e-5 * ref[0][4]
    s = sift(got, ntemplates=len(bank))
    assert s[0]["template"] == top["template"] and s[0]["ntemplates"] == 45
    assert s[0]["nhits"] >= 2 and s["nhits"].sum() == len(got)
    plain = PeriodicitySearch(6.0, sc.HARMS, flo=sc.FLO)(row[None, :], [0.0], sc.DT, nfft=sc.N)
    assert len(plain) == 0
