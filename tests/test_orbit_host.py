"""The orbit demodulation on the host: the oracle against its own definition,
the knot rule, the template bank, the ``.orbcands`` files and the arguments
that pdd_orbit_resample refuses before any HIP call.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import orbit_cases as oc
import orbit_oracle as oo
import sideband_cases as sc


@pytest.fixture(scope="module")
def exact():
    """name -> exact positions of all N output samples."""
    return {k: oo.positions(oc.ORBITS[k], np.arange(oc.N), oc.DT) for k in oc.NAMES}


@pytest.mark.parametrize("name", oc.NAMES)
def test_oracle_inverts_its_delay(exact, name):
    o, p = oc.ORBITS[name], exact[name]
    t = p * oc.DT
    res = (t - oo.delay(o, t)[0] + oo.delay(o, 0.0)[0]) / oc.DT - np.arange(oc.N)
    d = p - np.arange(oc.N)
    print("%s: beta %.3f, p - j in %.1f .. %.1f samples, residual %.2e samples"
          % (name, oo.beta(o), d.min(), d.max(), np.max(np.abs(res))))
    assert p[0] == 0.0
    assert np.max(np.abs(res)) <= 1e-9
    assert np.all(np.diff(p) > 0.0)
    assert int(np.sum((p < 0.0) | (p > oc.N - 1))) == oc.FILL_COUNT[name]


def test_excursions():
    """The spans the cases were chosen for, to the nearest sample."""
    want = {"circ": (-33, 7), "ecc": (-5, 24), "tight": (-1, 1), "wide": (-206, 64)}
    for name in oc.NAMES:
        d = oo.positions(oc.ORBITS[name], np.arange(oc.N), oc.DT) - np.arange(oc.N)
        assert (int(np.rint(d.min())), int(np.rint(d.max()))) == want[name], name


@pytest.mark.parametrize("name", ("circ", "tight", "wide"))
def test_circular_closed_form(name):
    pb, x, _, _, t0 = oc.ORBITS[name]
    t = np.linspace(-3.0, 20.0, 4001)
    want = x * np.sin(2.0 * np.pi * t / pb - 2.0 * np.pi * t0 / pb)
    assert np.max(np.abs(oo.delay(oc.ORBITS[name], t)[0] - want)) <= 1e-15 + 1e-13 * x


def test_kepler_solves_its_equation():
    M = np.linspace(-20.0, 20.0, 2001)
    for e in (0.0, 0.1, 0.4, 0.79, 0.8, 0.95, 0.999):
        E = oo.kepler(M, e)
        assert np.max(np.abs(E - e * np.sin(E) - M)) <= 1e-13, e


def test_product_helpers_agree_with_the_oracle(exact):
    from pypulsar_amd import orbit
    t = np.linspace(-1.0, 17.0, 501)
    for name in oc.NAMES:
        o = oc.ORBITS[name]
        assert np.max(np.abs(orbit.roemer(orbit.Orbit(*o), t) - oo.delay(o, t)[0])) <= 1e-13
        assert np.max(np.abs(orbit.positions(o, oc.N, oc.DT) - exact[name])) <= 1e-9
        assert abs(orbit.beta(o)[0] - oo.beta(o)) <= 1e-15
    both = orbit.roemer([oc.ORBITS["circ"], oc.ORBITS["ecc"]], t)
    assert both.shape == (2, len(t))
    assert np.array_equal(both[1], orbit.roemer(oc.ORBITS["ecc"], t))


@pytest.mark.parametrize("name", oc.NAMES)
def test_knot_rule(exact, name):
    """The rule's K, and the error of interpolating between exact knots at
    that K against its 1e-3 budget."""
    from pypulsar_amd import orbit
    o = oc.ORBITS[name]
    K = orbit.knot_spacing([o], oc.DT)
    assert K == oo.spacing([o], oc.DT) == oc.KNOT_K[name]
    err = np.max(np.abs(oo.interpolate(oo.knots(o, oc.N, K, oc.DT), oc.N, K) - exact[name]))
    print("%s: K = %d, interpolation error %.2e samples (budget 1e-3)" % (name, K, err))
    assert err <= 1e-3
    # several orbits in one launch: the smallest spacing
    assert orbit.knot_spacing([oc.ORBITS[k] for k in oc.NAMES], oc.DT) == 4
    assert orbit.knot_spacing([oc.IDENTITY], oc.DT) == 256


def test_sampling_modes():
    row = np.arange(8, dtype=np.float32) * 2.0
    p = np.asarray([-0.1, 0.0, 0.49, 0.5, 2.25, 6.5, 7.0, 7.01, np.nan])
    near = oo.sample(row, p, oo.NEAREST, -1.0)
    lin = oo.sample(row, p, oo.LINEAR, -1.0)
    assert near.tolist() == [-1.0, 0.0, 0.0, 2.0, 4.0, 14.0, 14.0, -1.0, -1.0]
    assert lin.tolist() == [-1.0, 0.0, float(np.float32(2.0) * np.float32(0.49)), 1.0, 4.5, 13.0,
                            14.0, -1.0, -1.0]
    assert near.dtype == lin.dtype == np.float32


def test_bad_orbits_are_refused():
    from pypulsar_amd import orbit
    good = oc.ORBITS["circ"]
    assert orbit.validate(good).shape == (1, 5)
    for bad in ((1.0, 0.02, 0.0, 0.0, 0.0),            # beta = 0.126
                (10.0, 0.1, 0.5, 0.0, 0.0),            # beta = 0.126 through 1 / (1 - e)
                (good[0], good[1], 1.0, 0.0, 0.0),
                (good[0], good[1], -0.1, 0.0, 0.0),
                (0.0, 0.0, 0.0, 0.0, 0.0),
                (-1.0, 0.0, 0.0, 0.0, 0.0),
                (good[0], -0.01, 0.0, 0.0, 0.0),
                (good[0], good[1], 0.0, np.nan, 0.0),
                (good[0], good[1], 0.0, 0.0, np.inf)):
        with pytest.raises(ValueError):
            orbit.validate([good, bad])
        with pytest.raises(ValueError):
            orbit.positions(bad, 16, oc.DT)


def test_bank_follows_the_rule():
    from pypulsar_amd import orbit
    args = (0.96, 0.99, 0.0031, 305.0, 8.192)
    bank = orbit.circular_bank(*args, mismatch=0.05)
    rule = oo.bank_counts(*args, m=0.05)
    assert len(bank) == sum(a * b for _, a, b in rule)
    assert not bank[:, 2].any() and not bank[:, 3].any()
    assert np.all(orbit.beta(bank) <= 0.1)
    at = 0
    for x, npsi, nw in rule:
        part = bank[at:at + npsi * nw]
        assert np.allclose(part[:, 1], x, rtol=1e-15, atol=0)
        w = 2.0 * np.pi / part[:, 0]
        cells = 2.0 * np.pi / 0.99 + (np.arange(nw) + 0.5) * (2.0 * np.pi / 0.96 -
                                                             2.0 * np.pi / 0.99) / nw
        assert np.allclose(w.reshape(nw, npsi), cells[:, None], rtol=1e-13, atol=0)
        psi = (-2.0 * np.pi * part[:, 4] / part[:, 0]).reshape(nw, npsi)
        assert np.allclose(psi, 2.0 * np.pi * np.arange(npsi)[None, :] / npsi, rtol=0, atol=1e-12)
        at += npsi * nw
    # the steps: dx = 2 m / f_top, and neighbours in psi differ by at most 2 m / (f_top x)
    assert abs(rule[0][0] - 2 * 0.05 / 305.0) <= 1e-18
    for x, npsi, _ in rule:
        assert 2.0 * np.pi / npsi <= 2 * 0.05 / (305.0 * x) * (1 + 1e-12)
    coarse = orbit.circular_bank(*args, mismatch=0.1)
    assert len(coarse) < len(bank)


def test_derived_recovery_bank():
    """The bank that follows the recovery case's sideband candidate (L = 256,
    q = 61) has 76 777 templates at m = 0.05, whichever of the three segments
    that hold the signal reported it; a limit below that raises with the
    count."""
    from pypulsar_amd import orbit
    for lo in (2313, 2377, 2441):
        args = oc.derived_bank_args(lo=lo)
        assert sum(a * b for _, a, b in oo.bank_counts(*args)) == 76777
        assert args[0] <= sc.PORB <= args[1] and args[2] >= oc.X_TRUE
    bank = orbit.circular_bank(*oc.derived_bank_args())
    assert bank.shape == (76777, 5)
    with pytest.raises(ValueError, match="76777"):
        orbit.circular_bank(*oc.derived_bank_args(), max_templates=100)


def node_power(series, orb):
    """Whitened power at the signal's bin of ``series`` demodulated by ``orb``
    (nearest mode, the rule's knots)."""
    K = oo.spacing([orb], sc.DT)
    out = oo.resample(series.astype(np.float32), orb, sc.DT, K, oo.NEAREST,
                      np.float32(series.mean()))
    return float(sc.whitened_powers(out)[2500])


def test_corner_retention():
    """Half a bank step away from the true orbit in all three coordinates at
    once -- the worst place between nodes -- at least half the power is kept
    (m = 0.05: 0.67 is measured here; m = 0.1 keeps about 0.3)."""
    series = sc.recovery_series(0)
    plain = float(sc.whitened_powers(series)[2500])
    node = node_power(series, oc.TRUE_ORBIT)
    m = oc.MISMATCH
    dx = 2.0 * m / sc.F0
    dpsi = 2.0 * m / (sc.F0 * oc.X_TRUE)
    dw = 2.0 * m / (sc.F0 * oc.X_TRUE * sc.N * sc.DT)
    worst = 1.0
    for sx, sp, sw in itertools.product((-0.5, 0.5), repeat=3):
        orb = oc.circular(oc.X_TRUE + sx * dx, oc.W0 + sw * dw, oc.PSI + sp * dpsi)
        worst = min(worst, node_power(series, orb) / node)
    print("power at bin 2500: plain %.2f, true orbit %.2f; worst half-step corner keeps %.3f"
          % (plain, node, worst))
    assert node > 3.0 * plain
    assert worst >= 0.5


def test_exact_orbit_collects_the_comb():
    """The true orbit puts the comb's power into bin 2500: 9.0, 7.8, 9.4 and
    7.7 sigma for seeds 0-3 where the plain search has at most 5.3."""
    import period_oracle as po
    for seed, want in zip(range(4), (9.0, 7.8, 9.4, 7.7)):
        series = sc.recovery_series(seed)
        K = oo.spacing([oc.TRUE_ORBIT], sc.DT)
        out = oo.resample(series.astype(np.float32), oc.TRUE_ORBIT, sc.DT, K, oo.NEAREST,
                          np.float32(series.mean()))
        p = sc.whitened_powers(out)
        k = int(np.argmax(p[sc.rlo():])) + sc.rlo()
        s = po.sigma(float(p[k]), 1)
        print("seed %d: bin %d at %.2f sigma" % (seed, k, s))
        assert k == 2500 and abs(s - want) <= 0.3


def fake_cands():
    from pypulsar_amd.orbit import ORBCAND_DTYPE
    c = np.zeros(5, dtype=ORBCAND_DTYPE)
    c["r"] = [2500, 2501, 5000, 1250, 3111]
    c["sigma"] = [10.4, 9.1, 7.0, 6.5, 6.2]
    c["numharm"] = [1, 1, 2, 1, 1]
    c["power"] = np.asarray([60.1, 50.3, 40.7, 30.9, 28.4], dtype=np.float32)
    c["template"] = [7, 8, 7, 3, 11]
    c["DM"] = 12.5
    c["freq"] = c["r"] / 8.192
    c["period"] = 1.0 / c["freq"]
    bank = np.asarray([oc.circular(0.003 + 1e-4 * k, oc.W0 * (1 + 1e-3 * k), 0.1 * k)
                       for k in range(12)])
    for k, name in enumerate(("pb", "x", "e", "omega", "t0")):
        c[name] = bank[c["template"], k]
    return c


def test_sift_and_files(tmp_path):
    from pypulsar_amd import orbit
    c = fake_cands()
    s = orbit.sift(c[::-1], ntemplates=12)
    assert s.dtype == orbit.SIFTED_DTYPE
    assert s["r"].tolist() == [2500, 3111] and s["nhits"].tolist() == [4, 1]
    assert s["template"].tolist() == [7, 11] and np.all(s["ntemplates"] == 12)
    fn = str(tmp_path / "a.orbcands")
    orbit.write_orbcands(s[::-1], fn)
    back = orbit.read_orbcands(fn)
    assert back.dtype.names == orbit.ORBCANDS_COLUMNS and len(back) == 2
    assert np.all(np.diff(back["sigma"]) <= 0)
    for name in orbit.ORBCANDS_COLUMNS:
        assert np.array_equal(back[name], s[name]), name     # exact: shortest round-trip form
        assert back[name].dtype == s[name].dtype
    orbit.write_orbcands_npz(s, str(tmp_path / "a_orbcands.npz"))
    z = np.load(str(tmp_path / "a_orbcands.npz"))
    assert sorted(z.files) == sorted(orbit.ORBCANDS_COLUMNS)
    for name in orbit.ORBCANDS_COLUMNS:
        assert np.array_equal(z[name], back[name]), name
    empty = orbit.sift(c[:0])
    orbit.write_orbcands(empty, fn)
    assert len(orbit.read_orbcands(fn)) == 0


def test_entry_point_refuses_before_any_hip_call():
    """As tests/test_abi.py does for pdd_shift_pad: argument validation comes
    before any HIP call, so it can be checked without a GPU.  The pointers are
    never dereferenced."""
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dt, fill = ctypes.c_double(1e-3), ctypes.c_float(0.0)

    def refused(*args):
        st = h.pdd_orbit_resample(*args)
        return st < 0, h.pdd_last_error()

    for row, orbs, out in ((None, p, p), (p, None, p), (p, p, None)):
        ok, msg = refused(row, 16, dt, orbs, 1, 16, 0, fill, out, 16, None, None)
        assert ok and b"null pointer" in msg
    for n in (-1, 0, 1, 1 << 31):
        ok, msg = refused(p, n, dt, p, 1, 16, 0, fill, p, max(n, 2), None, None)
        assert ok and b"n must be" in msg
    ok, msg = refused(p, 16, dt, p, 1, 16, 0, fill, p, 15, None, None)
    assert ok and b"ld_out" in msg
    for bad_dt in (0.0, -1e-3):
        ok, msg = refused(p, 16, ctypes.c_double(bad_dt), p, 1, 16, 0, fill, p, 16, None, None)
        assert ok and b"dt" in msg
    for K in (0, -4, 3, 24, 512):
        ok, msg = refused(p, 16, dt, p, 1, K, 0, fill, p, 16, None, None)
        assert ok and b"K must be" in msg
    for mode in (-1, 2):
        ok, msg = refused(p, 16, dt, p, 1, 16, mode, fill, p, 16, None, None)
        assert ok and b"mode" in msg
    ok, msg = refused(p, (1 << 31) - 1, dt, p, 1 << 30, 1, 0, fill, p, 1 << 31, None, None)
    assert ok and b"too many templates" in msg
    # no template: nothing to do, whatever else is passed
    assert h.pdd_orbit_resample(p, 16, dt, p, 0, 16, 0, fill, p, 16, None, None) == 0
