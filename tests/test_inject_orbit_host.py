"""Keplerian orbits in the injector's host model (pypulsar_amd/inject.py)
against their NumPy restatement (tests/inject_orbit_oracle.py), the grading of
the binary searches (pypulsar_amd/recovery.py) and the argument checks of
pdd_inject_orbit.  No GPU."""
import ctypes
import json
import math

import numpy as np
import pytest

import inject_oracle as io
import inject_orbit_oracle as ioo
import orbit_oracle as oo
from conftest import band
from pypulsar_amd import inject as inj
from pypulsar_amd import recovery as rec

DT = 64e-6

# (f, orbit (pb, x, e, omega, t0)): circular and wide; circular and tight; eccentric
ORBITS = {
    "wide": (30.0, (3600.0, 2.0, 0.0, 0.0, 700.0)),
    "tight": (500.0, (600.0, 0.5, 0.0, 0.0, 123.0)),
    "ecc": (100.0, (1800.0, 0.3, 0.6, 1.0, -250.0)),
}


def _pulsar(f, orb, **kw):
    kw.setdefault("dm", 100.0)
    kw.setdefault("amp", 5.0)
    return inj.PulsarSignal(f=f, pb=orb[0], x=orb[1], e=orb[2], omega=orb[3], t0=orb[4], **kw)


# ---------------------------------------------------------------- tables and constants
@pytest.mark.parametrize("name", sorted(ORBITS))
def test_orbit_arrays_against_the_oracle(name):
    f, orb = ORBITS[name]
    freqs = band(8)
    it = inj.Injector([_pulsar(f, orb, fd=1e-7)], freqs, DT, nbins=64)
    ophase, ometa, qtab = it.orbit_arrays()
    wp, wm, wq = ioo.orbit_arrays([io.sig_dict(s) for s in it.signals], freqs, DT)
    assert ophase.dtype == np.uint64 and ometa.dtype == np.int64 and qtab.dtype == np.float64
    assert np.array_equal(ophase, wp) and np.array_equal(ometa, wm)
    M = 1 << int(ometa[0, 0])
    assert qtab.shape == wq.shape == (M + 1,) and qtab[M] == qtab[0]
    err = float(np.max(np.abs(qtab - wq)))
    print("%s: m = %d, qtab against the bisection table: %.3g turns" % (name, ometa[0, 0], err))
    assert err <= 1e-9
    # the four arrays of pdd_inject do not know about the orbit
    plain = inj.Injector([inj.PulsarSignal(f=f, dm=100.0, amp=5.0, fd=1e-7)], freqs, DT, nbins=64)
    for a, b in zip(it.host_arrays(), plain.host_arrays()):
        assert np.array_equal(a, b)


def test_two_orbits_share_qtab():
    freqs = band(4)
    sigs = [_pulsar(*ORBITS["wide"]), inj.PulsarSignal(f=9.0, dm=3.0, amp=1.0),
            inj.BurstSignal(t=0.1, dm=5.0, amp=3.0, width=1e-3), _pulsar(*ORBITS["ecc"])]
    it = inj.Injector(sigs, freqs, DT, nbins=64)
    ophase, ometa, qtab = it.orbit_arrays()
    assert list(ometa[:, 0]) == [sigs[0].m, -1, -1, sigs[3].m]
    assert ometa[0, 2] == 0 and ometa[3, 2] == 8 * ((1 << sigs[0].m) + 1)
    assert qtab.size == (1 << sigs[0].m) + 1 + (1 << sigs[3].m) + 1
    assert not ophase[1].any() and not ophase[2].any() and ophase[0].any()
    wp, wm, wq = ioo.orbit_arrays([io.sig_dict(s) for s in sigs], freqs, DT)
    assert np.array_equal(ophase, wp) and np.array_equal(ometa, wm)
    assert np.max(np.abs(qtab - wq)) <= 1e-9


def test_table_size_is_minimal_and_capped():
    for name, (f, orb) in ORBITS.items():
        s = _pulsar(f, orb)
        A = f * orb[1] * (2 * math.pi) ** 2 / (1 - orb[2]) ** 3
        assert s.m == ioo.table_bits(f, orb) and 6 <= s.m <= 22
        assert A / (8.0 * 4.0 ** s.m) <= 1e-6
        assert s.m == 6 or A / (8.0 * 4.0 ** (s.m - 1)) > 1e-6, name
    assert _pulsar(1.0, (1000.0, 5e-4, 0.0, 0.0, 0.0)).m == 6   # the floor: 6e-7 turns at m = 6
    # beta = 6.3e-3, but f x (2 pi)^2 / (1 - e)^3 = 3.9e8 needs m = 23
    with pytest.raises(ValueError) as e:
        _pulsar(1000.0, (1e5, 10.0, 0.9, 0.0, 0.0))
    assert "f = " in str(e.value) and "x = " in str(e.value) and "e = " in str(e.value)


# ---------------------------------------------------------------- model accuracy
@pytest.mark.parametrize("name", sorted(ORBITS))
def test_integer_phase_against_the_direct_float64_phase(name):
    """10^4 random cells with i < 2^26, 64 channels, DM 100: the integer phase
    p within 2e-6 turns of Phi(t) evaluated directly with orbit.roemer (1e-6:
    the table's budget; 1e-6: the rounding of ostep over 2^26 samples times 2
    pi f x, and float64 round-off of the direct evaluation)."""
    from pypulsar_amd import orbit
    f, orb = ORBITS[name]
    freqs = band(64)
    fd, phi0 = (2e-7, 0.3) if name == "wide" else (0.0, 0.0)
    it = inj.Injector([_pulsar(f, orb, fd=fd, phi0=phi0)], freqs, DT, nbins=64)
    phase, drift, _, _ = it.host_arrays()
    ophase, ometa, qtab = it.orbit_arrays()
    rng = np.random.default_rng(5)
    i = np.concatenate([[0, 1, (1 << 26) - 1], rng.integers(0, 1 << 26, 10000 - 3)]).astype(np.int64)
    c = rng.integers(0, 64, i.size)
    p = ioo.job_phases(i, 0, phase, drift, ophase, ometa, qtab)[np.arange(i.size), c]
    delta = inj.channel_lags(100.0, freqs)[c]
    t = (i.astype(np.float64) + 0.5) * DT - delta
    D = orbit.roemer(orb, t) - orbit.roemer(orb, [0.0])[0]
    want = phi0 + f * t + fd * t * t / 2.0 - f * D
    err = p.astype(np.float64) * 2.0 ** -64 - (want - np.floor(want))
    err = np.abs(err - np.rint(err))
    print("%s: m = %d, largest phase error %.3g turns" % (name, ometa[0, 0], err.max()))
    assert err.max() <= 2e-6


# ---------------------------------------------------------------- the inverse property
INV = dict(n=8192, dt=1e-3, f=5.0, width=0.2, amp=10.0, orb=(3.0, 0.04, 0.0, 0.0, 0.7))
# the largest residual measured here, in units of the pulse amplitude summed
# over the four channels (the linear resampler's interpolation error, with the
# half-sample offset between a cell's centre (i + 1/2) dt and the resampler's i
# dt: f dt beta / 2 = 2e-4 turns)
INV_MEASURED = 1.54e-3
INV_BOUND = 2.0 * INV_MEASURED


def _inverse_residual(orb):
    n, dt, f = INV["n"], INV["dt"], INV["f"]
    freqs = band(4)
    base = dict(kind="pulsar", f=f, dm=0.0, amp=INV["amp"], width=INV["width"], phi0=0.1)
    with_orbit = dict(base, pb=INV["orb"][0], x=INV["orb"][1], e=INV["orb"][2],
                      omega=INV["orb"][3], t0=INV["orb"][4])
    zero = np.zeros((n, 4), dtype=np.float32)
    series = ioo.inject(zero, 0, [with_orbit], freqs, dt, B=1024).sum(axis=1, dtype=np.float32)
    plain = ioo.inject(zero, 0, [base], freqs, dt, B=1024).sum(axis=1, dtype=np.float32)
    assert np.array_equal(plain, io.inject(zero, 0, [base], freqs, dt, B=1024).sum(axis=1, dtype=np.float32))
    K = oo.spacing([orb], dt)
    pos = oo.interpolate(oo.knots(orb, n, K, dt), n, K)
    got = oo.resample(series, orb, dt, K, oo.LINEAR, 0.0)
    inside = (pos >= 0.0) & (pos <= n - 1.0)
    assert inside.sum() > n - 200
    peak = float(plain.max())
    return float(np.max(np.abs(got[inside] - plain[inside]))) / peak, \
        float(np.max(np.abs(series - plain))) / peak


def test_injected_then_demodulated_is_the_plain_pulsar():
    res, moved = _inverse_residual(INV["orb"])
    print("inverse property: residual %.3g of the peak (bound %.3g); the orbit moved the series "
          "by %.3g of the peak" % (res, INV_BOUND, moved))
    assert moved > 0.5          # f x = 0.2 turns of a 0.2-turn pulse
    assert res <= INV_BOUND
    # a wrong sign or a wrong t0 convention is an error of order the amplitude
    pb, x, e, om, t0 = INV["orb"]
    for wrong in ((pb, x, e, om, -t0), (pb, x, e, om + math.pi, t0), (pb, x, e, om, t0 + pb / 4)):
        assert _inverse_residual(wrong)[0] > 0.3, wrong


# ---------------------------------------------------------------- spec and truth
def test_spec_parsing_and_validation():
    freqs = band(8)
    ok = dict(kind="pulsar", f=200.0, dm=30.0, amp=2.0, pb=8.0, x=0.02)
    it = inj.Injector.from_spec([ok], freqs, 1e-3)
    s = it.signals[0]
    assert s.orbit == (8.0, 0.02, 0.0, 0.0, 0.0)
    tr = it.truth()[0]
    for key, want in (("pb", 8.0), ("x", 0.02), ("e", 0.0), ("omega", 0.0), ("t0", 0.0)):
        assert tr[key] == want and s.params()[key] == want
    assert abs(tr["beta"] - 0.02 * 2 * math.pi / 8.0) < 1e-15
    v = 0.02 * 2 * math.pi / 8.0   # max |dD/dt| of a circular orbit
    assert abs(tr["f_lo"] - 200.0 * (1 - v)) < 1e-6 and abs(tr["f_hi"] - 200.0 * (1 + v)) < 1e-6
    assert tr["f_lo"] >= 200.0 * (1 - v) and tr["f_hi"] <= 200.0 * (1 + v)  # (a chord, not the tangent)
    json.dumps(it.truth())
    full = inj.Injector.from_spec([dict(ok, e=0.3, omega=2.0, t0=-1.5)], freqs, 1e-3).signals[0]
    assert full.orbit == (8.0, 0.02, 0.3, 2.0, -1.5)
    for bad in (dict(ok, x=None), {k: v for k, v in ok.items() if k != "x"},
                {k: v for k, v in ok.items() if k != "pb"}):
        bad = {k: v for k, v in bad.items() if v is not None}
        with pytest.raises(ValueError, match="pb and x"):
            inj.Injector.from_spec([bad], freqs, 1e-3)
    with pytest.raises(ValueError, match="need an orbit"):
        inj.Injector.from_spec([dict(kind="pulsar", f=200.0, dm=30.0, amp=2.0, e=0.1)], freqs, 1e-3)
    with pytest.raises(ValueError, match="beta"):
        inj.Injector.from_spec([dict(ok, x=0.2)], freqs, 1e-3)      # beta = 0.157
    with pytest.raises(ValueError, match="e must be"):
        inj.Injector.from_spec([dict(ok, e=1.0)], freqs, 1e-3)
    with pytest.raises(ValueError, match=r"burst\): unknown field\(s\) pb, x"):
        inj.Injector.from_spec([dict(kind="burst", t=1.0, dm=30.0, amp=2.0, width=1e-3, pb=8.0,
                                     x=0.02)], freqs, 1e-3)
    # the strength as snr: the orbit does not enter matched_snr
    a = inj.Injector.from_spec([dict(kind="pulsar", f=200.0, dm=30.0, snr=20.0, pb=8.0, x=0.02)],
                               freqs, 1e-3, sigma_chan=4.0, n_samples=1 << 16)
    b = inj.Injector.from_spec([dict(kind="pulsar", f=200.0, dm=30.0, snr=20.0)], freqs, 1e-3,
                               sigma_chan=4.0, n_samples=1 << 16)
    assert a.signals[0].amp == b.signals[0].amp and a.truth()[0]["matched_snr"] == b.truth()[0]["matched_snr"]


def test_no_orbit_keys_is_todays_injector():
    freqs = band(8)
    spec = [dict(kind="pulsar", f=97.3, dm=35.0, amp=9.0, fd=3e-2, phi0=0.21),
            dict(kind="burst", t=0.01, dm=20.0, amp=30.0, width=1e-3)]
    it = inj.Injector.from_spec(spec, freqs, DT, nbins=64)
    assert not it.has_orbits()
    _, want = io.build([io.sig_dict(s) for s in it.signals], freqs, DT, 64)
    got = it.host_arrays()
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    # (the tables of the two derivations differ in the last place of float32)
    assert np.max(np.abs(got[3] - want[3])) <= 1e-6 * 30.0
    ophase, ometa, qtab = it.orbit_arrays()
    assert ophase.shape == (2, 8) and not ophase.any() and qtab.size == 0
    assert np.array_equal(ometa, [[-1, 0, 0], [-1, 0, 0]])
    tr = it.truth()[0]
    assert not any(k in tr for k in ("pb", "x", "e", "omega", "t0", "beta", "f_lo", "f_hi"))


# ---------------------------------------------------------------- matchers
FREQS, DMS, T = band(64), np.linspace(0, 100, 101), 64.0
TRUTH = [dict(kind="pulsar", f=200.0, dm=30.0, width=0.05, pb=8.0, x=0.02, e=0.0, omega=0.0, t0=1.0,
              beta=0.0157, f_lo=196.86, f_hi=203.14, matched_snr=40.0),
         dict(kind="pulsar", f=50.0, dm=70.0, width=0.05),
         dict(kind="burst", t=1.0, dm=5.0, width=1e-3)]


def _bin(rows):
    from pypulsar_amd.sideband import BINCAND_DTYPE
    out = np.zeros(len(rows), dtype=BINCAND_DTYPE)
    for i, (sigma, dm, lo, hi, porb, q) in enumerate(rows):
        out[i]["sigma"], out[i]["DM"], out[i]["freq_lo"], out[i]["freq_hi"] = sigma, dm, lo, hi
        out[i]["porb"], out[i]["q"], out[i]["L"] = porb, q, 256
    return out


def test_match_binaries():
    # the fundamental: the band meets [f_lo, f_hi], porb within 1.5 porb / q = 0.24
    rep = rec.match_binaries(TRUTH, _bin([(9.0, 30.0, 190.0, 198.0, 8.2, 51)]), T, DMS, FREQS, 1e-3)
    assert len(rep) == 1 and rep[0]["index"] == 0 and rep[0]["kind"] == "binary"
    r = rep[0]
    assert r["found"] and (r["h"], r["m"], r["porb_relation"]) == (1, 1, "pb")
    assert (r["sigma"], r["L"], r["q"]) == (9.0, 256, 51) and abs(r["porb_offset"] - 0.2) < 1e-12
    # pb / 2 at the second harmonic; the stronger of two matches is reported
    rep = rec.match_binaries(TRUTH, _bin([(9.0, 30.0, 190.0, 198.0, 8.2, 51),
                                          (12.0, 31.0, 398.0, 410.0, 4.05, 100)]), T, DMS, FREQS, 1e-3)
    r = rep[0]
    assert r["found"] and (r["h"], r["m"], r["porb_relation"]) == (2, 2, "pb/2") and r["sigma"] == 12.0
    assert rec.match_binaries(TRUTH, _bin([(9.0, 30.0, 190.0, 198.0, 16.3, 51)]), T, DMS, FREQS,
                              1e-3)[0]["porb_relation"] == "2*pb"
    # just outside each window: DM (2 steps), frequency band, porb (0.2412)
    for miss in ((9.0, 32.5, 190.0, 198.0, 8.2, 51), (9.0, 27.5, 190.0, 198.0, 8.2, 51),
                 (9.0, 30.0, 190.0, 196.8, 8.2, 51), (9.0, 30.0, 203.2, 210.0, 8.2, 51),
                 (9.0, 30.0, 190.0, 198.0, 8.25, 51), (9.0, 30.0, 190.0, 198.0, 7.77, 51)):
        r = rec.match_binaries(TRUTH, _bin([miss]), T, DMS, FREQS, 1e-3)[0]
        assert not r["found"] and r["sigma"] is None, miss
    # ... and just inside
    for hit in ((9.0, 32.0, 190.0, 198.0, 8.2, 51), (9.0, 30.0, 190.0, 196.9, 8.2, 51),
                (9.0, 30.0, 203.1, 210.0, 8.2, 51), (9.0, 30.0, 190.0, 198.0, 8.24, 51)):
        assert rec.match_binaries(TRUTH, _bin([hit]), T, DMS, FREQS, 1e-3)[0]["found"], hit
    assert rec.match_binaries(TRUTH, _bin([]), T, DMS, FREQS, 1e-3)[0]["found"] is False
    assert rec.match_binaries(TRUTH[1:], _bin([]), T, DMS, FREQS, 1e-3) == []


def _orb(rows):
    from pypulsar_amd.orbit import SIFTED_DTYPE
    out = np.zeros(len(rows), dtype=SIFTED_DTYPE)
    for i, (sigma, dm, freq, pb, x, t0) in enumerate(rows):
        for name, v in zip(("sigma", "DM", "freq", "pb", "x", "t0"), (sigma, dm, freq, pb, x, t0)):
            out[i][name] = v
    return out


def test_match_orbits():
    rep = rec.match_orbits(TRUTH, _orb([(15.0, 30.0, 200.01, 8.1, 0.019, 1.81 - 8.1)]), T, DMS,
                           FREQS, 1e-3)
    assert len(rep) == 1 and rep[0]["kind"] == "orbit"
    r = rep[0]
    assert r["found"] and r["harmonic"] == "f" and r["sigma"] == 15.0
    assert abs(r["freq_offset"] - 0.01) < 1e-9 and abs(r["pb_offset"] - 0.1) < 1e-12
    assert abs(r["x_offset"] + 0.001) < 1e-12
    assert abs(r["phase_offset"] - (1.81 / 8.1 - 1.0 / 8.0)) < 1e-12
    # the second harmonic of the demodulated pulsar, the stronger one wins
    r = rec.match_orbits(TRUTH, _orb([(15.0, 30.0, 200.01, 8.1, 0.019, 0.0),
                                      (18.0, 29.0, 400.03, 8.0, 0.02, 1.0)]), T, DMS, FREQS, 1e-3)[0]
    assert r["harmonic"] == "2*f" and r["sigma"] == 18.0 and r["phase_offset"] == 0.0
    # outside: frequency (1.5 / T = 0.0234; unwidened, although inside [f_lo, f_hi]) and DM
    for miss in ((15.0, 30.0, 200.03, 8.0, 0.02, 1.0), (15.0, 30.0, 201.0, 8.0, 0.02, 1.0),
                 (15.0, 32.5, 200.0, 8.0, 0.02, 1.0)):
        assert not rec.match_orbits(TRUTH, _orb([miss]), T, DMS, FREQS, 1e-3)[0]["found"], miss
    assert rec.match_orbits(TRUTH, _orb([]), T, DMS, FREQS, 1e-3)[0]["found"] is False


def test_match_pulsars_widens_for_an_orbit():
    from pypulsar_amd.periodicity import CAND_DTYPE
    cands = np.zeros(3, dtype=CAND_DTYPE)
    for i, (dm, f, s) in enumerate([(30.0, 203.15, 9.0), (30.0, 393.70, 8.0), (70.0, 50.03, 7.0)]):
        cands[i]["DM"], cands[i]["freq"], cands[i]["sigma"] = dm, f, s
    rep = rec.match_pulsars(TRUTH, cands, T, DMS, FREQS, 1e-3)
    # [f_lo - 1.5 / T, f_hi + 1.5 / T] = [196.837, 203.163]
    assert rep[0]["found"] and rep[0]["widened"] and rep[0]["harmonic"] == "f" and rep[0]["sigma"] == 9.0
    assert (rep[0]["f_lo"], rep[0]["f_hi"]) == (196.86, 203.14)
    # the plain pulsar keeps its window of 1.5 / T = 0.0234 Hz
    assert not rep[1]["found"] and "widened" not in rep[1]
    only2 = rec.match_pulsars(TRUTH, cands[1:], T, DMS, FREQS, 1e-3)[0]
    assert only2["found"] and only2["harmonic"] == "2*f"    # 2 f_lo - 3 / T = 393.673
    cands[0]["freq"] = 203.17
    assert rec.match_pulsars(TRUTH, cands[:1], T, DMS, FREQS, 1e-3)[0]["found"] is False


def test_write_report_keeps_its_layout(tmp_path):
    fn = str(tmp_path / "r.json")
    rec.write_report(fn, TRUTH, [dict(a=1)])
    assert sorted(json.load(open(fn))) == ["recovery", "truth"]
    rec.write_report(fn, TRUTH, [dict(a=1)], binaries=[dict(b=2)], orbits=[])
    got = json.load(open(fn))
    assert sorted(got) == ["binaries", "orbits", "recovery", "truth"] and got["binaries"] == [dict(b=2)]


# ---------------------------------------------------------------- the C ABI's refusals
def test_refusals_without_gpu():
    """Every refusal of pdd_inject_orbit comes before any device call: host
    buffers stand in for the device pointers and are never read."""
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()
    C, J, B = 8, 2, 64
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)

    def call(fn="pdd_inject_orbit", data=p, dtype=_lib.U8, n=16, C_=C, ld=C, t0=0, phase=p, tab=p,
             J_=J, B_=B, seed=0, vmax=255, ophase=p, meta=((7, 5, 0), (-1, 0, 0)), qtab=p,
             qlen=4096):
        m = None if meta is None else np.ascontiguousarray(np.array(meta, dtype=np.int64))
        args = [data, dtype, n, C_, ld, t0, phase, p, p, tab, J_, B_, seed, vmax]
        if fn == "pdd_inject_orbit":
            args += [ophase, None if m is None else m.ctypes.data, qtab, qlen]
        return getattr(h, fn)(*(args + [None]))

    cases = [dict(data=None), dict(dtype=_lib.U16), dict(n=-1), dict(C_=0), dict(ld=C - 1),
             dict(t0=-1), dict(t0=1 << 52), dict(J_=65), dict(J_=-1), dict(B_=32), dict(B_=96),
             dict(seed=-1), dict(seed=1 << 32), dict(vmax=0), dict(vmax=256), dict(tab=None),
             dict(phase=None)]
    for kw in cases:
        for fn in ("pdd_inject", "pdd_inject_orbit"):
            assert call(fn, **kw) == -1, (fn, kw)
            assert h.pdd_last_error().startswith(fn.encode() + b":"), (fn, kw, h.pdd_last_error())
    own = [dict(meta=None), dict(ophase=None), dict(qtab=None), dict(qtab=p + 4),
           dict(meta=((5, 5, 0), (-1, 0, 0))), dict(meta=((23, 5, 0), (-1, 0, 0))),
           dict(meta=((7, 5, 0), (-2, 0, 0))), dict(meta=((7, 5, 0), (64, 0, 0))),
           dict(meta=((7, 5, -8), (-1, 0, 0))), dict(meta=((7, 5, 4), (-1, 0, 0))),
           dict(meta=((7, 5, 8 * (4096 - 128)), (-1, 0, 0))), dict(qlen=128), dict(qlen=-1)]
    for kw in own:
        assert call(**kw) == -1, kw
        assert h.pdd_last_error().startswith(b"pdd_inject_orbit:"), (kw, h.pdd_last_error())
    # nothing to do is no error, with or without orbits; a table that just fits is accepted
    assert call(n=0) == 0 and call(J_=0, meta=None) == 0
    assert call(n=0, meta=((7, 5, 8 * (4096 - 129)), (-1, 0, 0))) == 0
    assert call(n=0, qlen=129) == 0
