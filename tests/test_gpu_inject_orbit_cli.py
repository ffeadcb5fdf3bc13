"""A pulsar in a Keplerian orbit injected from the command line and graded: the
two calibrated points of DESIGN.md §6p for the binary searches, and the
injected copy that bin/inject writes.  64 channels, 2^16 samples of 1 ms,
noise of sigma 4 (seed 77), the pulsar on a bin of the 2^16-point transform at
DM 30 with pb = 8 s, x = 0.02 lt-s (beta = 0.0157, 2 pi f x = 25 rad: about 25
sidebands a side, 8.2 bins apart) and matched S/N 40 (0.275 LSB per channel
sample)."""
import json

import numpy as np
import pytest

import inject_orbit_oracle as ioo

pytestmark = pytest.mark.gpu
DT = 1e-3
C, N = 64, 1 << 16
F = 13107.0 / (N * DT)
ORBIT = (8.0, 0.02, 0.0, 0.0, 1.3)
SNR = 40.0
SPEC = [dict(kind="pulsar", f=F, dm=30.0, snr=SNR, width=0.3, phi0=0.25, pb=ORBIT[0], x=ORBIT[1],
             t0=ORBIT[4])]
# The CPU chain for this seed (oracle injection -> spectra_oracle.sweep_plane
# at DM 30 -> orbit_oracle.resample, linear, with the injected orbit -> the
# period oracle on the row zero padded to 2^16, stages 1..16): the top
# candidate is bin 13107 (f) with 2 harmonics at sigma 42.665, 1.067 of the
# matched S/N; the row as it is has nothing above 4 sigma within 1.5 / T of f
# (its strongest line, a sideband at 197.25 Hz, has 6.17 sigma).
POINT1_SIGMA = 42.665
# ... and the sideband oracle on that row as it is (threshold 6): sigma 25.0
# at L = 512, q = 125 (porb = 8.000 s), 4 harmonics; nothing in the clean row.
PSR_ARGS = ["--lodm", "20", "--hidm", "40", "--numdms", "21", "--numharm", "1"]


def _freqs():
    foff = -300.0 / C
    return 1550.0 + foff / 2 + foff * np.arange(C)


def _noise():
    rng = np.random.default_rng(77)
    return np.clip(np.round(rng.normal(128.0, 4.0, (N, C))), 0, 255).astype(np.uint8)


def _fil(tmp_path, x_tc, name):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, 8 * x_tc.dtype.itemsize, DT, 1550.0 + foff / 2, foff)
    fn = str(tmp_path / name)
    fbm.write_filterbank(fn, params, hdr, x_tc)
    return fn


def _spec(tmp_path, spec, name="spec.json"):
    fn = str(tmp_path / name)
    with open(fn, "w") as f:
        json.dump(spec, f)
    return fn


def test_demodulated_with_the_true_orbit(gpu):
    """Point 1: device injection, the device sweep at the injected DM,
    Resampler("linear") with the injected orbit, the periodicity search of
    that row: the top candidate is at f within 1.5 / T at the CPU chain's
    sigma +- 4 (4 / S of the matched S/N); without demodulation the row has no
    candidate of 6 sigma within 1.5 / T of f."""
    import torch
    from pypulsar_amd.inject import Injector, robust_sigma
    from pypulsar_amd.orbit import Resampler
    from pypulsar_amd.periodicity import PeriodicitySearch
    from pypulsar_amd.sweep import DMSweep
    x = _noise()
    freqs = _freqs()
    it = Injector.from_spec(SPEC, freqs, DT, sigma_chan=robust_sigma(x), n_samples=N)
    S = it.truth()[0]["matched_snr"]
    assert abs(S - SNR) < 1e-9 and it.has_orbits()
    xd = torch.from_numpy(x).cuda()
    it.apply(xd, 0)
    sw = DMSweep([30.0], freqs, DT, dtype="u8")
    plane = sw(xd.t().contiguous()).float()
    sw.close()
    n = plane.shape[1]
    T = n * DT
    assert n == N - 27
    ps = PeriodicitySearch(4.0, (1, 2, 4, 8, 16), flo=1.0)
    dem = Resampler("linear")(plane[0], [ORBIT], DT)
    cands = ps(dem, [30.0], DT, nfft=N)
    top = cands[np.argmax(cands["sigma"])]
    plain = ps(plane, [30.0], DT, nfft=N)
    near = plain[np.abs(plain["freq"] - F) <= 1.5 / T]
    print("point 1: device sigma %.3f at %.5f Hz (%d harmonics), oracle chain %.3f; ratios to the "
          "matched S/N %.4f and %.4f; undemodulated: top %.2f sigma, near f: %s"
          % (top["sigma"], top["freq"], top["numharm"], POINT1_SIGMA, top["sigma"] / S,
             POINT1_SIGMA / S, plain["sigma"].max() if len(plain) else 0.0,
             near["sigma"].tolist()))
    assert abs(top["freq"] - F) <= 1.5 / T
    assert abs(top["sigma"] / S - POINT1_SIGMA / S) <= 4.0 / S
    assert not np.any(near["sigma"] >= 6.0)


def test_binary_found_by_the_whole_cli(gpu, tmp_path):
    """Point 2: pulsar_search --inject --sideband --orbit-follow 1 --recovery
    reports the binary found at porb = pb (m = 1) and the orbit found at f;
    the clean file gives neither."""
    from pypulsar_amd import orbit, recovery, sideband
    from pypulsar_amd.bin import pulsar_search as ps
    fn = _fil(tmp_path, _noise(), "psr.fil")
    spec = _spec(tmp_path, SPEC)
    args = PSR_ARGS + ["--sideband", "--orbit-follow", "1", "--orbit-mismatch", "0.15",
                       "--orbit-max-templates", "65536"]
    out = str(tmp_path / "fly.accelcands")
    assert ps.main(args + ["--inject", spec, "--recovery", "-o", out, fn]) == 0
    rep = json.load(open(str(tmp_path / "fly_recovery.json")))
    assert sorted(rep) == ["binaries", "orbits", "recovery", "truth"]
    tr = rep["truth"][0]
    assert tr["pb"] == 8.0 and tr["x"] == 0.02 and abs(tr["matched_snr"] - SNR) < 1e-9
    b, o, r = rep["binaries"][0], rep["orbits"][0], rep["recovery"][0]
    print("point 2: binary %s" % json.dumps(b, sort_keys=True))
    print("point 2: orbit %s" % json.dumps(o, sort_keys=True))
    print("point 2: pulsar %s" % json.dumps(r, sort_keys=True))
    assert len(rep["binaries"]) == len(rep["orbits"]) == 1
    assert b["found"] and b["m"] == 1 and b["porb_relation"] == "pb" and abs(b["cand_dm"] - 30.0) <= 2.0
    # the sideband oracle has 25 sigma on this row: 4 to spare and more
    assert b["sigma"] >= 6.0 + 4.0
    assert o["found"] and o["harmonic"] == "f" and abs(o["cand_dm"] - 30.0) <= 2.0
    assert r["widened"]
    # the clean file: the same tool, graded against the same truth
    out2 = str(tmp_path / "clean.accelcands")
    assert ps.main(args + ["-o", out2, fn]) == 0
    T = N * DT
    dms = np.linspace(20.0, 40.0, 21)
    bc = sideband.read_bincands(str(tmp_path / "clean.bincands"))
    oc = orbit.read_orbcands(str(tmp_path / "clean.orbcands"))
    assert not recovery.match_binaries(rep["truth"], bc, T, dms, _freqs(), DT)[0]["found"]
    assert not recovery.match_orbits(rep["truth"], oc, T, dms, _freqs(), DT)[0]["found"]


def test_inject_cli_and_frb_search_take_an_orbit(gpu, tmp_path):
    """bin/inject writes the oracle's bytes of a pulsar with an orbit and its
    truth carries the orbit; frb_search --inject of the same spec gives the
    candidates of that copy."""
    from pypulsar_amd.bin import frb_search as fs, inject as cli
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.inject import Injector
    x = _noise()[:20000]
    fn = _fil(tmp_path, x, "in.fil")
    spec = [dict(kind="pulsar", f=F, dm=30.0, amp=6.0, phi0=0.25, pb=8.0, x=0.02, e=0.3, omega=2.0,
                 t0=1.3),
            dict(kind="burst", t=7.0, dm=25.0, amp=12.0, width=4e-3)]
    sp = _spec(tmp_path, dict(signals=spec, seed=3))
    out = str(tmp_path / "out.fil")
    assert cli.main(["--spec", sp, "-o", out, "--block", "7000", fn]) == 0
    fb = fbm.filterbank(out)
    got = fb.read_all_samples().reshape(-1, C)
    it = Injector.from_spec(spec, fb.freqs, DT, seed=3)
    want = ioo.inject_arrays(x, 0, *it.host_arrays(), *it.orbit_arrays(), B=it.B, seed=3)
    assert not np.array_equal(want, x) and np.array_equal(got, want)
    truth = json.load(open(str(tmp_path / "out_truth.json")))
    assert [truth[0][k] for k in ("pb", "x", "e", "omega", "t0")] == [8.0, 0.02, 0.3, 2.0, 1.3]
    assert truth[0]["f_lo"] < F < truth[0]["f_hi"] and "pb" not in truth[1]
    args = ["--lodm", "0", "--hidm", "50", "--numdms", "26", "--block", "8192", "--no-zero-dm",
            "-t", "7"]
    a, b = str(tmp_path / "fly.singlepulse"), str(tmp_path / "pre.singlepulse")
    assert fs.main(args + ["--inject", sp, "-o", a, fn]) == 0
    assert fs.main(args + ["-o", b, out]) == 0
    text = open(a).read()
    assert text == open(b).read() and len(text.splitlines()) > 1
