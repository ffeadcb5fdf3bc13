"""Injection from the command line: bin/inject writes the oracle's bytes;
frb_search / pulsar_search --inject --recovery give the candidates of the
pre-injected file; an injected burst, a sub-LSB pulsar and an accelerated
pulsar come back where and as strong as the model says."""
import json

import numpy as np
import pytest

import inject_oracle as io
from conftest import u8_data

pytestmark = pytest.mark.gpu
DT = 64e-6
# found / matched S/N of the burst of test_burst_recovered_at_its_strength,
# from the CPU chain for that seed (oracle injection -> co-add by 2 ->
# spectra_oracle.sweep_plane -> search_oracle.search): sigma 12.079 for a
# matched S/N of 15 (the noise-free chain gives 0.935)
BURST_RATIO = 0.805


def _fil(tmp_path, x_tc, nbits=8, name="in.fil"):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C = x_tc.shape[1]
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, nbits, DT, 1550.0 + foff / 2, foff)
    fn = str(tmp_path / name)
    fbm.write_filterbank(fn, params, hdr, x_tc)
    return fn


def _spec(tmp_path, spec, name="spec.json"):
    fn = str(tmp_path / name)
    with open(fn, "w") as f:
        json.dump(spec, f)
    return fn


BURST_SPEC = [dict(kind="burst", t=9000 * DT, dm=40.0, snr=15.0, width=16 * DT)]


@pytest.fixture(scope="module")
def burst_data():
    return u8_data(128, 3 * 8192, 31).T.copy()  # [N, C], the noise of test_frb_search_cli


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_inject_cli_writes_the_oracle_bytes(gpu, tmp_path, burst_data, dtype):
    from pypulsar_amd.bin import inject as cli
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.inject import Injector, robust_sigma
    x = burst_data[:20000].astype(dtype)
    fn = _fil(tmp_path, x, 8 * x.dtype.itemsize)
    spec = BURST_SPEC + [dict(kind="pulsar", f=21.7, dm=15.0, amp=2.5, fd=0.1, phi0=0.4)]
    out = str(tmp_path / "out.fil")
    assert cli.main(["--spec", _spec(tmp_path, dict(signals=spec, seed=3, nbins=512)), "-o", out,
                     "--block", "7000", fn]) == 0
    fb = fbm.filterbank(out)
    got = fb.read_all_samples().reshape(-1, 128)
    assert got.dtype == dtype and fb.header_params == fbm.filterbank(fn).header_params
    it = Injector.from_spec(spec, fb.freqs, DT, sigma_chan=robust_sigma(x), n_samples=len(x),
                            nbins=512, seed=3)
    want = io.inject_arrays(x, 0, *it.host_arrays(), B=512, seed=3)
    assert not np.array_equal(want, x)
    assert np.array_equal(got, want)
    truth = json.load(open(str(tmp_path / "out_truth.json")))
    assert [t["kind"] for t in truth] == ["burst", "pulsar"]
    assert abs(truth[0]["matched_snr"] - 15.0) < 1e-9 and truth[0]["sample"] == 9000.0


def test_inject_cli_refusals(gpu, tmp_path, burst_data, capsys):
    from pypulsar_amd.bin import frb_search, inject as cli, pulsar_search
    from pypulsar_amd.formats import sigproc
    spec = _spec(tmp_path, BURST_SPEC)
    x = burst_data[:4096]
    # packed and 16-bit input are refused
    from pypulsar_amd.formats import filterbank as fbm
    params, hdr = sigproc.make_header(128, 2, DT, 1550.0 - 300.0 / 256, -300.0 / 128)
    fn2 = str(tmp_path / "two.fil")
    fbm.write_filterbank(fn2, params, hdr, sigproc.pack_bits(x & 3, 2))
    fn16 = _fil(tmp_path, x.astype(np.uint16), 16, "sixteen.fil")
    for bad in (fn2, fn16):
        with pytest.raises(SystemExit):
            cli.main(["--spec", spec, "-o", str(tmp_path / "o.fil"), bad])
        assert "not supported" in capsys.readouterr().err
    # so is --inject on 16-bit data, and snr against a noise level of 0, before the search starts
    flat = _fil(tmp_path, np.full((4096, 128), 2, dtype=np.uint8), name="flat.fil")
    for main in (frb_search.main, pulsar_search.main):
        with pytest.raises(SystemExit):
            main(["--inject", spec, fn16])
        assert "16-bit" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            main(["--inject", spec, flat])
        assert "noise level" in capsys.readouterr().err
    fn = _fil(tmp_path, x)
    with pytest.raises(SystemExit):
        frb_search.main(["--inject", spec, "--cutouts", "1", fn])
    assert "pypulsar_amd.bin.inject" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pulsar_search.main(["--inject", spec, "--fold", "1", "--fold-subbands", "4", fn])
    assert "pypulsar_amd.bin.inject" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        frb_search.main(["--recovery", fn])


def test_burst_recovered_at_its_strength(gpu, tmp_path, burst_data):
    """A burst of matched S/N 15 and FWHM 8 downsampled samples: found at its
    DM (+- 2 steps) and time, at BURST_RATIO +- 4 / S of its matched S/N; the
    on-the-fly run gives the candidates of the pre-injected file."""
    from pypulsar_amd.bin import frb_search as fs, inject as cli
    fn = _fil(tmp_path, burst_data)
    spec = _spec(tmp_path, BURST_SPEC)
    args = ["--lodm", "0", "--hidm", "80", "--numdms", "81", "--downsamp", "2", "--block", "8192",
            "--no-zero-dm", "-t", "6"]
    out = str(tmp_path / "fly.singlepulse")
    assert fs.main(args + ["--inject", spec, "--recovery", "-o", out, fn]) == 0
    pre = str(tmp_path / "pre.fil")
    assert cli.main(["--spec", spec, "-o", pre, fn]) == 0
    out2 = str(tmp_path / "pre.singlepulse")
    assert fs.main(args + ["-o", out2, pre]) == 0
    assert open(out).read() == open(out2).read()
    rep = json.load(open(str(tmp_path / "fly_recovery.json")))
    assert len(rep["truth"]) == 1 and len(rep["recovery"]) == 1
    r, S = rep["recovery"][0], rep["truth"][0]["matched_snr"]
    assert abs(S - 15.0) < 1e-9
    print("burst: sigma %.3f, matched %.3f, ratio %.3f (oracle chain %.3f)"
          % (r["sigma"], S, r["ratio"], BURST_RATIO))
    assert r["found"] and abs(r["dm_offset"]) <= 2.0 and abs(r["time_offset"]) <= 16 * DT
    assert abs(r["ratio"] - BURST_RATIO) <= 4.0 / S
    # the clean file has nothing there
    out3 = str(tmp_path / "clean.singlepulse")
    assert fs.main(args + ["-o", out3, fn]) == 0
    from pypulsar_amd.search import read_singlepulse
    c = read_singlepulse(out3)
    assert not np.any((np.abs(c["DM"] - 40.0) <= 2.0) & (np.abs(c["Time"] - 9000 * DT) <= 16 * DT)
                      & (c["Sigma"] >= 8.0))


def test_psrfits_input(gpu, tmp_path, burst_data):
    """A PSRFITS file and its SIGPROC twin: bin/inject writes the same samples
    under the same band and sample time from both (the noise level of an
    ``snr`` entry taken from the decoded rows), and frb_search --inject on the
    PSRFITS file (the decoder stream) gives the candidates of that copy."""
    from pypulsar_amd.bin import frb_search as fs, inject as cli
    from pypulsar_amd.formats import filterbank as fbm, psrfits
    x = burst_data
    freqs = 1550.0 - 300.0 / 128 * (np.arange(128) + 0.5)  # the band of _fil
    fits = str(tmp_path / "obs.fits")
    psrfits.write_search_psrfits(fits, x.reshape(12, 2048, 128), freqs, DT, 8)
    spec = _spec(tmp_path, BURST_SPEC)
    a, b = str(tmp_path / "from_fits.fil"), str(tmp_path / "from_fil.fil")
    assert cli.main(["--spec", spec, "-o", a, "--block", "7000", fits]) == 0
    assert cli.main(["--spec", spec, "-o", b, _fil(tmp_path, x)]) == 0
    fa, fb = fbm.filterbank(a), fbm.filterbank(b)
    assert fa.nbits == 8 and fa.tsamp == fb.tsamp and np.array_equal(fa.freqs, fb.freqs)
    got = fa.read_all_samples()
    assert not np.array_equal(got.reshape(x.shape), x)
    assert np.array_equal(got, fb.read_all_samples())
    assert open(a[:-4] + "_truth.json").read() == open(b[:-4] + "_truth.json").read()
    args = ["--lodm", "0", "--hidm", "80", "--numdms", "81", "--downsamp", "2", "--block", "8192",
            "--no-zero-dm", "-t", "6"]
    out, out2 = str(tmp_path / "fly.singlepulse"), str(tmp_path / "pre.singlepulse")
    assert fs.main(args + ["--inject", spec, "-o", out, fits]) == 0
    assert fs.main(args + ["-o", out2, a]) == 0
    text = open(out).read()
    assert text == open(out2).read() and len(text.splitlines()) > 1


def _pulsar_file(tmp_path):
    C, N = 64, 1 << 16
    rng = np.random.default_rng(77)
    x = np.clip(np.round(rng.normal(128.0, 4.0, (N, C))), 0, 255).astype(np.uint8)
    return _fil(tmp_path, x, name="psr.fil"), N


# on a bin of the 2^16-point transform: the search's scalloping is not the subject
PSR_F = 156.0 / ((1 << 16) * DT)
PSR_ARGS = ["--lodm", "20", "--hidm", "40", "--numdms", "21"]


def _check_fold_phase(base, dm, phi0):
    """The profile of ``<base>.npz`` / ``.bestprof`` peaks at the bin that the
    injected ``phi0`` implies, +- 1.  A pulse is where ``phi0 + f t`` is whole,
    t being the arrival at the highest channel, which is the time axis of the
    plane (it starts at sample 0); the fold gives sample i, at its centre, the
    phase ``f_fold (i + 1/2) dt``, so a pulse falls at ``-phi0 + (f_fold - f)
    t`` turns, and the written profile is aligned on the middle of the folded
    span T (fold.trial_shift is 0 there): ``-phi0 + (f_fold - f) T / 2``.
    ``f_fold`` comes back from the refined frequency and the best trial
    (fold.trial_to_ffdot).  Folded at a neighbouring DM trial, channel c comes
    ``(dm - dm_fold) lag_c`` later (lag_c: its lag per unit DM), the sum of
    the channels by the mean of that."""
    from pypulsar_amd.delays import delay_from_DM
    from pypulsar_amd.fold import read_bestprof
    z = np.load(base + ".npz")
    hdr, prof = read_bestprof(base + ".bestprof")
    nbins = len(prof)
    T = hdr["Data Folded"] * DT
    ia, ib = (int(v) for v in z["trial"])
    f_fold = float(z["f"]) + (ia - 4.0 * ib) / (nbins * T)
    freqs = 1550.0 - 300.0 / 64 * (np.arange(64) + 0.5)
    lag = np.mean(delay_from_DM(1.0, freqs) - delay_from_DM(1.0, freqs.max()))
    turns = -phi0 + (f_fold - PSR_F) * T / 2 + PSR_F * (dm - float(z["dm"])) * lag
    want = (turns % 1.0) * nbins
    got = int(np.argmax(prof))
    print("fold: DM %.2f, f_fold - f = %.3g / T, trial (%d, %d); peak in bin %d, phi0 implies %.2f"
          % (float(z["dm"]), (f_fold - PSR_F) * T, ia, ib, got, want))
    assert np.array_equal(prof, np.where(z["counts"] > 0, z["profile"] / z["counts"], 0.0))
    assert abs((got - want + nbins / 2) % nbins - nbins / 2) <= 1.0


def test_sub_lsb_pulsar_recovered(gpu, tmp_path):
    """A pulsar of about 0.3 LSB per channel sample (matched S/N 30) is the
    strongest candidate, within one Fourier bin and two DM steps; the same
    search without --inject has no candidate there; the on-the-fly run gives
    the candidates of the pre-injected file; --fold 1 puts the profile's peak
    at the bin phi0 implies."""
    from pypulsar_amd.bin import inject as cli, pulsar_search as ps
    from pypulsar_amd.periodicity import read_accelcands
    fn, N = _pulsar_file(tmp_path)
    T = N * DT
    spec = _spec(tmp_path, [dict(kind="pulsar", f=PSR_F, dm=30.0, snr=30.0, width=0.05, phi0=0.25)])
    out = str(tmp_path / "fly.accelcands")
    assert ps.main(PSR_ARGS + ["--inject", spec, "--recovery", "--fold", "1", "-o", out, fn]) == 0
    rep = json.load(open(str(tmp_path / "fly_recovery.json")))
    amp = rep["truth"][0]["amp"]
    print("pulsar amp %.3f LSB per channel sample" % amp)
    assert 0.2 <= amp <= 0.45
    r = rep["recovery"][0]
    top = read_accelcands(out)[0]
    print("top: %r; recovery: %s at %.4f Hz, sigma %.2f" % (top, r["harmonic"], r["cand_freq"] or 0,
                                                           r["sigma"] or 0))
    assert r["found"] and abs(r["dm_offset"]) <= 2.0
    assert abs(top.freq - PSR_F) <= 1.0 / T and abs(top.dm - 30.0) <= 2.0
    assert r["sigma"] <= top.sigma + 0.01
    _check_fold_phase(str(tmp_path / "fly_cand1"), 30.0, 0.25)
    pre = str(tmp_path / "pre.fil")
    assert cli.main(["--spec", spec, "-o", pre, fn]) == 0
    out2 = str(tmp_path / "pre.accelcands")
    assert ps.main(PSR_ARGS + ["-o", out2, pre]) == 0
    # (the entries are named after the input file)
    assert open(out).read().replace("psr_DM", "pre_DM") == open(out2).read()
    out3 = str(tmp_path / "clean.accelcands")
    assert ps.main(PSR_ARGS + ["-o", out3, fn]) == 0
    assert not [c for c in read_accelcands(out3)
                if abs(c.freq - PSR_F) <= 1.5 / T and abs(c.dm - 30.0) <= 2.0]


def test_accelerated_pulsar_recovered(gpu, tmp_path):
    from pypulsar_amd.bin import pulsar_search as ps
    from pypulsar_amd.periodicity import read_accelcands
    fn, N = _pulsar_file(tmp_path)
    T = N * DT
    z = 8.0
    fd = z / T ** 2
    spec = _spec(tmp_path, [dict(kind="pulsar", f=PSR_F, fd=fd, dm=30.0, snr=40.0, width=0.05)])
    out = str(tmp_path / "acc.accelcands")
    assert ps.main(PSR_ARGS + ["--zmax", "16", "--dz", "2", "--numharm", "8", "--inject", spec,
                               "--recovery", "-o", out, fn]) == 0
    top = read_accelcands(out)[0]
    print("accelerated: %r z = %.2f" % (top, top.z))
    # (the candidate's frequency is the mid-observation one)
    assert abs(top.freq - (PSR_F + fd * T / 2)) <= 1.5 / T and abs(top.dm - 30.0) <= 2.0
    assert abs(top.z - z) <= 2.0
    r = json.load(open(str(tmp_path / "acc_recovery.json")))["recovery"][0]
    assert r["found"]
