"""pulsar_search.py --sideband --orbit-follow on the small 8-bit filterbank of
tests/test_gpu_sideband_cli.py (the recovery signal at DM 0; restated in
tests/orbit_cases.py): ``<base>.orbcands`` and ``<base>_orbcands.npz``, the
strongest record against the true spin frequency and orbit, the fold of the
demodulated row; and without --orbit-follow the tool's bytes are what they
were."""
import os

import numpy as np
import pytest

import orbit_cases as oc
import sideband_cases as sc
from conftest import band

pytestmark = pytest.mark.gpu
ARGS = ["--lodm", "0", "--hidm", "5", "--numdms", "2", "--nfft", str(sc.N), "--numharm", "16"]
T = sc.N * sc.DT


@pytest.fixture(scope="module")
def binary_fil(tmp_path_factory):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    freqs = band(oc.C)
    x = oc.channel_data()
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(oc.C, 8, sc.DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path_factory.mktemp("orbit") / "compact.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    return fn


@pytest.fixture(scope="module")
def followed(gpu, binary_fil, tmp_path_factory):
    """(directory of the outputs, what the tool printed) of one run with
    --sideband --orbit-follow 1 --fold 1."""
    import contextlib
    import io
    from pypulsar_amd.bin import pulsar_search
    d = tmp_path_factory.mktemp("followed")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        status = pulsar_search.main(ARGS + ["--sideband", "--orbit-follow", "1", "--fold", "1",
                                            "-o", str(d / "compact.accelcands"), binary_fil])
    assert status == 0
    return d, text.getvalue()


def test_orbit_files(followed):
    from pypulsar_amd.orbit import ORBCANDS_COLUMNS, read_orbcands
    d, printed = followed
    assert "orbit follow-up 1" in printed and "orbit candidates" in printed
    back = read_orbcands(str(d / "compact.orbcands"))
    assert len(back) >= 1 and np.all(np.diff(back["sigma"]) <= 0)
    z = np.load(str(d / "compact_orbcands.npz"))
    assert sorted(z.files) == sorted(ORBCANDS_COLUMNS)
    for name in ORBCANDS_COLUMNS:
        assert np.array_equal(z[name], back[name]), name    # the file holds what was written


def test_top_record(followed):
    """The strongest record: the spin frequency to a bin, the orbital period
    within the sideband candidate's half-bin step, x within two bank steps,
    and more significant than anything the plain search saw at DM 0.  (On the
    unquantised seed-3 series the host finds 8.3 sigma at bin 2500 with x one
    step from the truth.)"""
    from pypulsar_amd.orbit import read_orbcands
    from pypulsar_amd.periodicity import read_accelcands
    from pypulsar_amd.sideband import read_bincands
    d, printed = followed
    top = read_orbcands(str(d / "compact.orbcands"))[0]
    side = read_bincands(str(d / "compact.bincands"))[0]
    plain = [c.sigma for c in read_accelcands(str(d / "compact.accelcands")) if abs(c.dm) < 1e-9]
    f_top = min(side["freq_hi"], 0.5 / sc.DT)   # one stage reaches the band below Nyquist
    dx = 2.0 * oc.MISMATCH / f_top
    print(printed)
    print("plain search at DM 0: %s; orbit top: sigma %.2f f %.4f Hz (true %.4f) pb %.5f s (true "
          "%.5f) x %.6f (true %.6f, dx %.6f) of %d templates"
          % (["%.2f" % v for v in plain], top["sigma"], top["freq"], sc.F0, top["pb"], sc.PORB,
             top["x"], oc.X_TRUE, dx, top["ntemplates"]))
    assert top["DM"] == 0.0 and top["e"] == 0.0 and top["omega"] == 0.0
    assert abs(top["freq"] - sc.F0) <= 1.0 / T
    assert abs(top["pb"] - sc.PORB) <= side["porb"] / side["q"]
    assert abs(top["x"] - oc.X_TRUE) <= 2.0 * dx
    assert top["sigma"] > 6.0 and all(top["sigma"] > v for v in plain)
    assert side["freq_lo"] <= top["freq"] <= side["freq_hi"]


def test_demodulated_fold(followed):
    d, printed = followed
    assert "orbcand 1:" in printed
    assert os.path.exists(str(d / "compact_orbcand1.bestprof"))
    z = np.load(str(d / "compact_orbcand1.npz"))
    assert abs(float(z["f"]) - sc.F0) <= 1.0 / T and float(z["dm"]) == 0.0


def test_without_orbit_follow_nothing_changes(gpu, followed, binary_fil, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    d, _ = followed
    out = str(tmp_path / "compact.accelcands")
    assert pulsar_search.main(ARGS + ["--sideband", "--fold", "1", "-o", out, binary_fil]) == 0
    for name in ("compact.accelcands", "compact.bincands"):
        assert open(str(tmp_path / name), "rb").read() == open(str(d / name), "rb").read(), name
    assert sorted(os.listdir(str(tmp_path))) == sorted(
        n for n in os.listdir(str(d)) if "orbcand" not in n)


def test_large_bank_is_skipped(gpu, binary_fil, tmp_path, capsys):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.orbit import read_orbcands
    out = str(tmp_path / "small.accelcands")
    assert pulsar_search.main(ARGS + ["--sideband", "--orbit-follow", "1", "--orbit-max-templates",
                                      "100", "-o", out, binary_fil]) == 0
    printed = capsys.readouterr().out
    assert "skipped" in printed and "exceed max_templates=100" in printed
    assert len(read_orbcands(str(tmp_path / "small.orbcands"))) == 0
    with pytest.raises(SystemExit):
        pulsar_search.main(ARGS + ["--orbit-follow", "1", binary_fil])
