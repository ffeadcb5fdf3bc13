"""pulsar_search.py --sideband on a small 8-bit filterbank that carries the
recovery signal of tests/sideband_cases.py at DM 0: ``<base>.bincands`` and
``<base>_bincands.npz``, the strongest sifted candidate; and without
--sideband the tool's bytes are what they were."""
import os

import numpy as np
import pytest

import sideband_cases as sc
from conftest import band

pytestmark = pytest.mark.gpu
C, SIGMA_CH = 16, 16.0
DMS = np.linspace(0.0, 5.0, 2)
ARGS = ["--lodm", "0", "--hidm", "5", "--numdms", "2", "--nfft", str(sc.N), "--numharm", "16"]


def channel_data(seed=3):
    """[C, N] uint8: noise of SIGMA_CH counts a channel around 128 and, in
    every channel (DM 0), the recovery signal with the amplitude that gives
    the channel sum the plane case's ratio of amplitude to noise: C a /
    (sqrt(C) SIGMA_CH) = AMP."""
    rng = np.random.default_rng(seed)
    a = sc.AMP * SIGMA_CH / np.sqrt(C)
    t = np.arange(sc.N) * sc.DT
    x = sc.BETA / (2.0 * np.pi * sc.F0)
    sig = a * np.cos(2.0 * np.pi * sc.F0 * (t - x * np.sin(2.0 * np.pi * t / sc.PORB + 0.7)))
    data = rng.normal(128.0, SIGMA_CH, (C, sc.N)) + sig[None, :]
    return np.clip(np.round(data), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def binary_fil(tmp_path_factory):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    freqs = band(C)
    x = channel_data()
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(C, 8, sc.DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path_factory.mktemp("sideband") / "compact.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    return fn


def test_cli_sideband(gpu, binary_fil, tmp_path, capsys):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import read_accelcands
    from pypulsar_amd.sideband import BINCAND_DTYPE, CAND_DTYPE, read_bincands, sift
    out = str(tmp_path / "compact.accelcands")
    assert pulsar_search.main(ARGS + ["--sideband", "-o", out, binary_fil]) == 0
    printed = capsys.readouterr().out
    assert "sideband candidates" in printed
    bfn, npz = str(tmp_path / "compact.bincands"), str(tmp_path / "compact_bincands.npz")
    assert os.path.exists(bfn) and os.path.exists(npz) and os.path.exists(out)
    back = read_bincands(bfn)
    assert len(back) >= 1 and np.all(np.diff(back["sigma"]) <= 0)
    z = np.load(npz)
    assert sorted(z.files) == sorted(BINCAND_DTYPE.names)
    for name in BINCAND_DTYPE.names:
        assert np.array_equal(z[name], back[name]), name    # the file holds what was written
    top = back[0]
    plain = [c for c in read_accelcands(out) if abs(c.dm) < 1e-9]
    print("plain search at DM 0: %s; sideband top: sigma %.2f DM %.1f porb %.5f s (true %.5f) "
          "L %d q %d H %d, f in [%.3f, %.3f) Hz (f0 %.3f)"
          % (["%.2f" % c.sigma for c in plain], top["sigma"], top["DM"], top["porb"], sc.PORB,
             top["L"], top["q"], top["numharm"], top["freq_lo"], top["freq_hi"], sc.F0))
    assert top["DM"] == 0.0
    assert abs(top["porb"] - sc.PORB) <= sc.N * sc.DT / (2.0 * top["L"])
    assert top["freq_lo"] <= sc.F0 < top["freq_hi"]
    # search_file hands the raw records back after the plain search's own result
    res = pulsar_search.search_file(binary_fil, DMS, nfft=sc.N, sideband={})
    assert len(res) == 3 and res[2].dtype == CAND_DTYPE
    s = sift(res[2])
    assert len(s) == len(back)
    for name in BINCAND_DTYPE.names:
        assert np.array_equal(s[name], back[name]), name
    plain_res = pulsar_search.search_file(binary_fil, DMS, nfft=sc.N)
    assert len(plain_res) == 2 and np.array_equal(plain_res[0], res[0])


def test_cli_options(gpu, binary_fil, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.sideband import read_bincands
    out = str(tmp_path / "opt.accelcands")
    assert pulsar_search.main(ARGS + ["--sideband", "--sb-minfft", "128", "--sb-maxfft", "512",
                                      "--sb-numharm", "2", "--sb-shift", "1", "--sb-clip", "12",
                                      "--sb-sigma", "5", "--zmax", "4", "-o", out, binary_fil]) == 0
    back = read_bincands(str(tmp_path / "opt.bincands"))
    assert len(back) >= 1
    assert set(back["L"]) <= {128, 256, 512} and set(back["numharm"]) <= {1, 2}
    assert back["sigma"].min() >= 5.0
    with pytest.raises(SystemExit):
        pulsar_search.main(ARGS + ["--sideband", "--sb-minfft", "48", binary_fil])


def test_cli_without_sideband_keeps_its_bytes(gpu, binary_fil, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import sift, write_accelcands
    out = str(tmp_path / "plain.accelcands")
    assert pulsar_search.main(ARGS + ["--sigma", "4", "-o", out, binary_fil]) == 0
    cands, _ = pulsar_search.search_file(binary_fil, DMS, sigma=4.0, nfft=sc.N,
                                         harms=(1, 2, 4, 8, 16))
    assert len(cands) > 0
    want = str(tmp_path / "want.accelcands")
    write_accelcands(sift(cands), want, basename="compact")
    assert open(out, "rb").read() == open(want, "rb").read()
    assert not os.path.exists(str(tmp_path / "plain.bincands"))
    assert not os.path.exists(str(tmp_path / "plain_bincands.npz"))
