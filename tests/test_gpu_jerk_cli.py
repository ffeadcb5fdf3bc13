"""pulsar_search.py --wmax on a small synthetic filterbank that carries a
pulsar with a jerk: the ``.accelcands`` names, ``<base>_jerkcands.npz``, the
strongest sifted candidate; and --zmax alone keeps its bytes."""
import os

import numpy as np
import pytest

from conftest import band
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = 64e-6
DMS = np.linspace(0.0, 15.0, 16)
# the fundamental's drift and jerk over NS samples (its 8th harmonic: z = 8, w = 40); samples a pulse
Z, W, PERIOD, NS = 1.0, 5.0, 32, 3980
ARGS = ["--lodm", "0", "--hidm", "15", "--numdms", "16", "--nfft", "4096", "--numharm", "8"]


@pytest.fixture(scope="module")
def jerk_fil(tmp_path_factory):
    """An 8-bit filterbank of 4200 samples with a pulse train at DM 8 whose
    frequency is 1 / 32 samples at the middle of the first NS samples, with a
    mean drift of Z and a jerk of W bins of 1 / NS over them."""
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C, N = 64, 4200
    freqs = band(C)
    rng = np.random.default_rng(34)
    x = rng.normal(128.0, 16.0, (C, N))
    delays = orc.sweep_table([8.0], freqs, DT)[0]
    t = np.arange(N, dtype=np.float64)
    v = t / NS
    ph = t / PERIOD + 0.5 * Z * (v * v - v) + W * (v ** 3 / 6.0 - v * v / 4.0 + v / 12.0)
    on = np.flatnonzero((ph % 1.0) < 2.0 / PERIOD)
    for c in range(C):
        tt = on + int(delays[c])
        x[c, tt[tt < N]] += 12.0
    x = np.clip(np.round(x), 0, 255).astype(np.uint8)
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path_factory.mktemp("jerk") / "tight.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    return fn


def test_cli_wmax(gpu, jerk_fil, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import read_accelcands
    out = str(tmp_path / "tight.accelcands")
    assert pulsar_search.main(ARGS + ["--zmax", "8", "--wmax", "40", "-o", out, jerk_fil]) == 0
    back = read_accelcands(out)
    assert len(back) >= 1
    top = back[0]
    assert top.accelfile == "tight_DM%.2f_ACCEL_8_JERK_40" % top.dm
    assert all(c.accelfile.endswith("_ACCEL_8_JERK_40") for c in back)
    npz = str(tmp_path / "tight_jerkcands.npz")
    assert os.path.exists(npz)
    jc = np.load(npz)
    assert sorted(jc.files) == sorted(["DM", "r", "period", "numharm", "sigma", "z", "w", "fd",
                                       "fdd", "accel", "jerk"])
    assert all(len(jc[k]) == len(back) for k in jc.files)
    assert np.all(np.diff(jc["sigma"]) <= 0)  # the order of the .accelcands file
    H = int(jc["numharm"][0])
    print("cli top: %r z = %.2f w = %.2f numharm = %d sigma = %.1f" % (top, jc["z"][0], jc["w"][0],
                                                                     H, jc["sigma"][0]))
    # the strongest sifted candidate is the injected one
    assert H == top.numharm and abs(jc["DM"][0] - top.dm) <= 0.005
    assert abs(top.dm - 8.0) <= 1.0
    assert abs(top.period - PERIOD * DT) <= 0.005 * PERIOD * DT
    assert abs(jc["z"][0] - top.z) <= 0.005
    # (the plane is a little shorter than NS samples: z within one bin)
    assert abs(jc["z"][0] - Z) <= 1.0
    assert abs(jc["w"][0] - W) <= 20.0 / H
    # the derived columns
    T = None
    cands, dt, plane = pulsar_search.search_file(jerk_fil, DMS, nfft=4096, harms=(1, 2, 4, 8),
                                                 zmax=8, wmax=40, return_plane=True)
    assert "w" in cands.dtype.names and "wbins" in cands.dtype.names
    T = plane.shape[1] * dt
    assert np.allclose(jc["fd"], jc["z"] / T ** 2) and np.allclose(jc["fdd"], jc["w"] / T ** 3)
    assert np.allclose(jc["accel"], jc["fd"] * 299792458.0 * jc["period"])
    assert np.allclose(jc["jerk"], jc["fdd"] * 299792458.0 * jc["period"])


def test_cli_wmax_implies_the_search_and_folds(gpu, jerk_fil, tmp_path):
    """--wmax without --zmax searches w alone (nz = 1), and --fold starts at the
    first sample's frequency and derivative."""
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import SiftedCandidate, read_accelcands
    out = str(tmp_path / "w.accelcands")
    assert pulsar_search.main(ARGS + ["--wmax", "40", "--fold", "1", "-o", out, jerk_fil]) == 0
    back = read_accelcands(out)
    assert len(back) >= 1 and back[0].accelfile.endswith("_ACCEL_0_JERK_40")
    assert all(c.z == 0.0 for c in back)
    assert os.path.exists(str(tmp_path / "w_jerkcands.npz"))
    assert os.path.exists(str(tmp_path / "w_cand1.bestprof"))
    c = SiftedCandidate(8.0, 128.0, 2.0e-3, 8, 100.0, 20.0, row=8, z=2.0, fd=0.5, w=10.0, fdd=0.25)
    s, = pulsar_search.first_sample_starts([c], 4.0)
    assert s is not c and c.fd == 0.5 and c.period == 2.0e-3
    assert s.fd == 0.5 - 0.5 * 0.25 * 4.0 == 0.0
    assert abs(s.freq - (500.0 - 0.5 * 0.5 * 4.0 + 0.25 * 16.0 / 12.0)) <= 1e-10
    c.fdd = 0.125
    s, = pulsar_search.first_sample_starts([c], 4.0)
    assert s.fd == 0.25
    assert abs((s.freq - 0.5 * s.fd * 4.0) - (500.0 - 1.0 + 0.125 * 16.0 / 12.0)) <= 1e-10


def test_cli_zmax_alone_keeps_its_bytes(gpu, jerk_fil, tmp_path):
    """Without --wmax the tool takes the acceleration search's path: the bytes
    of search_file + sift + write_accelcands without their jerk arguments, and
    no jerkcands file."""
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import sift, write_accelcands
    out = str(tmp_path / "plain.accelcands")
    assert pulsar_search.main(ARGS + ["--zmax", "8", "-o", out, jerk_fil]) == 0
    cands, _ = pulsar_search.search_file(jerk_fil, DMS, nfft=4096, harms=(1, 2, 4, 8), zmax=8)
    assert "z" in cands.dtype.names and "w" not in cands.dtype.names and len(cands) > 0
    want = str(tmp_path / "want.accelcands")
    write_accelcands(sift(cands), want, basename="tight", zmax=8)
    assert open(out, "rb").read() == open(want, "rb").read()
    assert b"_ACCEL_8:" in open(out, "rb").read() and b"JERK" not in open(out, "rb").read()
    assert not os.path.exists(str(tmp_path / "plain_jerkcands.npz"))
