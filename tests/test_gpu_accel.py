"""The acceleration search on the GPU (pdd_acc_correlate, pdd_acc_search,
pypulsar_amd.accel.AccelSearch) against the NumPy restatement
(tests/accel_oracle.py), and end to end through sifting, the .accelcands file,
the fold and the CLI.  FFT lengths used in this file: 4096 and 5000 only."""
import numpy as np
import pytest

import accel_oracle as ao
from conftest import band
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = 64e-6
ZMAX = 24
CASES = ((3000, 4096), (4096, 4096), (4700, 5000))
IBL = 40  # whitening blocks of the recovery cases (see tests/test_accel_oracle.py)


def _rows(n, nfft):
    """Three raw rows: the two chirps of the recovery cases and noise."""
    x = ao.chirp_rows(n, nfft, 350.3, 4.0, seed=1, rows=3)
    t = np.arange(n, dtype=np.float64)
    v = t / n
    for h in range(1, 5):
        x[1] += (300.0 * np.cos(2 * np.pi * (h * 305.75 * t / nfft - 2.5 * h * (v * v - v))
                                + 0.3 * h)).astype(np.float32)
    return np.round(x)


@pytest.fixture(scope="module")
def planes(gpu):
    """Per case: the GPU's whitened spectrum (a strided view), its powers, the
    plane of pdd_acc_correlate and the float64 oracle plane of the same
    complex64 spectrum -- computed once, shared and left unchanged."""
    import torch
    from pypulsar_amd.accel import AccelSearch
    out = {}
    acc = AccelSearch(sigma_threshold=3.5, zmax=ZMAX, initialbuflen=IBL)
    for n, nfft in CASES:
        xd = torch.from_numpy(_rows(n, nfft)).cuda()
        powers, white = acc.ps.normalise(acc.ps.spectrum(xd, nfft), want_spectrum=True)
        nn = nfft // 2
        big = torch.zeros((3, nn + 37), dtype=torch.complex64, device="cuda")
        big[:] = 7.0e5  # (a correlation that reads past a row's nn bins shows)
        big[:, :nn] = white
        view = big[:, :nn]
        assert view.stride(0) == nn + 37
        P = acc.correlate(view, n)
        torch.cuda.synchronize()
        t, hw, M = ao.taps(n, nfft, ZMAX)
        wh = white.cpu().numpy()
        ref = np.stack([ao.plane(wh[d], t, M) for d in range(3)])
        out[(n, nfft)] = dict(view=view, powers=powers.cpu().numpy(), P=P, Ph=P.cpu().numpy(),
                              ref=ref, hw=hw, M=M)
    return acc, out


@pytest.mark.parametrize("n,nfft", CASES)
def test_correlate_vs_oracle(planes, n, nfft):
    acc, out = planes
    c = out[(n, nfft)]
    nn = nfft // 2
    assert c["Ph"].shape == (3, 25, 2 * nn) and c["Ph"].dtype == np.float32
    eta = n / float(nfft)
    assert c["hw"].min() == int(np.ceil(16 / eta)) and c["hw"].max() == int(np.ceil(28 / eta))
    err = np.max(np.abs(c["Ph"].astype(np.float64) - c["ref"])) / np.max(c["ref"])
    print("correlate n=%d nfft=%d: max |P - P_ref| / max P_ref = %.3g (M = %d)"
          % (n, nfft, err, c["M"]))
    assert err <= 2e-5
    # deterministic: the same bits on a second launch
    again = acc.correlate(c["view"], n).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.int32), c["Ph"].view(np.int32))
    if n == nfft:
        # z = 0 at whole bins without padding: the whitened power itself
        p = c["powers"]
        e0 = np.max(np.abs(c["Ph"][:, 12, 0::2] - p)) / np.max(p)
        print("correlate n=nfft=%d: z = 0 whole bins against normalise: %.3g" % (n, e0))
        assert e0 <= 1e-5


def test_correlate_refuses_bad_arguments(planes):
    import ctypes
    import torch
    from pypulsar_amd import _lib
    acc, out = planes
    c = out[(3000, 4096)]
    taps, hw, M = acc._bank(3000, 4096, c["view"].device)
    P = torch.empty((3, 25, 4096), dtype=torch.float32, device="cuda")
    bad = hw.copy()
    bad[3] = M + 1
    for h, nz in ((bad, 25), (hw, 24)):
        with pytest.raises(_lib.PddError):
            _lib.call("pdd_acc_correlate", _lib.ptr(torch.view_as_real(c["view"])), 3, 2048,
                      c["view"].stride(0), _lib.ptr(taps), h.ctypes.data_as(ctypes.c_void_p), nz,
                      M, _lib.ptr(P), _lib.stream_ptr())
    cands = torch.empty((4, 6), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    harms = np.asarray([1, 17], dtype=np.int32)
    thr = np.asarray([1.0, 2.0], dtype=np.float32)
    with pytest.raises(_lib.PddError):
        _lib.call("pdd_acc_search", _lib.ptr(P), 3, 25, 4096,
                  harms.ctypes.data_as(ctypes.c_void_p), 2, thr.ctypes.data_as(ctypes.c_void_p),
                  1, _lib.ptr(cands), 4, _lib.ptr(count), _lib.stream_ptr())


def _record_set(c, k):
    c = c[:k].cpu().numpy()
    assert np.all(c[:, 5] == 0)
    return {tuple(int(v) for v in r[:5]) for r in c}


@pytest.mark.parametrize("harms", [(1, 2, 4, 8), (1, 3)])
@pytest.mark.parametrize("n,nfft", [(3000, 4096), (4700, 5000)])
def test_search_vs_oracle_own_plane(planes, n, nfft, harms):
    from pypulsar_amd.accel import AccelSearch
    _, out = planes
    c = out[(n, nfft)]
    acc = AccelSearch(sigma_threshold=3.5, zmax=ZMAX, harms=harms)
    dt = 2.5 / nfft  # flo = 1 Hz: rlo = 3
    assert acc.rlo(nfft, dt) == 3
    cd, k = acc.raw(c["P"], nfft, dt)
    got = _record_set(cd, int(k.item()))
    assert len(got) == int(k.item())  # no duplicates
    want = ao.candidates(c["Ph"], harms, acc.thr, 3)
    assert len(want) > 10
    assert got == want
    recs = acc.collect(cd, k, [1.0, 2.0, 3.0], n, nfft, dt)
    assert len(recs) == len(got) and np.all(recs["sigma"] >= 3.5 - 1e-6)
    assert np.allclose(recs["freq"], recs["r"] / (nfft * dt))
    assert np.allclose(recs["zbins"], recs["z"] * nfft / n)
    assert np.allclose(recs["fd"], recs["z"] / (n * dt) ** 2)


@pytest.mark.parametrize("harms", [(1, 2, 4, 8), (1, 3)])
def test_search_synthetic_ties_and_edges(gpu, harms):
    """A [2][13][1000] plane of small integers (ties everywhere) with maxima
    planted on every edge and corner and across the boundaries of the
    254-position tiles."""
    import torch
    from pypulsar_amd.accel import AccelSearch
    rng = np.random.default_rng(17)
    P = rng.integers(0, 5, (2, 13, 1000)).astype(np.float32)
    for d, j, i in ((0, 0, 999), (0, 12, 999), (0, 0, 500), (0, 12, 501), (1, 6, 999),
                    (1, 0, 2 * harms[-1]), (1, 12, 2 * harms[-1]), (0, 5, 2), (0, 5, 255),
                    (0, 6, 256), (1, 7, 509), (1, 7, 510), (1, 3, 763), (1, 4, 764)):
        P[d, j, i] = 40.0
    acc = AccelSearch(sigma_threshold=2.0, zmax=12, harms=harms)  # (H = 1: S >= 3.8)
    assert acc.nz == 13
    cd, k = acc.raw(torch.from_numpy(P).cuda(), 1000, 1.0 / 1000)  # rlo = 1
    got = _record_set(cd, int(k.item()))
    want = ao.candidates(P, harms, acc.thr, 1)
    assert len(want) > 100
    assert got == want
    assert (0, 999, -6, 1, int(np.float32(40.0).view(np.int32))) in got


def test_search_overflow(planes):
    from pypulsar_amd.accel import AccelSearch
    _, out = planes
    acc = AccelSearch(sigma_threshold=3.0, zmax=ZMAX, max_cands=2)
    cd, k = acc.raw(out[(3000, 4096)]["P"], 4096, 2.5 / 4096)
    assert int(k.item()) > 2
    with pytest.raises(RuntimeError):
        acc.collect(cd, k, [1.0, 2.0, 3.0], 3000, 4096, 2.5 / 4096)


# ---- end to end: plane -> AccelSearch -> sift -> .accelcands -> fold ----

def test_end_to_end(gpu, tmp_path):
    import torch
    from pypulsar_amd.accel import ACCEL_CAND_DTYPE, AccelSearch
    from pypulsar_amd.fold import Folder
    from pypulsar_amd.periodicity import (PeriodicitySearch, read_accelcands, sift,
                                          write_accelcands)
    n, nfft, dt = 3000, 4096, 1e-3
    x = ao.chirp_rows(n, nfft, 350.3, 4.0, seed=2, signal=False, rows=5)
    x[3] = ao.chirp_rows(n, nfft, 350.3, 4.0, seed=1)[0]
    plane = torch.from_numpy(x).cuda()
    dms = np.arange(5) * 2.0
    acc = AccelSearch(zmax=ZMAX, initialbuflen=IBL)
    cands = acc(plane, dms, dt, nfft=nfft)
    assert cands.dtype == ACCEL_CAND_DTYPE and len(cands) > 0
    # (row batches change nothing)
    np.testing.assert_array_equal(cands, acc(plane, dms, dt, row_batch=2, nfft=nfft))
    s = sift(cands)
    top = s[0]
    print("top: %r z = %.2f fd = %.4f; %d records, %d sifted" % (top, top.z, top.fd, len(cands),
                                                                  len(s)))
    assert top.row == 3 and top.dm == 6.0
    assert abs(top.r - 350.3) <= 0.25 and top.z == 4.0
    T = n * dt
    assert abs(top.fd - 4.0 / (T * T)) <= 1e-12
    # the z = 0 search of the same plane sees the smeared harmonics at best
    ps = PeriodicitySearch(6.0, (1, 2, 4, 8), initialbuflen=IBL)
    flat = ps(plane, dms, dt, nfft=nfft)
    best0 = float(flat["sigma"].max()) if len(flat) else 0.0
    print("sigma: accelerated %.2f, z = 0 search %.2f" % (top.sigma, best0))
    assert top.sigma > best0
    # the file carries z and round-trips
    fn = str(tmp_path / "acc.accelcands")
    write_accelcands(s, fn, basename="acc", zmax=ZMAX)
    back = read_accelcands(fn)
    assert len(back) == len(s)
    b = back[0]
    assert b.accelfile == "acc_DM6.00_ACCEL_%d" % ZMAX and b.candnum == 1
    assert b.z == 4.0 and abs(b.r - top.r) <= 0.005 and b.numharm == top.numharm
    assert [abs(q.z - p.z) <= 0.005 for p, q in zip(s, back)] == [True] * len(s)
    # the fold starts at the candidate's fd and stays within one step of it
    folder = Folder()
    fc = folder(plane, dms, dt, [top], dm_halfwidth=0)[0]
    step = 8.0 / (folder.nbins * folder.span(n, dt) ** 2)
    print("fold: fd = %.4f Hz/s (z / T^2 = %.4f, step %.4f), trial %r, chi2 %.1f"
          % (fc.fd, 4.0 / (T * T), step, fc.trial, fc.chi2))
    assert abs(fc.fd - 4.0 / (T * T)) <= step * (1 + 1e-9)
    assert abs(fc.f_fold - (top.freq - 0.5 * top.fd * T)) <= 1e-12
    assert fc.sigma > 6.0


# ---- the CLI ----

CLI_DMS = np.linspace(0.0, 15.0, 16)
CLI_Z, CLI_PERIOD, CLI_NS = 6.0, 32, 3980  # drift over CLI_NS samples; samples a pulse


@pytest.fixture(scope="module")
def accel_fil(tmp_path_factory):
    """An 8-bit filterbank of 4200 samples with a pulse train at DM 8 whose
    frequency, 1 / 32 samples at the middle of the first CLI_NS samples,
    drifts CLI_Z bins of 1 / CLI_NS over them."""
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C, N = 64, 4200
    freqs = band(C)
    rng = np.random.default_rng(33)
    x = rng.normal(128.0, 16.0, (C, N))
    delays = orc.sweep_table([8.0], freqs, DT)[0]
    t = np.arange(N, dtype=np.float64)
    fd = CLI_Z / float(CLI_NS) ** 2
    ph = (1.0 / CLI_PERIOD - 0.5 * fd * CLI_NS) * t + 0.5 * fd * t * t
    on = np.flatnonzero((ph % 1.0) < 2.0 / CLI_PERIOD)
    for c in range(C):
        tt = on + int(delays[c])
        x[c, tt[tt < N]] += 12.0
    x = np.clip(np.round(x), 0, 255).astype(np.uint8)
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(C, 8, DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path_factory.mktemp("accel") / "bin.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    return fn


def test_cli_zmax(gpu, accel_fil, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import read_accelcands
    out = str(tmp_path / "bin.accelcands")
    assert pulsar_search.main(["--lodm", "0", "--hidm", "15", "--numdms", "16", "--nfft", "4096",
                               "--zmax", str(ZMAX), "--numharm", "32", "-o", out,
                               accel_fil]) == 0
    back = read_accelcands(out)
    assert len(back) >= 1
    top = back[0]
    print("cli top: %r z = %.2f" % (top, top.z))
    assert top.accelfile == "bin_DM%.2f_ACCEL_%d" % (top.dm, ZMAX)
    assert abs(top.dm - 8.0) <= 1.0
    # (the plane is a little shorter than CLI_NS samples: z within one bin)
    assert abs(top.z - CLI_Z) <= 1.0
    assert abs(top.period - CLI_PERIOD * DT) <= 0.005 * CLI_PERIOD * DT
    assert top.numharm <= 16 and len(top.hits) >= 2


def test_cli_without_zmax_keeps_its_bytes(gpu, accel_fil, tmp_path):
    """Without --zmax the tool takes the periodicity search's path: the bytes
    of search_file + sift + write_accelcands with their defaults."""
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.periodicity import sift, write_accelcands
    out = str(tmp_path / "plain.accelcands")
    assert pulsar_search.main(["--lodm", "0", "--hidm", "15", "--numdms", "16", "--nfft", "4096",
                               "-o", out, accel_fil]) == 0
    cands, _ = pulsar_search.search_file(accel_fil, CLI_DMS, nfft=4096)
    assert "z" not in cands.dtype.names and len(cands) > 0
    want = str(tmp_path / "want.accelcands")
    write_accelcands(sift(cands), want, basename="bin")
    assert open(out, "rb").read() == open(want, "rb").read()
    assert b"_ACCEL_0:" in open(out, "rb").read()
