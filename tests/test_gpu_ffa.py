"""Fast-folding search on the GPU (pypulsar_amd/ffa.py, pdd_ffa_* kernels)
against the NumPy restatement tests/ffa_oracle.py: the butterfly bit for bit,
the preparation and the score to the project's float bar, the candidate rule
as a set, and a dispersed slow pulsar from the filterbank to the fold."""
import os

import numpy as np
import pytest

import ffa_oracle as fo
from conftest import band, rel_err
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu


def _int_rows(seed, D, n):
    """Integer-valued rows centred on 0: sums of 4096 rows stay below 2^24."""
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(0.0, 1024.0, (D, n))).astype(np.float32)


def _strided(x, ld):
    import torch
    big = torch.full((x.shape[0], ld), 7.0e5, dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = torch.from_numpy(np.array(x)).cuda()
    return big[:, :x.shape[1]]


def _search(**kw):
    from pypulsar_amd.ffa import FFASearch
    args = dict(period_min=0.02, period_max=0.06, bins_min=16, bins_max=40)
    args.update(kw)
    return FFASearch(**args)


# ---- transform ----

# (n, p0): M = 135 with zero rows up to Mp = 256; M = Mp with p0 a multiple of
# 32; Mp = 4096 in two passes; M = Mp = 2 at a long profile; the shortest profile
SHAPES = [(5003, 37), (4096, 64), (40001, 19), (2000, 1000), (4099, 8)]


@pytest.mark.parametrize("n,p0", SHAPES)
def test_transform_integer_rows(gpu, n, p0):
    fs = _search()
    x = _int_rows(n + p0, 3, n)
    view = _strided(x, n + 13)
    assert view.stride(0) != n
    got = fs.transform(view, p0).cpu().numpy()
    M, K, kpass, npass = fs.plan_info(n, p0)
    assert M == n // p0 and (1 << K) == fo.mp_of(M) and got.shape == (3, 1 << K, p0)
    want = np.stack([fo.transform(x[d], p0) for d in range(3)])
    assert np.max(np.abs(want)) < 2 ** 24
    np.testing.assert_array_equal(got, want)
    again = fs.transform(view, p0).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32))


def test_plan_info_split(gpu):
    fs = _search()
    M, K, kpass, npass = fs.plan_info(40001, 19)
    assert (M, K) == (2105, 12) and npass == 2 and kpass < K   # K2 = K - kpass > 0
    M, K, kpass, npass = fs.plan_info(5003, 37)
    assert (M, K) == (135, 8) and npass == 1 and kpass == K     # K2 == 0
    # two passes take 500 bins up to Mp = 1024 ...
    assert fs.plan_info(500 * (1 << 10), 500)[3] == 2
    # ... and longer profiles or series a third, through the second workspace buffer
    assert fs.plan_info(1000 * (1 << 10), 1000)[3] == 3


def test_transform_three_passes(gpu):
    # p0 = 1000: 16 rows fit in LDS, so Mp = 512 takes three passes of three
    # stages through both workspace buffers
    fs = _search()
    n, p0 = 300 * 1000 + 17, 1000
    assert fs.plan_info(n, p0) == (300, 9, 3, 3)
    x = _int_rows(9, 1, n)
    got = fs.transform(_strided(x, n + 3), p0).cpu().numpy()
    np.testing.assert_array_equal(got[0], fo.transform(x[0], p0))


@pytest.mark.parametrize("n,p0", [(5003, 37), (40001, 19)])
def test_transform_float_rows(gpu, n, p0):
    # the same adds in the same order, no contraction: equal bits
    fs = _search()
    x = np.random.default_rng(n).normal(0.0, 1.0, (2, n)).astype(np.float32)
    got = fs.transform(_strided(x, n + 5), p0).cpu().numpy()
    want = np.stack([fo.transform(x[d], p0) for d in range(2)])
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


# ---- prep ----

@pytest.mark.parametrize("f,L", [(3, 400), (3, 5000), (1, 1000), (7, 100)])
def test_prep(gpu, f, L):
    fs = _search()
    n = 5003
    x = _int_rows(f * 100 + 7, 3, n) + np.float32(4096.0)
    x[1] += np.round(np.linspace(0.0, 3000.0, n)).astype(np.float32)   # a drifting baseline
    x[2] = 5.0                                                           # a constant row
    n_ds = n // f
    nchunk = max(1, n_ds // L)
    assert (nchunk == 1) == (L == 5000) and n_ds * f <= n
    yp, sig = fs.prep(_strided(x, n + 9), f, L=L)
    yp, sig = yp.cpu().numpy(), sig.cpu().numpy()
    want_y, want_s = fo.prep(x, f, L)
    assert yp.shape == want_y.shape == (3, n_ds) and yp.dtype == np.float32
    assert rel_err(yp, want_y) <= 1e-5
    assert rel_err(sig, want_s) <= 1e-5
    assert sig[2] == 0.0 and not np.any(yp[2])
    # integer rows: the downsampled sums are exact -- a chunk of one sample
    # short of the series leaves nothing but the mean to remove
    y0, _ = fs.prep(_strided(x[:1], n + 9), f, L=n_ds)
    y = fo.downsample(x[:1], f)
    np.testing.assert_array_equal(
        y0.cpu().numpy(), (y.astype(np.float64) - np.mean(y.astype(np.float64))).astype(np.float32))


# ---- periodogram ----

PG_N, PG_DT, PG_DETREND = 20000, 1e-3, 2.0


@pytest.fixture(scope="module")
def pg_case():
    """Three rows (noise, noise + a pulse train, constant) and the oracle's
    periodogram of the plan (1, 20, 40), (2, 20, 30): built once."""
    rng = np.random.default_rng(4)
    x = rng.normal(100.0, 10.0, (3, PG_N)).astype(np.float32)
    t = np.arange(PG_N)
    x[1, (t % 27.31) < 2.0] += 8.0
    x[2] = 7.0
    plan = fo.ffa_plan(PG_N, PG_DT, 0.02, 0.06, 16, 40)
    assert plan == [(1, 20, 40), (2, 20, 30)]
    # (within the first step n // p0 crosses 512: Mp = 1024 up to p0 = 38, 512 at 39)
    assert fo.mp_of(PG_N // 38) == 1024 and fo.mp_of(PG_N // 39) == 512
    snr, wid, margin = fo.periodogram(x, PG_DT, plan, detrend=PG_DETREND, bins_max=40)
    for a in (x, snr, wid, margin):
        a.setflags(write=False)
    return x, plan, snr, wid, margin


def test_periodogram(gpu, pg_case):
    x, plan, want, want_w, margin = pg_case
    fs = _search(detrend=PG_DETREND)
    assert fs.plan(PG_N, PG_DT) == plan
    snr, widx, table = fs.periodogram(_strided(x, PG_N + 11), PG_DT)
    got, got_w = snr.cpu().numpy(), widx.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and got_w.dtype == np.uint8
    for a, b in zip(table, fo.trial_table(PG_N, PG_DT, plan)):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(got))
    print("periodogram rel_err %.3g" % rel_err(got, want))
    assert rel_err(got, want) <= 1e-5
    # the constant row: sigma == 0, an all-zero periodogram
    assert not np.any(got[2]) and not np.any(got_w[2])
    # the pulse train at 27.31 ms is the strongest trial of its row
    k = int(np.argmax(got[1]))
    assert abs(table[0][k] - 0.02731) < 2e-5 and got[1, k] > 20.0
    # width index: equal wherever the oracle's choice is clear
    clear = margin > 1e-4
    print("width index compared on %.2f%% of the entries" % (100.0 * clear.mean()))
    assert clear.mean() >= 0.99
    np.testing.assert_array_equal(got_w[clear], want_w[clear])

    # two row batches, and two problem batches per row: the same bits
    slot = 4 * 1024 * 38                       # bytes of the first step's largest problem
    for bound, what in ((2 * 20 * slot, "rows"), (10 * slot, "problems")):
        s2, w2, _ = fs.periodogram(_strided(x, PG_N + 11), PG_DT, workspace_bytes=bound)
        np.testing.assert_array_equal(s2.cpu().numpy().view(np.int32), got.view(np.int32), what)
        np.testing.assert_array_equal(w2.cpu().numpy(), got_w, what)


# ---- candidates ----

def _record_set(c, k):
    return {(int(a), int(b)) for a, b, _, _ in c[:k].cpu().numpy()}


def test_candidates(gpu, pg_case):
    import torch
    x = pg_case[0]
    fs = _search(detrend=PG_DETREND, snr_threshold=3.0)
    snr, widx, table = fs.periodogram(torch.from_numpy(np.array(x)).cuda(), PG_DT)
    c, k = fs.raw(snr, widx)
    n = int(k.item())
    got = _record_set(c, n)
    want = fo.candidates(snr.cpu().numpy(), 3.0)
    assert len(got) == n and len(want) > 50
    assert got == want
    recs = fs.collect(c, k, [1.0, 2.0, 3.0], table, PG_N, PG_DT)
    assert len(recs) == n and recs.dtype.names[:8] == ("DM", "row", "r", "freq", "period",
                                                        "numharm", "power", "sigma")
    assert recs["r"].dtype == np.float64 and np.all(np.diff(recs["row"]) >= 0)
    np.testing.assert_allclose(recs["r"], PG_N * PG_DT / recs["period"])
    assert np.all(recs["numharm"] == 1) and np.all(recs["sigma"] >= 3.0)
    np.testing.assert_array_equal(recs["power"].astype(np.float64), recs["sigma"])
    np.testing.assert_allclose(recs["duty"], recs["width"] / recs["nbins"])
    top = recs[np.argmax(recs["sigma"])]
    assert top["row"] == 1 and abs(top["period"] - 0.02731) < 2e-5 and top["ds"] == 1

    # a plateau of equal neighbours (its first entry only) and a peak at each
    # end of a row, across the 254-trial tiles of the kernel
    s = np.random.default_rng(8).normal(0.0, 1.0, (2, 700)).astype(np.float32)
    s[0, 0], s[0, -1], s[1, 0], s[1, -1] = 9.0, 9.5, 2.0, 9.0
    s[0, 100:104] = 7.0
    s[1, 252:256] = 6.0          # a plateau across a tile boundary
    s[1, 507:509] = 5.0
    sd = torch.from_numpy(s).cuda()
    wd = torch.zeros((2, 700), dtype=torch.uint8, device="cuda")
    c, k = fs.raw(sd, wd)
    got = _record_set(c, int(k.item()))
    assert got == fo.candidates(s, 3.0)
    assert {(0, 0), (0, 699), (1, 699), (0, 100), (1, 252), (1, 507)} <= got
    assert not {(1, 0), (0, 101), (1, 253), (1, 508)} & got

    # overflow of max_cands raises
    small = _search(snr_threshold=3.0, max_cands=2)
    c, k = small.raw(sd, wd)
    assert int(k.item()) > 2
    with pytest.raises(RuntimeError):
        small.collect(c, k, [1.0, 2.0], (np.zeros(700),) * 5, 700, 1.0)


def test_empty_plane(gpu):
    import torch
    from pypulsar_amd.ffa import FFA_CAND_DTYPE
    fs = _search()
    out = fs(torch.empty((0, PG_N), dtype=torch.float32, device="cuda"), [], PG_DT)
    assert len(out) == 0 and out.dtype == FFA_CAND_DTYPE
    snr, widx, table = fs.periodogram(torch.empty((0, PG_N), dtype=torch.float32, device="cuda"),
                                      PG_DT)
    assert snr.shape == (0, len(table[0])) and widx.shape == snr.shape


# ---- end to end: filterbank -> sweep -> FFA -> sift -> fold, and the CLI ----

E2E_DT = 2.5e-4
E2E_DMS = np.linspace(52.5, 67.5, 16)     # 1 pc/cc steps around the injected DM 60
E2E_PERIOD, E2E_WIDTH = 400.37, 6          # samples: a duty cycle of 1.5 %
E2E_ARGS = dict(period_min=0.08, period_max=0.13, bins_min=250, bins_max=500)


@pytest.fixture(scope="module")
def slow_pulsar():
    C, N = 64, 1 << 16
    freqs = band(C)
    rng = np.random.default_rng(33)
    x = rng.normal(128.0, 16.0, (C, N))
    delays = orc.sweep_table([60.0], freqs, E2E_DT)[0]
    t0 = np.round(17.0 + E2E_PERIOD * np.arange(int(N / E2E_PERIOD) + 1)).astype(np.int64)
    for c in range(C):
        for w in range(E2E_WIDTH):
            t = t0 + w + int(delays[c])
            x[c, t[t < N]] += 5.0
    return freqs, np.clip(np.round(x), 0, 255).astype(np.uint8)


def _check_top(top, step, trial_step):
    assert abs(top.dm - 60.0) <= step, top
    return abs(top.period - E2E_PERIOD * E2E_DT) / trial_step


def test_end_to_end(gpu, slow_pulsar, tmp_path):
    import torch
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.ffa import FFASearch
    from pypulsar_amd.fold import Folder
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.periodicity import read_accelcands, sift
    from pypulsar_amd.sweep import DMSweep
    freqs, x = slow_pulsar
    step = E2E_DMS[1] - E2E_DMS[0]
    sw = DMSweep(E2E_DMS, freqs, E2E_DT, dtype="f32")
    plane = sw(torch.from_numpy(x).cuda().float(), trim=True)
    D, n = plane.shape
    fs = FFASearch(**E2E_ARGS)
    cands = fs(plane, E2E_DMS, E2E_DT)
    batched = fs(plane, E2E_DMS, E2E_DT, row_batch=5)        # (row batches change nothing)
    np.testing.assert_array_equal(cands, batched)
    s = sift(cands)
    top = s[0]
    rec = cands[np.argmax(cands["sigma"])]
    Mp = fo.mp_of(n // int(rec["ds"]) // int(rec["nbins"]))
    trial_step = rec["ds"] * E2E_DT / (Mp - 1)
    off = _check_top(top, step, trial_step)
    print("top: %r, %d bins wide, %.2f trial steps from the injected period" % (
        top, rec["width"], off))
    assert abs(top.row - 7.5) <= 1.5 and off <= rec["width"] + 1
    assert top.sigma >= 8.0 and len(top.hits) >= 3
    folded = Folder(32, 64)(plane, E2E_DMS, E2E_DT, s[:1])
    sw.close()
    assert folded[0].sigma > 8.0 and abs(folded[0].dm - 60.0) <= step
    # (the fold's own period step is P^2 / (64 T), ten trial steps)
    assert abs(folded[0].period - E2E_PERIOD * E2E_DT) <= (E2E_PERIOD * E2E_DT) ** 2 / (
        64 * n * E2E_DT)

    # the CLI on the same data: .ffacands with that candidate first
    C = x.shape[0]
    foff = float(freqs[1] - freqs[0])
    params, hdr = sigproc.make_header(C, 8, E2E_DT, float(freqs[0]), foff, src_raj=123456.789,
                                      src_dej=-123456.5)
    fn = str(tmp_path / "slow.fil")
    fbm.write_filterbank(fn, params, hdr, x.T.copy())
    common = ["--lodm", "52.5", "--hidm", "67.5", "--numdms", "16"]
    assert pulsar_search.main(common + [fn]) == 0
    assert os.path.exists(str(tmp_path / "slow.accelcands"))
    assert not os.path.exists(str(tmp_path / "slow.ffacands"))
    assert pulsar_search.main(common + ["--ffa", "--ffa-pmin", "0.08", "--ffa-pmax", "0.13",
                                        "--fold", "1", fn]) == 0
    back = read_accelcands(str(tmp_path / "slow.ffacands"))
    assert len(back) == len(s)
    b = back[0]
    assert _check_top(b, step, trial_step) <= rec["width"] + 1
    assert abs(b.dm - top.dm) <= 0.005 and abs(b.sigma - top.sigma) <= 0.005
    assert abs(b.period - top.period) <= 0.5e-9 and len(b.hits) == len(top.hits)
    assert os.path.exists(str(tmp_path / "slow_ffacand1.bestprof"))
    assert os.path.exists(str(tmp_path / "slow_ffacand1.npz"))
