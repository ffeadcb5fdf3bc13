"""The jerk search on the GPU (pdd_acc_correlate per w slab, pdd_jerk_search,
pypulsar_amd.jerk.JerkSearch) against the NumPy restatement
(tests/jerk_oracle.py): the volume, the record sets of every k_jerk_step<H>,
synthetic volumes with ties and maxima on every edge and seam, overflow,
refusals, and the recovery of a pulsar with a jerk.  FFT lengths used in this
file: 4096 and 5000 (and the synthetic ni = 2042)."""
import ctypes

import numpy as np
import pytest

import accel_oracle as ao
import jerk_oracle as jo

pytestmark = pytest.mark.gpu
ZMAX, WMAX = 8, 40
CASES = ((3000, 4096), (4700, 5000))
IBL = 40  # whitening blocks of the recovery cases (see tests/test_accel_oracle.py)


@pytest.fixture(scope="module")
def vols(gpu):
    """Per case: the GPU's whitened spectrum of two rows (a pulsar with a jerk
    and noise; a strided view), the volume of JerkSearch.correlate and the
    float64 oracle volume of the same complex64 spectrum -- computed once,
    shared and left unchanged."""
    import torch
    from pypulsar_amd.jerk import JerkSearch
    out = {}
    js = JerkSearch(sigma_threshold=3.5, zmax=ZMAX, wmax=WMAX, initialbuflen=IBL)
    assert (js.nw, js.nz, js.L0, js.J0) == (5, 9, 2, 4)
    for n, nfft in CASES:
        x = jo.jerk_rows(n, nfft, 350.3, 2.0, 10.0, seed=1, rows=2)
        xd = torch.from_numpy(x).cuda()
        _, white = js.ps.normalise(js.ps.spectrum(xd, nfft), want_spectrum=True)
        nn = nfft // 2
        big = torch.zeros((2, nn + 37), dtype=torch.complex64, device="cuda")
        big[:] = 7.0e5  # (a correlation that reads past a row's nn bins shows)
        big[:, :nn] = white
        view = big[:, :nn]
        V = js.correlate(view, n)
        torch.cuda.synchronize()
        t, hw, M = jo.taps(n, nfft, ZMAX, 2, WMAX, 20)
        wh = white.cpu().numpy()
        ref = np.stack([jo.volume(wh[d], t, M) for d in range(2)], axis=1)
        out[(n, nfft)] = dict(view=view, V=V, Vh=V.cpu().numpy(), ref=ref, M=M)
    return js, out


@pytest.mark.parametrize("n,nfft", CASES)
def test_correlate_vs_oracle(vols, n, nfft):
    from pypulsar_amd.accel import AccelSearch
    js, out = vols
    c = out[(n, nfft)]
    nn = nfft // 2
    assert c["Vh"].shape == (5, 2, 9, 2 * nn) and c["Vh"].dtype == np.float32
    assert c["ref"].shape == c["Vh"].shape
    for l in range(5):
        err = np.max(np.abs(c["Vh"][l].astype(np.float64) - c["ref"][l])) / np.max(c["ref"][l])
        print("correlate n=%d nfft=%d slab w=%d: max |P - P_ref| / max P_ref = %.3g (M = %d)"
              % (n, nfft, (l - 2) * 20, err, c["M"]))
        assert err <= 2e-5
    # the w = 0 slab has the bits of the acceleration search's plane
    acc = AccelSearch(sigma_threshold=3.5, zmax=ZMAX, initialbuflen=IBL)
    P = acc.correlate(c["view"], n).cpu().numpy()
    np.testing.assert_array_equal(P.view(np.int32), c["Vh"][2].view(np.int32))


def _record_set(c, k):
    c = c[:k].cpu().numpy()
    assert c.shape[1] == 8 and np.all(c[:, 6:] == 0)
    return {tuple(int(v) for v in r[:6]) for r in c}


@pytest.mark.parametrize("harms", [(1, 2, 4, 8), (1, 3), (16,)])
@pytest.mark.parametrize("n,nfft", CASES)
def test_search_vs_oracle_own_volume(vols, n, nfft, harms):
    from pypulsar_amd.jerk import JerkSearch
    _, out = vols
    c = out[(n, nfft)]
    js = JerkSearch(sigma_threshold=3.5, zmax=ZMAX, wmax=WMAX, harms=harms)
    dt = 2.5 / nfft  # flo = 1 Hz: rlo = 3
    assert js.rlo(nfft, dt) == 3
    cd, k = js.raw(c["V"], nfft, dt)
    got = _record_set(cd, int(k.item()))
    assert len(got) == int(k.item())  # no duplicates
    want = jo.candidates(c["Vh"], harms, js.thr, 3)
    print("harms %r: %d records" % (harms, len(want)))
    assert len(want) > 10
    assert got == want
    recs = js.collect(cd, k, [1.0, 2.0], n, nfft, dt)
    assert len(recs) == len(got) and np.all(recs["sigma"] >= 3.5 - 1e-6)
    assert np.allclose(recs["wbins"], recs["w"] * nfft / n)
    assert np.allclose(recs["fdd"], recs["w"] / (n * dt) ** 3)
    assert np.allclose(recs["jerk"], recs["fdd"] * 299792458.0 / recs["freq"])


def test_nw1_is_the_acceleration_search(vols):
    """One w slab: the records of pdd_acc_search with lc = 0 on the same plane;
    and nz = 1, nw = 3 against the oracle."""
    from pypulsar_amd.accel import AccelSearch
    from pypulsar_amd.jerk import JerkSearch
    _, out = vols
    c = out[(3000, 4096)]
    dt = 2.5 / 4096
    P = c["V"][2].contiguous()
    acc = AccelSearch(sigma_threshold=3.5, zmax=ZMAX)
    ca, ka = acc.raw(P, 4096, dt)
    ca = ca[:int(ka.item())].cpu().numpy()
    want = {(int(r[0]), int(r[1]), int(r[2]), 0, int(r[3]), int(r[4])) for r in ca}
    assert len(want) > 10
    js = JerkSearch(sigma_threshold=3.5, zmax=ZMAX, wmax=0)
    assert js.nw == 1
    cd, k = js.raw(P[None], 4096, dt)
    assert _record_set(cd, int(k.item())) == want
    # nz = 1: the z = 0 rows of three slabs
    V = c["V"][1:4, :, 4:5].contiguous()
    js = JerkSearch(sigma_threshold=3.5, zmax=0, wmax=20, harms=(1, 2, 5))
    assert (js.nw, js.nz) == (3, 1)
    cd, k = js.raw(V, 4096, dt)
    want = jo.candidates(V.cpu().numpy(), (1, 2, 5), js.thr, 3)
    assert len(want) > 10
    assert _record_set(cd, int(k.item())) == want


NI = 2 * 1021  # not a multiple of the 254-position tile


def _synthetic(harms, rlo, seed):
    """[3][2][5][NI] of small integers (ties everywhere) with 40s planted at
    both edges of every axis, at i = ilo + 253, 254, 255 of every stage (the
    seam of the first two workgroups) and as equal pairs across each axis and
    across seams."""
    rng = np.random.default_rng(seed)
    V = rng.integers(0, 5, (3, 2, 5, NI)).astype(np.float32)
    cells = [(0, 0, 0, NI - 1), (2, 0, 4, NI - 1), (0, 1, 4, NI - 1), (2, 1, 0, NI - 1),
             (1, 0, 2, NI - 1), (0, 0, 2, 700), (2, 1, 2, 701), (1, 1, 0, 900), (1, 0, 4, 901)]
    for H in harms:
        ilo = 2 * H * rlo
        if ilo >= NI:
            continue
        cells += [(0, 0, 0, ilo), (2, 1, 4, ilo), (1, 0, 2, ilo + 253), (1, 1, 2, ilo + 254),
                  (2, 0, 3, ilo + 255), (0, 1, 1, ilo + 507), (0, 1, 1, ilo + 508),  # tie, seam
                  (2, 1, 1, ilo + 253), (2, 1, 1, ilo + 254)]                        # tie, seam
    # ties across l, across j, and across a diagonal that crosses a seam
    cells += [(0, 0, 3, 1200), (1, 0, 3, 1200), (1, 1, 1, 1300), (1, 1, 2, 1300),
              (0, 0, 1, 2 * rlo + 253), (1, 0, 2, 2 * rlo + 254)]
    for l, d, j, i in cells:
        if 0 <= i < NI:
            V[l, d, j, i] = 40.0
    return V


@pytest.mark.parametrize("harms,rlo", [((1, 2, 4, 8), 1), ((1, 3, 5, 6, 7, 9, 10, 11), 1),
                                       ((2, 4, 8, 12, 13, 14, 15, 16), 2),
                                       ((1, 2, 4, 8), 128)])
def test_search_synthetic_ties_and_edges(gpu, harms, rlo):
    """Integer-valued volumes: every sum is exact, ties are everywhere.  With
    rlo = 128 the stage H = 8 has ilo = 2048 >= ni and is skipped."""
    import torch
    from pypulsar_amd.jerk import JerkSearch
    V = _synthetic(harms, rlo, 17 + rlo)
    js = JerkSearch(sigma_threshold=2.0, zmax=4, wmax=20, harms=harms)  # (H = 1: S >= 3.8)
    assert (js.nw, js.nz) == (3, 5)
    dt = (rlo - 0.5) / NI
    assert js.rlo(NI, dt) == rlo
    cd, k = js.raw(torch.from_numpy(V).cuda(), NI, dt)
    got = _record_set(cd, int(k.item()))
    assert len(got) == int(k.item())
    want = jo.candidates(V, harms, js.thr, rlo)
    print("harms %r rlo %d: %d records" % (harms, rlo, len(want)))
    assert len(want) > 100
    assert got == want
    b40 = int(np.float32(40.0).view(np.int32))
    assert (0, NI - 1, -2, -1, 1, b40) in got or harms[0] != 1
    if rlo == 128:
        assert {r[4] for r in got} == {1, 2, 4}
    # the same bits and the same set on a second launch
    cd2, k2 = js.raw(torch.from_numpy(V).cuda(), NI, dt)
    assert _record_set(cd2, int(k2.item())) == got


def test_search_no_rows(gpu):
    """D = 0: nothing is launched, nothing is counted."""
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.jerk import JerkSearch
    js = JerkSearch(sigma_threshold=2.0, zmax=4, wmax=20)
    V = torch.empty((3, 0, 5, NI), dtype=torch.float32, device="cuda")
    cd, k = js.raw(V, NI, 0.5 / NI)
    assert int(k.item()) == 0
    # the entry point itself with D = 0
    one = torch.zeros(8, dtype=torch.float32, device="cuda")
    cands = torch.empty((4, 8), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.call("pdd_jerk_search", _lib.ptr(one), 0, 3, 5, NI,
              js.harms.ctypes.data_as(ctypes.c_void_p), len(js.harms),
              js.thr.ctypes.data_as(ctypes.c_void_p), 1, _lib.ptr(one), 8, _lib.ptr(cands), 4,
              _lib.ptr(count), _lib.stream_ptr())
    assert int(count.item()) == 0
    assert len(js.collect(cands, count, [], 100, NI, 1e-3)) == 0


def test_search_overflow(vols):
    from pypulsar_amd.jerk import JerkSearch
    _, out = vols
    js = JerkSearch(sigma_threshold=3.0, zmax=ZMAX, wmax=WMAX, max_cands=2)
    V = out[(3000, 4096)]["V"]
    cd, k = js.raw(V, 4096, 2.5 / 4096)
    total = int(k.item())
    assert total > 2 and cd.shape == (2, 8)
    want = jo.candidates(out[(3000, 4096)]["Vh"], js.harms, js.thr, 3)
    assert total == len(want)  # the count is reported in full
    assert _record_set(cd, 2) <= want and len(_record_set(cd, 2)) == 2  # stored up to max_cands
    with pytest.raises(RuntimeError):
        js.collect(cd, k, [1.0, 2.0], 3000, 4096, 2.5 / 4096)


def test_search_refuses_bad_arguments(gpu):
    import torch
    from pypulsar_amd import _lib
    nw, D, nz, ni = 3, 1, 5, 512
    V = torch.zeros((nw, D, nz, ni), dtype=torch.float32, device="cuda")
    scratch = torch.zeros(3 * D * nz * ni, dtype=torch.float32, device="cuda")
    cands = torch.empty((4, 8), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    harms = np.asarray([1, 2], dtype=np.int32)
    thr = np.asarray([1.0, 2.0], dtype=np.float32)
    hp, tp = harms.ctypes.data_as(ctypes.c_void_p), thr.ctypes.data_as(ctypes.c_void_p)
    good = dict(vol=_lib.ptr(V), D=D, nw=nw, nz=nz, ni=ni, harms=hp, n_harms=2, thr=tp, rlo=1,
                scratch=_lib.ptr(scratch), scratch_floats=scratch.numel(),
                cands=_lib.ptr(cands), max_cands=4, count=_lib.ptr(count))
    order = ("vol", "D", "nw", "nz", "ni", "harms", "n_harms", "thr", "rlo", "scratch",
             "scratch_floats", "cands", "max_cands", "count")

    def run(**kw):
        a = dict(good, **kw)
        _lib.call("pdd_jerk_search", *([a[k] for k in order] + [_lib.stream_ptr()]))

    run()  # (the good call passes)
    bad17 = np.asarray([1, 17], dtype=np.int32)
    for kw in (dict(nw=4), dict(nw=65), dict(nz=4), dict(nz=257), dict(vol=None),
               dict(scratch=None), dict(count=None), dict(cands=None), dict(harms=None),
               dict(thr=None), dict(scratch_floats=3 * D * nz * ni - 1), dict(rlo=0),
               dict(harms=bad17.ctypes.data_as(ctypes.c_void_p)), dict(n_harms=9)):
        with pytest.raises(_lib.PddError):
            run(**kw)
    torch.cuda.synchronize()
    assert int(count.item()) == 0  # (a plane of zeros: nothing above 1.0; nothing refused ran)


# ---- recovery: a pulsar with a jerk through JerkSearch.__call__ ----

@pytest.fixture(scope="module")
def recovery(gpu):
    """Four rows (seeds 0-3) of a four-harmonic pulsar at r = 350.3, z = 2, w =
    10; the records of JerkSearch.__call__ and the volume of the same rows."""
    import torch
    from pypulsar_amd.jerk import JerkSearch
    n, nfft, dt = 3000, 4096, 1e-3
    x = np.concatenate([jo.jerk_rows(n, nfft, 350.3, 2.0, 10.0, seed=s) for s in range(4)])
    plane = torch.from_numpy(x).cuda()
    dms = np.arange(4) * 2.0
    js = JerkSearch(zmax=ZMAX, wmax=WMAX, initialbuflen=IBL)
    recs = js(plane, dms, dt, nfft=nfft)
    _, white = js.ps.normalise(js.ps.spectrum(plane, nfft), want_spectrum=True)
    Vh = js.correlate(white, n).cpu().numpy()
    return dict(js=js, plane=plane, dms=dms, dt=dt, n=n, nfft=nfft, recs=recs, Vh=Vh)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_recovery(recovery, seed):
    from pypulsar_amd.jerk import JERK_CAND_DTYPE
    recs, js = recovery["recs"], recovery["js"]
    assert recs.dtype == JERK_CAND_DTYPE
    r4 = recs[(recs["row"] == seed) & (recs["numharm"] == 4)]
    assert len(r4) > 0
    top = r4[np.argmax(r4["power"])]
    S4 = jo.stage_sum(recovery["Vh"][:, seed], 4)
    ilo = 2 * 4 * js.rlo(recovery["nfft"], recovery["dt"])
    best0 = float(S4[js.L0, :, ilo:].max())
    print("seed %d: top stage-4 record r = %.3f z = %.2f w = %.2f S = %.1f; best of the w = 0 "
          "slab %.1f (%.3f of it)" % (seed, top["r"], top["z"], top["w"], top["power"], best0,
                                      best0 / top["power"]))
    # the cell i = 2802, jc dz = 8, lc dw = 40 of the top harmonic's grid
    assert top["r"] * 8 == 2802 and top["z"] * 4 == 8 and top["w"] * 4 == 40
    assert (top["r"], top["z"], top["w"]) == (350.25, 2.0, 10.0)
    assert np.float32(top["power"]) == S4[js.L0 + 2, js.J0 + 4, 2802]
    assert best0 <= 0.9 * top["power"]
    T = recovery["n"] * recovery["dt"]
    assert abs(top["fdd"] - 10.0 / T ** 3) <= 1e-15
    assert top["DM"] == 2.0 * seed


def test_call_batches_and_wmax0(recovery):
    """Row batches change nothing; wmax = 0 gives the acceleration search's
    records with w = 0; a workspace too small for one row is refused."""
    from pypulsar_amd.accel import AccelSearch
    from pypulsar_amd.jerk import JerkSearch
    c = recovery
    again = c["js"](c["plane"], c["dms"], c["dt"], row_batch=3, nfft=c["nfft"])
    np.testing.assert_array_equal(again, c["recs"])
    acc = AccelSearch(zmax=ZMAX, initialbuflen=IBL)(c["plane"], c["dms"], c["dt"], nfft=c["nfft"])
    j0 = JerkSearch(zmax=ZMAX, wmax=0, initialbuflen=IBL)(c["plane"], c["dms"], c["dt"],
                                                        nfft=c["nfft"])
    assert len(acc) > 0 and len(j0) == len(acc)
    for name in acc.dtype.names:
        np.testing.assert_array_equal(j0[name], acc[name])
    for name in ("w", "wbins", "fdd", "jerk"):
        assert np.all(j0[name] == 0.0)
    small = JerkSearch(zmax=ZMAX, wmax=WMAX, workspace_bytes=1 << 20)
    assert small.row_bytes(4096) == (24 + 4 * 9 * 8) * 4096
    with pytest.raises(ValueError, match="nfft.*zmax.*wmax"):
        small(c["plane"], c["dms"], c["dt"], nfft=c["nfft"])
    assert JerkSearch(zmax=ZMAX, wmax=WMAX, workspace_bytes=4 << 20).row_batch(4096) == 3
