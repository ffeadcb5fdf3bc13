"""The acceleration search's kernels (pypulsar_amd/csrc/pdd_accel.hip) at the
edges tests/test_gpu_accel.py does not reach, against the NumPy restatement
(tests/accel_oracle.py): k_acc_correlate at nz = 1..255 (every remainder of
its 4-z register block it can meet: nz is odd), M = 16..512, rows shorter than
a tile and than M, dz = 1, 2, 3, on noise and on impulses; k_acc_search<H> for
every H = 1..16 at nz = 1, 3, 13, 255, with short and skipped stages.
Synthetic spectra and planes go straight into AccelSearch.correlate and
AccelSearch.raw; the one FFT length used in this file is 4096."""
import collections

import numpy as np
import pytest

import accel_oracle as ao

pytestmark = pytest.mark.gpu

# (n, nfft, zmax, dz) -> (nz, M, nn)
BANKS = {(200, 200, 0, 2): (1, 16, 100),
         (100, 200, 4, 2): (5, 36, 100),
         (90, 200, 10, 3): (7, 46, 100),
         (600, 1024, 7, 1): (15, 34, 512),
         (1024, 1024, 6, 2): (7, 19, 512),
         (1026, 1026, 2, 2): (3, 17, 513),
         (1144, 4096, 254, 2): (255, 512, 2048)}
PAD = 37  # bins between the rows of a spectrum, filled with 7e5


def _padded(F):
    """complex64 rows [D, nn] -> a strided device view of them inside a wider
    buffer filled with 7e5 (a correlation that reads past a row shows)."""
    import torch
    D, nn = F.shape
    big = torch.zeros((D, nn + PAD), dtype=torch.complex64, device="cuda")
    big[:] = 7.0e5
    big[:, :nn] = torch.from_numpy(F).cuda()
    view = big[:, :nn]
    assert view.stride(0) == nn + PAD
    return view


# ---- 1. correlation of noise against the float64 oracle ----

@pytest.mark.parametrize("n,nfft,zmax,dz", sorted(BANKS))
def test_correlate_edges_vs_oracle(gpu, n, nfft, zmax, dz):
    import torch
    from pypulsar_amd.accel import AccelSearch
    nz, M, nn = BANKS[(n, nfft, zmax, dz)]
    acc = AccelSearch(zmax=zmax, dz=dz)
    assert acc.nz == nz
    rng = np.random.default_rng(1000 + n)
    F = ((rng.normal(size=(2, nn)) + 1j * rng.normal(size=(2, nn))) / np.sqrt(2.0)
         ).astype(np.complex64)  # unit variance a bin
    view = _padded(F)
    P = acc.correlate(view, n)
    torch.cuda.synchronize()
    Ph = P.cpu().numpy()
    assert Ph.shape == (2, nz, 2 * nn) and Ph.dtype == np.float32
    t, hw, Mo = ao.taps(n, nfft, zmax, dz)
    assert (t.shape[0], Mo, nfft // 2) == (nz, M, nn)
    ref = np.stack([ao.plane(F[d], t, Mo) for d in range(2)])
    err = np.max(np.abs(Ph.astype(np.float64) - ref)) / np.max(ref)
    print("correlate (n, nfft, zmax, dz) = (%d, %d, %d, %d): nz = %d (mod 4: %d), M = %d, nn = %d: "
          "max |P - P_ref| / max P_ref = %.3g" % (n, nfft, zmax, dz, nz, nz % 4, M, nn, err))
    assert err <= 2e-5
    # deterministic: the same bits on a second launch
    again = acc.correlate(view, n).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.int32), Ph.view(np.int32))
    if zmax == 0:
        # z = 0 at whole bins without padding: the power of the spectrum itself
        p = np.abs(F.astype(np.complex128)) ** 2
        e0 = np.max(np.abs(Ph[:, 0, 0::2] - p)) / np.max(p)
        print("correlate n = nfft = %d: z = 0 whole bins against |F|^2: %.3g" % (n, e0))
        assert e0 <= 1e-5


# ---- 2. impulse rows: every tap at its place ----

@pytest.mark.parametrize("bank,rows", [
    ((1144, 4096, 254, 2), ((0, 2047), (511, 1536))),
    ((90, 200, 10, 3), ((0,), (99,), (50,)))])
def test_correlate_impulses_are_the_taps(gpu, bank, rows):
    """A row that is 1 + 0i at a bin k and 0 elsewhere leaves the tap itself in
    the accumulator of every position k0 with |k - k0| <= hw_j, so P[d][j][2 k0
    + phi] is re^2 + im^2 of the float32 tap [j, phi, M + (k - k0)]: two
    products and a sum, three float32 roundings of relative 2^-24 each
    (contraction only removes one), within 2^-22; every other position is an
    exact 0 -- also those within the half-width of the z value's group, where
    the padded taps are 0."""
    import torch
    from pypulsar_amd.accel import AccelSearch, template_bank
    n, nfft, zmax, dz = bank
    nz, M, nn = BANKS[bank]
    taps, hw, M2 = template_bank(n, nfft, zmax, dz)
    assert (len(hw), M2) == (nz, M)
    for bins in rows:  # the supports of a row's impulses do not overlap
        assert all(b - a > 2 * M for a, b in zip(bins, bins[1:]))
    F = np.zeros((len(rows), nn), dtype=np.complex64)
    for d, bins in enumerate(rows):
        F[d, list(bins)] = 1.0
    acc = AccelSearch(zmax=zmax, dz=dz)
    P = acc.correlate(_padded(F), n)
    torch.cuda.synchronize()
    Ph = P.cpu().numpy()
    for d, bins in enumerate(rows):
        want, support = ao.impulse_plane(taps, hw, M, nn, bins)
        assert support.sum() == sum(2 * (min(nn - 1, k + int(h)) - max(0, k - int(h)) + 1)
                                    for k in bins for h in hw)
        assert np.all(want[support] > 0)
        assert np.all(Ph[d][~support] == 0.0)
        np.testing.assert_allclose(Ph[d][support].astype(np.float64), want[support],
                                   rtol=2.0 ** -22, atol=0.0)


# ---- 3. the search: every k_acc_search<H> against the oracle, as sets ----

LIST_A = (1, 3, 5, 6, 7, 9, 10, 11)
LIST_B = (2, 4, 8, 12, 13, 14, 15, 16)
SHAPES = ((1, 1000), (3, 1000), (13, 1000), (255, 600))  # (nz, ni)
# Thresholds (sigma) of the float planes.  The cells of a stage are sums of H
# exponential(1) values; a candidate must be a local maximum of about nine
# cells.  At nz = 13 and 255 sigma 3 leaves every stage more than the 20 the
# tests ask of the oracle; a plane of one or three z rows has too few cells
# for that, and is searched at sigma 1.
FLOAT_SIGMA = {1: 1.0, 3: 1.0, 13: 3.0, 255: 3.0}


def _integer_planes(nz, ni, harms):
    """[2][nz][ni] of integers 0..4 (ties everywhere) with 40.0 planted on
    every corner and edge, on both sides of the boundaries of the 254-position
    tiles of stage 1 and of the list's largest stage, and at the first
    position that stage searches (rlo = 1)."""
    rng = np.random.default_rng(17 + nz)
    P = rng.integers(0, 5, (2, nz, ni)).astype(np.float32)
    top, mid = nz - 1, nz // 2
    j = lambda v: min(v, top)  # noqa: E731
    hi = 2 * harms[-1]
    for d, jj, i in ((0, 0, ni - 1), (0, top, ni - 1), (0, 0, ni // 2), (0, top, ni // 2 + 1),
                     (1, mid, ni - 1), (1, 0, hi), (1, top, hi), (0, j(5), 2), (0, j(5), 255),
                     (0, j(6), 256), (1, j(7), 509), (1, j(7), 510), (1, j(3), 763),
                     (1, j(4), 764), (0, j(9), hi + 253), (0, j(10), hi + 254),
                     (1, j(2), hi + 507), (1, j(1), hi + 508), (1, 0, 0), (1, top, 0)):
        if i < ni:
            P[d, jj, i] = 40.0
    return P


def _float_planes(nz, ni):
    rng = np.random.default_rng(29 + nz)
    P = rng.exponential(1.0, (2, nz, ni)).astype(np.float32)
    assert P.dtype == np.float32
    return P


def _record_set(c, k):
    c = c[:k].cpu().numpy()
    assert np.all(c[:, 5] == 0)
    return set(map(tuple, c[:, :5].tolist()))


def _search(P, harms, sigma, rlo):
    """raw() of a host plane -> (the set of records, asserted free of
    duplicates; the float32 thresholds)."""
    import torch
    from pypulsar_amd.accel import AccelSearch
    D, nz, ni = P.shape
    acc = AccelSearch(sigma_threshold=sigma, zmax=nz - 1, harms=harms)
    assert acc.nz == nz
    dt = (rlo - 0.5) / ni  # flo = 1 Hz
    assert acc.rlo(ni, dt) == rlo
    cd, k = acc.raw(torch.from_numpy(P).cuda(), ni, dt)
    k = int(k.item())
    assert k <= acc.max_cands
    got = _record_set(cd, k)
    assert len(got) == k  # no duplicates
    return got, acc.thr


def _per_stage(cands, harms):
    n = collections.Counter(c[3] for c in cands)
    return [n[H] for H in harms]


@pytest.mark.parametrize("harms", [LIST_A, LIST_B])
@pytest.mark.parametrize("nz,ni", SHAPES)
def test_search_every_instance_integer_planes(gpu, nz, ni, harms):
    P = _integer_planes(nz, ni, harms)
    got, thr = _search(P, harms, 2.0, 1)
    want = ao.candidates(P, harms, thr, 1)
    counts = _per_stage(want, harms)
    print("search integers nz=%d ni=%d harms=%r: candidates per stage %r" % (nz, ni, harms, counts))
    assert min(counts) >= 20
    assert got == want
    # planted cells that stage 1 must report whatever surrounds them
    if harms[0] == 1:
        bits = int(np.float32(40.0).view(np.int32))
        assert (0, ni - 1, -(nz // 2), 1, bits) in got and (0, ni - 1, nz // 2, 1, bits) in got


@pytest.mark.parametrize("harms", [LIST_A, LIST_B])
@pytest.mark.parametrize("nz,ni", SHAPES)
def test_search_every_instance_float_planes(gpu, nz, ni, harms):
    """Exponential float32 planes: the float32 sum in ascending h is the only
    order that gives the oracle's bits, and the record carries the bits."""
    P = _float_planes(nz, ni)
    got, thr = _search(P, harms, FLOAT_SIGMA[nz], 1)
    want = ao.candidates(P, harms, thr, 1)
    counts = _per_stage(want, harms)
    print("search floats nz=%d ni=%d harms=%r sigma=%.1f: candidates per stage %r"
          % (nz, ni, harms, FLOAT_SIGMA[nz], counts))
    assert min(counts) >= 20
    assert got == want


@pytest.mark.parametrize("rlo,last,positions", [(40, 12, 40), (31, 16, 8)])
def test_search_short_and_skipped_stages(gpu, rlo, last, positions):
    """[2][13][1000] with list B: at rlo = 40 stage 12 searches 40 positions
    (less than a tile) and stages 13..16 start past the plane; at rlo = 31
    stage 16 searches 8."""
    ni = 1000
    assert ni - 2 * last * rlo == positions
    assert [H for H in LIST_B if 2 * H * rlo < ni][-1] == last
    P = _float_planes(13, ni)
    got, thr = _search(P, LIST_B, 0.0, rlo)
    want = ao.candidates(P, LIST_B, thr, rlo)
    counts = _per_stage(want, LIST_B)
    print("search rlo=%d: candidates per stage %r" % (rlo, counts))
    # 2 x 13 x `positions` cells, about half above the sigma = 0 threshold
    # (the median), a local maximum in about nine cells, more on the edges:
    # 8 positions hold about 2 * 13 * 8 / 18 = 11 candidates
    assert counts[LIST_B.index(last)] >= 5
    assert all(n >= 20 for H, n in zip(LIST_B, counts) if H < last)
    assert all(n == 0 for H, n in zip(LIST_B, counts) if H > last)
    assert got == want
    assert min(c[1] for c in got if c[3] == last) >= 2 * last * rlo


@pytest.mark.parametrize("harms", [LIST_A, LIST_B])
def test_search_every_stage_skipped(gpu, harms):
    """ni = 100 at rlo = 60: the first position of stage 1 is 120.  Nothing
    is launched: the count stays 0 and the candidate buffer as it was."""
    import ctypes
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.accel import AccelSearch
    P = _float_planes(13, 100)
    got, thr = _search(P, harms, 0.0, 60)
    assert got == set() and ao.candidates(P, harms, thr, 60) == set()
    acc = AccelSearch(sigma_threshold=0.0, zmax=12, harms=harms)
    cands = torch.full((64, 6), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.call("pdd_acc_search", _lib.ptr(torch.from_numpy(P).cuda()), 2, 13, 100,
              acc.harms.ctypes.data_as(ctypes.c_void_p), len(acc.harms),
              acc.thr.ctypes.data_as(ctypes.c_void_p), 60, _lib.ptr(cands), 64,
              _lib.ptr(count), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    assert bool(torch.all(cands == -7))


# ---- 4. dz = 1 end to end ----

def test_dz1_end_to_end(gpu):
    import torch
    from pypulsar_amd.accel import AccelSearch
    n, nfft, harms = 3000, 4096, (1, 2, 3, 4)
    acc = AccelSearch(zmax=8, dz=1, harms=harms, initialbuflen=40)
    assert acc.nz == 17 and acc.J0 == 8
    xd = torch.from_numpy(ao.chirp_rows(n, nfft, 350.3, 4.0, seed=1, rows=3)).cuda()
    _, white = acc.ps.normalise(acc.ps.spectrum(xd, nfft), want_spectrum=True)
    P = acc.correlate(white, n)
    torch.cuda.synchronize()
    Ph, wh = P.cpu().numpy(), white.cpu().numpy()
    t, hw, M = ao.taps(n, nfft, 8, dz=1)
    ref = np.stack([ao.plane(wh[d], t, M) for d in range(3)])
    err = np.max(np.abs(Ph.astype(np.float64) - ref)) / np.max(ref)
    print("dz = 1: max |P - P_ref| / max P_ref = %.3g (nz = %d, M = %d)" % (err, acc.nz, M))
    assert err <= 2e-5
    dt = 2.5 / nfft  # flo = 1 Hz: rlo = 3
    assert acc.rlo(nfft, dt) == 3
    cd, k = acc.raw(P, nfft, dt)
    got = _record_set(cd, int(k.item()))
    assert len(got) == int(k.item())
    want = ao.candidates(Ph, harms, acc.thr, 3)
    print("dz = 1: candidates per stage %r" % (_per_stage(want, harms),))
    assert len(want) > 0 and got == want
    recs = acc.collect(cd, k, [1.0, 2.0, 3.0], n, nfft, dt)
    assert len(recs) == len(got)
    # z = jc dz / H with dz = 1, and what follows from it
    rows = sorted((d, H, i / (2.0 * H), jc / float(H)) for d, i, jc, H, _ in got)
    assert [(int(r["row"]), int(r["numharm"]), float(r["r"]), float(r["z"])) for r in recs] == rows
    np.testing.assert_allclose(recs["zbins"], recs["z"] * nfft / n, rtol=1e-15)
    np.testing.assert_allclose(recs["fd"], recs["z"] / (n * dt) ** 2, rtol=1e-15)
    top = recs[np.argmax(recs["sigma"])]
    print("dz = 1: strongest %r" % (top,))
    assert top["row"] == 0 and abs(top["r"] - 350.3) <= 0.25 and abs(top["z"] - 4.0) <= 0.5
