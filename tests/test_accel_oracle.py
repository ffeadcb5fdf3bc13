"""The NumPy restatement of the acceleration search (tests/accel_oracle.py)
against the quadrature of its response, a fixture made by running the
reference's PrestoFFT.interpolate (tests/golden/make_golden_interp.py) and
planted drifting signals.  CPU only."""
import os

import numpy as np
import pytest

import accel_oracle as ao
import period_oracle as po
from conftest import GOLDEN

ZS = (0, 2, -2, 12, -37, 50)


@pytest.fixture(scope="module")
def gi():
    return np.load(os.path.join(GOLDEN, "golden_interp.npz"), allow_pickle=False)


@pytest.mark.parametrize("z", ZS)
def test_closed_form_vs_quadrature(z):
    x = np.linspace(-30.0, 30.0, 1201)
    err = np.max(np.abs(ao.response(x, z) - ao.response_quad(x, z, 8192)))
    print("z=%d: closed form - quadrature(8192): max abs %.3g" % (z, err))
    assert err <= 1e-6


@pytest.mark.parametrize("z", ZS)
def test_product_response_is_the_oracles(z):
    from pypulsar_amd import accel
    x = np.linspace(-30.0, 30.0, 1201)
    got = accel.z_response(x, z)
    assert got.dtype == np.complex128
    assert np.max(np.abs(got - ao.response_quad(x, z, 8192))) <= 1e-6


@pytest.mark.parametrize("n,nfft", [(3000, 4096), (4096, 4096), (4700, 5000)])
def test_taps_norm_and_product_bank(n, nfft):
    eta = n / float(nfft)
    t, hw, M = ao.taps(n, nfft, 24)
    assert t.shape == (25, 2, 2 * M + 1) and M == hw.max()
    assert hw[12] == int(np.ceil(16 / eta)) and hw[0] == hw[24] == int(np.ceil(28 / eta))
    np.testing.assert_allclose(np.sum(np.abs(t) ** 2, axis=2), eta, rtol=1e-12)
    for j in range(25):  # zero beyond the half-width
        assert np.all(t[j, :, :M - hw[j]] == 0) and np.all(t[j, :, M + hw[j] + 1:] == 0)
    if n == nfft:  # z = 0 at a whole bin without padding: a delta
        want = np.zeros(2 * M + 1)
        want[M] = 1.0
        np.testing.assert_allclose(t[12, 0], want, atol=1e-15)
    from pypulsar_amd import accel
    taps, hw2, M2 = accel.template_bank(n, nfft, 24)
    assert taps.dtype == np.float32 and taps.shape == (25, 2, 2 * M + 1, 2)
    assert M2 == M and np.array_equal(hw2, hw) and hw2.dtype == np.int32
    ref = np.stack((t.real, t.imag), axis=-1)
    assert np.max(np.abs(taps - ref)) <= 2.0 ** -24  # rounded once (|t| <= 1)


@pytest.mark.parametrize("m", [2, 32])
def test_interpolate_reference_golden(gi, m):
    spec, r, ref = gi["spec"], gi["r"], gi["interp_m%d" % m]
    got = ao.interpolate_reference(spec, r, m)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("interpolate m=%d: max err / max|ref| = %.3g" % (m, err))
    assert err <= 1e-6
    # the reference's sinc(pi d) is not the interpolation kernel: at a whole
    # bin it does not return the coefficient, the corrected form does
    whole = r == np.round(r)
    assert whole.sum() >= 50
    k = r[whole].astype(int)
    fixed = ao.interpolate_reference(spec, r, m, corrected=True)
    assert np.max(np.abs(fixed[whole] - spec[k])) <= 1e-6 * np.max(np.abs(spec))
    assert np.max(np.abs(got[whole] - spec[k])) > 1e-2 * np.max(np.abs(spec))


@pytest.mark.parametrize("m", [2, 32])
def test_corrected_interpolation_is_the_z0_correlation(gi, m):
    """sum_k F[k] exp(-i pi (r - k)) sinc(r - k) = sum_k F[k] conj(W(k - r; 0)):
    the templates' sign and phase convention is the reference's."""
    spec, r = gi["spec"].astype(np.complex128), gi["r"]
    k = np.round(r).astype(int)[:, None] + np.arange(-(m // 2), m // 2 + 1)
    want = np.sum(spec[k] * np.conj(ao.response(k - r[:, None], 0.0)), axis=1)
    got = ao.interpolate_reference(spec, r, m, corrected=True)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_plane_z0_is_the_whitened_power():
    F = ao.whitened(ao.chirp_rows(4096, 4096, 305.75, -5.0, seed=3)[0], 4096)
    t, hw, M = ao.taps(4096, 4096, 4)
    P = ao.plane(F, t, M)
    assert P.shape == (5, 4096)
    p = np.abs(F.astype(np.complex128)) ** 2
    assert np.max(np.abs(P[2, 0::2] - p)) <= 1e-12 * p.max()


# Whitening blocks of the recovery cases.  With the default initialbuflen = 6
# the blocks near bin 350 of these 2048-bin spectra are 35 bins long, and a
# strong drifting signal raises its own block medians: a tone of whitened power
# 64 has sidelobes of 64 / (pi x)^2 = 0.26 at x = 5 bins -- beside a noise
# median of 0.69 -- and a drift of 16 bins fills half a block outright.  That
# is a property of the reference's whitening on short spectra, not of the
# search: measured on seeds 0..7, the stage-4 maximum of the first case was
# 120..159 with initialbuflen = 6, 187..260 with 20 and 191..281 with 40
# (expected 257; at the right cell every time).  The recovery is therefore
# tested with initialbuflen = 40 (blocks of 200 bins, the golden fixtures'
# second setting).  The noise moves S_4 by about sqrt(2 S) = 9 %; the second
# case (expected 352) gave 252..322 over the same seeds -- its odd harmonics'
# z = -5, -15 fall between the even z of the grid.  The seed is fixed at 1.
RECOVERY_IBL = 40
RECOVERY = [(3000, 4096, 350.3, 4.0, 1), (4096, 4096, 305.75, -5.0, 1)]


@pytest.mark.parametrize("n,nfft,r,z,seed", RECOVERY)
def test_recovery(n, nfft, r, z, seed):
    amp, sig = 300.0, 1024.0
    thr = [po.threshold_power(6.0, H) for H in (1, 2, 4)]
    t, hw, M = ao.taps(n, nfft, 24)
    J0 = 12
    F = ao.whitened(ao.chirp_rows(n, nfft, r, z, amp, 4, seed)[0], nfft, RECOVERY_IBL)
    P = ao.plane(F, t, M).astype(np.float32)
    S4 = ao.stage_sum(P, 4)
    rlo = 8
    j, i = np.unravel_index(np.argmax(S4[:, 8 * rlo:]), S4[:, 8 * rlo:].shape)
    i += 8 * rlo
    want = 4 * amp * amp * n / (4 * sig * sig)
    print("n=%d: stage-4 maximum %.1f (expected %.1f) at r = %.3f, z = %.2f"
          % (n, S4[j, i], want, i / 8.0, (j - J0) * 2 / 4.0))
    assert abs(i / 8.0 - r) <= 0.25
    assert (j - J0) * 2 / 4.0 == z
    assert abs(S4[j, i] - want) <= 0.25 * want
    c = ao.candidates(P[None], (1, 2, 4), thr, rlo)
    assert (0, int(i), int(j - J0), 4, int(S4[j, i:i + 1].view(np.int32)[0])) in c
    # noise alone: the noise mean of the plane is 1 and nothing reaches 6
    # sigma, with either whitening
    for ibl in (6, RECOVERY_IBL):
        F0 = ao.whitened(ao.chirp_rows(n, nfft, r, z, seed=seed, signal=False)[0], nfft, ibl)
        P0 = ao.plane(F0, t, M).astype(np.float32)
        m = P0[:, 64:].mean(axis=1)
        print("n=%d, initialbuflen=%d: noise mean of the plane per z: %.3f .. %.3f"
              % (n, ibl, m.min(), m.max()))
        assert 0.85 <= m.min() and m.max() <= 1.15
        assert ao.candidates(P0[None], (1, 2, 4), thr, rlo) == set()


def _brute(P, harms, thr, rlo):
    """The candidate rule cell by cell."""
    D, nz, ni = P.shape
    J0 = (nz - 1) // 2
    out = set()
    for d in range(D):
        for H, t in zip(harms, thr):
            S = ao.stage_sum(P[d], H)
            ilo = 2 * H * rlo

            def val(j, i):
                return S[j, i] if 0 <= j < nz and ilo <= i < ni else np.float32(-np.inf)
            for j in range(nz):
                for i in range(ilo, ni):
                    s = S[j, i]
                    before = [val(j - 1, i - 1), val(j - 1, i), val(j - 1, i + 1), val(j, i - 1)]
                    after = [val(j, i + 1), val(j + 1, i - 1), val(j + 1, i), val(j + 1, i + 1)]
                    if s >= np.float32(t) and all(s > b for b in before) and \
                            all(s >= a for a in after):
                        out.add((d, i, j - J0, H, int(np.float32(s).view(np.int32))))
    return out


def test_candidate_rule_ties_and_edges():
    P = np.ones((1, 5, 12), dtype=np.float32)
    P[0, 0, 2] = 9.0                    # the first searched column, the first z row
    P[0, 4, 11] = 8.0                   # the last corner
    P[0, 2, 5] = P[0, 2, 6] = 7.0       # a tie along i: the first wins
    P[0, 3, 8] = P[0, 4, 8] = 6.0       # a tie along z: the first wins
    P[0, 1, 10] = P[0, 2, 9] = 5.0      # a diagonal tie: (1, 10) precedes (2, 9)
    P[0, 2, 1] = 50.0                   # below ilo = 2: not searched, not a neighbour
    got = ao.candidates(P, (1,), (4.0,), 1)
    cells = {(j + 2, i) for _, i, j, _, _ in got}
    assert cells == {(0, 2), (4, 11), (2, 5), (3, 8), (1, 10)}
    assert got == _brute(P, (1,), (4.0,), 1)
    # a random plane with many ties, two stages
    rng = np.random.default_rng(8)
    Q = rng.integers(0, 4, (2, 7, 60)).astype(np.float32)
    for harms in ((1, 2, 4), (1, 3)):
        thr = [2.0 * H for H in harms]
        a, b = ao.candidates(Q, harms, thr, 2), _brute(Q, harms, thr, 2)
        assert len(b) > 5 and a == b


def test_stage_sum_floors_negative_z():
    nz, ni = 5, 24
    P = (100.0 * np.arange(nz)[:, None] + np.zeros(ni)).astype(np.float32)  # P[j][i] = 100 j
    S = ao.stage_sum(P, 3)
    # jc = -2: rows J0 + floor((-2 h + 1) / 3) = 2 + (-1, -1, -2) = 1, 1, 0 (truncation: 2, 1, 0)
    assert S[0, 0] == 100.0 + 100.0 + 0.0
    # jc = -1: floor((-h + 1) / 3) = 0, -1, -1 -> rows 2, 1, 1
    assert S[1, 0] == 200.0 + 100.0 + 100.0
    # jc = 2: floor((2 h + 1) / 3) = 1, 1, 2 -> rows 3, 3, 4
    assert S[4, 0] == 300.0 + 300.0 + 400.0
    # columns: (i h + H / 2) // H; the h = H term is the cell itself
    Q = (np.zeros(nz)[:, None] + np.arange(ni)).astype(np.float32)
    S = ao.stage_sum(Q, 4)
    i = np.arange(ni)
    np.testing.assert_array_equal(S[2], ((i + 2) // 4 + (2 * i + 2) // 4 + (3 * i + 2) // 4 + i))


# ---- the banks, grids and records of the edge cases (tests/test_gpu_accel_edges.py) ----

@pytest.mark.parametrize("n,nfft,zmax,dz,nz,M", [(90, 200, 10, 3, 7, 46), (600, 1024, 7, 1, 15, 34),
                                                 (1144, 4096, 254, 2, 255, 512)])
def test_product_bank_other_dz_and_limits(n, nfft, zmax, dz, nz, M):
    from pypulsar_amd import accel
    t, hw, Mo = ao.taps(n, nfft, zmax, dz)
    taps, hw2, M2 = accel.template_bank(n, nfft, zmax, dz)
    assert Mo == M2 == M and len(hw) == nz and np.array_equal(hw2, hw)
    assert taps.dtype == np.float32 and taps.shape == (nz, 2, 2 * M + 1, 2)
    ref = np.stack((t.real, t.imag), axis=-1)
    err = np.max(np.abs(taps - ref))
    print("bank (%d, %d, %d, %d): max |taps - oracle| = %.3g" % (n, nfft, zmax, dz, err))
    assert err <= 2.0 ** -24  # rounded once (|t| <= 1)
    zs, J0 = accel.z_grid(zmax, dz)
    assert J0 == zmax // dz and np.array_equal(zs, ao.grid(zmax, dz)[0])


def test_bank_and_grid_limits():
    from pypulsar_amd import accel
    # (127 + 16) / (1143 / 4096) = 512.45: a half-width of 513
    assert ao.taps(1143, 4096, 254)[2] == 513
    with pytest.raises(ValueError):
        accel.template_bank(1143, 4096, 254)
    with pytest.raises(ValueError):
        accel.z_grid(256, 2)  # 257 z values
    assert len(accel.z_grid(254, 2)[0]) == 255
    zs, J0 = accel.z_grid(10, 3)
    assert J0 == 3 and np.array_equal(zs, [-9.0, -6.0, -3.0, 0.0, 3.0, 6.0, 9.0])


@pytest.mark.parametrize("dz", [1, 3])
def test_to_records_other_dz(dz):
    from pypulsar_amd import accel
    n, nfft, dt = 3000, 4096, 1e-3
    bits = int(np.float32(30.0).view(np.int32))
    # (row, i, jc, H, bits, 0)
    c = np.asarray([[0, 700, 0, 1, bits, 0], [0, 2102, -2, 3, bits, 0], [1, 2101, 0, 3, bits, 0],
                    [1, 2804, 7, 4, bits, 0], [0, 1401, -8, 2, bits, 0], [1, 1050, -1, 3, bits, 0]],
                   dtype=np.int32)
    recs = accel.to_records(c, [10.0, 20.0], n, nfft, dt, dz)
    want = sorted((int(d), int(H), i / (2.0 * H), jc * dz / float(H)) for d, i, jc, H, _, _ in c)
    assert [(int(r["row"]), int(r["numharm"]), float(r["r"]), float(r["z"])) for r in recs] == want
    zero = recs["z"] == 0
    assert zero.sum() == 2 and not np.any(np.signbit(recs["z"][zero]))  # jc = 0: 0.0, not -0.0
    assert not np.any(np.signbit(recs["zbins"][zero])) and not np.any(np.signbit(recs["fd"][zero]))
    assert np.array_equal(recs["DM"], 10.0 * (recs["row"] + 1))
    T = n * dt
    np.testing.assert_allclose(recs["zbins"], recs["z"] * nfft / n, rtol=1e-15)
    np.testing.assert_allclose(recs["fd"], recs["z"] / (T * T), rtol=1e-15)
    np.testing.assert_allclose(recs["freq"], recs["r"] / (nfft * dt), rtol=1e-15)
    np.testing.assert_allclose(recs["accel"], recs["fd"] * accel.C_LIGHT / recs["freq"], rtol=1e-15)
    assert np.array_equal(np.sign(recs["accel"]), np.sign(recs["z"]))


@pytest.mark.parametrize("H", [5, 7, 16])
def test_stage_sum_against_the_definition(H):
    """S[j][i] = the float32 sum in ascending h of P[J0 + floor((jc h + H // 2)
    / H)][floor((i h + H // 2) / H)], cell by cell with exact fractions."""
    from fractions import Fraction
    from math import floor
    nz, ni, J0 = 3, 41, 1
    P = np.random.default_rng(H).exponential(1.0, (nz, ni)).astype(np.float32)
    S = ao.stage_sum(P, H)
    assert S.dtype == np.float32 and S.shape == (nz, ni)
    for j in range(nz):
        for i in range(ni):
            s = None
            for h in range(1, H + 1):
                v = P[J0 + floor(Fraction((j - J0) * h + H // 2, H)), floor(Fraction(i * h + H // 2, H))]
                s = v if s is None else np.float32(s + v)
            assert s.dtype == np.float32 and S[j, i] == s
    # the floors, for one negative row by hand: jc = -1, H = 7 (H // 2 = 3):
    # floor((3 - h) / 7) = 0 for h <= 3 and -1 beyond
    if H == 7:
        Q = (100.0 * np.arange(nz)[:, None] + np.zeros(ni)).astype(np.float32)
        assert ao.stage_sum(Q, 7)[0, 0] == 3 * 100.0 + 4 * 0.0


def test_float32_correlation_is_within_the_gpu_bar():
    """A plain sequential float32 evaluation of the sums of the largest bank
    (M = 512, nn = 2048) against the float64 plane: the bar of the GPU tests,
    max |P - P_ref| / max P_ref <= 2e-5, leaves a correct kernel about
    tenfold margin."""
    n, nfft = 1144, 4096
    t, hw, M = ao.taps(n, nfft, 254)
    assert M == 512 and (hw[0], hw[127], hw[254]) == (512, 58, 512)
    t = t[[0, 127, 254]]
    rng = np.random.default_rng(5)
    F = ((rng.normal(size=2048) + 1j * rng.normal(size=2048)) / np.sqrt(2.0)).astype(np.complex64)
    ref = ao.plane(F, t, M)
    got = ao.plane_f32(F, t, M)
    assert got.dtype == np.float32
    err = np.max(np.abs(got.astype(np.float64) - ref)) / np.max(ref)
    print("float32 sequential, M = 512: max |P - P_ref| / max P_ref = %.3g" % err)
    assert err <= 2e-5


def test_impulse_plane_is_the_plane_of_an_impulse():
    n, nfft = 90, 200
    t, hw, M = ao.taps(n, nfft, 10, 3)
    F = np.zeros(100, dtype=np.complex128)
    F[[0, 99]] = 1.0
    pairs = np.stack((t.real, t.imag), axis=-1)
    P, support = ao.impulse_plane(pairs, hw, M, 100, (0, 99))
    np.testing.assert_allclose(P, ao.plane(F, t, M), rtol=1e-12, atol=1e-300)
    assert np.all(P[~support] == 0) and np.all(P[support] > 0)
    assert support[3].sum() == 2 * 2 * (hw[3] + 1) and hw[3] == 36
