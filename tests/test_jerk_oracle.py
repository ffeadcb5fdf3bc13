"""The jerk search on the host: the product's response (pypulsar_amd/jerk.py,
Gauss-Legendre panels) against the oracle's (tests/jerk_oracle.py, composite
Simpson) and the Fresnel closed form, its symmetries, the template bank, a
noise-free tone and the oracle's own stage and candidate rules.  CPU only."""
import numpy as np
import pytest

import accel_oracle as ao
import jerk_oracle as jo

ZW = ((0, 0), (2, 0), (-37, 0), (50, 0), (6, 40), (-8, 100), (100, 600))
X = np.arange(-240, 241) / 4.0  # |x| <= 60 in quarter bins


@pytest.mark.parametrize("z,w", ZW)
def test_response_vs_independent_rule(z, w):
    from pypulsar_amd import accel, jerk
    got = jerk.w_response(X, z, w)
    assert got.dtype == np.complex128 and got.shape == X.shape
    err = np.max(np.abs(got - jo.response(X, z, w)))
    print("(z, w) = (%d, %d): Gauss-Legendre - Simpson(16384): max abs %.3g" % (z, w, err))
    assert err <= 1e-6
    if w == 0:
        # the package's quadrature (not only its w = 0 shortcut) and the closed forms
        quad = jerk._responses(X, [(float(z), 0.0)])[0]
        e2 = np.max(np.abs(quad - accel.z_response(X, z)))
        e3 = np.max(np.abs(got - ao.response(X, z)))
        print("    w = 0: quadrature - z_response %.3g; w_response - oracle closed form %.3g"
              % (e2, e3))
        assert e2 <= 1e-6 and e3 <= 1e-6


@pytest.mark.parametrize("z,w", [(6, 40), (-8, 100), (100, 600), (3, -20)])
def test_response_symmetries(z, w):
    from pypulsar_amd import jerk
    a = jerk.w_response(X, z, w)
    b = jerk.w_response(-X, z, w)
    e1 = np.max(np.abs(jerk.w_response(X, -z, -w) - np.conj(b)))
    e2 = np.max(np.abs(jerk.w_response(X, z, -w) - np.exp(-2j * np.pi * X) * b))
    print("(z, w) = (%d, %d): symmetries to %.3g, %.3g" % (z, w, e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert np.max(np.abs(a)) <= 1.0 + 1e-12


@pytest.mark.parametrize("n,nfft", [(3000, 4096), (4096, 4096), (4700, 5000)])
def test_bank(n, nfft):
    from pypulsar_amd import accel, jerk
    eta = n / float(nfft)
    zmax, wmax = 8, 40
    taps, hw, M = jerk.template_bank(n, nfft, zmax, 2, wmax, 20)
    zs, J0, ws, L0 = jo.grid(zmax, 2, wmax, 20)
    assert (len(ws), len(zs), L0, J0) == (5, 9, 2, 4)
    assert taps.dtype == np.float32 and taps.shape == (5, 9, 2, 2 * M + 1, 2)
    assert hw.dtype == np.int32 and hw.shape == (5, 9) and M == hw.max()
    want_hw = jo.half_widths(zs, ws, eta)
    assert np.array_equal(hw, want_hw)
    assert hw[0, 0] == int(np.ceil((4.0 + 40.0 / 12.0 + 16.0) / eta))
    # sum |t|^2 = eta to float32 rounding (every tap rounded once: 2^-24 relative)
    s = np.sum(taps.astype(np.float64) ** 2, axis=(3, 4))
    assert np.max(np.abs(s - eta)) <= 4 * 2.0 ** -24 * eta
    for l in range(5):
        for j in range(9):  # zero beyond the half-width
            assert np.all(taps[l, j, :, :M - hw[l, j]] == 0)
            assert np.all(taps[l, j, :, M + hw[l, j] + 1:] == 0)
    # the w = 0 slab is the acceleration search's bank, bit for bit
    t0, hw0, M0 = accel.template_bank(n, nfft, zmax, 2)
    assert np.array_equal(hw0, hw[L0])
    np.testing.assert_array_equal(taps[L0, :, :, M - M0:M + M0 + 1].view(np.int32),
                                  t0.view(np.int32))
    assert np.all(taps[L0, :, :, :M - M0] == 0) and np.all(taps[L0, :, :, M + M0 + 1:] == 0)
    # against the oracle's taps (Simpson), rounded once
    t, hw2, M2 = jo.taps(n, nfft, zmax, 2, wmax, 20)
    assert M2 == M
    ref = np.stack((t.real, t.imag), axis=-1)
    assert np.max(np.abs(taps - ref)) <= 2.0 ** -24 + 1e-6
    # wmax = 0: the acceleration search's bank with a leading axis of 1
    t1, hw1, M1 = jerk.template_bank(n, nfft, zmax, 2, 0, 20)
    assert t1.shape == (1,) + t0.shape and M1 == M0
    np.testing.assert_array_equal(t1[0].view(np.int32), t0.view(np.int32))


def test_bank_limits():
    from pypulsar_amd import jerk
    with pytest.raises(ValueError):  # M = ceil((100 + 50 + 16) / 0.244) > 512
        jerk.template_bank(1000, 4096, 200, 2, 600, 20)
    with pytest.raises(ValueError):  # 65 w trials
        jerk.w_grid(640, 20)
    ws, L0 = jerk.w_grid(100, 20)
    assert L0 == 5 and np.array_equal(ws, np.arange(-100, 101, 20))
    ws, L0 = jerk.w_grid(0)
    assert L0 == 0 and np.array_equal(ws, [0.0])


def _tone_power(F, rr, z, w, eta, resp):
    """|sum_k F[k] t(k)|^2 with t = conj(W(eta (k - rr); z, w)) over the
    bank's support around round(rr), scaled to sum |t|^2 = eta."""
    hw = int(np.ceil((abs(z) / 2.0 + abs(w) / 12.0 + 16.0) / eta))
    k = int(np.round(rr)) + np.arange(-hw, hw + 1)
    t = np.conj(resp(eta * (k - rr), z, w))
    t *= np.sqrt(eta / np.sum(np.abs(t) ** 2))
    return float(np.abs(np.sum(F[k] * t)) ** 2)


def test_noise_free_tone():
    """A tone of (r, z, w) = (300.3, 6, 40) peaks at its own template, and no
    w = 0 template within r +- 6 (steps of 0.25) and z +- 12 (steps of 1)
    reaches 0.7 of it."""
    from pypulsar_amd import accel, jerk
    n, nfft, r, z, w = 2048, 4096, 300.3, 6.0, 40.0
    eta = n / float(nfft)
    F = jo.tone_spectrum(n, nfft, r, z, w)
    own = _tone_power(F, r, z, w, eta, jerk.w_response)
    print("own template: %.4f of the tone's power (support of the bank)" % own)
    assert 0.97 <= own <= 1.0 + 1e-9  # (the energy inside the support)
    for dr in (-0.25, 0.0, 0.25):
        for dz in (-1.0, 0.0, 1.0):
            for dw in (-20.0, 0.0, 20.0):
                if (dr, dz, dw) != (0.0, 0.0, 0.0):
                    p = _tone_power(F, r + dr, z + dz, w + dw, eta, jerk.w_response)
                    assert p < own, (dr, dz, dw, p / own)
    side = [_tone_power(F, r, z, ww, eta, jerk.w_response) / own for ww in (20.0, 60.0)]
    print("w = 20, 60 at the tone's own (r, z), not scanned: %.3f, %.3f of it" % tuple(side))
    best = 0.0
    zr = lambda x, zz, ww: accel.z_response(x, zz)  # noqa: E731
    for zz in np.arange(z - 12.0, z + 12.5, 1.0):
        for rr in np.arange(r - 6.0, r + 6.01, 0.25):
            best = max(best, _tone_power(F, rr, zz, 0.0, eta, zr))
    print("best w = 0 template: %.3f of it" % (best / own))
    assert best / own <= 0.7


def test_oracle_stage_sum_small():
    """stage_sum by hand on a tiny volume: floors in both template axes."""
    rng = np.random.default_rng(3)
    P = rng.integers(0, 9, (3, 5, 24)).astype(np.float32)
    for H in (1, 2, 3):
        S = jo.stage_sum(P, H)
        for l in range(3):
            for j in range(5):
                for i in range(24):
                    want = np.float32(0)
                    for h in range(1, H + 1):
                        ll = 1 + int(np.floor(((l - 1) * h + H // 2) / float(H)))
                        jj = 2 + int(np.floor(((j - 2) * h + H // 2) / float(H)))
                        want = np.float32(want + P[ll, jj, (i * h + H // 2) // H])
                    assert S[l, j, i] == want, (H, l, j, i)
    # nw = 1: the acceleration oracle's
    np.testing.assert_array_equal(jo.stage_sum(P[1:2], 3)[0], ao.stage_sum(P[1], 3))


def test_oracle_candidates_plateaus():
    """Plateaus across l, j and i on a hand-made volume: exactly the first
    cell of each in (l, j, i) order is reported."""
    P = np.zeros((3, 1, 5, 40), dtype=np.float32)
    P[0, 0, 1, 10] = P[1, 0, 1, 10] = 9.0   # across l
    P[1, 0, 3, 20] = P[1, 0, 4, 20] = 8.0   # across j
    P[2, 0, 2, 30] = P[2, 0, 2, 31] = 7.0   # across i
    P[0, 0, 0, 39] = 6.0                    # a corner of the volume
    P[2, 0, 4, 2] = 5.0                     # the first searched position (rlo = 1)
    P[2, 0, 3, 1] = 50.0                    # below the searched range: not seen
    P[0, 0, 3, 5] = P[1, 0, 4, 6] = 4.0     # across a diagonal of l, j and i
    got = jo.candidates(P, (1,), (3.0,), 1)
    b = lambda v: int(np.float32(v).view(np.int32))  # noqa: E731
    assert got == {(0, 10, -1, -1, 1, b(9.0)), (0, 20, 1, 0, 1, b(8.0)),
                   (0, 30, 0, 1, 1, b(7.0)), (0, 39, -2, -1, 1, b(6.0)),
                   (0, 2, 2, 1, 1, b(5.0)), (0, 5, 1, -1, 1, b(4.0))}
    # nw = 1: the acceleration oracle's rule
    rng = np.random.default_rng(5)
    Q = rng.integers(0, 4, (1, 2, 7, 300)).astype(np.float32)
    want = {(d, i, jc, 0, H, s) for d, i, jc, H, s in ao.candidates(Q[0], (1, 2), (2.0, 3.0), 1)}
    assert len(want) > 20
    assert jo.candidates(Q, (1, 2), (2.0, 3.0), 1) == want
