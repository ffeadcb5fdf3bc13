"""NumPy float64 restatement of the acceleration search (test infrastructure:
no product path imports it; it imports nothing of the product).

Restates, freshly, what pypulsar_amd/accel.py and
pypulsar_amd/csrc/pdd_accel.hip implement:

* ``response_quad`` / ``response``  the response of a signal drifting ``z``
      bins of 1/T over the observation at an offset of ``x`` bins,
      ``W(x; z) = int_0^1 exp(2 pi i [-x v + z (v^2 - v) / 2]) dv``, by midpoint
      quadrature and by its closed form (Fresnel integrals);
* ``interpolate_reference``  PrestoFFT.interpolate (formats/prestofft.py:76-96)
      verbatim -- with its ``np.sinc(pi * d)`` -- and with the sinc corrected;
* ``grid`` / ``taps``  the z grid, the half-widths and the normalised taps;
* ``plane``  ``P[j][i] = |sum_e F[k0 + e] t[j][phi][e]|^2``; ``plane_f32``
      the same sums the plain way in float32; ``impulse_plane``  the plane of
      a row of unit impulses, from given taps;
* ``stage_sum`` / ``candidates``  the harmonic stages on the top harmonic's
      grid (float32, ascending h) and the candidate rule.

Pinned to a fixture made by running the reference (tests/golden/
make_golden_interp.py) by tests/test_accel_oracle.py.
"""
import numpy as np


def response_quad(x, z, N=8192):
    """W(x; z) by the midpoint rule with N points (complex128)."""
    x = np.asarray(x, dtype=np.float64)
    v = (np.arange(N, dtype=np.float64) + 0.5) / N
    ph = -x[..., None] * v + 0.5 * float(z) * (v * v - v)
    return np.exp(2j * np.pi * ph).mean(axis=-1)


def response(x, z):
    """W(x; z) in closed form.  z = 0: exp(-i pi x) sinc(x).  z > 0: with
    q = (x + z / 2) / z the phase is pi z (v - q)^2 - pi z q^2, so with
    u = sqrt(2 z) (v - q)
        W = exp(-i pi z q^2) / sqrt(2 z) * [C(u) + i S(u)] from u(0) to u(1);
    z < 0: W(x; z) = conj(W(-x; -z))."""
    from scipy.special import fresnel
    x = np.asarray(x, dtype=np.float64)
    z = float(z)
    if z == 0.0:
        return np.exp(-1j * np.pi * x) * np.sinc(x)
    if z < 0.0:
        return np.conj(response(-x, -z))
    q = (x + 0.5 * z) / z
    a = np.sqrt(2.0 * z)
    s1, c1 = fresnel(a * (1.0 - q))
    s0, c0 = fresnel(a * (0.0 - q))
    return np.exp(-1j * np.pi * z * q * q) / a * ((c1 - c0) + 1j * (s1 - s0))


def interpolate_reference(fft, r, m=32, corrected=False):
    """PrestoFFT.interpolate restated: the ``m + 1`` coefficients around
    round(r) times exp(-i pi (r - k)) times the sinc term.  The reference
    passes pi (r - k) to np.sinc, which multiplies by pi itself; ``corrected``
    uses np.sinc(r - k), the Fourier interpolation kernel."""
    fft = np.asarray(fft)
    r = np.asarray(r, dtype=np.float64)
    k = np.round(r).astype("int")[:, np.newaxis] + np.arange(-(m // 2), m // 2 + 1)
    d = r[:, np.newaxis] - k
    sincterm = np.sinc(d) if corrected else np.sinc(np.pi * d)
    return np.sum(fft[k] * np.exp(-1.0j * np.pi * d) * sincterm, axis=1)


def grid(zmax, dz=2):
    """(z values float64 [nz], J0): z_j = (j - J0) dz, J0 = zmax // dz."""
    J0 = int(zmax) // int(dz)
    return (np.arange(2 * J0 + 1) - J0) * float(dz), J0


def half_widths(zs, eta):
    return np.asarray([int(np.ceil((abs(z) / 2.0 + 16.0) / eta)) for z in zs], dtype=np.int64)


def taps(n, nfft, zmax, dz=2):
    """(t complex128 [nz][2][2 M + 1], hw [nz], M): t[j][phi][M + e] =
    conj(W(eta (e - phi / 2); z_j)) for |e| <= hw_j, 0 beyond, each (j, phi)
    set scaled to sum |t|^2 = eta."""
    eta = float(n) / float(nfft)
    zs, _ = grid(zmax, dz)
    hw = half_widths(zs, eta)
    M = int(hw.max())
    t = np.zeros((len(zs), 2, 2 * M + 1), dtype=np.complex128)
    for j, z in enumerate(zs):
        e = np.arange(-hw[j], hw[j] + 1, dtype=np.float64)
        for phi in (0, 1):
            w = np.conj(response(eta * (e - 0.5 * phi), z))
            w *= np.sqrt(eta / np.sum(np.abs(w) ** 2))
            t[j, phi, M - hw[j]:M + hw[j] + 1] = w
    return t, hw, M


def plane(F, t, M):
    """F: complex [nn] (one row); returns P float64 [nz][2 nn]."""
    F = np.asarray(F).astype(np.complex128)
    nn = len(F)
    Fp = np.concatenate((np.zeros(M, dtype=np.complex128), F, np.zeros(M, dtype=np.complex128)))
    nz = t.shape[0]
    P = np.empty((nz, 2 * nn), dtype=np.float64)
    for j in range(nz):
        for phi in (0, 1):
            # A[k0] = sum_e Fp[k0 + M + e] t[M + e]: a correlation
            A = np.correlate(Fp, np.conj(t[j, phi]), mode="valid")
            assert len(A) == nn
            P[j, phi::2] = np.abs(A) ** 2
    return P


def plane_f32(F, t, M):
    """``plane`` evaluated the plain way in float32: the taps rounded to
    float32, the sum over e sequential from e = -M, every product and every
    addition rounded (no fused multiply-add).  F: complex64 [nn]; t as from
    ``taps`` (any subset of its z); returns P float32 [nz][2 nn]."""
    F = np.asarray(F).astype(np.complex64)
    nn = len(F)
    z = np.zeros(M, dtype=np.float32)
    fr = np.concatenate((z, F.real.astype(np.float32), z))
    fi = np.concatenate((z, F.imag.astype(np.float32), z))
    tr, ti = t.real.astype(np.float32), t.imag.astype(np.float32)
    P = np.empty((t.shape[0], 2 * nn), dtype=np.float32)
    for j in range(t.shape[0]):
        for phi in (0, 1):
            re = np.zeros(nn, dtype=np.float32)
            im = np.zeros(nn, dtype=np.float32)
            for e in np.flatnonzero((tr[j, phi] != 0) | (ti[j, phi] != 0)):
                a, b = fr[e:e + nn], fi[e:e + nn]
                re = (re + a * tr[j, phi, e]) - b * ti[j, phi, e]
                im = (im + a * ti[j, phi, e]) + b * tr[j, phi, e]
            P[j, phi::2] = re * re + im * im
            assert re.dtype == np.float32
    return P


def impulse_plane(t, hw, M, nn, bins):
    """The plane of a row that is 1 + 0i at ``bins`` and 0 elsewhere, from
    taps given as (re, im) pairs [nz][2][2 M + 1][2] (of any float type; the
    arithmetic is float64): A[j][2 k0 + phi] = sum over the bins k with
    |k - k0| <= hw_j of t[j][phi][M + (k - k0)].  Returns (P float64 [nz][2
    nn], support bool [nz][2 nn]: the positions within hw_j of a bin)."""
    t = np.asarray(t, dtype=np.float64)
    t = t[..., 0] + 1j * t[..., 1]
    nz = t.shape[0]
    A = np.zeros((nz, 2 * nn), dtype=np.complex128)
    support = np.zeros((nz, 2 * nn), dtype=bool)
    for j in range(nz):
        for k in bins:
            k0 = np.arange(max(0, k - int(hw[j])), min(nn, k + int(hw[j]) + 1))
            for phi in (0, 1):
                A[j, 2 * k0 + phi] += t[j, phi, M + (k - k0)]
                support[j, 2 * k0 + phi] = True
    return A.real * A.real + A.imag * A.imag, support


def stage_sum(P, H):
    """S_H of a float32 plane [nz][ni], float32, ascending h from the h = 1
    term: S[j][i] = sum_h P[J0 + floor((jc h + H / 2) / H)][(i h + H / 2) // H]."""
    P = np.asarray(P, dtype=np.float32)
    nz, ni = P.shape
    J0 = (nz - 1) // 2
    H = int(H)
    i = np.arange(ni, dtype=np.int64)
    jc = np.arange(nz, dtype=np.int64) - J0
    S = None
    for h in range(1, H + 1):
        js = J0 + np.floor_divide(jc * h + H // 2, H)  # (floors for negative jc)
        ii = (i * h + H // 2) // H
        term = P[js[:, None], ii[None, :]]
        S = term.copy() if S is None else S + term
        assert S.dtype == np.float32
    return S


def candidates(P, harms, thr, rlo):
    """{(row, i, jc, H, float32 bits of S)} of float32 planes [D][nz][ni]."""
    P = np.asarray(P, dtype=np.float32)
    D, nz, ni = P.shape
    J0 = (nz - 1) // 2
    out = set()
    for d in range(D):
        for H, t in zip(harms, thr):
            H = int(H)
            ilo = 2 * H * int(rlo)
            if ilo >= ni:
                continue
            S = stage_sum(P[d], H)[:, ilo:]
            pad = np.full((nz + 2, S.shape[1] + 2), -np.inf, dtype=np.float32)
            pad[1:-1, 1:-1] = S
            c = pad[1:-1, 1:-1]
            hit = c >= np.float32(t)
            for dj, di in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):
                hit &= c > pad[1 + dj:nz + 1 + dj, 1 + di:S.shape[1] + 1 + di]
            for dj, di in ((0, 1), (1, -1), (1, 0), (1, 1)):
                hit &= c >= pad[1 + dj:nz + 1 + dj, 1 + di:S.shape[1] + 1 + di]
            for j, i in zip(*np.nonzero(hit)):
                out.add((d, int(i) + ilo, int(j) - J0, H, int(S[j, i:i + 1].view(np.int32)[0])))
    return out


# ---- inputs shared by the CPU and GPU tests ----

def chirp_rows(n, nfft, r, z, amp=300.0, nharm=4, seed=0, signal=True, rows=1):
    """float32 rows [rows, n] of integers around 524288 with Gaussian noise of
    sigma 1024 (raw sweep rows) and, in row 0, ``nharm`` equal harmonics of
    amplitude ``amp``: harmonic h has the mid-observation frequency ``h r``
    (bins of the spectrum padded to nfft) and drifts ``h z`` bins of 1 / (n
    dt) over the row."""
    rng = np.random.default_rng(seed)
    x = 524288.0 + rng.normal(0.0, 1024.0, (rows, n))
    if signal:
        t = np.arange(n, dtype=np.float64)
        v = t / n
        for h in range(1, nharm + 1):
            x[0] += amp * np.cos(2 * np.pi * (h * r * t / nfft + 0.5 * h * z * (v * v - v)) + 0.3 * h)
    return np.round(x).astype(np.float32)


def whitened(x, nfft, initialbuflen=6, maxbuflen=200):
    """One row -> the whitened complex64 spectrum of nfft // 2 bins: float64
    mean removed, zero padded, FFT, period_oracle.deredden."""
    import period_oracle as po
    x = np.asarray(x, dtype=np.float64)
    p = np.zeros(nfft, dtype=np.float64)
    p[:len(x)] = (x - x.mean()).astype(np.float32)
    return po.deredden(np.fft.rfft(p)[:nfft // 2].astype(np.complex64), initialbuflen, maxbuflen)
