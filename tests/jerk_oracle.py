"""NumPy float64 restatement of the jerk search (test infrastructure: no
product path imports it; it imports nothing of the product).  Built on
tests/accel_oracle.py.

Restates, freshly, what pypulsar_amd/jerk.py and pypulsar_amd/csrc/pdd_jerk.hip
implement:

* ``response``  the response of a signal of mean drift ``z`` and jerk ``w``
      (bins of 1/T) at an offset of ``x`` bins,
      ``W(x; z, w) = int_0^1 exp(2 pi i [-x v + z (v^2 - v) / 2
                                          + w (v^3 / 6 - v^2 / 4 + v / 12)]) dv``,
      by the composite SIMPSON rule on 16384 equal intervals (the package
      uses Gauss-Legendre panels: another rule and another resolution);
* ``grid`` / ``half_widths`` / ``taps``  the (w, z) grid, the half-widths
      ``ceil((|z| / 2 + |w| / 12 + 16) / eta)`` and the normalised taps;
* ``volume`` / ``volume_f32``  ``accel_oracle.plane`` / ``plane_f32`` of every
      w slab;
* ``stage_sum`` / ``candidates``  the harmonic stages on the top harmonic's
      grid in both template axes (float32, ascending h) and the 26-neighbour
      candidate rule;
* ``jerk_rows``  ``accel_oracle.chirp_rows`` with the cubic phase term.
"""
import numpy as np

import accel_oracle as ao


def response(x, z, w, N=16384, chunk=160):
    """W(x; z, w) by the composite Simpson rule with N intervals (complex128).
    Error: about (Phi' / N)^4 / 180 with Phi' <= 2 pi (|x| + |z| / 2 + |w| /
    12) the largest phase rate: 8e-8 at |x| = 60, z = 100, w = 600."""
    x = np.asarray(x, dtype=np.float64)
    xs = x.ravel()
    v = np.arange(N + 1, dtype=np.float64) / N
    c = np.full(N + 1, 2.0)
    c[1::2] = 4.0
    c[0] = c[-1] = 1.0
    g = (c / (3.0 * N)) * np.exp(2j * np.pi * (0.5 * float(z) * (v * v - v) + float(w) * (
        v ** 3 / 6.0 - v * v / 4.0 + v / 12.0)))
    out = np.empty(len(xs), dtype=np.complex128)
    for a in range(0, len(xs), chunk):
        out[a:a + chunk] = np.exp(-2j * np.pi * xs[a:a + chunk, None] * v[None, :]) @ g
    return out.reshape(x.shape)


def grid(zmax, dz=2, wmax=0, dw=20):
    """(z values [nz], J0, w values [nw], L0)."""
    zs, J0 = ao.grid(zmax, dz)
    L0 = int(wmax) // int(dw)
    return zs, J0, (np.arange(2 * L0 + 1) - L0) * float(dw), L0


def half_widths(zs, ws, eta):
    return np.asarray([[int(np.ceil((abs(z) / 2.0 + abs(w) / 12.0 + 16.0) / eta)) for z in zs]
                       for w in ws], dtype=np.int64)


def taps(n, nfft, zmax, dz=2, wmax=0, dw=20):
    """(t complex128 [nw][nz][2][2 M + 1], hw [nw][nz], M): t[l][j][phi][M + e]
    = conj(W(eta (e - phi / 2); z_j, w_l)) for |e| <= hw_lj, 0 beyond, each set
    scaled to sum |t|^2 = eta.  (w = 0: the closed form of accel_oracle.)"""
    eta = float(n) / float(nfft)
    zs, _, ws, _ = grid(zmax, dz, wmax, dw)
    hw = half_widths(zs, ws, eta)
    M = int(hw.max())
    t = np.zeros((len(ws), len(zs), 2, 2 * M + 1), dtype=np.complex128)
    for l, w in enumerate(ws):
        for j, z in enumerate(zs):
            e = np.arange(-hw[l, j], hw[l, j] + 1, dtype=np.float64)
            xx = eta * np.stack((e, e - 0.5))  # phi = 0, 1
            both = np.conj(ao.response(xx, z) if w == 0 else response(xx, z, w))
            for phi in (0, 1):
                r = both[phi] * np.sqrt(eta / np.sum(np.abs(both[phi]) ** 2))
                t[l, j, phi, M - hw[l, j]:M + hw[l, j] + 1] = r
    return t, hw, M


def volume(F, t, M):
    """F: complex [nn] (one row); returns P float64 [nw][nz][2 nn]."""
    return np.stack([ao.plane(F, t[l], M) for l in range(t.shape[0])])


def volume_f32(F, t, M):
    """``volume`` the plain way in float32 (accel_oracle.plane_f32 per slab)."""
    return np.stack([ao.plane_f32(F, t[l], M) for l in range(t.shape[0])])


def stage_sum(P, H):
    """S_H of a float32 volume [nw][nz][ni], float32, ascending h from the h =
    1 term: S[l][j][i] = sum_h P[L0 + floor((lc h + H / 2) / H)]
    [J0 + floor((jc h + H / 2) / H)][(i h + H / 2) // H]."""
    P = np.asarray(P, dtype=np.float32)
    nw, nz, ni = P.shape
    J0, L0 = (nz - 1) // 2, (nw - 1) // 2
    H = int(H)
    i = np.arange(ni, dtype=np.int64)
    jc = np.arange(nz, dtype=np.int64) - J0
    lc = np.arange(nw, dtype=np.int64) - L0
    S = None
    for h in range(1, H + 1):
        ls = L0 + np.floor_divide(lc * h + H // 2, H)  # (floors for negative lc, jc)
        js = J0 + np.floor_divide(jc * h + H // 2, H)
        ii = (i * h + H // 2) // H
        term = P[ls[:, None, None], js[None, :, None], ii[None, None, :]]
        S = term.copy() if S is None else S + term
        assert S.dtype == np.float32
    return S


_OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if (a, b, c) != (0, 0, 0)]


def candidates(P, harms, thr, rlo):
    """{(row, i, jc, lc, H, float32 bits of S)} of float32 volumes
    [nw][D][nz][ni]: S >= thr, > the 13 neighbours before the cell in (l, j, i)
    order, >= the 13 after; outside [0, nw) x [0, nz) x [2 H rlo, ni): -inf."""
    P = np.asarray(P, dtype=np.float32)
    nw, D, nz, ni = P.shape
    J0, L0 = (nz - 1) // 2, (nw - 1) // 2
    out = set()
    for d in range(D):
        for H, t in zip(harms, thr):
            H = int(H)
            ilo = 2 * H * int(rlo)
            if ilo >= ni:
                continue
            S = stage_sum(P[:, d], H)[:, :, ilo:]
            m = S.shape[2]
            pad = np.full((nw + 2, nz + 2, m + 2), -np.inf, dtype=np.float32)
            pad[1:-1, 1:-1, 1:-1] = S
            hit = S >= np.float32(t)
            for dl, dj, di in _OFFSETS:
                nb = pad[1 + dl:nw + 1 + dl, 1 + dj:nz + 1 + dj, 1 + di:m + 1 + di]
                hit &= (S > nb) if (dl, dj, di) < (0, 0, 0) else (S >= nb)
            for l, j, i in zip(*np.nonzero(hit)):
                out.add((d, int(i) + ilo, int(j) - J0, int(l) - L0, H,
                         int(S[l, j, i:i + 1].view(np.int32)[0])))
    return out


# ---- inputs shared by the CPU and GPU tests ----

def jerk_rows(n, nfft, r, z, w, amp=300.0, nharm=4, seed=0, signal=True, rows=1):
    """accel_oracle.chirp_rows with a jerk: harmonic h has the mid-observation
    frequency ``h r`` (bins of the spectrum padded to nfft), the mean drift ``h
    z`` and the jerk ``h w`` (bins of 1 / (n dt))."""
    rng = np.random.default_rng(seed)
    x = 524288.0 + rng.normal(0.0, 1024.0, (rows, n))
    if signal:
        t = np.arange(n, dtype=np.float64)
        v = t / n
        for h in range(1, nharm + 1):
            ph = h * r * t / nfft + 0.5 * h * z * (v * v - v) + h * w * (
                v ** 3 / 6.0 - v * v / 4.0 + v / 12.0)
            x[0] += amp * np.cos(2 * np.pi * ph + 0.3 * h)
    return np.round(x).astype(np.float32)


def tone_spectrum(n, nfft, r, z, w):
    """The noise-free complex spectrum [nfft // 2] of exp(i phase) with
    frequency r (bins of the padded spectrum), drift z and jerk w over n
    samples, scaled to unit power at its own template."""
    t = np.arange(n, dtype=np.float64)
    v = t / n
    ph = r * t / nfft + 0.5 * z * (v * v - v) + w * (v ** 3 / 6.0 - v * v / 4.0 + v / 12.0)
    x = np.zeros(nfft, dtype=np.complex128)
    x[:n] = np.exp(2j * np.pi * ph)
    return np.fft.fft(x)[:nfft // 2] / n
