"""NumPy restatement of the sideband search (test infrastructure: no product
path imports it; it imports nothing of the product).

Restates, freshly, what pypulsar_amd/sideband.py and
pypulsar_amd/csrc/pdd_sideband.hip implement:

* ``segments``    the starts ``lo_j = rlo + j stride`` of the mini-FFT
                  segments of a row of ``nn`` bins (``stride = L >> shift``);
* ``mini``        the normalised half-bin mini spectrum ``M[0..L)`` of every
                  segment, in float64 from float32 powers;
* ``candidates``  the stage sums (float32, ascending harmonic) and the
                  local-maximum rule on float32 ``M``.
"""
import numpy as np

INTERBIN = np.pi ** 2 / 16.0


def segments(nn, rlo, L, shift=2):
    """int64 starts of the segments of length ``L``: none when ``nn - rlo <
    L``, else ``(nn - rlo - L) // stride + 1`` of them, ``stride`` apart."""
    nn, rlo, L = int(nn), int(rlo), int(L)
    stride = L >> int(shift)
    if nn - rlo < L:
        return np.empty(0, dtype=np.int64)
    nseg = (nn - rlo - L) // stride + 1
    return rlo + stride * np.arange(nseg, dtype=np.int64)


def mini(powers, rlo, L, shift=2, clip=0.0):
    """float64 [nseg, L] of one row of float32 powers: ``M[2k] = L |A_k|^2 /
    A_0^2``, ``M[2k+1] = (pi^2 / 16) L |A_k - A_{k+1}|^2 / A_0^2`` with ``A``
    the spectrum of the segment clipped at ``clip`` (> 0); all 0 where ``A_0
    <= 0``."""
    p = np.asarray(powers, dtype=np.float32)
    assert p.ndim == 1
    los = segments(len(p), rlo, L, shift)
    out = np.zeros((len(los), L), dtype=np.float64)
    for j, lo in enumerate(los):
        x = p[lo:lo + L].astype(np.float64)
        if clip > 0:
            x = np.minimum(x, np.float64(np.float32(clip)))
        A = np.fft.rfft(x)  # k = 0 .. L/2
        a0 = A[0].real
        if not a0 > 0:
            continue
        out[j, 0::2] = L * np.abs(A[:-1]) ** 2 / a0 ** 2
        out[j, 1::2] = INTERBIN * L * np.abs(A[:-1] - A[1:]) ** 2 / a0 ** 2
    return out


def stage_sum(M, H):
    """S_H[q] = sum_{h=1..H} M[h q], q < L // H; float32, ascending h."""
    M = np.asarray(M, dtype=np.float32)
    nout = len(M) // H
    s = M[:nout].copy()
    for h in range(2, H + 1):
        s += M[0:h * nout:h]
    return s


def candidates(M, harms, thr, qlo=4):
    """{(seg, q, H, float32 bits of S_H[q])} of float32 ``M`` [nseg, L]: q of
    [qlo, L // H) with S_H[q] >= thr[H's index], > S_H[q-1] and >= S_H[q+1];
    neighbours outside the range count as -inf."""
    M = np.asarray(M, dtype=np.float32)
    assert M.ndim == 2
    out = set()
    for H, t in zip(harms, thr):
        H = int(H)
        nout = M.shape[1] // H
        if nout <= qlo or not len(M):
            continue
        # stage_sum of every segment at once (the same float32 additions)
        s = M[:, :nout].copy()
        for h in range(2, H + 1):
            s += M[:, 0:h * nout:h]
        s = s[:, qlo:]
        edge = np.full((len(s), 1), -np.inf, dtype=np.float32)
        left = np.concatenate((edge, s[:, :-1]), axis=1)
        right = np.concatenate((s[:, 1:], edge), axis=1)
        hit = (s >= np.float32(t)) & (s > left) & (s >= right)
        for j, i in np.argwhere(hit):
            out.add((int(j), int(i) + qlo, H, int(s[j, i:i + 1].view(np.int32)[0])))
    return out
