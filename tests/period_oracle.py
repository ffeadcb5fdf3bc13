"""NumPy restatement of the periodicity search (test infrastructure: no
product path imports it; it imports nothing of the product).

Restates, freshly, what pypulsar_amd/periodicity.py and
pypulsar_amd/csrc/pdd_period.hip implement:

* ``table``         the whitening blocks of PrestoFFT.deredden
                    (formats/prestofft.py:157-191);
* ``deredden``      that method's result from a complex64 spectrum (float64
                    lines between block medians, complex64 result);
* ``harmonic_sum``  PrestoFFT.harmonic_sum (:98-113) with py2's integer
                    divisions, float32 ``+=`` in ascending harmonic;
* ``candidates``    the local-maximum rule of pdd_ps_search on float32
                    harmonic sums;
* ``sigma`` / ``threshold_power``  the single-trial significance
                    ``norm.isf(chi2.sf(2 S, 2 H))`` and its inverse.

Pinned to fixtures made by running the reference (tests/golden/
make_golden_period.py) by tests/test_period_oracle.py.
"""
import numpy as np

LN2 = np.log(2.0)


def table(nn, initialbuflen=6, maxbuflen=200):
    offs, lens = [], []
    off, ln = 1, initialbuflen
    nxt_off = off + ln
    nxt_len = maxbuflen if nxt_off > maxbuflen else int(initialbuflen * np.log(nxt_off))
    offs.append(off)
    lens.append(ln)
    while nxt_off + nxt_len < nn:
        offs.append(nxt_off)
        lens.append(nxt_len)
        nxt_off += nxt_len
        nxt_len = min(int(initialbuflen * np.log(nxt_off)), maxbuflen)
    return np.asarray(offs, dtype=np.int32), np.asarray(lens, dtype=np.int32)


def medians(powers, offs, lens):
    """Block levels: np.median of each block / ln 2 (float64)."""
    return np.asarray([np.median(powers[o:o + n]) / LN2 for o, n in zip(offs, lens)],
                      dtype=np.float64)


def linevals(med, offs, lens, nn):
    """The whitening level of every bin >= 1 (float64; entry 0 unused)."""
    line = np.ones(nn, dtype=np.float64)
    B = len(offs)
    assert B >= 2
    for j in range(B - 1):
        tot = float(lens[j] + lens[j + 1])
        slope = (med[j + 1] - med[j]) / tot
        line[offs[j]:offs[j] + lens[j]] = med[j] + slope * (0.5 * tot - np.arange(lens[j]))
    line[offs[B - 1]:] = line[offs[B - 1] - 1]
    return line


def deredden(fft, initialbuflen=6, maxbuflen=200):
    """complex64 spectrum -> complex64 whitened spectrum (bin 0 = 1 + 0j)."""
    fft = np.asarray(fft, dtype=np.complex64)
    nn = len(fft)
    powers = np.abs(fft) ** 2
    offs, lens = table(nn, initialbuflen, maxbuflen)
    line = linevals(medians(powers, offs, lens), offs, lens, nn)
    out = fft.astype(np.complex128)
    out[1:] *= 1.0 / np.sqrt(line[1:])
    out[0] = 1.0
    return out.astype(np.complex64)


def harmonic_sum(powers, nharm):
    """S_H[k] = sum_{h=1..H} P[h k], k < nn // H; float32, ascending h."""
    powers = np.asarray(powers, dtype=np.float32)
    nout = len(powers) // nharm
    s = powers[:nout].copy()
    for h in range(2, nharm + 1):
        s += powers[0:h * nout:h]
    return s


def candidates(powers, harms, thr, rlo):
    """{(row, k, H, float32 bits of S_H[k])} of float32 powers [D, nn]: bin k
    of [rlo, nn // H) with S_H[k] >= thr[H's index], > S_H[k-1] and >=
    S_H[k+1]; neighbours outside the range count as -inf."""
    powers = np.asarray(powers, dtype=np.float32)
    out = set()
    for d in range(powers.shape[0]):
        for H, t in zip(harms, thr):
            s = harmonic_sum(powers[d], int(H))[rlo:]
            if len(s) == 0:
                continue
            left = np.concatenate(([-np.inf], s[:-1])).astype(np.float32)
            right = np.concatenate((s[1:], [-np.inf])).astype(np.float32)
            hit = (s >= np.float32(t)) & (s > left) & (s >= right)
            for i in np.flatnonzero(hit):
                out.add((d, int(i) + rlo, int(H), int(s[i:i + 1].view(np.int32)[0])))
    return out


def sigma(S, H):
    """norm.isf(chi2.sf(2 S, 2 H)); where the probability underflows, the x
    with norm.logsf(x) == chi2.logsf(2 S, 2 H) by bisection."""
    from scipy.stats import chi2, norm
    S = float(S)
    p = chi2.sf(2.0 * S, 2 * H)
    if p > 1e-280:
        return float(norm.isf(p))
    # ln Q(H, S) = -S + ln sum_{j<H} S^j / j!, summed from the largest term
    j = np.arange(H, dtype=np.float64)
    from scipy.special import gammaln
    t = j * np.log(S) - gammaln(j + 1)
    logp = -S + t.max() + np.log(np.sum(np.exp(t - t.max())))
    lo, hi = 0.0, 1e4
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if norm.logsf(mid) > logp:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def threshold_power(sig, H):
    """S with sigma(S, H) == sig (for probabilities chi2.isf represents)."""
    from scipy.stats import chi2, norm
    return 0.5 * float(chi2.isf(norm.sf(sig), 2 * H))
