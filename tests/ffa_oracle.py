"""NumPy restatement of the fast-folding (FFA) search (include/pdd.h, the
pdd_ffa_* entry points): the plan, downsampling and detrending, the radix-2
fast-folding butterfly in integer index arithmetic, the matched boxcar score
and the candidate rule.  Imports nothing from the product."""
import math

import numpy as np

DEFAULT_WIDTHS = (1, 2, 3, 4, 6, 9, 13, 19, 28, 42)


# ---- plan ----

def ffa_plan(n, dt, period_min, period_max, bins_min=250, bins_max=500):
    """[(f, b_lo, b_hi)]: the step searches base periods b_lo .. b_hi - 1 bins
    on the series downsampled by f."""
    n, bins_min, bins_max = int(n), int(bins_min), int(bins_max)
    if not (8 <= bins_min and 2 * bins_min <= bins_max <= 1024):
        raise ValueError("need 8 <= bins_min, 2 bins_min <= bins_max <= 1024")
    if not (period_min >= bins_min * dt and period_max > period_min):
        raise ValueError("need bins_min * dt <= period_min < period_max")
    steps, P = [], float(period_min)
    while P < period_max:
        f = max(1, int(math.floor(P / (bins_min * dt))))
        dts = f * dt
        b_lo = int(math.floor(P / dts))
        b_hi = min(bins_max, int(math.ceil(period_max / dts)))
        if b_hi <= b_lo:
            break  # (rounding at the very end of the range)
        if n // f < 2 * b_hi:
            raise ValueError("series of %d samples too short for a period of %g s"
                             % (n, b_hi * dts))
        steps.append((f, b_lo, b_hi))
        P = b_hi * dts
    return steps


def mp_of(M):
    """max(2, next power of two >= M)."""
    return max(2, 1 << int(M - 1).bit_length())


def chunk_len(detrend, dts, bins_max):
    return max(2 * int(bins_max), int(math.ceil(detrend / dts)))


def trial_table(n, dt, plan):
    """(period, p0, s, f, M) arrays of a row's trial axis."""
    per, p0s, ss, fs, Ms = [], [], [], [], []
    for f, b_lo, b_hi in plan:
        n_ds, dts = n // f, f * dt
        for p0 in range(b_lo, b_hi):
            M = n_ds // p0
            Mp = mp_of(M)
            s = np.arange(Mp - 1)
            per.append((p0 + s / float(Mp - 1)) * dts)
            p0s.append(np.full(Mp - 1, p0))
            ss.append(s)
            fs.append(np.full(Mp - 1, f))
            Ms.append(np.full(Mp - 1, M))
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.empty(0, t)  # noqa: E731
    return cat(per, np.float64), cat(p0s, np.int64), cat(ss, np.int64), cat(fs, np.int64), \
        cat(Ms, np.int64)


# ---- prepare ----

def downsample(x, f):
    """y[i] = x[f i] + .. + x[f i + f - 1], float32, ascending."""
    x = np.asarray(x, dtype=np.float32)
    n_ds = x.shape[-1] // f
    y = x[..., 0:n_ds * f:f].copy()
    for q in range(1, f):
        y = y + x[..., q:n_ds * f:f]
    return y


def baseline(y, L):
    """float64 base(i) of one row: the line between the chunk means."""
    n_ds = len(y)
    nchunk = max(1, n_ds // L)
    starts = np.arange(nchunk) * L
    ends = np.append(starts[1:], n_ds)
    means = np.asarray([np.mean(y[a:b].astype(np.float64)) for a, b in zip(starts, ends)])
    ctr = starts + 0.5 * (ends - starts - 1)
    i = np.arange(n_ds, dtype=np.float64)
    base = np.empty(n_ds, dtype=np.float64)
    base[i < ctr[0]] = means[0]
    base[i >= ctr[-1]] = means[-1]
    for c in range(nchunk - 1):
        m = (i >= ctr[c]) & (i < ctr[c + 1])
        base[m] = means[c] + (means[c + 1] - means[c]) * ((i[m] - ctr[c]) / (ctr[c + 1] - ctr[c]))
    return base


def prep(x, f, L):
    """(y' float32 [D, n_ds], sigma float64 [D]) of rows x [D, n]."""
    y = downsample(np.atleast_2d(x), f)
    yp = np.empty_like(y)
    sig = np.empty(len(y), dtype=np.float64)
    for d in range(len(y)):
        yp[d] = (y[d].astype(np.float64) - baseline(y[d], L)).astype(np.float32)
        v = yp[d].astype(np.float64)
        var = np.sum(v * v) / len(v) - (np.sum(v) / len(v)) ** 2
        sig[d] = math.sqrt(var) if var > 0.0 else 0.0
    return yp, sig


# ---- transform ----

def butterfly(rows):
    """[Mp, p0] float32 rows (Mp a power of two) -> [Mp, p0] trial profiles:
    merging transformed half blocks head, tail of m / 2 rows,
    out[s][b] = head[s >> 1][b] + tail[s >> 1][(b + ((s + 1) >> 1)) mod p0]."""
    x = np.asarray(rows, dtype=np.float32)
    Mp, p0 = x.shape
    assert Mp >= 1 and Mp & (Mp - 1) == 0
    blocks = x.reshape(Mp, 1, p0)
    b = np.arange(p0)
    m = 1
    while m < Mp:
        m *= 2
        head, tail = blocks[0::2], blocks[1::2]
        s = np.arange(m)
        idx = (b[None, :] + ((s + 1) >> 1)[:, None]) % p0          # [m, p0]
        h = head[:, s >> 1, :]
        t = np.take_along_axis(tail[:, s >> 1, :], np.broadcast_to(idx, h.shape), axis=2)
        blocks = h + t                                              # float32, head + tail
    return blocks[0]


def butterfly_recursive(rows):
    """The definition, literally (slow; for the tests)."""
    x = np.asarray(rows, dtype=np.float32)
    m, p0 = x.shape
    if m == 1:
        return x.copy()
    head, tail = butterfly_recursive(x[:m // 2]), butterfly_recursive(x[m // 2:])
    out = np.empty_like(x)
    for s in range(m):
        out[s] = head[s >> 1] + np.roll(tail[s >> 1], -((s + 1) >> 1))
    return out


def shift(s, r, m):
    """Bins by which row r of m is advanced in trial s (the closed form of the
    recursion)."""
    if m == 1:
        return 0
    if r < m // 2:
        return shift(s >> 1, r, m // 2)
    return ((s + 1) >> 1) + shift(s >> 1, r - m // 2, m // 2)


def direct(rows, s):
    """sum_r roll(x[r], -shift(s, r)) (float64: a check of the index algebra)."""
    x = np.asarray(rows, dtype=np.float64)
    m = len(x)
    return sum(np.roll(x[r], -shift(s, r, m)) for r in range(m))


def transform(yprime, p0):
    """[Mp, p0] profiles of one row and base period."""
    y = np.asarray(yprime, dtype=np.float32)
    M = len(y) // p0
    Mp = mp_of(M)
    rows = np.zeros((Mp, p0), dtype=np.float32)
    rows[:M] = y[:M * p0].reshape(M, p0)
    return butterfly(rows)


# ---- score ----

def boxcar_snr(prof, M, sigma, widths=DEFAULT_WIDTHS, ducy_max=0.2):
    """snr_w float64 [nw_admitted, T] of profiles [T, b]."""
    x = np.asarray(prof, dtype=np.float32)
    T_, b = x.shape
    P = np.cumsum(x, axis=1, dtype=np.float32)
    c = np.concatenate([np.zeros((T_, 1), np.float32), P], axis=1)   # c[i] = x[0] + .. + x[i-1]
    tot = P[:, -1]
    wmax = max(1, int(math.floor(ducy_max * float(b))))
    b0 = np.arange(b)
    out = []
    for w in widths:
        if w > wmax or w >= b:
            break
        e = b0 + w
        inside = c[:, np.minimum(e, b)] - c[:, b0]
        wrapped = (tot[:, None] - c[:, b0]) + c[:, np.maximum(e - b, 0)]
        S = np.where(e[None, :] <= b, inside, wrapped).astype(np.float32).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append((S.astype(np.float64) - float(w) * tot.astype(np.float64) / float(b)) /
                       (sigma * math.sqrt(float(M) * float(w) * (1.0 - float(w) / float(b)))))
    return np.asarray(out, dtype=np.float64).reshape(len(out), T_)


def score(prof, M, sigma, widths=DEFAULT_WIDTHS, ducy_max=0.2):
    """(snr float32 [T], width index uint8 [T], runner-up margin float64 [T])
    of profiles [T, b]; margin: (best - second best) / |best| (inf with one
    width)."""
    T_ = len(prof)
    if not sigma > 0.0:
        return np.zeros(T_, np.float32), np.zeros(T_, np.uint8), np.full(T_, np.inf)
    sw = boxcar_snr(prof, M, sigma, widths, ducy_max)
    if not len(sw):
        return np.zeros(T_, np.float32), np.zeros(T_, np.uint8), np.full(T_, np.inf)
    wi = np.argmax(sw, axis=0)            # (the first, narrower, on ties)
    best = sw[wi, np.arange(T_)]
    if len(sw) > 1:
        rest = sw.copy()
        rest[wi, np.arange(T_)] = -np.inf
        margin = (best - rest.max(axis=0)) / np.maximum(np.abs(best), 1e-300)
    else:
        margin = np.full(T_, np.inf)
    return best.astype(np.float32), wi.astype(np.uint8), margin


def periodogram(x, dt, plan, widths=DEFAULT_WIDTHS, ducy_max=0.2, detrend=1.0, bins_max=500):
    """(snr float32 [D, ntrial], width index uint8, margin float64) of rows x."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    snr, wid, mar = [], [], []
    for f, b_lo, b_hi in plan:
        yp, sig = prep(x, f, chunk_len(detrend, f * dt, bins_max))
        for p0 in range(b_lo, b_hi):
            M = yp.shape[1] // p0
            rs, rw, rm = [], [], []
            for d in range(len(yp)):
                a, b, c = score(transform(yp[d], p0)[:-1], M, sig[d], widths, ducy_max)
                rs.append(a), rw.append(b), rm.append(c)
            snr.append(np.asarray(rs)), wid.append(np.asarray(rw)), mar.append(np.asarray(rm))
    return np.concatenate(snr, axis=1), np.concatenate(wid, axis=1), np.concatenate(mar, axis=1)


# ---- candidates ----

def candidates(snr, threshold):
    """{(row, k)}: snr[k] >= threshold, > snr[k-1], >= snr[k+1] (missing
    neighbours: -inf)."""
    snr = np.atleast_2d(np.asarray(snr, dtype=np.float32))
    D, nt = snr.shape
    pad = np.full((D, 1), -np.inf, dtype=np.float32)
    left = np.concatenate([pad, snr[:, :-1]], axis=1)
    right = np.concatenate([snr[:, 1:], pad], axis=1)
    hit = (snr >= np.float32(threshold)) & (snr > left) & (snr >= right)
    return {(int(d), int(k)) for d, k in zip(*np.nonzero(hit))}
