"""Single-pulse search (pdd_search.hip: k_sp_stats, k_sp_search) on the paths
and inputs test_gpu_search.py leaves out: every dispatch branch of the two
kernels, rows shaped like a sweep plane (a large offset under the noise),
outliers at a chunk's first sample, exact ties, views with hostile
neighbours, the start limit and the continuation called directly, a
zero-variance chunk inside a live row, and overflow accounting.

Reference: the float64 oracle (oracle/search_oracle.py).  Comparison rule:
search_check.check (S/N within 1e-4 max(1, |s|); (start, width) exact unless
the oracle's margin is a near-tie; one-sided candidates only at the
threshold).  So that the rule cannot hide a failure, every case that uses it
needs at least 5 oracle candidates and at most 10 % of its compared windows
excused (_verdict).  The seeds were chosen by running the oracle alone on the
CPU; the candidate / excused counts they gave are listed with each case.

Plane-like rows sit at BASE = 524288 (a u8 sweep over 4096 channels x 128)
and are integer valued.  There x - mean is exact in f32 but the stored f32
mean is rounded to ulp(BASE)/2 = 1/32, so a boxcar of w samples carries an
S/N error up to sqrt(w) / (32 sigma): that term is stated as its own addend
(_plane_extra) wherever such rows are searched."""
import functools

import numpy as np
import pytest

from oracle import search_oracle as so
from search_check import check

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 3, 4, 6, 9, 14, 20, 30, 45, 70, 100, 150)
BASE = 524288.0
ULP_BASE = float(np.spacing(np.float32(BASE)))  # 1/16


# ---------------------------------------------------------------- data (NumPy)

def _noise_rows(D, n, seed, npulse=4, broad=False, at_zero=False):
    """The recipe of test_search_vs_oracle: N(0, 1) rows, npulse pulses of
    random width per row, one clear detection in row 0.  broad: a 1000-sample
    pulse per row across a chunk seam (the widest boxcar's target); at_zero: a
    pulse at start 0 of every row (the only start of n_starts = 1)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (D, n))
    for d in range(D):
        for _ in range(npulse):
            w = int(rng.integers(1, 60))
            t = int(rng.integers(0, max(1, n - w)))
            x[d, t:t + w] += rng.uniform(0.5, 4.0)
        if broad:
            t = 512 + 1024 * int(rng.integers(0, 6))
            x[d, t:t + 1000] += rng.uniform(0.5, 0.8)
        if at_zero:
            x[d, 0:int(rng.integers(1, 40))] += rng.uniform(2.0, 5.0)
    x[0, n // 3:n // 3 + 3] += 8.0
    return x


def _plane_rows(D, n, seed, sigma):
    """The same rows as a u8 sweep makes them: BASE + integer noise of sigma."""
    return BASE + np.round(sigma * _noise_rows(D, n, seed))


def _plane_extra(sigma):
    return lambda w: np.sqrt(w) * (ULP_BASE / 2) / sigma


def _outlier_rows(L, raise_sigma, sigma, seed):
    """Plane rows of 5 chunks + 1 sample; in chunks 0, 2 and 3 of every row the
    first sample is raised by raise_sigma x sigma and an ordinary 8 sigma pulse
    (4 samples of 4 sigma) sits elsewhere in the chunk."""
    x = _plane_rows(4, 5 * L + 1, seed, sigma)
    for k in (0, 2, 3):
        x[:, k * L] += raise_sigma * sigma
        t = k * L + L // 2 + 37
        x[:, t:t + 4] += 4 * sigma
    return x


def _seam_rows(D, na, nb, seed):
    """(g): rows of na + nb samples whose strongest pulses straddle, touch or
    lie just past the seam at na."""
    x = _noise_rows(D, na + nb, seed)
    x[0, na + 5:na + 30] += 4.0      # wholly in the next plane: reached by boxcars only
    x[1, na - 10:na + 12] += 4.0
    x[2, na - 100:na + 40] += 2.0
    x[3, na - 1:na + 1] += 12.0
    return x.astype(np.float32)


def _tie_rows(L):
    """Two equal rows of 6 x 1024 + 1 integer samples in {0, +-1, +-2}; every
    chunk of L sums to 0 and its squares to L, so mean = 0, std = 1 and z = x
    exactly (f32 and f64).  Base: +1, -1 alternating (no boxcar above S/N 1).
    Planted in window 1 (starts 1024..2047), all S/N 2.0 exactly: sixteen
    values summing to 8 (w = 16), two runs of four +1 (w = 4; starts 1324 and
    1724: threads 44 and 188 of the block, waves 0 and 2), then a lone +2
    (w = 1).  Window 5 (block 1) holds the same without the +2.  Each chunk
    is rebalanced away from the plants: three samples zeroed per +2 (squares
    -3, sum -1), then +1 -> -1 flips for the remaining even excess; these only
    lower boxcar sums."""
    n = 6 * 1024 + 1
    x = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    busy = np.zeros(n, dtype=bool)
    plants = [(16, 1124), (4, 1324), (4, 1724), (1, 1924), (16, 5220), (4, 5420), (4, 5820)]
    for kind, t in plants:
        if kind == 16:
            x[t:t + 16] = np.tile([1.0, 1.0, 1.0, -1.0], 4)
        elif kind == 4:
            x[t:t + 4] = 1.0
        else:
            x[t] = 2.0
        busy[t - 40:t + 56] = True
    for c0 in range(0, n - L + 1, L):
        ev = iter([p for p in range(c0 + 8, c0 + L - 8, 8) if not busy[p - 4:p + 8].any()])
        for _ in range(int((x[c0:c0 + L] == 2.0).sum())):
            x[next(ev)] = 0.0
            x[next(ev)] = 0.0
            x[next(ev) + 1] = 0.0
        s = int(x[c0:c0 + L].sum())
        assert s >= 0 and s % 2 == 0
        for _ in range(s // 2):
            x[next(ev)] = -1.0
        assert x[c0:c0 + L].sum() == 0 and (x[c0:c0 + L] ** 2).sum() == L
    return np.stack([x, x])


@functools.lru_cache(maxsize=None)
def _view_plane():
    """(f): the plane and its oracle, shared by the six cases, never changed."""
    x = _noise_rows(4, 9001, 41).astype(np.float32)
    x.setflags(write=False)
    return x, so.search(x.astype(np.float64), WIDTHS, 4.0, 1000)


# ------------------------------------------------------------------- checking

def _verdict(got, x, widths, thr, L, n_starts=None, snr_extra=None):
    """Oracle of x (the values the device saw) and the shared rule, with the
    two conditions that keep the rule honest.  Prints the counts."""
    ora, margins = so.search(np.asarray(x, dtype=np.float64), widths, thr, L, n_starts=n_starts)
    excused, compared, worst = check(got, ora, margins, thr, snr_extra)
    print("candidates %d, compared %d, excused %d, worst S/N error %.3g of max(1, |s|)"
          % (len(ora), compared, excused, worst))
    assert len(ora) >= 5, len(ora)
    assert excused <= 0.1 * compared, (excused, compared)
    return ora


def _stats_bars(mean_g, istd_g, x, L, thr, w_max=150):
    """(b)'s bars on device chunk statistics against the oracle's, both from
    the 1e-4 S/N bar: 1/std within 1e-4 relative (S/N is linear in it);
    |d mean| istd sqrt(w_max) within 1e-4 thr plus, as its own addend, the f32
    representation of the mean, ulp(mean)/2 istd sqrt(w_max).  A chunk of zero
    variance must give istd == 0 exactly.  Returns the worst of each."""
    mean_o, istd_o = so.chunk_stats(np.asarray(x, dtype=np.float64), L)
    mean_g = mean_g.cpu().numpy().astype(np.float64)
    istd_g = istd_g.cpu().numpy().astype(np.float64)
    assert mean_g.shape == mean_o.shape and istd_g.shape == istd_o.shape
    live = istd_o > 0
    np.testing.assert_array_equal(istd_g[~live], 0.0)
    e_istd = float(np.max(np.abs(istd_g[live] - istd_o[live]) / istd_o[live]))
    rep = np.spacing(mean_o.astype(np.float32)).astype(np.float64) / 2 * istd_o * np.sqrt(w_max)
    e_mean = np.abs(mean_g - mean_o) * istd_o * np.sqrt(w_max)
    over = float(np.max((e_mean - rep)[live]))  # negative: inside the representation term
    print("L %d: worst 1/std error %.3g (bar 1e-4), worst mean term %.3g, beyond its f32 "
          "representation term by %.3g (bar %.3g)"
          % (L, e_istd, float(e_mean.max()), over, 1e-4 * thr))
    assert e_istd <= 1e-4, e_istd
    assert np.all(e_mean <= 1e-4 * thr + rep), over
    return e_istd, over


def _run(sp, plane, D, **kw):
    c, k = sp.raw(plane, **kw)
    return sp.collect(c, k, np.arange(D) * 1.0, 1e-3)


def _dev(x):
    import torch
    t = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


# ----------------------------------------------------- (a) the dispatch paths

W32 = tuple(range(1, 33))
# name, D, n, L, widths, threshold, seed -- and what the oracle alone gave on
# the CPU for that seed (candidates / excused).  Rows are contiguous, so row d
# starts d * n floats into the storage: with odd n its misalignment is d mod 4.
PATHS = [
    # packed-f32 interior blocks (t0 = 0, 4096) with zoff = 0, 1, 2, 3 and 0
    # again, and the tail block (t0 = 8192)
    ("misaligned-interior", 5, 9001, 1000, WIDTHS, 4.0, 11),
    # chunk boundaries inside 16-byte groups (the nx select), staged, 3 blocks
    ("odd-chunk-length", 4, 9001, 333, WIDTHS, 4.0, 12),
    # 85 chunks under a full block: nks > 64 -> the unstaged loads
    ("many-chunks", 3, 9001, 50, WIDTHS, 4.0, 13),
    # L < 4 -> the unstaged loads; |z| <= sqrt(2) in a chunk of 3, so thr 1.5
    ("tiny-chunks", 3, 9001, 3, WIDTHS, 1.5, 14),
    # maxw = 1025: span == kSpSpan in block 0, staged for the row with mis = 0,
    # unstaged for mis = 1, 2, 3 (span + mis > kSpSpan); P[kSpSpan] is read
    ("widest-boxcar", 4, 9001, 1024, (1, 32, 1025), 4.0, 15),
    # kSpMaxWidths = 32 widths
    ("most-widths", 2, 5000, 1000, W32, 4.0, 16),
    # k_sp_stats beyond one pass of its i0 loop (L > 1024)
    ("long-chunks-2500", 3, 9001, 2500, WIDTHS, 4.0, 17),
    # ... a chunk longer than a search block (one staged statistic per block)
    ("long-chunks-5000", 3, 9001, 5000, WIDTHS, 4.0, 28),
    # ... one chunk for the whole row (L >= n)
    ("single-chunk", 3, 9001, 20000, WIDTHS, 4.0, 19),
]


@pytest.mark.parametrize("name,D,n,L,widths,thr,seed", PATHS, ids=[c[0] for c in PATHS])
def test_dispatch_paths(gpu, name, D, n, L, widths, thr, seed):
    """Every dispatch branch of k_sp_search / k_sp_stats against the oracle
    (see PATHS for the path each case pins).  CPU-checked for these seeds,
    candidates / excused: misaligned-interior 23 / 0, odd-chunk-length 16 / 0,
    many-chunks 7 / 0, tiny-chunks 27 / 0, widest-boxcar 17 / 0 (3 of them at
    w = 1025), most-widths 6 / 0, long-chunks-2500 14 / 0, long-chunks-5000
    11 / 0, single-chunk 12 / 0."""
    from pypulsar_amd.search import SinglePulseSearch
    x = _noise_rows(D, n, seed, broad=(name == "widest-boxcar")).astype(np.float32)
    got = _run(SinglePulseSearch(threshold=thr, widths=widths, detrendlen=L), _dev(x), D)
    ora = _verdict(got, x, widths, thr, L)
    if name == "widest-boxcar":
        assert any(w == 1025 for _, _, w, _ in ora)
        assert 1025 in set(got["Downfact"])


# ------------------------------------------------- (b) chunk statistics alone

@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "view"])
@pytest.mark.parametrize("L", [30, 333, 1000, 1024, 2500, 5000])
def test_chunk_stats_plane_rows(gpu, L, view):
    """k_sp_stats on plane-like rows (BASE + round(1024 N(0, 1))) against
    chunk_stats in float64: 4 rows of 5 L + 1 samples, so chunks start at
    every alignment (both load paths), L > 1024 takes several passes of the
    i0 loop, and the last chunk is a single sample (istd == 0, mean == that
    sample).  view: the rows 1 float into a buffer with row stride n + 7.
    Bars: _stats_bars with the threshold 4.0 of the searches above."""
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    D, n = 4, 5 * L + 1
    x = BASE + np.round(1024 * np.random.default_rng(100 + L).normal(0, 1, (D, n)))
    if view:
        buf = torch.full((D, n + 7), float("nan"), device="cuda")
        plane = buf[:, 1:1 + n]
        plane.copy_(_dev(x))
    else:
        plane = _dev(x)
    mean, istd = SinglePulseSearch(detrendlen=L).stats(plane)
    torch.cuda.synchronize()
    _stats_bars(mean, istd, x, L, 4.0)
    np.testing.assert_array_equal(mean[:, -1].cpu().numpy(), x[:, -1].astype(np.float32))


# -------------------------------------------- (c) plane-like rows, end to end

@pytest.mark.parametrize("sigma", [1024, 64])
def test_plane_like_rows(gpu, sigma):
    """Search of integer rows at BASE with noise sigma (D = 4, n = 9001,
    L = 1000, threshold 4): S/N within 1e-4 max(1, |s|) + sqrt(w) ulp(BASE)/2
    / sigma, the second term being the rounding of the stored f32 mean; the
    near-tie margin is of the same size.  CPU-checked, candidates / excused:
    sigma 1024: 19 / 0; sigma 64: 19 / 0."""
    from pypulsar_amd.search import SinglePulseSearch
    x = _plane_rows(4, 9001, 21, sigma)
    got = _run(SinglePulseSearch(threshold=4.0, widths=WIDTHS, detrendlen=1000), _dev(x), 4)
    _verdict(got, x, WIDTHS, 4.0, 1000, snr_extra=_plane_extra(sigma))


# ------------------------------- (d) an outlier at the chunk's first sample

@pytest.mark.parametrize("sigma", [1024, 64])
@pytest.mark.parametrize("raise_sigma", [100, 300])
@pytest.mark.parametrize("L", [1024, 4096])
def test_outlier_at_chunk_start(gpu, L, raise_sigma, sigma):
    """The first sample of chunks 0, 2, 3 raised by 100 / 300 sigma (a bright
    pulse or an RFI spike at a chunk start), an ordinary 8 sigma pulse
    elsewhere in each: k_sp_stats' shift must not be spoilt by that one
    sample.  With K = row[0] the shifted sums cancelled (S2/len - m1^2 with
    m1 = 300 sigma); K is now the mean of every fourth sample of the first
    256, which one sample moves by 1/64 of its height.  Measured on the
    MI355X, worst 1/std error: with K = row[0] 2.0e-4, 1.9e-4, 6.2e-4, 3.7e-4
    in the four L = 4096 cases (failing) and 4.5e-5 to 1.0e-4 at L = 1024;
    with the pilot mean at most 4.5e-7.  Bars: (b)'s on the statistics, (c)'s
    on S/N.  The threshold is 0.4 (the outlier inflates its
    chunk's std up to 9.4 x, squashing the pulse to S/N 0.85), so nearly
    every window holds a candidate.  CPU-checked, candidates / excused:
    L = 1024: 20 / 0 (of 24 windows); L = 4096: 80 / 0 at sigma 1024, 80 / 1
    at sigma 64 (of 84 windows)."""
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    thr = 0.4
    x = _outlier_rows(L, raise_sigma, sigma, 31)
    plane = _dev(x)
    sp = SinglePulseSearch(threshold=thr, widths=WIDTHS, detrendlen=L)
    mean, istd = sp.stats(plane)
    torch.cuda.synchronize()
    _stats_bars(mean, istd, x, L, thr)
    _verdict(_run(sp, plane, 4), x, WIDTHS, thr, L, snr_extra=_plane_extra(sigma))


# ------------------------------------------------------------- (e) exact ties

@pytest.mark.parametrize("L", [1024, 512])
def test_exact_ties(gpu, L):
    """The tie rule, smallest width then smallest start, on rows where every
    float operation is exact (_tie_rows): in window 1 four boxcars -- and the
    w = 4 ones once more one start later -- reach S/N 2.0 exactly; the winner
    is w = 1 although its start is the last.  In window 5 the winner is
    w = 4 at the earlier run (the later one belongs to another wave: the
    cross-wave min-key reduction of pass 2), not the w = 16 boxcar that starts
    before both.  Row 1 is misaligned by one float.  Sigma is float32(2.0) bit
    for bit; no near-tie exemption.  threshold 2.0 keeps the candidates
    (>=), the next float32 above drops them all."""
    from pypulsar_amd.search import SinglePulseSearch
    widths = (1, 2, 4, 16)
    x = _tie_rows(L)
    D, n = x.shape
    # the oracle alone first: 2.0 is the maximum of both windows, attained by
    # at least three (width, start) pairs, and nothing else reaches 2.0
    z = so.normalise(x, L)
    np.testing.assert_array_equal(z[:, :n - 1], x[:, :n - 1])
    snr = {w: so.boxcar_snr(z, w) for w in widths}
    for win in range(6):
        lo, hi = 1024 * win, 1024 * win + 1024
        best = max(float(snr[w][0, lo:hi].max()) for w in widths)
        ties = [(w, lo + int(t)) for w in widths for t in np.flatnonzero(snr[w][0, lo:hi] == 2.0)]
        if win in (1, 5):
            assert best == 2.0 and len(ties) >= 3, (win, best, ties)
            assert {w for w, _ in ties} == ({1, 4, 16} if win == 1 else {4, 16})
            assert sum(w == 4 for w, _ in ties) >= 2
        else:
            assert best < 2.0 and not ties
    want = [(d, t, w) for d in range(D) for t, w in ((1924, 1), (5420, 4))]
    ora, margins = so.search(x, widths, 2.0, L)
    assert [(d, t, w) for d, t, w, _ in ora] == want and all(s == 2.0 for _, _, _, s in ora)
    assert all(m == 0.0 for m in margins)

    plane = _dev(x)
    got = _run(SinglePulseSearch(threshold=2.0, widths=widths, detrendlen=L), plane, D)
    assert [(int(r), int(t), int(w)) for r, t, w in
            zip(got["row"], got["Sample"], got["Downfact"])] == want
    np.testing.assert_array_equal(got["Sigma"].view(np.uint32),
                                  np.full(len(want), np.float32(2.0).view(np.uint32)))
    above = float(np.nextafter(np.float32(2.0), np.float32(np.inf)))
    assert len(_run(SinglePulseSearch(threshold=above, widths=widths, detrendlen=L), plane, D)) == 0


# --------------------------------------- (f) views and hostile neighbours

@pytest.mark.parametrize("filler", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_view_with_hostile_neighbours(gpu, off, filler):
    """A [4, 9001] plane at column offset 1, 2, 3 of a [4, 9009] buffer of NaN
    (or 1e30): row d is misaligned by (d + off) mod 4 and its 16-byte groups
    reach into the filler on both sides.  The staged loads may read those
    granules but the i + e >= 0 && i + e < span select must keep them out of
    z, and k_sp_stats must stay inside the row: candidates equal the oracle
    of the plane alone, every Sigma finite, the filler untouched.  CPU-checked:
    15 candidates, 0 excused."""
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    x, (ora, margins) = _view_plane()
    D, n = x.shape
    buf = torch.full((D, n + 8), filler, dtype=torch.float32, device="cuda")
    plane = buf[:, off:off + n]
    plane.copy_(_dev(x))
    assert plane.stride(0) == n + 8 and (plane.data_ptr() // 4) % 4 == off
    got = _run(SinglePulseSearch(threshold=4.0, widths=WIDTHS, detrendlen=1000), plane, D)
    assert np.all(np.isfinite(got["Sigma"]))
    excused, compared, _ = check(got, ora, margins, 4.0)
    assert len(ora) >= 5 and excused <= 0.1 * compared, (len(ora), excused, compared)
    out = torch.cat([buf[:, :off], buf[:, off + n:]], dim=1)
    assert bool(torch.isnan(out).all() if filler != filler else (out == filler).all())
    np.testing.assert_array_equal(plane.cpu().numpy(), x)


# ------------------------------------- (g) the start limit and continuation

@pytest.mark.parametrize("n_starts", [5000, 4096, 1])
def test_start_limit(gpu, n_starts):
    """raw(n_starts=...) on n = 9001 against the oracle's start limit: 5000
    ends inside block 1 (its windows 4 and, partly, 5; the i < nss select),
    4096 leaves one interior block, 1 leaves start 0 alone (6 rows, each with
    a pulse at 0).  Boxcars still reach past the limit.  CPU-checked,
    candidates / excused: 5000: 18 / 0; 4096: 14 / 0; 1: 6 / 0."""
    from pypulsar_amd.search import SinglePulseSearch
    x = _noise_rows(6, 9001, 51, at_zero=True).astype(np.float32)
    sp = SinglePulseSearch(threshold=4.0, widths=WIDTHS, detrendlen=1000)
    got = _run(sp, _dev(x), 6, n_starts=n_starts)
    assert np.all(got["Sample"] < n_starts)
    _verdict(got, x, WIDTHS, 4.0, 1000, n_starts=n_starts)


def test_continuation_inside_a_block(gpu):
    """raw(nxt=...) away from StreamingSearch's alignments: a first plane of
    3000 columns (L = 500; row stride 3005, so rows misaligned) continued by
    the first 149 columns of a 700-column plane (row stride 700) with the
    statistics of that whole plane, n_starts = 3000.  The seam lies inside
    search block 0; pulses straddle it.  Equal to the oracle of the
    concatenated rows under the same start limit.  CPU-checked: 9
    candidates (3 of them at the seam), 0 excused."""
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    D, na, nb, L = 4, 3000, 700, 500
    x = _seam_rows(D, na, nb, 61)
    buf = torch.zeros((D, na + 5), device="cuda")
    a = buf[:, :na]
    a.copy_(torch.from_numpy(x[:, :na]).cuda())
    b = _dev(x[:, na:])
    sp = SinglePulseSearch(threshold=4.0, widths=WIDTHS, detrendlen=L)
    got = _run(sp, a, D, nxt=(b[:, :149], sp.stats(b)), n_starts=na)
    assert np.all(got["Sample"] < na)
    _verdict(got, x, WIDTHS, 4.0, L, n_starts=na)


# --------------------------------- (h) a zero-variance chunk in a live row

def test_zero_variance_chunk_inside_live_row(gpu):
    """One chunk of rows 1 and 2 (plane-like, sigma 1024) is constant at BASE:
    its istd is 0, so z is 0 there, and no candidate may lie wholly inside it
    (boxcars reaching out of it still count); everything else equals the
    oracle.  CPU-checked: 15 candidates, 0 excused."""
    import torch
    from pypulsar_amd.search import SinglePulseSearch
    L = 1000
    x = _plane_rows(4, 9001, 71, 1024)
    dead = {1: 3, 2: 5}
    for d, k in dead.items():
        x[d, k * L:(k + 1) * L] = BASE
    plane = _dev(x)
    sp = SinglePulseSearch(threshold=4.0, widths=WIDTHS, detrendlen=L)
    mean, istd = sp.stats(plane)
    torch.cuda.synchronize()
    for d, k in dead.items():
        assert float(istd[d, k]) == 0.0 and float(mean[d, k]) == BASE
    got = _run(sp, plane, 4)
    for r, t, w in zip(got["row"], got["Sample"], got["Downfact"]):
        k = dead.get(int(r))
        assert k is None or not (k * L <= t and t + w <= (k + 1) * L), (r, t, w)
    _verdict(got, x, WIDTHS, 4.0, L, snr_extra=_plane_extra(1024))


# ------------------------------------------------- (i) overflow accounting

def test_overflow_accounting(gpu):
    """threshold 1.0 makes every one of the 4 x 9 windows a candidate (the
    oracle's weakest window maximum is checked to be well above it) with
    max_cands = 8: count is the oracle's K exactly, the 8 slots written are
    distinct (row, window) members of the oracle's set with its (start, width,
    S/N), and collect raises."""
    from pypulsar_amd.search import SinglePulseSearch
    x = _noise_rows(4, 9001, 81).astype(np.float32)
    ora, margins = so.search(x.astype(np.float64), WIDTHS, 1.0, 1000)
    K = len(ora)
    assert K == 36 and min(s for _, _, _, s in ora) > 2.0
    og = {(d, t // 1024): (t, w, s, m) for (d, t, w, s), m in zip(ora, margins)}
    sp = SinglePulseSearch(threshold=1.0, widths=WIDTHS, detrendlen=1000, max_cands=8)
    c, count = sp.raw(_dev(x))
    assert int(count.item()) == K
    c = c.cpu().numpy()
    assert c.shape == (8, 4)
    keys = [(int(r), int(t) // 1024) for r, t in c[:, :2]]
    assert len(set(keys)) == 8 and set(keys) <= set(og)
    for (r, t, w, bits), key in zip(c, keys):
        ot, ow, s, m = og[key]
        assert abs(float(np.int32(bits).view(np.float32)) - s) <= 1e-4 * max(1.0, abs(s))
        assert m <= 1e-4 * abs(s) or (int(t), int(w)) == (ot, ow)
    with pytest.raises(RuntimeError):
        sp.collect(*sp.raw(_dev(x)), np.arange(4) * 1.0, 1e-3)
