"""The host side of the birdie zapper (pypulsar_amd/zap.py) without a GPU:
``.zaplist`` reading and writing against the text the reference's
``write_zaplist`` wrote (tests/golden/make_golden_zaplist.py), the frequency
<-> bin rules, the threshold against a Monte-Carlo run, and the finder's
rule (tests/zap_oracle.py) on the synthetic planes."""
import math
import os

import numpy as np
import pytest

import zap_oracle as zo
from conftest import GOLDEN

GOLDEN_TXT = os.path.join(GOLDEN, "golden_zaplist.txt")
DT = zo.DT


def _columns(fn):
    rows = [l.split() for l in open(fn) if l.strip() and not l.startswith("#")]
    return (np.asarray([float(r[0]) for r in rows]), np.asarray([float(r[1]) for r in rows]))


# ---- files ----

def test_read_golden():
    from pypulsar_amd.zap import read_zaplist
    zl = read_zaplist(GOLDEN_TXT)
    f, w = _columns(GOLDEN_TXT)
    g = np.load(os.path.join(GOLDEN, "golden_zaplist.npz"))
    assert len(zl) == len(g["runs"]) == len(f)
    np.testing.assert_array_equal(zl.freqs, f)
    np.testing.assert_array_equal(zl.widths, w)
    assert zl.freqs.dtype == zl.widths.dtype == np.float64
    # (the text holds 15 digits of the reference's float64 columns)
    np.testing.assert_allclose(zl.freqs, g["mid"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(zl.widths, g["width"], rtol=1e-14, atol=0)
    # a baryv changes nothing without B lines
    np.testing.assert_array_equal(read_zaplist(GOLDEN_TXT, baryv=1e-4).freqs, f)


def test_read_comments_and_bary_lines(tmp_path):
    from pypulsar_amd.zap import read_zaplist
    fn = str(tmp_path / "b.zaplist")
    with open(fn, "w") as f:
        f.write("# a comment\n\n  60.0  0.5\n#  70.0  1.0\nB 100.0  0.25\n   50.0   0.125\n"
                "B200.0 1.0\n")
    zl = read_zaplist(fn)
    np.testing.assert_array_equal(zl.freqs, [50.0, 60.0, 100.0, 200.0])
    np.testing.assert_array_equal(zl.widths, [0.125, 0.5, 0.25, 1.0])
    v = 1e-4
    zl = read_zaplist(fn, baryv=v)
    np.testing.assert_array_equal(zl.freqs, [50.0, 60.0, 100.0 * (1 + v), 200.0 * (1 + v)])
    np.testing.assert_array_equal(zl.widths, [0.125, 0.5, 0.25 * (1 + v), 1.0 * (1 + v)])


def test_write_matches_golden_format(tmp_path):
    from pypulsar_amd.zap import Zaplist, read_zaplist, write_zaplist
    g = np.load(os.path.join(GOLDEN, "golden_zaplist.npz"))
    fn = str(tmp_path / "w.zaplist")
    write_zaplist(fn, Zaplist(g["mid"], g["width"]))
    data = lambda p: [l for l in open(p) if not l.startswith("#")]  # noqa: E731
    assert data(fn) == data(GOLDEN_TXT)
    # the header: comment lines only, as many as the reference's
    head = lambda p: [l for l in open(p) if l.startswith("#")]  # noqa: E731
    assert len(head(fn)) == len(head(GOLDEN_TXT)) == 5
    assert head(fn)[1:] == head(GOLDEN_TXT)[1:]
    back = read_zaplist(fn)
    f, w = _columns(GOLDEN_TXT)
    np.testing.assert_array_equal(back.freqs, f)
    np.testing.assert_array_equal(back.widths, w)


# ---- bins ----

@pytest.mark.parametrize("nfft", [4096, 5000])
def test_bins_round_trip(tmp_path, nfft):
    from pypulsar_amd.zap import Zaplist, read_zaplist, write_zaplist
    nn = nfft // 2
    b = np.asarray([[1, 1], [7, 9], [300, 300], [517, 519], [1000, 1900], [nn - 1, nn - 1]],
                   dtype=np.int32)
    zl = Zaplist.from_bins(b, nfft, DT)
    got = zl.bins(nfft, DT, nn)
    assert got.dtype == np.int32 and got.shape == (len(b), 2)
    np.testing.assert_array_equal(got, b)
    np.testing.assert_array_equal(zl.bins(nfft, DT), b)  # (nn defaults to nfft // 2)
    f, w = zo.from_bins(b, nfft, DT)
    np.testing.assert_array_equal(zl.freqs, f)
    np.testing.assert_array_equal(zl.widths, w)
    np.testing.assert_array_equal(zo.to_bins(f, w, nfft, DT, nn), b)
    # an interval that spans the whole range
    e = np.asarray([[1, nn - 1]], dtype=np.int32)
    np.testing.assert_array_equal(Zaplist.from_bins(e, nfft, DT).bins(nfft, DT, nn), e)
    # ... and through a file
    fn = str(tmp_path / "rt.zaplist")
    write_zaplist(fn, zl)
    np.testing.assert_array_equal(read_zaplist(fn).bins(nfft, DT, nn), b)


def test_bins_merge_and_clip():
    from pypulsar_amd.zap import Zaplist
    nfft, nn = 4096, 2048
    T = nfft * DT
    mk = lambda iv: Zaplist.from_bins(np.asarray(iv), nfft, DT)  # noqa: E731
    # overlapping and touching intervals merge; an isolated one stays
    zl = mk([[10, 20], [15, 30], [31, 40], [42, 43]])
    np.testing.assert_array_equal(zl.bins(nfft, DT, nn), [[10, 40], [42, 43]])
    # unsorted input is sorted
    zl = Zaplist([500.0 / T, 100.0 / T], [0.0, 2.0 / T])
    np.testing.assert_array_equal(zl.freqs, [100.0 / T, 500.0 / T])
    np.testing.assert_array_equal(zl.bins(nfft, DT, nn), [[99, 101], [500, 500]])
    # a frequency between two bins takes both
    np.testing.assert_array_equal(Zaplist([100.5 / T], [0.0]).bins(nfft, DT, nn), [[100, 101]])
    # outside [1, nn - 1]: clipped or dropped
    zl = Zaplist([0.0, (nn + 5.0) / T, (nn - 1.0) / T, 3000.0 / T], [6.0 / T, 20.0 / T, 0.0, 4.0 / T])
    np.testing.assert_array_equal(zl.bins(nfft, DT, nn), [[1, 3], [nn - 5, nn - 1]])
    assert Zaplist([0.0], [0.0]).bins(nfft, DT, nn).shape == (0, 2)
    assert Zaplist().bins(nfft, DT, nn).shape == (0, 2)
    # the oracle's rule is the same
    np.testing.assert_array_equal(zo.to_bins(zl.freqs, zl.widths, nfft, DT, nn),
                                  zl.bins(nfft, DT, nn))
    # two lists merged
    both = mk([[10, 20]]).merged(mk([[18, 25], [100, 100]]))
    np.testing.assert_array_equal(both.bins(nfft, DT, nn), [[10, 25], [100, 100]])


# ---- the finder's statistics ----

def test_rows_and_rank():
    from pypulsar_amd.zap import BirdieFinder
    bf = BirdieFinder()
    np.testing.assert_array_equal(bf.select_rows(9), np.arange(9))
    np.testing.assert_array_equal(bf.select_rows(33), np.arange(33))
    sel = bf.select_rows(1024)
    assert len(sel) == 33 and sel[0] == 0 and sel[-1] == 1023 and np.all(np.diff(sel) > 0)
    np.testing.assert_array_equal(sel, zo.select_rows(1024, 33))
    assert BirdieFinder(rows=5).select_rows(3).tolist() == [0, 1, 2]
    # the median of an odd number of rows; the upper of the two middle ones otherwise
    assert [bf.rank(R) for R in (1, 2, 9, 32, 33, 64)] == [1, 1, 5, 16, 17, 32]
    assert BirdieFinder(percent=75.0).rank(16) == 12
    assert BirdieFinder(percent=100.0).rank(7) == 7
    assert BirdieFinder(percent=1.0).rank(7) == 1
    with pytest.raises(AssertionError):
        BirdieFinder(rows=65)
    # where percent / 100 (R - 1) is an integer the order statistic is the
    # interpolated percentile
    rng = np.random.default_rng(1)
    for R, pc in ((9, 50.0), (33, 50.0), (5, 50.0), (5, 100.0)):
        P = rng.exponential(1.0, (R, 40)).astype(np.float32)
        want = np.percentile(P, pc, axis=0)
        np.testing.assert_array_equal(zo.order_statistic(P, BirdieFinder(percent=pc).rank(R)),
                                      want.astype(np.float32))


def test_threshold_closed_forms():
    from scipy.stats import norm
    from pypulsar_amd.zap import BirdieFinder
    for nsig in (3.0, 5.0):
        assert BirdieFinder(nsig=nsig).threshold(1) == pytest.approx(-math.log(norm.sf(nsig)),
                                                                     rel=1e-12)
    for R, pc in ((1, 50.0), (9, 50.0), (32, 50.0), (33, 50.0), (16, 75.0), (64, 50.0)):
        t = [BirdieFinder(percent=pc, nsig=s).threshold(R) for s in (2.0, 3.0, 4.0, 5.0, 6.0)]
        assert np.all(np.diff(t) > 0), (R, pc, t)
        # the oracle solves the binomial tail instead of inverting the beta function
        for s, x in zip((2.0, 3.0, 4.0, 5.0, 6.0), t):
            assert x == pytest.approx(zo.threshold(R, pc, s), rel=1e-9)
    # the maximum of R values: 1 - (1 - e^-x)^R = p
    p = norm.sf(4.0)
    assert BirdieFinder(percent=100.0, nsig=4.0).threshold(8) == pytest.approx(
        -math.log1p(-(1.0 - p) ** (1.0 / 8)), rel=1e-9)


@pytest.mark.parametrize("R,percent", [(1, 50.0), (9, 50.0), (32, 50.0), (33, 50.0), (16, 75.0)])
def test_threshold_monte_carlo(R, percent):
    """400 000 columns of R Exp(1) values: the fraction whose rank-th smallest
    exceeds the threshold is norm.sf(3) within 4 binomial standard
    deviations."""
    from scipy.stats import norm
    from pypulsar_amd.zap import BirdieFinder
    bf = BirdieFinder(percent=percent, nsig=3.0)
    N = 400000
    rng = np.random.default_rng(12345)
    x = rng.exponential(1.0, (R, N))
    stat = np.partition(x, bf.rank(R) - 1, axis=0)[bf.rank(R) - 1]
    p = norm.sf(3.0)
    k = int(np.sum(stat > bf.threshold(R)))
    sd = math.sqrt(N * p * (1.0 - p))
    print("R %d percent %g: %d exceed, expected %.1f, %.2f sd" % (R, percent, k, N * p,
                                                                  (k - N * p) / sd))
    assert abs(k - N * p) <= 4.0 * sd


# ---- the finder's rule on the synthetic planes ----

@pytest.fixture(scope="module", params=zo.SHAPES, ids=lambda s: "D%d_n%d" % s[:2])
def whitened(request):
    D, n, nfft = request.param
    return request.param, zo.whiten(zo.synthetic_plane(D, n, nfft, A=150.0), nfft)


@pytest.mark.parametrize("nsig", [4.0, 5.0])
def test_oracle_finder(whitened, nsig):
    (D, n, nfft), powers = whitened
    rlo = max(1, int(math.ceil(1.0 * nfft * DT)))
    iv, pct = zo.find(powers, rlo, rows=33, percent=50.0, nsig=nsig, grow=0)
    flagged = set()
    for lo, hi in iv:
        flagged.update(range(lo, hi + 1))
    noise = np.delete(pct[rlo:], np.arange(515, 520) - rlo)
    print("D %d nsig %g: flagged %s, threshold %.3f, pct[517] %.2f, largest noise value %.3f"
          % (D, nsig, sorted(flagged), zo.threshold(D, 50.0, nsig), pct[517], noise.max()))
    assert zo.BIRDIE_BIN in flagged
    assert flagged <= {516, 517, 518}
    assert nfft // 64 not in flagged
    # the pulsar is there -- above the single-harmonic threshold of a 6 sigma
    # search, -ln norm.sf(6) = 20.7 -- in its own row, not in the median
    print("pulsar power %.1f" % powers[zo.PULSAR_ROW, nfft // 64])
    assert powers[zo.PULSAR_ROW, nfft // 64] > 20.7
    assert pct[nfft // 64] < zo.threshold(D, 50.0, nsig)


def test_flag_grow_and_merge():
    from pypulsar_amd.zap import BirdieFinder
    nn = 64
    pct = np.full(nn, 0.5, dtype=np.float32)
    pct[[1, 2, 10, 13, 30, 31, 32, 63]] = 100.0
    for grow, want in ((0, [[2, 2], [10, 10], [13, 13], [30, 32], [63, 63]]),
                       (1, [[1, 3], [9, 14], [29, 33], [62, 63]]),
                       (3, [[1, 5], [7, 16], [27, 35], [60, 63]])):
        bf = BirdieFinder(rows=9, nsig=5.0, grow=grow)
        got = bf.flag(pct, 9, rlo=2)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(zo.flag(pct, 9, 2, 50.0, 5.0, grow), want)
        assert got.dtype == np.int32
    assert BirdieFinder().flag(np.zeros(nn, np.float32), 9, 1).shape == (0, 2)
    # "above" the threshold: a bin at it is not flagged
    bf = BirdieFinder(rows=9, grow=0)
    t = bf.threshold(9)
    assert bf.flag(np.asarray([0.0, 0.0, t, np.nextafter(t, 9.0)]), 9, 1).tolist() == [[3, 3]]


def test_oracle_fill():
    rng = np.random.default_rng(2)
    p = rng.exponential(1.0, (3, 50)).astype(np.float32)
    s = (rng.normal(0, 1, (3, 50)) + 1j * rng.normal(0, 1, (3, 50))).astype(np.complex64)
    q, t = zo.fill(p, [[1, 1], [7, 9]], s)
    m = np.zeros(50, dtype=bool)
    m[[1, 7, 8, 9]] = True
    assert np.all(q[:, m] == 1.0) and np.array_equal(q[:, ~m], p[:, ~m])
    assert np.all(t[:, m].real == np.float32(0.70710677)) and np.array_equal(t[:, ~m], s[:, ~m])
    # of unit power to float32 rounding
    assert abs(float(np.abs(t[0, 7]) ** 2) - 1.0) < 2e-7
