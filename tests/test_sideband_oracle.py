"""The sideband oracle (tests/sideband_oracle.py) against the definition, the
recovery case of DESIGN.md §6q on the CPU, and the host side of
pypulsar_amd.sideband: sifting and ``.bincands`` files.  No GPU."""
import numpy as np
import pytest

import period_oracle as po
import sideband_cases as sc
import sideband_oracle as so


def test_mini_is_the_definition():
    """L = 32: the literal O(L^2) sums of the definition."""
    L, rlo = 32, 3
    rng = np.random.default_rng(5)
    p = rng.exponential(1.0, 100).astype(np.float32)
    p[40] = 30.0
    for clip in (0.0, 8.0):
        got = so.mini(p, rlo, L, shift=2, clip=clip)
        los = so.segments(len(p), rlo, L, 2)
        assert got.shape == (len(los), L)
        for j, lo in enumerate(los):
            x = p[lo:lo + L].astype(np.float64)
            if clip:
                x = np.minimum(x, clip)
            A = np.asarray([sum(x[i] * np.exp(-2j * np.pi * i * k / L) for i in range(L))
                            for k in range(L // 2 + 1)])
            want = np.empty(L)
            for k in range(L // 2):
                want[2 * k] = L * abs(A[k]) ** 2 / A[0].real ** 2
                want[2 * k + 1] = np.pi ** 2 / 16 * L * abs(A[k] - A[k + 1]) ** 2 / A[0].real ** 2
            np.testing.assert_allclose(got[j], want, rtol=1e-10, atol=1e-12)
    # a dead stretch: A_0 <= 0 gives M = 0
    assert not so.mini(np.zeros(100, np.float32), rlo, L).any()


def test_segments():
    L, rlo = 64, 7
    stride = L >> 2
    assert len(so.segments(rlo + L - 1, rlo, L)) == 0               # nn - rlo < L
    assert so.segments(rlo + L, rlo, L).tolist() == [rlo]            # nn - rlo == L
    s = so.segments(rlo + L + 3 * stride + (stride - 1), rlo, L)      # a remainder of stride - 1
    assert s.tolist() == [rlo + j * stride for j in range(4)]
    assert s[-1] + L <= rlo + L + 3 * stride + (stride - 1)
    assert so.segments(rlo + 4 * L, rlo, L, shift=0).tolist() == [rlo + j * L for j in range(4)]
    assert len(so.segments(rlo + L + 8, rlo, L, shift=3)) == 2


def test_candidates_edges_and_ties():
    """Plateaus: the first bin of a run of equal sums is the candidate; the
    neighbours outside [qlo, L // H) count as -inf."""
    M = np.ones((1, 32), dtype=np.float32)
    M[0, 4] = 5.0       # q = qlo
    M[0, 31] = 6.0      # q = L - 1, stage 1's last
    M[0, 10:13] = 3.0   # a plateau
    got = so.candidates(M, (1,), (2.0,), qlo=4)
    assert {(c[1], c[2]) for c in got} == {(4, 1), (31, 1), (10, 1)}


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_recovery(seed):
    """A comb the plain search does not see.  The prototype measured sigma 8.2
    to 11.0 over the four seeds; the bar of 7 is the lowest of those less one,
    against float32 rounding differences."""
    p = sc.whitened_powers(sc.recovery_series(seed))
    harms = (1, 2, 4, 8, 16)
    thr = np.asarray([po.threshold_power(6.0, h) for h in harms], dtype=np.float32)
    assert po.candidates(p[None], harms, thr, sc.rlo()) == set()
    best = sc.oracle_search(p)[0]
    sigma, L, lo, q, H, _ = best
    print("seed %d: L=%d lo=%d q=%d H=%d sigma=%.2f (true q %.2f)"
          % (seed, L, lo, q, H, sigma, 2 * 256 / sc.NORB))
    assert L == 256
    assert abs(q - 2 * L / sc.NORB) <= 1
    assert sigma >= 7


def test_clip_tames_a_lone_line():
    """One bin of power 400 in noise: unclipped, its flat mini spectrum is full
    of local maxima above threshold (the prototype measured 6323 candidates
    against 67 with the clip)."""
    rng = np.random.default_rng(11)
    p = rng.exponential(1.0, 4096).astype(np.float32)
    p[2000] = 400.0
    clipped = sc.oracle_search(p, clip=po.threshold_power(6.0, 1))
    plain = sc.oracle_search(p, clip=0.0)
    print("candidates: %d clipped, %d unclipped" % (len(clipped), len(plain)))
    assert len(clipped) < len(plain)


# ---- pypulsar_amd.sideband's host side ----

def _records(rows):
    """CAND_DTYPE records from (row, L, lo, q, sigma) with nfft dt = 8.192 s."""
    from pypulsar_amd import sideband as sb
    out = np.zeros(len(rows), dtype=sb.CAND_DTYPE)
    Tn = sc.N * sc.DT
    for i, (row, L, lo, q, sigma) in enumerate(rows):
        out[i] = (float(row) * 0.5, row, L, lo, q, 1, 20.0 + i, sigma, (lo + L / 2) / Tn,
                  lo / Tn, (lo + L) / Tn, q * Tn / (2.0 * L))
    return out


def test_sift():
    from pypulsar_amd import sideband as sb
    c = _records([
        (0, 256, 2377, 61, 9.0),    # the signal
        (0, 256, 2441, 61, 8.0),    # the overlapping next segment: merges
        (1, 256, 2377, 62, 7.5),    # another row, one half-bin step away: merges
        (2, 128, 2473, 15, 7.0),    # porb half of q = 30.5 at L = 128, i.e. ratio 2: merges
        (0, 256, 3500, 61, 6.5),    # a disjoint frequency range: apart
        (0, 256, 2377, 90, 6.2),    # another porb: apart
    ])
    s = sb.sift(c)
    assert s["sigma"].tolist() == [9.0, 6.5, 6.2]
    assert s["nhits"].tolist() == [4, 1, 1]
    assert s["ndms"].tolist() == [3, 1, 1]
    assert (s["lo"][0], s["q"][0], s["L"][0]) == (2377, 61, 256)
    s2 = sb.sift(c, min_dms=2)
    assert s2["sigma"].tolist() == [9.0] and s2["ndms"].tolist() == [3]
    assert len(sb.sift(c[:0])) == 0


def test_bincands_round_trip(tmp_path):
    from pypulsar_amd import sideband as sb
    s = sb.sift(_records([(0, 256, 2377, 61, 9.123456789012345), (3, 1024, 9000, 245, 7.25),
                          (1, 256, 2441, 61, 8.0)]))
    fn = str(tmp_path / "x.bincands")
    sb.write_bincands(s, fn)
    back = sb.read_bincands(fn)
    assert back.dtype == sb.BINCAND_DTYPE and len(back) == len(s) == 2
    for name in sb.BINCAND_DTYPE.names:
        assert np.array_equal(back[name], s[name]), name
    sb.write_bincands_npz(s, str(tmp_path / "x_bincands.npz"))
    z = np.load(str(tmp_path / "x_bincands.npz"))
    for name in sb.BINCAND_DTYPE.names:
        assert np.array_equal(z[name], s[name]), name
    sb.write_bincands(s[:0], fn)
    assert len(sb.read_bincands(fn)) == 0
