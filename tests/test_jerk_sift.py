"""Sifting and .accelcands naming of jerk-search records (host only): the
``wbins`` term of ``periodicity.sift`` and ``write_accelcands(wmax=...)``."""
import numpy as np


def _recs(rows, dtype):
    out = np.zeros(len(rows), dtype=dtype)
    for k, (r, zbins, wbins, sigma, dm) in enumerate(rows):
        out[k]["r"], out[k]["sigma"], out[k]["DM"] = r, sigma, dm
        out[k]["row"], out[k]["numharm"], out[k]["power"] = int(dm), 1, 10.0 * sigma
        out[k]["period"] = 1.0 / r
        out[k]["z"] = out[k]["zbins"] = zbins
        if "wbins" in dtype.names:
            out[k]["w"] = out[k]["wbins"] = wbins
            out[k]["fdd"] = wbins / 8.0
    return out


def test_sift_widens_by_a_twelfth_of_the_w_difference():
    from pypulsar_amd.accel import ACCEL_CAND_DTYPE
    from pypulsar_amd.jerk import JERK_CAND_DTYPE
    from pypulsar_amd.periodicity import sift
    # r differs by 4: beyond rtol_bins = 1.5; with w differing by 36 the tolerance is 1.5 + 3
    rows = [(100.0, 0.0, 40.0, 20.0, 1.0), (104.0, 0.0, 4.0, 10.0, 2.0)]
    s = sift(_recs(rows, JERK_CAND_DTYPE))
    assert len(s) == 1 and s[0].hits == [(1.0, 20.0), (2.0, 10.0)]
    assert (s[0].w, s[0].fdd, s[0].z) == (40.0, 5.0, 0.0)
    # w differing by 24: 1.5 + 2 < 4, two candidates
    rows[1] = (104.0, 0.0, 16.0, 10.0, 2.0)
    s = sift(_recs(rows, JERK_CAND_DTYPE))
    assert [c.r for c in s] == [100.0, 104.0] and [c.w for c in s] == [40.0, 16.0]
    # a second harmonic 3 bins off 2 x 100: w 116 against 2 x 40 widens to 1.5 + 3, w 84 to
    # 1.5 + 1 / 3 only
    rows[1] = (203.0, 0.0, 116.0, 10.0, 2.0)
    assert len(sift(_recs(rows, JERK_CAND_DTYPE))) == 1
    rows[1] = (203.0, 0.0, 84.0, 10.0, 2.0)
    assert len(sift(_recs(rows, JERK_CAND_DTYPE))) == 2
    # records without the field sift exactly as before (w and fdd stay 0)
    rows = [(100.0, 0.0, 40.0, 20.0, 1.0), (104.0, 0.0, 4.0, 10.0, 2.0)]
    s = sift(_recs(rows, ACCEL_CAND_DTYPE))
    assert len(s) == 2 and all(c.w == 0.0 and c.fdd == 0.0 for c in s)
    # w equal everywhere: the z rule alone
    a = _recs([(100.0, 6.0, 20.0, 20.0, 1.0), (103.0, 0.0, 20.0, 10.0, 2.0)], JERK_CAND_DTYPE)
    b = _recs([(100.0, 6.0, 0.0, 20.0, 1.0), (103.0, 0.0, 0.0, 10.0, 2.0)], ACCEL_CAND_DTYPE)
    assert len(sift(a)) == len(sift(b)) == 1


def test_write_accelcands_jerk_names(tmp_path):
    from pypulsar_amd.jerk import JERK_CAND_DTYPE
    from pypulsar_amd.periodicity import read_accelcands, sift, write_accelcands
    s = sift(_recs([(100.0, 2.0, 40.0, 20.0, 1.0), (317.3, 0.0, 0.0, 10.0, 2.0)], JERK_CAND_DTYPE))
    a, b, c = (str(tmp_path / n) for n in ("a", "b", "c"))
    write_accelcands(s, a, basename="obs", zmax=8)
    write_accelcands(s, b, basename="obs", zmax=8, wmax=0)
    write_accelcands(s, c, basename="obs", zmax=8, wmax=40)
    assert open(a, "rb").read() == open(b, "rb").read()  # the default keeps the bytes
    assert b"JERK" not in open(a, "rb").read()
    back = read_accelcands(c)
    assert [x.accelfile for x in back] == ["obs_DM1.00_ACCEL_8_JERK_40",
                                           "obs_DM2.00_ACCEL_8_JERK_40"]
    assert [x.candnum for x in back] == [1, 2] and back[0].z == 2.0
    # the same columns: only the names differ
    la, lc = open(a).read().splitlines(), open(c).read().splitlines()
    assert len(la) == len(lc)
    assert [x.split()[1:] for x in la[1:]] == [x.split()[1:] for x in lc[1:]]
