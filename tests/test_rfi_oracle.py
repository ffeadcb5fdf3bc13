"""RFI excision on the CPU: the oracle's rule recovers the injected cells of
the seeded inputs with margins (so the GPU comparison in test_gpu_rfi.py
cannot sit on a coin flip), the host-side decision of pypulsar_amd.rfi equals
the oracle's, and an RFIMask survives the ``.mask`` round trip through
formats/rfifind.py."""
import numpy as np
import pytest
from scipy.stats import norm

import rfi_oracle as ro

# largest relative difference of `pow` between the oracle with its transform
# in float32 and in float64, over the inputs of test_gpu_rfi.py (measured:
# 2.6e-7 .. 4.3e-7); the device bound is 4 x this (another butterfly order)
POW_REL_F32 = 4.5e-7


@pytest.fixture(scope="module", params=sorted(ro.CASES))
def case(request):
    P, nint, C, seed = ro.CASES[request.param]
    x, want = ro.make_input(P, nint, C, seed)
    return P, x, want, ro.stats(x, P)


def test_power_threshold():
    from pypulsar_amd import rfi
    for P, val in ((256, 15.21), (1024, 16.60)):
        nb = P // 2
        thr = -np.log(1.0 - (1.0 - norm.sf(4.0)) ** (1.0 / nb))
        assert abs(thr - val) < 0.005
        assert abs(ro.pthr(4.0, P) - thr) < 1e-9
        assert abs(rfi.power_threshold(4.0, P) - thr) < 1e-8 * thr


def test_oracle_recovers_injections_with_margin(case):
    P, x, want, (avg, std, pw) = case
    margins = []
    mask = ro.decide(avg, std, pw, P, margins=margins)
    np.testing.assert_array_equal(mask, want)
    m = np.asarray(margins)
    assert m.size and not np.any((m > 0.99) & (m < 1.01)), m[(m > 0.99) & (m < 1.01)]
    # (pow on the flagged side of its threshold too)
    thr = ro.pthr(4.0, P)
    assert not np.any((pw > 0.99 * thr) & (pw < 1.01 * thr))


def test_host_decision_equals_oracle(case):
    from pypulsar_amd import rfi
    P, x, want, (avg, std, pw) = case
    np.testing.assert_array_equal(rfi.decide(avg, std, pw, P), ro.decide(avg, std, pw, P))
    mask = ro.decide(avg, std, pw, P)
    np.testing.assert_array_equal(rfi.channel_fill(avg, mask), ro.fill(avg, mask))
    # a channel without an unflagged interval takes the band median
    f = ro.fill(avg, mask)
    dead = np.flatnonzero(mask.all(axis=0))
    assert dead.size and np.all(f[dead] == np.median(f[~mask.all(axis=0)]))


def test_float32_transform_bound():
    worst = 0.0
    for name in sorted(ro.CASES):
        P, nint, C, seed = ro.CASES[name]
        for dtype in (np.uint8, np.float32):
            x, _ = ro.make_input(P, nint, C, seed, dtype)
            _, _, p64 = ro.stats(x, P)
            _, _, p32 = ro.stats(x, P, np.float32)
            nz = p64 > 0
            worst = max(worst, float(np.max(np.abs(p32[nz] - p64[nz]) / p64[nz])))
    x = ro.small_input()[:, :16]
    for xx in (x, x.astype(np.float32) * 0.37):
        _, _, p64 = ro.stats(xx, 100)
        _, _, p32 = ro.stats(xx, 100, np.float32)
        worst = max(worst, float(np.max(np.abs(p32 - p64) / p64)))
    print("float32 transform: max relative pow difference %.3g" % worst)
    assert worst <= POW_REL_F32


def test_mask_file_round_trip(tmp_path):
    from pypulsar_amd import rfi
    from pypulsar_amd.formats import rfifind
    rng = np.random.default_rng(5)
    nint, C, P = 7, 40, 96
    mask = rng.random((nint, C)) < 0.1
    mask[:, 11] = True   # a fully zapped channel
    mask[4, :] = True    # a fully zapped interval
    fill = rng.normal(100, 5, C)
    m = rfi.RFIMask(mask, P, fill, time_sig=9.0, freq_sig=3.5, mjd=55000.25, tsamp=64e-6,
                    lofreq=1250.5, df=0.25)
    fn = str(tmp_path / "x_rfifind.mask")
    m.write(fn)
    r = rfifind.rfifind(fn)
    assert (r.nchan, r.nint, r.ptsperint) == (C, nint, P)
    assert (r.time_sig, r.freq_sig, r.MJD, r.lofreq, r.df) == (9.0, 3.5, 55000.25, 1250.5, 0.25)
    assert r.dtint == P * 64e-6
    assert r.mask_zap_chans == {11}
    assert list(r.mask_zap_ints) == [4]
    got = rfifind.get_mask(r, 0, nint * P)
    np.testing.assert_array_equal(got, np.repeat(mask, P, axis=0).T)
    back = rfi.RFIMask.from_file(fn, fill=fill)
    np.testing.assert_array_equal(back.mask, mask)
    assert back.ptsperint == P and back.dtint == m.dtint
    assert abs(m.masked_fraction - mask.mean()) < 1e-15
