"""pdd_sb_search / pypulsar_amd.sideband on the device against
tests/sideband_oracle.py: the mini spectra of every mini-FFT length, the
candidate rule on the device's own spectra, the edges, the refused arguments
and the recovery case end to end.

The powers are strided views into buffers whose padding columns hold 7e5: a
lane that read at or beyond column nn of a row would show in every figure."""
import ctypes

import numpy as np
import pytest

import period_oracle as po
import sideband_cases as sc
import sideband_oracle as so

pytestmark = pytest.mark.gpu

NN, NFFT, DT = 40000, 80000, 1e-3   # rlo = ceil(1 Hz * 80 s) = 80
RLO = 80
POISON = 7e5
LOG2S = list(range(5, 15))
SIGMA = 3.5
MINI_BAR = 2e-5                     # the project's float32 bar (the accel correlation's)


def poisoned(torch, host, pad=37):
    """[D, nn] strided device view of ``host`` inside a [D, nn + pad] buffer
    whose padding holds POISON."""
    host = np.asarray(host, dtype=np.float32)
    D, nn = host.shape
    buf = torch.full((D, nn + pad), POISON, dtype=torch.float32, device="cuda")
    view = buf[:, :nn]
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) == nn + pad
    return view


def make_host_powers():
    """Row 0: the whitened powers of a comb (the recovery signal at n = 80000,
    amp 0.12); row 1: exponential noise with one line of power 400; row 2: a
    dead row."""
    rng = np.random.default_rng(7)
    n = NFFT
    t = np.arange(n) * DT
    T = n * DT
    f0 = 20000.4 / T
    x = sc.BETA / (2.0 * np.pi * f0)
    series = rng.standard_normal(n) + 0.12 * np.cos(
        2.0 * np.pi * f0 * (t - x * np.sin(2.0 * np.pi * t * sc.NORB / T + 0.7)))
    p = np.zeros((3, NN), dtype=np.float32)
    p[0] = sc.whitened_powers(series)
    p[1] = rng.exponential(1.0, NN).astype(np.float32)
    p[1, 12345] = 400.0
    return p


@pytest.fixture(scope="module")
def host_powers():
    return make_host_powers()


@pytest.fixture(scope="module")
def dev_powers(gpu, host_powers):
    import torch
    return poisoned(torch, host_powers)


def searcher(**kw):
    from pypulsar_amd.sideband import SidebandSearch
    kw.setdefault("max_cands", 1 << 16)
    return SidebandSearch(**kw)


def device_set(s, powers, nfft=NFFT, dt=DT):
    """(cands as a set of (row, L, lo, q, H, bits), count, number of records)."""
    import torch
    c, k = s.raw(powers, nfft, dt)
    torch.cuda.synchronize()
    k = int(k.item())
    rec = c[:min(k, s.max_cands)].cpu().numpy()
    return {(int(r[0]), 1 << int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]))
            for r in rec}, k, len(rec)


def oracle_set(dump, L, harms, sigma, qlo, shift, nn=NN, rlo=RLO):
    """The oracle's candidates of a device dump [D, nseg, L]."""
    thr = np.asarray([po.threshold_power(sigma, h) for h in harms], dtype=np.float32)
    los = so.segments(nn, rlo, L, shift)
    assert dump.shape[1:] == (len(los), L)
    return {(d, L, int(los[j]), q, H, bits)
            for d in range(dump.shape[0])
            for j, q, H, bits in so.candidates(dump[d], harms, thr, qlo)}


@pytest.mark.parametrize("e", LOG2S)
def test_mini_spectrum(gpu, host_powers, dev_powers, e):
    """max |M - M_ref| / max M_ref against the float64 oracle, the bits of a
    second launch, and the dead row."""
    import torch
    L = 1 << e
    s = searcher(minfft=L, maxfft=L)
    a = s.mini(dev_powers, NFFT, DT, L)
    b = s.mini(dev_powers, NFFT, DT, L)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a.cpu().numpy()
    assert got.shape == (3, len(so.segments(NN, RLO, L)), L) and got.shape[1] >= 1
    assert not got[2].any()
    worst = 0.0
    for d in (0, 1):
        ref = so.mini(host_powers[d], RLO, L, 2, s.clip)
        worst = max(worst, float(np.max(np.abs(got[d] - ref)) / np.max(ref)))
    print("L = %5d: mini spectrum error %.2e (bar %.0e), clip %.3f" % (L, worst, MINI_BAR, s.clip))
    assert np.isfinite(got).all() and got.max() < 1e5
    assert worst <= MINI_BAR


@pytest.mark.parametrize("harms", [(1, 2, 4), (1, 3)])
@pytest.mark.parametrize("e", LOG2S)
def test_candidates_vs_oracle_own_dump(gpu, dev_powers, e, harms):
    L = 1 << e
    s = searcher(sigma_threshold=SIGMA, minfft=L, maxfft=L, harms=harms, qlo=4)
    got, k, nrec = device_set(s, dev_powers)
    want = oracle_set(s.mini(dev_powers, NFFT, DT, L).cpu().numpy(), L, harms, SIGMA, 4, 2)
    print("L = %5d harms %s: %d candidates" % (L, harms, k))
    assert k == nrec == len(got), "duplicates or overflow"
    assert k > 10
    assert got == want
    assert not any(c[0] == 2 for c in got)


@pytest.mark.parametrize("shift,clip", [(0, "auto"), (3, "auto"), (2, 0.0), (1, 5.0)])
def test_shift_and_clip(gpu, host_powers, dev_powers, shift, clip):
    L = 128
    s = searcher(sigma_threshold=SIGMA, minfft=L, maxfft=L, shift=shift, clip=clip)
    dump = s.mini(dev_powers, NFFT, DT, L).cpu().numpy()
    ref = so.mini(host_powers[1], RLO, L, shift, s.clip)
    assert float(np.max(np.abs(dump[1] - ref)) / np.max(ref)) <= MINI_BAR
    got, k, nrec = device_set(s, dev_powers)
    assert k == nrec == len(got) and k > 10
    assert got == oracle_set(dump, L, (1, 2, 4), SIGMA, 4, shift)
    if clip == 0.0:
        # the unclipped line of power 400 floods its segments with maxima
        clipped, _, _ = device_set(searcher(sigma_threshold=SIGMA, minfft=L, maxfft=L), dev_powers)
        on_line = lambda cs: sum(1 for c in cs if c[0] == 1 and c[2] <= 12345 < c[2] + L)  # noqa: E731
        print("candidates on the line's segments: %d unclipped, %d clipped"
              % (on_line(got), on_line(clipped)))
        assert on_line(got) > on_line(clipped)


@pytest.mark.parametrize("e", [5, 8, 11, 14])
def test_one_segment_and_none(gpu, host_powers, e):
    """nn - rlo == L: one segment, read to the last column and no further;
    nn - rlo == L - 1: nothing, count stays 0."""
    import torch
    L = 1 << e
    rlo = 3
    s = searcher(sigma_threshold=2.0, minfft=L, maxfft=L, flo=rlo / (NFFT * DT))
    assert s.rlo(NFFT, DT) == rlo
    p = poisoned(torch, host_powers[:, 100:100 + rlo + L])
    dump = s.mini(p, NFFT, DT, L).cpu().numpy()
    assert dump.shape == (3, 1, L)
    ref = so.mini(host_powers[1, 100:100 + rlo + L], rlo, L, 2, s.clip)
    assert float(np.max(np.abs(dump[1] - ref)) / np.max(ref)) <= MINI_BAR
    got, k, _ = device_set(s, p)
    assert k == len(got)
    assert got == oracle_set(dump, L, (1, 2, 4), 2.0, 4, 2, nn=rlo + L, rlo=rlo)
    assert {c[2] for c in got} <= {rlo}
    short = poisoned(torch, host_powers[:, 100:100 + rlo + L - 1])
    got, k, _ = device_set(s, short)
    assert k == 0 and not got
    assert s.mini(short, NFFT, DT, L).shape == (3, 0, L)


def test_no_rows_and_overflow(gpu, dev_powers):
    s = searcher(sigma_threshold=SIGMA, minfft=64, maxfft=256)
    got, k, _ = device_set(s, dev_powers[:0])
    assert k == 0 and not got
    full, k, _ = device_set(s, dev_powers)
    assert k == len(full) > 50
    assert {c[1] for c in full} == {64, 128, 256}     # one shared cands / count pair
    small = searcher(sigma_threshold=SIGMA, minfft=64, maxfft=256, max_cands=5)
    c, cnt = small.raw(dev_powers, NFFT, DT)
    assert int(cnt.item()) == k                        # the count goes on
    got = {(int(r[0]), 1 << int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]))
           for r in c.cpu().numpy()}
    assert len(got) == 5 and got <= full
    with pytest.raises(RuntimeError, match="exceed max_cands"):
        small.collect(c, cnt, np.zeros(3), NFFT, DT)
    rec = s.collect(*s.raw(dev_powers, NFFT, DT), dms=np.arange(3.0), nfft=NFFT, dt=DT)
    assert len(rec) == k
    order = list(zip(rec["row"], rec["L"], rec["lo"], rec["numharm"], rec["q"]))
    assert order == sorted(order)
    T = NFFT * DT
    assert np.allclose(rec["porb"], rec["q"] * T / (2.0 * rec["L"]))
    assert np.allclose(rec["freq_lo"], rec["lo"] / T)
    assert np.allclose(rec["freq_hi"], (rec["lo"] + rec["L"]) / T)
    assert np.allclose(rec["freq"], 0.5 * (rec["freq_lo"] + rec["freq_hi"]))
    assert np.array_equal(rec["DM"], rec["row"].astype(np.float64))


def test_ties_and_range_edges(gpu):
    """Small-integer powers of period 4, (4, 0, 2, 2): every segment of L = 32
    has A_0 = 64, A_8 = 16 + 16i, A_16 = 32 and nothing else, so -- exactly, in
    float32 as on paper -- M is 0 but for M[0] = 32, M[1] = 32 c, M[15] = M[17]
    = 4 c, M[16] = 4 and M[31] = 8 c (c = pi^2 / 16).  With thresholds of 0 the
    zeros tie everywhere; stage 1 has its maximum at q = L - 1, stage 2 at q =
    L / 2 - 1 and stage 4 at q = qlo = 4: the neighbours outside count as
    -inf."""
    import torch
    L, rlo, nseg_ = 32, 5, 71     # two workgroups, the second one partly filled
    nn = rlo + L + 8 * (nseg_ - 1) + 7
    pat = np.asarray([4, 0, 2, 2], dtype=np.float32)
    host = np.tile(pat[(np.arange(nn) - rlo) % 4], (2, 1))   # (the pattern starts at rlo)
    s = searcher(minfft=L, maxfft=L, harms=(1, 2, 4), clip=0.0, flo=rlo / (NFFT * DT))
    s.thr[:] = 0.0
    p = poisoned(torch, host)
    got, k, nrec = device_set(s, p)
    c = np.float32(np.pi ** 2 / 16)
    M = np.zeros((1, L), dtype=np.float32)
    M[0, 0], M[0, 1], M[0, 15], M[0, 16], M[0, 17], M[0, 31] = 32, 32 * c, 4 * c, 4, 4 * c, 8 * c
    # (the float64 oracle agrees, up to its rounding residue in the zeros)
    assert np.allclose(so.mini(host[0], rlo, L, 2, 0.0), M, rtol=1e-6, atol=1e-12)
    dump = s.mini(p, NFFT, DT, L).cpu().numpy()
    assert dump.shape == (2, nseg_, L)
    assert np.allclose(dump, M[None], rtol=1e-6, atol=1e-12)
    per_seg = so.candidates(M, (1, 2, 4), (0.0, 0.0, 0.0), 4)
    keys = {(q, H) for _, q, H, _ in per_seg}
    assert {(31, 1), (16, 1), (15, 2), (8, 2), (4, 4)} <= keys
    want = {(d, L, rlo + 8 * j, q, H) for d in range(2) for j in range(nseg_) for q, H in keys}
    assert k == nrec == len(got)
    assert {c_[:5] for c_ in got} == want
    powers = {(q, H): np.asarray([b], np.int32).view(np.float32)[0] for _, q, H, b in per_seg}
    for c_ in got:
        v = np.asarray([c_[5]], np.int32).view(np.float32)[0]
        assert np.isclose(v, powers[c_[3], c_[4]], rtol=1e-6, atol=1e-12)


def test_bad_arguments(gpu, dev_powers):
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.sideband import twiddle_table
    tw = torch.from_numpy(twiddle_table(128)).cuda()
    cands = torch.zeros((16, 6), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    harms = np.asarray([1, 2, 4], dtype=np.int32)
    thr = np.asarray([50.0, 50.0, 50.0], dtype=np.float32)

    def go(nn=NN, ld=dev_powers.stride(0), rlo=RLO, log2L=7, shift=2, h=harms, nharm=3, qlo=4):
        _lib.call("pdd_sb_search", _lib.ptr(dev_powers), 3, nn, ld, rlo, log2L, shift,
                  ctypes.c_float(0.0), h.ctypes.data_as(ctypes.c_void_p), nharm,
                  thr.ctypes.data_as(ctypes.c_void_p), qlo, _lib.ptr(tw), None, _lib.ptr(cands), 16,
                  _lib.ptr(count), _lib.stream_ptr())

    go()  # the good call
    torch.cuda.synchronize()
    before = int(count.item())
    bad = [dict(log2L=4), dict(log2L=15), dict(shift=-1), dict(shift=4), dict(nharm=0),
           dict(nharm=5), dict(h=np.asarray([1, 1, 2], np.int32)),
           dict(h=np.asarray([2, 1, 4], np.int32)), dict(h=np.asarray([0, 1, 2], np.int32)),
           dict(h=np.asarray([1, 2, 9], np.int32)), dict(qlo=0), dict(qlo=17),
           dict(ld=NN - 1), dict(rlo=0)]
    for kw in bad:
        with pytest.raises(_lib.PddError, match="pdd_sb_search"):
            go(**kw)
    torch.cuda.synchronize()
    assert int(count.item()) == before  # (nothing was launched)


def test_recovery_end_to_end(gpu):
    """The recovery case, seed 1, as row 1 of a 3-row plane: the best sifted
    candidate is the oracle's, and the plain search has nothing in that row."""
    import torch
    from pypulsar_amd.periodicity import PeriodicitySearch
    from pypulsar_amd.sideband import SidebandSearch, sift
    series = sc.recovery_series(1)
    want = sc.oracle_search(sc.whitened_powers(series))[0]
    rng = np.random.default_rng(99)
    plane = np.stack([rng.standard_normal(sc.N), series, rng.standard_normal(sc.N)])
    dev = torch.from_numpy(plane.astype(np.float32)).cuda()
    dms = np.asarray([0.0, 1.0, 2.0])
    cands = SidebandSearch()(dev, dms, sc.DT)
    best = sift(cands)[0]
    print("device: L=%d lo=%d q=%d H=%d sigma=%.3f; oracle: %r"
          % (best["L"], best["lo"], best["q"], best["numharm"], best["sigma"], want))
    assert (best["row"], best["DM"]) == (1, 1.0)
    assert (best["L"], best["lo"], best["q"], best["numharm"]) == want[1:5]
    assert abs(best["sigma"] - want[0]) <= 1e-3 * want[0]
    assert abs(best["porb"] - sc.PORB) <= sc.N * sc.DT / (2.0 * best["L"])
    assert best["freq_lo"] <= sc.F0 < best["freq_hi"]
    plain = PeriodicitySearch(6.0)(dev, dms, sc.DT)
    assert not np.any(plain["row"] == 1)
