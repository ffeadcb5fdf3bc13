"""RFI excision on the GPU (pypulsar_amd.rfi; pdd_rfi.hip): the device
statistics against the oracle (tests/rfi_oracle.py), the mask decided from
them, the in-place replacement, the masked stream against a one-shot run on
the host-masked array, and frb_search --rfifind end to end."""
import os

import numpy as np
import pytest

import rfi_oracle as ro
from conftest import band

pytestmark = pytest.mark.gpu
DT = 64e-6
# relative bound of `pow` (and of all three float32-input statistics): 4 x the
# float32-against-float64 transform difference of the oracle on these inputs
# (4.3e-7 measured, asserted <= 4.5e-7 by test_rfi_oracle.py); the factor 4
# for rocFFT's different butterfly order
POW_RTOL = 4 * 4.5e-7


def _inputs(dtype):
    """{name: (x view [T, C] (numpy), backing array, P)}"""
    out = {}
    for name in sorted(ro.CASES):
        P, nint, C, seed = ro.CASES[name]
        x, _ = ro.make_input(P, nint, C, seed, dtype)
        out[name] = (x, x, P)
    base = ro.small_input()
    if dtype == np.float32:
        base = base.astype(np.float32) * np.float32(0.37)
    out["p100"] = (base[:, :16], base, 100)
    return out


@pytest.fixture(scope="module")
def oracle_stats():
    res = {}
    for dtype in (np.uint8, np.float32):
        for name, (x, base, P) in _inputs(dtype).items():
            res[(np.dtype(dtype).name, name)] = (x, base, P, ro.stats(x, P))
    return res


def _device_stats(base, C, P, **kw):
    import torch
    from pypulsar_amd.rfi import RFIFind
    xd = torch.from_numpy(np.ascontiguousarray(base)).cuda()[:, :C]
    return tuple(a.cpu().numpy() for a in RFIFind(P, **kw).stats(xd))


def _close(got, want, rtol):
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(np.abs(want), 1e-300) * (want != 0))) if want.size else 0.0
    print("max relative error %.3g (bound %.3g)" % (worst, rtol))
    assert np.all(err <= rtol * np.abs(want)), worst


@pytest.mark.parametrize("name", ["p256", "p1024", "p100"])
def test_stats_u8(gpu, oracle_stats, name):
    x, base, P, (avg, std, pw) = oracle_stats[("uint8", name)]
    g_avg, g_std, g_pw = _device_stats(base, x.shape[1], P)
    assert g_avg.dtype == np.float64 and g_avg.shape == avg.shape
    np.testing.assert_array_equal(g_avg, avg)
    np.testing.assert_array_equal(g_std, std)
    _close(g_pw, pw, POW_RTOL)


@pytest.mark.parametrize("name", ["p256", "p1024", "p100"])
def test_stats_f32(gpu, oracle_stats, name):
    x, base, P, want = oracle_stats[("float32", name)]
    got = _device_stats(base, x.shape[1], P)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        _close(g, w, POW_RTOL)


def test_stats_edges(gpu):
    import torch
    from pypulsar_amd.rfi import RFIFind
    rng = np.random.default_rng(8)
    x = np.clip(np.rint(rng.normal(100, 6, (3 * 64 + 5, 20))), 0, 255).astype(np.uint8)
    x[:, 7] = 131  # a constant channel
    for xx in (x, x.astype(np.float32) * np.float32(1.1)):
        avg, std, pw = (a.cpu().numpy() for a in RFIFind(64).stats(torch.from_numpy(xx).cuda()))
        assert avg.shape == (3, 20)
        assert not np.isnan(avg).any() and not np.isnan(std).any() and not np.isnan(pw).any()
        assert np.all(std[:, 7] == 0) and np.all(pw[:, 7] == 0)
        assert np.all(np.delete(std, 7, axis=1) > 0) and np.all(np.delete(pw, 7, axis=1) > 0)
        # T < ptsperint: no interval
        e = RFIFind(64).stats(torch.from_numpy(xx[:63]).cuda())
        assert all(tuple(a.shape) == (0, 20) for a in e)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_stats_channel_batches(gpu, dtype):
    """The workspace forced small (one tile of channels a batch) gives the
    statistics of one batch."""
    from pypulsar_amd.rfi import RFIFind
    rng = np.random.default_rng(9)
    C, P = 300, 64
    x = np.clip(np.rint(rng.normal(100, 6, (4 * P + 5, C))), 0, 255).astype(np.uint8)
    if dtype == np.float32:
        x = x.astype(np.float32) * np.float32(0.9)
    import torch
    assert RFIFind(P, workspace_bytes=1).chan_batch(4, C, torch.from_numpy(x).dtype) < C
    assert RFIFind(P).chan_batch(4, C, torch.from_numpy(x).dtype) == C
    one = _device_stats(x, C, P)
    many = _device_stats(x, C, P, workspace_bytes=1)
    want = ro.stats(x, P)
    np.testing.assert_array_equal(many[0], one[0])
    np.testing.assert_array_equal(many[1], one[1])
    _close(many[2], one[2], POW_RTOL)
    _close(many[2], want[2], POW_RTOL)
    if dtype == np.uint8:
        np.testing.assert_array_equal(one[0], want[0])
        np.testing.assert_array_equal(one[1], want[1])


@pytest.mark.parametrize("name", ["p256", "p1024"])
def test_mask_equals_oracle(gpu, oracle_stats, name):
    """The mask decided from the device statistics equals the oracle's: every
    cell (the margins are asserted by test_rfi_oracle.py)."""
    import torch
    from pypulsar_amd.rfi import RFIFind
    x, base, P, (avg, std, pw) = oracle_stats[("uint8", name)]
    want = ro.decide(avg, std, pw, P)
    finder = RFIFind(P)
    # streamed in three uneven chunks (tails carried over) and in one block
    n = x.shape[0]
    cuts = [0, n // 2 + 11, n // 2 + 11 + n // 3, n]  # (no chunk longer than the first)
    first = cuts[1]
    chunks = [torch.from_numpy(x[a:b]).pin_memory() for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(c.shape[0] <= first for c in chunks)
    g = finder.accumulate(chunks)
    np.testing.assert_array_equal(g[0], avg)
    np.testing.assert_array_equal(g[1], std)
    mask = finder.mask_from_stats(*g)
    np.testing.assert_array_equal(mask.mask, want)
    np.testing.assert_array_equal(mask.mask, ro.make_input(*ro.CASES[name])[1])
    np.testing.assert_array_equal(mask.fill, ro.fill(avg, want))
    one = finder.mask_from_stats(*finder.stats(torch.from_numpy(x).cuda()))
    np.testing.assert_array_equal(one.mask, want)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_apply(gpu, tmp_path, dtype):
    """t0 not a multiple of ptsperint, a block that runs past the bitmap's
    last interval, C = 48 in rows of 64: equals numpy.where(get_mask, fill,
    raw); the padding between rows is untouched."""
    import torch
    from pypulsar_amd.formats import rfifind
    from pypulsar_amd.rfi import RFIMask
    rng = np.random.default_rng(12)
    C, ld, P, nint = 48, 64, 50, 9
    t0, n = 2 * P + 17, 8 * P  # rows t0 .. t0 + n: the bitmap ends at nint P < t0 + n
    mask = rng.random((nint, C)) < 0.15
    mask[:, 5] = True
    mask[6, :] = True
    mask[3, 32:48] = True
    fill = rng.normal(100, 20, C)
    m = RFIMask(mask, P, fill)
    fn = str(tmp_path / "a_rfifind.mask")
    m.write(fn)
    r = rfifind.rfifind(fn)
    raw = rng.integers(0, 256, (n, ld)).astype(np.uint8)
    if dtype == np.float32:
        raw = (raw.astype(np.float32) - np.float32(77.25))
    xd = torch.from_numpy(raw.copy()).cuda()
    m.apply(xd[:, :C], t0)
    got = xd.cpu().numpy()
    n_in = nint * P - t0  # rows inside the bitmap
    f = np.clip(np.rint(fill), 0, 255).astype(np.uint8) if dtype == np.uint8 \
        else fill.astype(np.float32)
    want = raw.copy()
    want[:n_in, :C] = np.where(rfifind.get_mask(r, t0, n_in).T, f[None, :], raw[:n_in, :C])
    assert (want != raw).any()
    np.testing.assert_array_equal(got[:, :C], want[:, :C])
    np.testing.assert_array_equal(got[:, C:], raw[:, C:])
    # an unaligned view (rows of 48 from an odd offset) takes the scalar path
    flat = torch.from_numpy(raw[:, :C].copy().reshape(-1)).cuda()
    pad = torch.cat([flat.new_zeros(1), flat])
    view = pad[1:].view(n, C)
    m.apply(view, t0)
    np.testing.assert_array_equal(view.cpu().numpy(), want[:, :C])
    assert pad[0].item() == 0


@pytest.mark.parametrize("zdm", ["float", "wrap"])
def test_stream_masked(gpu, zdm):
    """StreamingSweep(rfimask=m) over 3 chunks equals, bit for bit, the
    one-shot run on the host-masked array; rfimask=None the unmasked one."""
    import torch
    from oracle import spectra_oracle as orc
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.rfi import RFIMask
    from pypulsar_amd.stream import StreamingSweep
    from pypulsar_amd.sweep import DMSweep
    C, block, ds = 64, 2048, 2
    freqs = band(C)
    dms = np.linspace(0.0, 100.0, 16)
    N = 2 * block + 1000
    rng = np.random.default_rng(31)
    x = np.clip(np.rint(rng.normal(128, 16, (N, C))), 0, 255).astype(np.uint8)
    P = 300  # intervals straddle the block seams; the bitmap ends before the stream does
    nint = 15
    mask = rng.random((nint, C)) < 0.1
    mask[:, 9] = True
    mask[6, :] = True
    fill = rng.normal(128, 10, C)
    m = RFIMask(mask, P, fill)
    xm = x.copy()
    big = np.repeat(mask, P, axis=0)
    xm[:nint * P] = np.where(big, np.clip(np.rint(fill), 0, 255).astype(np.uint8)[None, :],
                             x[:nint * P])
    assert (xm != x).any() and nint * P < N

    def stream(arr, rfimask):
        st = StreamingSweep(dms, freqs, DT, block=block, downsamp=ds, zero_dm=zdm, rfimask=rfimask)
        assert st.ov > 0
        chunks = [torch.from_numpy(arr[i:i + block]).pin_memory() for i in range(0, N, block)]
        assert len(chunks) == 3
        got = np.concatenate([p.cpu().numpy() for _, p in st(chunks)], axis=1)
        st.close()
        return got

    def one_shot(arr):
        if zdm == "wrap":
            return orc.sweep_plane(orc.zdm_int_downsample(arr, ds, "wrap").astype(np.float64),
                                   orc.sweep_table(dms, freqs, DT * ds))
        xd = torch.from_numpy(arr).cuda()
        f32 = torch.empty((C, N // ds), dtype=torch.float32, device="cuda")
        call("pdd_zdm_downsample", ptr(xd), _lib.U8, N, C, C, ds, 1, ptr(f32), f32.stride(0),
             stream_ptr())
        sw = DMSweep(dms, freqs, DT * ds)
        out = sw(f32).cpu().numpy()
        sw.close()
        return out

    want_masked, want_plain = one_shot(xm), one_shot(x)
    assert not np.array_equal(want_masked, want_plain)
    got = stream(x, m)
    assert got.shape == want_masked.shape
    np.testing.assert_array_equal(got, want_masked)
    np.testing.assert_array_equal(stream(x, None), want_plain)


def test_pulsar_search_mask(gpu, tmp_path):
    """pulsar_search --rfifind (one-shot statistics of the resident file)
    leaves the oracle's mask, and --mask with that file gives its candidates."""
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.rfi import RFIMask
    P, nint, C, seed = ro.CASES["p256"]
    x, want = ro.make_input(P, nint, C, seed)
    x = x[:nint * P]
    freqs = band(C)
    params, hdr = sigproc.make_header(C, 8, DT, freqs[0], freqs[1] - freqs[0])
    fn = str(tmp_path / "psr.fil")
    fbm.write_filterbank(fn, params, hdr, x)
    dms = np.linspace(0.0, 20.0, 8)
    a, _ = pulsar_search.search_file(fn, dms, sigma=4.0, rfifind=P * DT)
    mfn = str(tmp_path / "psr_rfifind.mask")
    m = RFIMask.from_file(mfn)
    assert m.ptsperint == P
    np.testing.assert_array_equal(m.mask, want)
    b, _ = pulsar_search.search_file(fn, dms, sigma=4.0, maskfile=mfn)
    plain, _ = pulsar_search.search_file(fn, dms, sigma=4.0)
    np.testing.assert_array_equal(a, b)
    print("%d candidates masked, %d plain" % (len(a), len(plain)))
    assert not np.array_equal(a, plain)


def test_frb_search_rfifind_end_to_end(gpu, tmp_path):
    """A small file with the injections, bursts of narrow-band interference
    and one dispersed pulse: frb_search --rfifind recovers the pulse with
    fewer candidates than the plain run, and waterfaller reads the mask."""
    from pypulsar_amd.bin import frb_search, waterfaller
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.search import read_singlepulse
    P, nint, C = 256, 64, 64
    x, _ = ro.make_input(P, nint, C, 1, np.float32)
    x = x[:nint * P]
    N = x.shape[0]
    freqs = band(C)
    dms = np.linspace(0.0, 100.0, 64)
    dm = dms[32]
    # interference: 6-sample bursts in three neighbouring channels of interval 10
    rng = np.random.default_rng(4)
    for t in 10 * P + rng.choice(P - 8, 5, replace=False):
        x[t:t + 6, 44:47] += 140.0
    # the pulse: 2 samples of +20 a channel along the DM sweep from sample 9000
    from oracle import spectra_oracle as orc
    delay = np.rint((orc.delay_from_DM(dm, freqs) - orc.delay_from_DM(dm, freqs.max())) / DT)
    delay = delay.astype(int)
    for c in range(C):
        x[9000 + delay[c]:9002 + delay[c], c] += 20.0
    x = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    foff = freqs[1] - freqs[0]
    params, hdr = sigproc.make_header(C, 8, DT, freqs[0], foff)
    fn = str(tmp_path / "obs.fil")
    fbm.write_filterbank(fn, params, hdr, x)
    common = ["--lodm", "0", "--hidm", "100", "--numdms", "64", "--downsamp", "1", "--block",
              "4096", "-t", "7"]
    plain, masked = str(tmp_path / "plain.singlepulse"), str(tmp_path / "masked.singlepulse")
    assert frb_search.main(common + ["-o", plain, fn]) == 0
    assert frb_search.main(common + ["--rfifind", "%.6f" % (P * DT), "-o", masked, fn]) == 0
    a, b = read_singlepulse(plain), read_singlepulse(masked)
    print("%d candidates without, %d with --rfifind" % (len(a), len(b)))
    assert len(b) < len(a)
    hit = b[(np.abs(b["DM"] - dm) < 4.0) & (np.abs(b["Sample"] - 9000) < 40)]
    assert len(hit) and hit["Sigma"].max() > 10.0
    mfn = str(tmp_path / "obs_rfifind.mask")
    assert os.path.exists(mfn)
    png = str(tmp_path / "wf.png")
    assert waterfaller.main(["-T", "0.0", "-n", "3000", "-d", "0", "--mask", mfn, "--outfile",
                             png, fn]) == 0
    # the same mask through --mask gives the candidates of --rfifind
    again = str(tmp_path / "again.singlepulse")
    assert frb_search.main(common + ["--mask", mfn, "-o", again, fn]) == 0
    assert len(read_singlepulse(again)) < len(a)
