"""pdd_inject on the GPU (pypulsar_amd/inject.py, csrc/pdd_inject.hip)
against the NumPy restatement of its cell arithmetic
(tests/inject_oracle.py::inject_arrays on the injector's own job tables), bit
for bit, uint8 and float32."""
import numpy as np
import pytest

import inject_oracle as io
from conftest import band

pytestmark = pytest.mark.gpu
DT = 64e-6
T0S = [0, 12345, (1 << 32) + 7]
NS = [1, 63, 65, 4099]


def _signals(J, t0, n=4099):
    """J signals around the block [t0, t0 + n): pulsars (with fd, fdd and a
    [start, stop) range among them) and bursts, some of which begin before
    and end after the block."""
    from pypulsar_amd.inject import BurstSignal, PulsarSignal
    tb = t0 * DT
    span = n * DT
    base = [
        PulsarSignal(f=97.3, dm=35.0, amp=9.0, fd=3e-2, fdd=-2e-3, phi0=0.21, width=0.08,
                     start=t0 + 40, stop=t0 + n - 70),
        # a sweep longer than the block: begins before, ends after it
        BurstSignal(t=tb - 0.05, dm=320.0, amp=40.0, width=2e-3, spectral_index=-1.0),
        PulsarSignal(f=431.0, dm=12.0, amp=-6.0, width=0.2, tau=2e-4),
        # a pulse wider than the block
        BurstSignal(t=tb + 0.5 * span, dm=5.0, amp=25.0, width=0.4),
        BurstSignal(t=tb + 0.3 * span, dm=60.0, amp=300.0, width=5e-4, tau=3e-4),
        PulsarSignal(f=11.0, dm=80.0, amp=4.0, fdd=5e-3, phi0=0.9, width=0.02, stop=t0 + n // 2),
    ]
    out = []
    rng = np.random.default_rng(J)
    while len(out) < J:
        k = len(out)
        if k < len(base):
            out.append(base[k])
        elif k % 2:
            out.append(BurstSignal(t=tb + float(rng.uniform(-0.1, 1.1)) * span,
                                   dm=float(rng.uniform(0, 200)), amp=float(rng.uniform(5, 60)),
                                   width=float(rng.uniform(2e-4, 3e-3))))
        else:
            out.append(PulsarSignal(f=float(rng.uniform(2, 500)), dm=float(rng.uniform(0, 100)),
                                    amp=float(rng.uniform(-3, 6)), fd=float(rng.uniform(-1e-2, 1e-2)),
                                    width=float(rng.uniform(0.02, 0.3))))
    return out


_CACHE = {}


def _injector(C, B, J, t0, seed=11, vmax=255, descending=True):
    from pypulsar_amd.inject import Injector
    key = (C, B, J, t0, seed, vmax, descending)
    if key not in _CACHE:
        freqs = band(C, descending=descending) if C > 1 else np.array([1400.0])
        _CACHE[key] = Injector(_signals(J, t0), freqs, DT, nbins=B, seed=seed, vmax=vmax)
    return _CACHE[key]


def _data(n, ld, dtype, seed=0, lo=0, hi=256):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(lo, hi, (n, ld)).astype(np.uint8)
    return rng.normal(100.0, 20.0, (n, ld)).astype(np.float32)


def _want(it, x, t0, C, vmax=None):
    """the backing array [n, ld] with its first C columns injected"""
    out = x.copy()
    out[:, :C] = io.inject_arrays(x[:, :C], t0, *it.host_arrays(), B=it.B, seed=it.seed,
                                  vmax=it.vmax if vmax is None else vmax)
    return out


def _run(it, x, t0, C, stream=None):
    import torch
    xd = torch.from_numpy(x.copy()).cuda()
    ret = it.apply(xd[:, :C], t0, stream=stream)
    assert ret.data_ptr() == xd.data_ptr()
    torch.cuda.synchronize()
    return xd.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("pad", [0, 16])
@pytest.mark.parametrize("C", [1, 13, 60, 64, 272])
def test_shapes(gpu, C, pad, dtype):
    t0 = 12345
    it = _injector(C, 64, 3, t0)
    for n in NS:
        x = _data(n, C + pad, dtype, seed=n)
        got = _run(it, x, t0, C)
        want = _want(it, x, t0, C)
        assert n < 4099 or not np.array_equal(want, x)
        assert np.array_equal(got, want), (n, int((got != want).sum()))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("B,J,t0,C", [(4096, 1, 0, 60), (4096, 3, (1 << 32) + 7, 13),
                                      (64, 64, (1 << 32) + 7, 60), (1024, 6, 0, 272),
                                      (64, 64, 0, 13), (256, 6, 12345, 64)])
def test_jobs_tables_and_start_samples(gpu, B, J, t0, C, dtype):
    it = _injector(C, B, J, t0, descending=(J != 6))
    n = 4099
    x = _data(n, C, dtype, seed=J)
    got = _run(it, x, t0, C)
    want = _want(it, x, t0, C)
    assert not np.array_equal(want, x)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_column_offset_view(gpu, dtype):
    """C and ld are multiples of 4 but the view starts one column in, so its
    pointer is not aligned to four cells: the per-element path, and the
    columns on both sides of the view keep their values."""
    import torch
    C, t0, n = 64, 12345, 4099
    it = _injector(C, 64, 3, t0)
    x = _data(n, C + 16, dtype, seed=5)
    xd = torch.from_numpy(x.copy()).cuda()
    view = xd[:, 1:C + 1]
    assert view.data_ptr() % (4 * x.itemsize) != 0 and view.stride(0) % 4 == 0
    it.apply(view, t0)
    want = x.copy()
    want[:, 1:C + 1] = io.inject_arrays(x[:, 1:C + 1], t0, *it.host_arrays(), B=it.B, seed=it.seed,
                                        vmax=it.vmax)
    assert not np.array_equal(want, x)
    assert np.array_equal(xd.cpu().numpy(), want)


@pytest.mark.parametrize("level", [0, 255])
def test_clip_at_both_ends(gpu, level):
    from pypulsar_amd.inject import Injector, PulsarSignal
    C, t0 = 64, 0
    it = Injector([PulsarSignal(f=97.3, dm=35.0, amp=40.0, width=0.08),
                   PulsarSignal(f=61.0, dm=10.0, amp=-40.0, width=0.1, fd=1e-2)], band(C), DT,
                  nbins=256, seed=4)
    x = np.full((4099, C), level, dtype=np.uint8)
    got = _run(it, x, t0, C)
    want = _want(it, x, t0, C)
    assert np.array_equal(got, want)
    # the clip acted: some sums fell outside 0..255
    assert (want == level).sum() > 0 and (want != level).sum() > 0


def test_vmax_3(gpu):
    C, t0 = 60, 12345
    it = _injector(C, 64, 3, t0, vmax=3)
    x = _data(4099, C, np.uint8, lo=0, hi=4)
    got = _run(it, x, t0, C)
    assert np.array_equal(got, _want(it, x, t0, C)) and got.max() == 3
    # the call's vmax overrides the injector's
    import torch
    it255 = _injector(C, 64, 3, t0)
    xd = torch.from_numpy(x.copy()).cuda()
    it255.apply(xd, t0, vmax=3)
    assert np.array_equal(xd.cpu().numpy(), _want(it255, x, t0, C, vmax=3))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_other_stream_and_split_invariance(gpu, dtype):
    import torch
    C, t0, n = 272, (1 << 32) + 7, 4099
    it = _injector(C, 64, 3, t0)
    x = _data(n, C, dtype, seed=3)
    want = _want(it, x, t0, C)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        xd = torch.from_numpy(x.copy()).cuda()
        it.apply(xd, t0, stream=st)
    st.synchronize()
    assert np.array_equal(xd.cpu().numpy(), want)
    # one call equals two calls on the halves at their own start samples
    for cut in (2048, 1, 4098, 63):
        yd = torch.from_numpy(x.copy()).cuda()
        it.apply(yd[:cut], t0)
        it.apply(yd[cut:], t0 + cut)
        assert np.array_equal(yd.cpu().numpy(), want), cut


def test_nothing_to_do_leaves_every_byte(gpu):
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd.inject import BurstSignal, Injector, PulsarSignal
    C, n = 60, 4099
    freqs = band(C)
    x = _data(n, C + 16, np.uint8, seed=8, lo=0, hi=256)
    x[:7] = 255  # above a small vmax: an untouched cell is not clipped either
    # J = 0
    assert np.array_equal(_run(Injector([], freqs, DT), x, 0, C), x)
    # jobs whose ranges miss the block
    far = Injector([BurstSignal(t=50.0, dm=10.0, amp=90.0, width=1e-3),
                    PulsarSignal(f=30.0, dm=10.0, amp=50.0, start=n + 5, stop=n + 900),
                    PulsarSignal(f=30.0, dm=10.0, amp=50.0, start=0, stop=0)], freqs, DT, nbins=64,
                   vmax=3)
    assert np.array_equal(_run(far, x, 0, C), x)
    assert not np.array_equal(_run(far, x, n + 5, C), x)
    # refused calls touch nothing
    xd = torch.from_numpy(x.copy()).cuda()
    ph, dr, rg, tb = far._device_arrays(xd.device)
    h = _lib.lib()

    def call(n_=n, C_=C, ld=C + 16, t0=0, J=3, B=64, seed=0, vmax=255, dtype=_lib.U8, tab=tb):
        return h.pdd_inject(_lib.ptr(xd), dtype, n_, C_, ld, t0, _lib.ptr(ph), _lib.ptr(dr),
                            _lib.ptr(rg), None if tab is None else _lib.ptr(tab), J, B, seed, vmax,
                            _lib.stream_ptr())

    for kw in (dict(J=65), dict(J=-1), dict(B=32), dict(B=8192), dict(B=96), dict(vmax=0),
               dict(vmax=256), dict(seed=1 << 32), dict(seed=-1), dict(ld=C - 1), dict(t0=-1),
               dict(n_=-1), dict(C_=0), dict(dtype=_lib.U16), dict(tab=None),
               dict(t0=(1 << 52))):
        assert call(**kw) == -1, kw
        assert h.pdd_last_error().startswith(b"pdd_inject"), kw
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)
    assert h.pdd_inject(None, _lib.U8, n, C, C, 0, None, None, None, None, 0, 64, 0, 255, None) == -1
    assert call(n_=0) == 0 and call(J=0, tab=None) == 0
    assert np.array_equal(xd.cpu().numpy(), x)
