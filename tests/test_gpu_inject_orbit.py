"""pdd_inject_orbit on the GPU (pypulsar_amd/inject.py, csrc/pdd_inject.hip)
against the NumPy restatement of its cell arithmetic
(tests/inject_orbit_oracle.py::inject_arrays on the injector's own job tables),
bit for bit, uint8 and float32."""
import numpy as np
import pytest

import inject_oracle as io
import inject_orbit_oracle as ioo
from conftest import band

pytestmark = pytest.mark.gpu
DT = 64e-6
N = 130  # five orbit tiles of 32 rows (three plain ones of 64), the last partial
T0S = [0, (1 << 33) + 7]


def _jobs(t0, n=N, inside=False):
    """An orbital pulsar, a plain one with fd != 0, a burst, an orbital pulsar
    with e = 0.6 -- in this order (the float32 sums are ordered).  ``inside``:
    the first job begins and ends inside a tile."""
    from pypulsar_amd.inject import BurstSignal, PulsarSignal
    tb = t0 * DT
    rng = dict(start=t0 + 37, stop=t0 + 59) if inside else {}
    return [PulsarSignal(f=311.0, dm=35.0, amp=9.0, phi0=0.21, width=0.08, pb=0.9, x=4e-3, t0=0.2,
                         **rng),
            PulsarSignal(f=97.3, dm=12.0, amp=-6.0, fd=3e-2, fdd=-2e-3, width=0.2, tau=2e-4),
            BurstSignal(t=tb + 0.4 * n * DT, dm=60.0, amp=300.0, width=5e-4, tau=3e-4),
            PulsarSignal(f=61.0, dm=80.0, amp=7.0, fd=1e-3, width=0.03, pb=2.5, x=0.01, e=0.6,
                         omega=1.0, t0=-0.4, stop=t0 + n - 9)]


_CACHE = {}


def _injector(C, t0, kind="mixed", seed=11):
    from pypulsar_amd.inject import Injector, PulsarSignal
    key = (C, t0, kind, seed)
    if key not in _CACHE:
        freqs = band(C) if C > 1 else np.array([1400.0])
        if kind == "mixed":
            sigs = _jobs(t0)
        elif kind == "inside":
            sigs = _jobs(t0, inside=True)
        elif kind == "wrap":
            # pb = 50 samples at beta = 0.05: m = 6, psi wraps 2.6 times in 130 rows
            sigs = [PulsarSignal(f=20.0, dm=35.0, amp=40.0, width=0.1, pb=50 * DT,
                                 x=0.05 * 50 * DT / (2 * np.pi), t0=3e-4)]
        elif kind == "m17":
            sigs = [PulsarSignal(f=500.0, dm=35.0, amp=40.0, width=0.1, pb=600.0, x=2.0, t0=100.0)]
        else:
            sigs = [s for s in _jobs(t0) if getattr(s, "orbit", None) is None]
        _CACHE[key] = Injector(sigs, freqs, DT, nbins=256, seed=seed)
    return _CACHE[key]


def _data(n, ld, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, ld)).astype(np.uint8)
    return rng.normal(100.0, 20.0, (n, ld)).astype(np.float32)


def _want(it, x, t0, C):
    """the backing array [n, ld] with its first C columns injected"""
    out = x.copy()
    out[:, :C] = ioo.inject_arrays(x[:, :C], t0, *it.host_arrays(), *it.orbit_arrays(), B=it.B,
                                   seed=it.seed, vmax=it.vmax)
    return out


def _run(it, x, t0, C, cuts=()):
    import torch
    xd = torch.from_numpy(x.copy()).cuda()
    edges = [0] + list(cuts) + [x.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        it.apply(xd[a:b, :C], t0 + a)
    torch.cuda.synchronize()
    return xd.cpu().numpy()


def _check(it, C, ld, t0, dtype, n=N, cuts=()):
    x = _data(n, ld, dtype, seed=C)
    want = _want(it, x, t0, C)
    assert not np.array_equal(want, x)
    got = _run(it, x, t0, C, cuts)
    assert np.array_equal(got, want), int((got != want).sum())
    return want


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("t0", T0S)
def test_four_channels_a_thread(gpu, t0, dtype):
    it = _injector(8, t0)
    assert list(it.orbit_arrays()[1][:, 0] >= 0) == [True, False, False, True]
    want = _check(it, 8, 8, t0, dtype)
    # the orbit is in the bytes: the same jobs without their orbits give others
    x = _data(N, 8, dtype, seed=8)
    assert not np.array_equal(want, io.inject_arrays(x, t0, *it.host_arrays(), B=it.B, seed=it.seed))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("C,ld", [(5, 5), (8, 9)])
def test_one_channel_a_thread(gpu, C, ld, dtype):
    _check(_injector(C, 12345), C, ld, 12345, dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_two_channel_groups_and_a_range_inside_a_tile(gpu, dtype):
    t0 = (1 << 33) + 7
    _check(_injector(260, t0, "inside"), 260, 260, t0, dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("kind,m", [("wrap", 6), ("m17", 17)])
def test_table_sizes_and_wrap(gpu, kind, m, dtype):
    t0 = 7 if kind == "wrap" else (1 << 33) + 7
    it = _injector(8, t0, kind)
    ophase, ometa, qtab = it.orbit_arrays()
    assert ometa[0, 0] == m and qtab.size == (1 << m) + 1
    if kind == "wrap":
        # the orbital phase wraps inside the block and the last knot is read
        step = int(ometa[0, 1])
        psi = [(int(ophase[0, 0]) + (t0 + r) * step) % (1 << 64) for r in range(N)]
        assert sum(b < a for a, b in zip(psi[:-1], psi[1:])) >= 2
        assert any(p >> (64 - m) == (1 << m) - 1 for p in psi)
    _check(it, 8, 8, t0, dtype)
    if kind == "wrap":
        _check(_injector(5, t0, kind), 5, 5, t0, dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_pieces_equal_the_whole(gpu, dtype):
    t0 = (1 << 33) + 7
    _check(_injector(8, t0), 8, 8, t0, dtype, cuts=(1, 63, 64))
    _check(_injector(5, t0), 5, 5, t0, dtype, cuts=(1, 63, 64))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_old_and_new_entry_agree_without_orbits(gpu, dtype):
    import torch
    from pypulsar_amd import _lib
    C, t0 = 8, 12345
    it = _injector(C, t0, "plain")
    assert not it.has_orbits() and len(it.jobs) == 2
    x = _data(N, C, dtype, seed=2)
    want = io.inject_arrays(x, t0, *it.host_arrays(), B=it.B, seed=it.seed)
    assert not np.array_equal(want, x)
    old = _run(it, x, t0, C)
    xd = torch.from_numpy(x.copy()).cuda()
    ph, dr, rg, tb = it._device_arrays(xd.device)
    ometa = it.orbit_arrays()[1]
    assert (ometa[:, 0] == -1).all()
    code = _lib.U8 if dtype == np.uint8 else _lib.F32
    _lib.call("pdd_inject_orbit", _lib.ptr(xd), code, N, C, C, t0, _lib.ptr(ph), _lib.ptr(dr),
              _lib.ptr(rg), _lib.ptr(tb), len(it.jobs), it.B, it.seed, it.vmax, None,
              ometa.ctypes.data, None, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(old, want) and np.array_equal(xd.cpu().numpy(), want)


def test_refused_calls_touch_nothing(gpu):
    import torch
    from pypulsar_amd import _lib
    C, t0 = 8, 0
    it = _injector(C, t0)
    x = _data(N, C, np.uint8, seed=4)
    xd = torch.from_numpy(x.copy()).cuda()
    ph, dr, rg, tb = it._device_arrays(xd.device)
    oph, ometa, qt = it._device_orbit_arrays(xd.device)
    h = _lib.lib()
    for bad in ((0, 0, 5), (0, 0, 23), (0, 2, -8), (0, 2, 12), (3, 2, 8 * qt.numel())):
        meta = ometa.copy()
        meta[bad[0], bad[1]] = bad[2]
        assert h.pdd_inject_orbit(_lib.ptr(xd), _lib.U8, N, C, C, t0, _lib.ptr(ph), _lib.ptr(dr),
                                  _lib.ptr(rg), _lib.ptr(tb), len(it.jobs), it.B, it.seed, it.vmax,
                                  _lib.ptr(oph), meta.ctypes.data, _lib.ptr(qt), qt.numel(),
                                  _lib.stream_ptr()) == -1, bad
        assert h.pdd_last_error().startswith(b"pdd_inject_orbit:")
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)
