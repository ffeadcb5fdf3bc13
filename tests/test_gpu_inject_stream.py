"""The injector in the stream (StreamingSweep / StreamingSearch(injector=...))
and in pulsar_search.search_file: the planes and candidates of a run that
injects block by block equal, bit for bit, those of the same run over the
array injected whole with Injector.apply(..., 0) first."""
import numpy as np
import pytest

from conftest import band, u8_data

pytestmark = pytest.mark.gpu
DT = 64e-6
C, BLOCK, NBLK = 128, 8192, 3
N = BLOCK * (NBLK - 1) + 5000
DMS = np.linspace(0.0, 150.0, 32)


def _injector(vmax=255):
    from pypulsar_amd.inject import BurstSignal, Injector, PulsarSignal
    sigs = [PulsarSignal(f=57.3, dm=60.0, amp=3.0, fd=0.5, phi0=0.3, width=0.06),
            # across the first seam, its sweep reaching into the overlap
            BurstSignal(t=(BLOCK - 300) * DT, dm=120.0, amp=30.0, width=6e-4),
            BurstSignal(t=(2 * BLOCK + 100) * DT, dm=40.0, amp=20.0, width=1.5e-3, tau=4e-4),
            PulsarSignal(f=3.7, dm=10.0, amp=-2.0, width=0.2, start=3000, stop=BLOCK + 4000)]
    return Injector(sigs, band(C), DT, nbins=256, seed=5, vmax=vmax)


def _chunks(x):
    import torch
    return [torch.from_numpy(x[i:i + BLOCK]).pin_memory() for i in range(0, len(x), BLOCK)]


def _planes(st, chunks, **kw):
    import torch
    out = [(t0, p.cpu().numpy()) for t0, p in st(chunks, **kw)]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for (ta, pa), (tb, pb) in zip(a, b):
        assert ta == tb and pa.shape == pb.shape
        np.testing.assert_array_equal(pa, pb)


@pytest.mark.parametrize("ds", [1, 2])
@pytest.mark.parametrize("mode", ["wrap", "int", "float", "none"])
def test_stream_equals_stream_of_injected_array(gpu, mode, ds):
    import torch
    from pypulsar_amd.stream import StreamingSweep
    it = _injector()
    x = u8_data(N, C, 31)
    pre = it.apply(torch.from_numpy(x).cuda(), 0).cpu().numpy()
    assert not np.array_equal(pre, x)
    plain = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=ds, zero_dm=mode)
    want = _planes(plain, _chunks(pre))
    clean = _planes(plain, _chunks(x))
    plain.close()
    st = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=ds, zero_dm=mode, injector=it)
    assert st.ov > 0
    got = _planes(st, _chunks(x))
    _same(got, want)
    assert not np.array_equal(got[0][1], clean[0][1])
    # a resumed run
    _same(_planes(st, _chunks(x)[1:], start_block=1), want[1:])
    st.close()


def test_stream_float32_and_mask_order(gpu):
    """float32 blocks; and with a mask the injected signal is excised too
    (the injector runs before the mask)."""
    import torch
    from pypulsar_amd.rfi import RFIMask
    from pypulsar_amd.stream import StreamingSweep
    it = _injector()
    x = u8_data(N, C, 37).astype(np.float32)
    pre = it.apply(torch.from_numpy(x).cuda(), 0).cpu().numpy()
    mask = np.zeros((N // 1024 + 1, C), dtype=bool)
    mask[7:9] = True   # the intervals of the first burst
    mask[:, 5] = True
    rm = RFIMask(mask, 1024, np.full(C, 128.0))
    for kw in ({}, dict(rfimask=rm)):
        plain = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="float",
                               dtype=torch.float32, **kw)
        want = _planes(plain, _chunks(pre))
        plain.close()
        st = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="float",
                            dtype=torch.float32, injector=it, **kw)
        _same(_planes(st, _chunks(x)), want)
        st.close()


def test_stream_2bit_packed(gpu):
    """Packed input with an injector: unpacked (never the fused prologue),
    clipped to 2^nbits - 1; equal to the 8-bit stream of the values injected
    whole with vmax = 3."""
    import torch
    from lowbit_oracle import lowbit_data
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.stream import StreamingSweep
    it = _injector()
    x = lowbit_data(N, C, 2, 41)
    pre = it.apply(torch.from_numpy(x).cuda(), 0, vmax=3).cpu().numpy()
    assert pre.max() == 3 and not np.array_equal(pre, x)
    plain = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="int")
    want = _planes(plain, _chunks(pre))
    plain.close()
    st = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="int", nbits=2,
                        injector=it)
    assert not st.fused and st.unpacked is not None
    no_inj = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="int", nbits=2)
    assert no_inj.fused  # (without an injector this geometry takes the fused prologue)
    no_inj.close()
    _same(_planes(st, _chunks(sigproc.pack_bits(x, 2))), want)
    st.close()


def test_without_an_injector_nothing_changes(gpu):
    from pypulsar_amd.stream import StreamingSweep
    x = u8_data(N, C, 43)
    a = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="wrap")
    b = StreamingSweep(DMS, band(C), DT, block=BLOCK, downsamp=2, zero_dm="wrap", injector=None)
    assert a.exact == b.exact and a.mode == b.mode
    _same(_planes(a, _chunks(x)), _planes(b, _chunks(x)))
    a.close()
    b.close()
