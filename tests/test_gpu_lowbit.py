"""1-, 2- and 4-bit filterbanks on the GPU: pdd_unpack_bits against the host
codec, the fused packed prologue (pdd_zdm_packed_int_downsample) against
pdd_zdm_int_downsample on the host-unpacked bytes, StreamingSweep(nbits=b) on
packed chunks against the 8-bit stream of the same values, and the two search
CLIs on a packed file and its 8-bit twin.  Every comparison is exact
(integers)."""
import numpy as np
import pytest

from conftest import band
from lowbit_oracle import lowbit_data

pytestmark = pytest.mark.gpu
DT = 64e-6
NBITS = [1, 2, 4]
MODES = {"none": 0, "int": 1, "wrap": 2}


def _pack(x, nbits):
    from pypulsar_amd.formats import sigproc
    return sigproc.pack_bits(x, nbits)


def _padded(rows, ld, fill=0xA5):
    """Device copy of the host rows [n, w] in a buffer whose rows are ``ld``
    bytes apart (the padding holds ``fill``); returns (buffer, view)."""
    import torch
    n, w = rows.shape
    buf = torch.full((max(n, 1), ld), fill, dtype=torch.uint8, device="cuda")
    if n:
        buf[:n, :w] = torch.from_numpy(rows).cuda()
    return buf


# ---------------------------------------------------------------- pdd_unpack_bits
# (nbits, C): 1-byte rows; rows of 145 and 25 bytes (no multiple of the vector
# path's 16 channels); 12-byte rows (the narrow path); and, for every nbits,
# a row the 16-channel vector path takes
UNPACK_CASES = [(1, 8), (1, 1160), (2, 100), (4, 24), (4, 96), (1, 128), (2, 192)]


@pytest.mark.parametrize("pad_in,pad_out", [(0, 0), (16, 0), (0, 16), (5, 3)])
@pytest.mark.parametrize("nbits,C", UNPACK_CASES)
def test_unpack_bits(gpu, nbits, C, pad_in, pad_out):
    """Unpadded, a padded ld_in_bytes, a padded ld_out, and odd strides (which
    take the vector cases down the narrow path too)."""
    import torch
    from pypulsar_amd._lib import call, ptr, stream_ptr
    nspec = 77
    x = lowbit_data(nspec, C, nbits, 10 + nbits)
    p = _pack(x, nbits)
    src = _padded(p, p.shape[1] + pad_in)
    out = torch.full((nspec, C + pad_out), 0x5A, dtype=torch.uint8, device="cuda")
    call("pdd_unpack_bits", ptr(src), nbits, nspec, C, src.stride(0), ptr(out), out.stride(0),
         stream_ptr())
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, :C], x)
    assert (got[:, C:] == 0x5A).all()   # nothing written into the padding


@pytest.mark.parametrize("nbits", NBITS)
def test_unpack_bits_no_spectra(gpu, nbits):
    import torch
    from pypulsar_amd._lib import call, ptr, stream_ptr
    from pypulsar_amd.stream import unpack_bits
    src = torch.zeros((1, 16), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 128), 0x5A, dtype=torch.uint8, device="cuda")
    call("pdd_unpack_bits", ptr(src), nbits, 0, 128 // nbits, 16, ptr(out), 128, stream_ptr())
    assert (out.cpu().numpy() == 0x5A).all()
    assert unpack_bits(src[:0], nbits, 128 // nbits).shape == (0, 128 // nbits)


def test_unpack_wrapper(gpu):
    import torch
    from pypulsar_amd.stream import unpack_bits
    x = lowbit_data(300, 1024, 2, 14)
    got = unpack_bits(torch.from_numpy(_pack(x, 2)).cuda(), 2, 1024)
    np.testing.assert_array_equal(got.cpu().numpy(), x)


# ---------------------------------------------------------------- fused prologue
# Channels per nbits: a 16-byte packed row, and more than one 256-channel tile
# of k_packed_zdm_ds with the last tile partial
FUSED_C = {1: (128, 1152), 2: (64, 320), 4: (32, 288)}
FUSED_CASES = ([(b, m, f) for b in NBITS for m in ("none", "int", "wrap") for f in (1, 2, 4)]
               + [(b, "none", f) for b in NBITS for f in (16, 64)]
               + [(4, "int", 32)])


def _fused_vs_8bit(nbits, mode, factor, C, offset):
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import call, ptr, stream_ptr
    # a second, partial tile of 64 outputs and a dropped trailing group
    nspec = 64 * factor + 5 * factor + (factor - 1)
    nout = nspec // factor
    x = lowbit_data(nspec, C, nbits, 100 * nbits + factor)
    p = _pack(x, nbits)
    src = _padded(p, p.shape[1] + 16)
    got = torch.full((C, nout + 3), -1, dtype=torch.int16, device="cuda")
    call("pdd_zdm_packed_int_downsample", ptr(src), nbits, nspec, C, src.stride(0), factor,
         MODES[mode], offset, ptr(got), got.stride(0), stream_ptr())
    # the 8-bit entry point on the unpacked bytes.  Its INT range check wants
    # offset >= 255 factor whatever the values are, so it runs at its own
    # offset and the (exact, integer) difference of the two is taken out
    ref_off = 255 * factor if mode == "int" else offset
    xd = torch.from_numpy(x).cuda()
    ref = torch.full((C, nout + 3), -1, dtype=torch.int16, device="cuda")
    call("pdd_zdm_int_downsample", ptr(xd), _lib.U8, nspec, C, C, factor, MODES[mode], ref_off,
         ptr(ref), ref.stride(0), stream_ptr())
    g = got.cpu().numpy().astype(np.int64) & 0xffff
    r = ref.cpu().numpy().astype(np.int64) & 0xffff
    np.testing.assert_array_equal(g[:, :nout], r[:, :nout] - ref_off + offset)
    assert (g[:, nout:] == 0xffff).all()   # nothing past n_out written


@pytest.mark.parametrize("nbits,mode,factor", FUSED_CASES)
def test_fused_prologue_equals_8bit(gpu, nbits, mode, factor):
    vmax = (1 << nbits) - 1
    offset = vmax * factor if mode == "int" else 0   # (4-bit INT at 32: 480)
    for C in FUSED_C[nbits]:
        _fused_vs_8bit(nbits, mode, factor, C, offset)


@pytest.mark.parametrize("nbits", NBITS)
def test_fused_prologue_other_offsets(gpu, nbits):
    """The offset is added as it is, for every mode."""
    vmax = (1 << nbits) - 1
    C = FUSED_C[nbits][1]
    _fused_vs_8bit(nbits, "none", 2, C, 7)
    _fused_vs_8bit(nbits, "wrap", 2, C, 1000)
    _fused_vs_8bit(nbits, "int", 2, C, 2 * vmax + 11)


def test_fused_prologue_short_block(gpu):
    """Fewer spectra than one group: nothing is written."""
    import torch
    from pypulsar_amd._lib import call, ptr, stream_ptr
    src = torch.zeros((3, 16), dtype=torch.uint8, device="cuda")
    img = torch.full((32, 4), -1, dtype=torch.int16, device="cuda")
    call("pdd_zdm_packed_int_downsample", ptr(src), 4, 3, 32, 16, 4, 1, 60, ptr(img), 4,
         stream_ptr())
    assert (img.cpu().numpy() == -1).all()


# ---------------------------------------------------------------- the stream
def _run_stream(st, chunks):
    import torch
    parts = [(t0, p.cpu().numpy()) for t0, p in st(chunks)]
    torch.cuda.synchronize()
    st.close()
    return parts


def _stream_setup(nbits, seed):
    C, block = 128, 2048
    N = 2 * block + 1000   # three blocks, the last short
    x = lowbit_data(N, C, nbits, seed)
    dms = np.linspace(0.0, 60.0, 24)
    return C, block, N, x, dms, band(C)


def _chunks(a, block):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a[i:i + block])).pin_memory()
            for i in range(0, a.shape[0], block)]


def _same(parts, want):
    assert len(parts) == len(want) == 3
    for (ta, pa), (tb, pb) in zip(parts, want):
        assert ta == tb and pa.shape == pb.shape
        np.testing.assert_array_equal(pa, pb)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nbits", NBITS)
def test_stream_packed_equals_8bit(gpu, nbits, masked):
    from pypulsar_amd.rfi import RFIMask
    from pypulsar_amd.stream import StreamingSweep
    C, block, N, x, dms, freqs = _stream_setup(nbits, 40 + nbits)
    ds, ppi = 2, 512
    masks = [None, None]
    if masked:
        rng = np.random.default_rng(5)
        m = rng.random((-(-N // ppi), C)) < 0.02
        m[:, 9] = True
        m[3, :] = True
        masks = [RFIMask(m, ppi, np.ones(C)) for _ in range(2)]
    st = StreamingSweep(dms, freqs, DT, block=block, downsamp=ds, zero_dm="int", nbits=nbits,
                        rfimask=masks[0])
    assert st.max_bin > 0 and st.ov > 0   # the overlap crosses the block seams
    assert st.exact and st.fused == (not masked)
    assert (st.unpacked is not None) == masked
    assert st.raw[0].shape[1] == C * nbits // 8
    if not masked:
        vmax = (1 << nbits) - 1
        assert (st.offset, st.input_max) == (ds * vmax, 2 * ds * vmax)
    got = _run_stream(st, _chunks(_pack(x, nbits), block))
    ref = StreamingSweep(dms, freqs, DT, block=block, downsamp=ds, zero_dm="int",
                         rfimask=masks[1])
    want = _run_stream(ref, _chunks(x, block))
    _same(got, want)
    assert got[0][1].shape[1] == block // ds and np.abs(got[0][1]).max() > 0


def test_stream_4bit_downsamp16_equals_float(gpu):
    """4-bit values co-added by 16 stay <= 240: the fused path feeds the exact
    16-bit sweep where 8-bit data cannot (255 x 16 > 1023).  The float32
    stream of the same values sums the same integers."""
    import torch
    from pypulsar_amd.stream import StreamingSweep
    C, block, N, x, dms, freqs = _stream_setup(4, 47)
    dms = dms * 2   # DM 120: 109 bins at the coarser sampling, overlap 1744 < block
    st = StreamingSweep(dms, freqs, DT, block=block, downsamp=16, zero_dm=False, nbits=4)
    assert st.fused and st.exact and st.mode == "none" and st.input_max == 240
    assert st.max_bin > 0
    with pytest.raises(ValueError):
        StreamingSweep(dms, freqs, DT, block=block, downsamp=16, zero_dm="int")
    got = _run_stream(st, _chunks(_pack(x, 4), block))
    ref = StreamingSweep(dms, freqs, DT, block=block, downsamp=16, zero_dm=False,
                         dtype=torch.float32)
    assert not ref.exact
    want = _run_stream(ref, _chunks(x.astype(np.float32), block))
    _same(got, want)


def test_stream_auto_mode_on_packed_input(gpu):
    """'auto' on packed input: the exact integer filter where its bound fits,
    else float; on 8-bit input it is unchanged."""
    from pypulsar_amd.stream import StreamingSweep
    freqs, dms = band(128), np.linspace(0.0, 20.0, 4)
    kw = dict(block=2048, zero_dm="auto")
    for nbits, ds, mode, fused in [(2, 2, "int", True), (4, 32, "int", True),
                                   (4, 64, "float", False), (1, 64, "int", True)]:
        st = StreamingSweep(dms, freqs, DT, downsamp=ds, nbits=nbits, **kw)
        assert (st.mode, st.fused) == (mode, fused), (nbits, ds)
        st.close()
    st = StreamingSweep(dms, freqs, DT, downsamp=2, **kw)
    assert st.mode == "wrap" and not st.fused and st.nbits == 8
    st.close()
    # unaligned packed rows (12 bytes): the unpacked path
    st = StreamingSweep(dms[:2], band(96), DT, downsamp=2, nbits=1, **kw)
    assert not st.fused and st.unpacked is not None and st.mode == "int"
    st.close()


# ---------------------------------------------------------------- the CLIs
def _fil(tmp_path, x_tc, nbits, name):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C = x_tc.shape[1]
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, nbits, DT, 1550.0 + foff / 2, foff)
    fn = str(tmp_path / name)
    fbm.write_filterbank(fn, params, hdr, _pack(x_tc, nbits) if nbits < 8 else x_tc)
    return fn


@pytest.mark.parametrize("nbits", NBITS)
def test_get_spectra_on_packed_file(gpu, tmp_path, nbits):
    """The host-unpacking reader feeds the existing consumers unchanged."""
    from pypulsar_amd.formats import filterbank as fbm
    x = lowbit_data(50, 32, nbits, 70 + nbits)
    a = fbm.filterbank(_fil(tmp_path, x, nbits, "packed.fil")).get_spectra(10, 30)
    b = fbm.filterbank(_fil(tmp_path, x, 8, "eight.fil")).get_spectra(10, 30)
    assert a.starttime == b.starttime and a.data.shape == (32, 30)
    np.testing.assert_array_equal(np.asarray(a.data), np.asarray(b.data))
    np.testing.assert_array_equal(np.asarray(a.data), x[10:40].T.astype(np.float64))


def test_frb_search_2bit_file_equals_8bit_twin(gpu, tmp_path):
    from pypulsar_amd.bin import frb_search as fs
    from pypulsar_amd.delays import delay_from_DM
    C, N, block = 128, 3 * 8192, 8192
    x = np.random.default_rng(61).integers(0, 3, (N, C)).astype(np.uint8)   # [N, C] file order
    freqs = band(C)
    bins = np.round((delay_from_DM(40.0, freqs) - delay_from_DM(40.0, freqs.max())) / DT)
    for c in range(C):
        x[9000 + int(bins[c]):9000 + int(bins[c]) + 8, c] += 1
    dms = np.linspace(0.0, 80.0, 81)
    a = fs.search_file(_fil(tmp_path, x, 2, "two.fil"), dms, downsamp=2, block=block,
                       zero_dm=False, threshold=8.0)
    b = fs.search_file(_fil(tmp_path, x, 8, "eight.fil"), dms, downsamp=2, block=block,
                       zero_dm=False, threshold=8.0)
    assert len(a) >= 1
    best = a[np.argmax(a["Sigma"])]
    assert abs(best["DM"] - 40.0) <= 2.0 and abs(best["Time"] - 9000 * DT) <= 16 * DT
    assert a.dtype == b.dtype
    np.testing.assert_array_equal(a, b)


def test_pulsar_search_4bit_file_equals_8bit_twin(gpu, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    from pypulsar_amd.delays import delay_from_DM
    C, N, period = 64, 1 << 14, 64
    freqs = band(C)
    rng = np.random.default_rng(62)
    x = rng.normal(7.0, 2.0, (N, C))
    bins = np.round((delay_from_DM(60.0, freqs) - delay_from_DM(60.0, freqs.max()))
                    / DT).astype(int)
    for c in range(C):
        for w in range(2):
            x[np.arange(7 + w + bins[c], N, period), c] += 3.0
    x = np.clip(np.round(x), 0, 15).astype(np.uint8)
    dms = np.linspace(52.5, 67.5, 16)
    a, dta = pulsar_search.search_file(_fil(tmp_path, x, 4, "four.fil"), dms, nfft=1 << 14)
    b, dtb = pulsar_search.search_file(_fil(tmp_path, x, 8, "eight.fil"), dms, nfft=1 << 14)
    assert dta == dtb == DT and len(a) >= 1
    assert a.dtype == b.dtype
    np.testing.assert_array_equal(a, b)
