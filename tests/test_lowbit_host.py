"""1-, 2- and 4-bit SIGPROC filterbanks on the host: the packed sample codec
(formats/sigproc.py pack_bits / unpack_bits), the reader on packed files
(formats/filterbank.py) and the argument checks of the two device entry points
(pdd_unpack_bits, pdd_zdm_packed_int_downsample), which run before any HIP
call.  No GPU."""
import ctypes

import numpy as np
import pytest

from lowbit_oracle import lowbit_data

DT = 64e-6
NBITS = [1, 2, 4]


def _fil(tmp_path, x_tc, nbits, name="in.fil", nifs=1):
    """Filterbank file of the values x_tc [n, C], packed to ``nbits``."""
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    C = x_tc.shape[1]
    foff = -300.0 / C
    params, hdr = sigproc.make_header(C, nbits, DT, 1550.0 + foff / 2, foff, nifs=nifs)
    data = sigproc.pack_bits(x_tc, nbits) if nbits < 8 else x_tc
    fn = str(tmp_path / name)
    fbm.write_filterbank(fn, params, hdr, data)
    return fn, data


# ---------------------------------------------------------------- codec
def test_bit_order_by_hand():
    from pypulsar_amd.formats import sigproc
    b = np.array([[0xB4]], dtype=np.uint8)
    assert sigproc.unpack_bits(b, 4).tolist() == [[4, 11]]
    assert sigproc.unpack_bits(b, 2).tolist() == [[0, 1, 3, 2]]
    assert sigproc.unpack_bits(b, 1).tolist() == [[0, 0, 1, 0, 1, 1, 0, 1]]
    assert sigproc.pack_bits([[4, 11]], 4).tolist() == [[0xB4]]
    assert sigproc.pack_bits([[0, 1, 3, 2]], 2).tolist() == [[0xB4]]
    assert sigproc.pack_bits([[0, 0, 1, 0, 1, 1, 0, 1]], 1).tolist() == [[0xB4]]


@pytest.mark.parametrize("nbits", NBITS)
def test_codec_round_trip(nbits):
    from pypulsar_amd.formats import sigproc
    x = lowbit_data(37, 48, nbits, 1)
    p = sigproc.pack_bits(x, nbits)
    assert p.dtype == np.uint8 and p.shape == (37, 48 * nbits // 8)
    u = sigproc.unpack_bits(p, nbits)
    assert u.dtype == np.uint8 and u.shape == x.shape
    np.testing.assert_array_equal(u, x)
    # every byte value, both ways
    allb = np.arange(256, dtype=np.uint8).reshape(1, 256)
    np.testing.assert_array_equal(sigproc.pack_bits(sigproc.unpack_bits(allb, nbits), nbits), allb)


def test_4bit_equals_psrfits_unpack():
    from pypulsar_amd.formats import psrfits, sigproc
    b = np.random.default_rng(2).integers(0, 256, (9, 20)).astype(np.uint8)
    np.testing.assert_array_equal(sigproc.unpack_bits(b, 4).reshape(-1),
                                  psrfits.unpack_4bit(b.reshape(-1)))


@pytest.mark.parametrize("nbits", NBITS)
def test_pack_refuses_overflow(nbits):
    from pypulsar_amd.formats import sigproc
    x = np.zeros((2, 8), dtype=np.uint8)
    x[1, 3] = 1 << nbits
    with pytest.raises(ValueError):
        sigproc.pack_bits(x, nbits)
    with pytest.raises(ValueError):
        sigproc.pack_bits(np.zeros((2, 8)), 3)
    with pytest.raises(ValueError):
        sigproc.unpack_bits(np.zeros((2, 8), dtype=np.uint8), 8)


# ---------------------------------------------------------------- reader
@pytest.mark.parametrize("nbits", NBITS)
def test_reader_on_packed_file(tmp_path, nbits):
    from pypulsar_amd.formats import filterbank as fbm
    C, N = 32, 50
    x = lowbit_data(N, C, nbits, 3)
    fn, packed = _fil(tmp_path, x, nbits)
    fb = fbm.filterbank(fn)
    assert fb.header["nbits"] == nbits and fb.nbits == nbits and fb.packed is True
    assert fb.nchans == C and fb.tsamp == DT and fb.header["nifs"] == 1
    assert fb.dtype == "uint8"
    assert fb.bytes_per_spectrum == C * nbits // 8
    assert fb.number_of_samples == N
    buf = np.full((20, C), 77, dtype=np.uint8)
    assert fb.read_block_into(40, buf) == 10
    np.testing.assert_array_equal(buf[:10], x[40:])
    full = np.empty((N, C), dtype=np.uint8)
    assert fb.read_block_into(0, full) == N
    np.testing.assert_array_equal(full, x)
    pb = np.zeros((N, fb.bytes_per_spectrum), dtype=np.uint8)
    assert fb.read_packed_into(0, pb) == N
    np.testing.assert_array_equal(pb, packed)
    pb2 = np.zeros((20, fb.bytes_per_spectrum), dtype=np.uint8)
    assert fb.read_packed_into(40, pb2) == 10
    np.testing.assert_array_equal(pb2[:10], packed[40:])
    allv = fb.read_all_samples()
    assert allv.dtype == np.uint8
    np.testing.assert_array_equal(allv.reshape(N, C), x)
    fb.seek_to_sample(7)
    np.testing.assert_array_equal(fb.read_sample(), x[7])
    np.testing.assert_array_equal(fb.read_Nsamples(3).reshape(3, C), x[8:11])
    # the refusals of read_block_into
    with pytest.raises(ValueError):
        fb.read_packed_into(0, np.zeros((N, fb.bytes_per_spectrum + 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        fb.read_packed_into(0, np.zeros((N, 2 * fb.bytes_per_spectrum), dtype=np.uint8)[:, ::2])
    with pytest.raises(ValueError):
        fb.read_packed_into(0, np.zeros((N, fb.bytes_per_spectrum), dtype=np.int8))
    fb.close()


def test_reader_large_block_unpacks_in_place(tmp_path):
    """read_block_into unpacks inside ``out`` in several steps; more rows than
    one step holds come out right."""
    from pypulsar_amd.formats import filterbank as fbm
    x = lowbit_data(5000, 512, 2, 4)
    fn, _ = _fil(tmp_path, x, 2)
    fb = fbm.filterbank(fn)
    buf = np.empty((5000, 512), dtype=np.uint8)
    assert fb.read_block_into(0, buf) == 5000
    np.testing.assert_array_equal(buf, x)
    fb.close()


@pytest.mark.parametrize("nbits,C", [(1, 12), (2, 10), (4, 7)])
def test_reader_refuses_partial_bytes(tmp_path, nbits, C):
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import sigproc
    params, hdr = sigproc.make_header(C, nbits, DT, 1500.0, -1.0)
    fn = str(tmp_path / "odd.fil")
    fbm.write_filterbank(fn, params, hdr, np.zeros(64, dtype=np.uint8))
    with pytest.raises(ValueError):
        fbm.filterbank(fn)


def test_reader_refuses_packed_nifs(tmp_path):
    from pypulsar_amd.formats import filterbank as fbm
    fn, _ = _fil(tmp_path, lowbit_data(8, 32, 2, 5), 2, nifs=2)
    with pytest.raises(ValueError):
        fbm.filterbank(fn)


def test_8bit_file_is_not_packed(tmp_path):
    from pypulsar_amd.formats import filterbank as fbm
    x = np.random.default_rng(6).integers(0, 256, (50, 32)).astype(np.uint8)
    fn, _ = _fil(tmp_path, x, 8)
    fb = fbm.filterbank(fn)
    assert fb.packed is False and fb.nbits == 8 and fb.dtype == "uint8"
    a = np.zeros((20, 32), dtype=np.uint8)
    b = np.zeros((20, 32), dtype=np.uint8)
    assert fb.read_block_into(40, a) == 10 and fb.read_packed_into(40, b) == 10
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a[:10], x[40:])
    fb.close()


def test_zero_dm_filter_refuses_packed_input(tmp_path):
    from pypulsar_amd.bin import zero_dm_filter as z
    fn, _ = _fil(tmp_path, lowbit_data(50, 32, 2, 7), 2)
    out = tmp_path / "out.fil"
    with pytest.raises(ValueError, match="packed"):
        z.filter_file(fn, str(out))
    assert not out.exists()


# ---------------------------------------------------------------- ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    return _lib, _lib.lib()


def test_abi_declares_the_entry_points():
    from test_abi import declared_symbols
    _l, h = _lib()
    decl = declared_symbols()
    for name in ("pdd_unpack_bits", "pdd_zdm_packed_int_downsample"):
        assert name in decl and name in _l.EXPORTS and hasattr(h, name)
    assert sorted(_l.EXPORTS) == decl


def test_entry_points_refuse_bad_arguments_without_gpu():
    """Validation comes before any HIP call (no pointer is dereferenced)."""
    _l, h = _lib()
    # 16-byte aligned host addresses, never read
    raw = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    o = ctypes.c_void_p(a.value + 2048)

    st = h.pdd_unpack_bits(None, 2, 4, 64, 16, o, 64, None)
    assert st < 0 and b"null pointer" in h.pdd_last_error()
    st = h.pdd_unpack_bits(a, 2, 4, 64, 16, None, 64, None)
    assert st < 0 and b"null pointer" in h.pdd_last_error()
    st = h.pdd_unpack_bits(a, 3, 4, 64, 24, o, 64, None)
    assert st < 0 and b"nbits 3" in h.pdd_last_error()
    st = h.pdd_unpack_bits(a, 2, 4, 10, 16, o, 64, None)   # 20 bits per row
    assert st < 0 and b"multiple of 8" in h.pdd_last_error()
    st = h.pdd_unpack_bits(a, 2, 4, 64, 15, o, 64, None)   # stride below the row
    assert st < 0 and b"stride" in h.pdd_last_error()

    f = h.pdd_zdm_packed_int_downsample
    st = f(None, 2, 128, 64, 16, 2, _l.ZDM_NONE, 0, o, 64, None)
    assert st < 0 and b"null pointer" in h.pdd_last_error()
    st = f(a, 2, 128, 64, 16, 2, _l.ZDM_NONE, 0, None, 64, None)
    assert st < 0 and b"null pointer" in h.pdd_last_error()
    st = f(a, 3, 128, 64, 16, 2, _l.ZDM_NONE, 0, o, 64, None)
    assert st < 0 and b"nbits 3" in h.pdd_last_error()
    st = f(a, 2, 128, 64, 16, 3, _l.ZDM_NONE, 0, o, 64, None)
    assert st < 0 and b"factor" in h.pdd_last_error()
    # misaligned packed rows: the stride, the row length, the base address
    st = f(a, 2, 128, 64, 24, 2, _l.ZDM_NONE, 0, o, 64, None)
    assert st < 0 and b"16-byte aligned" in h.pdd_last_error()
    st = f(a, 4, 128, 24, 16, 2, _l.ZDM_NONE, 0, o, 64, None)   # 12-byte rows
    assert st < 0 and b"16-byte aligned" in h.pdd_last_error()
    st = f(ctypes.c_void_p(a.value + 4), 2, 128, 64, 16, 2, _l.ZDM_NONE, 0, o, 64, None)
    assert st < 0 and b"16-byte aligned" in h.pdd_last_error()
    st = f(a, 2, 128, 64, 16, 2, _l.ZDM_NONE, 0, o, 63, None)
    assert st < 0 and b"ld_out" in h.pdd_last_error()
    # the range check: INT needs offset >= factor (2^nbits - 1); nothing past 65535
    st = f(a, 4, 128, 32, 16, 32, _l.ZDM_INT, 479, o, 64, None)
    assert st < 0 and b"offset 479" in h.pdd_last_error()
    st = f(a, 4, 128, 32, 16, 2, _l.ZDM_NONE, 65535 - 29, o, 64, None)
    assert st < 0 and b"cannot hold" in h.pdd_last_error()
    st = f(a, 2, 128, 64, 16, 4, _l.ZDM_WRAP, 65535 - 1019, o, 64, None)   # WRAP: 255 factor
    assert st < 0 and b"cannot hold" in h.pdd_last_error()
