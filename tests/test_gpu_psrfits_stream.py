"""PSRFITS search-mode input on the GPU: pdd_psrfits_block against the NumPy
restatement (tests/psrfits_stream_oracle.py) and against the existing
pdd_psrfits_subints, StreamingSweep(decoder=...) on SUBINT row chunks against
the existing 8-bit / float32 chunk streams of the same values, and the three
CLIs on a PSRFITS file against its SIGPROC twin.  Every comparison is exact:
integers, or bit-identical float32."""
import os
import zlib

import numpy as np
import pytest

import psrfits_stream_oracle as pso
from conftest import band
from oracle import spectra_oracle as orc

pytestmark = pytest.mark.gpu
DT = 64e-6
U8, F32 = 1, 0
NSUB = 4
_CASES = {}


class Case(object):
    pass


def _case(tmpdir, nbits, nchan, nsblk, npol=1, pol_type="AA+BB", extra=False, unit=False,
          nsub=NSUB):
    """A written file's rows and what they decode to: distinct random scale,
    offset and weight per subint and channel (weights include 0).  ``unit``:
    weights in {0, 1} only (the integer form's precondition; scales and
    offsets are still random, for the caller to switch off).  ``extra``: a
    1-byte column ahead of DATA makes data_off odd."""
    key = (nbits, nchan, nsblk, npol, pol_type, extra, unit, nsub)
    if key in _CASES:
        return _CASES[key]
    from pypulsar_amd.formats import fits, psrfits
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    shape = (nsub, nsblk, npol, nchan)
    if nbits == 32:
        data = rng.normal(0, 40, shape).astype(np.float32)
    elif nbits == 16:
        data = rng.integers(-32768, 32768, shape).astype(np.int16)
    else:
        data = rng.integers(0, 1 << nbits, shape).astype(np.uint8)
    c = Case()
    c.data = data
    c.scl = rng.uniform(0.5, 2.0, (nsub, npol * nchan)).astype(np.float32)
    c.off = rng.normal(0, 5, (nsub, npol * nchan)).astype(np.float32)
    c.wts = (rng.integers(0, 2, (nsub, nchan)) if unit
             else rng.integers(0, 4, (nsub, nchan)) / 2).astype(np.float32)
    fn = os.path.join(str(tmpdir), "case%d.fits" % len(_CASES))
    freqs = band(nchan)
    if not extra:
        psrfits.write_search_psrfits(fn, data if npol > 1 else data[:, :, 0, :], freqs, DT, nbits,
                                     c.scl, c.off, c.wts, npol=npol, pol_type=pol_type)
    else:
        body = {4: lambda d: (d[:, 0::2] & 15) | ((d[:, 1::2] & 15) << 4), 8: lambda d: d,
                16: lambda d: d.astype(">i2"), 32: lambda d: d.astype(">f4")}[nbits](
                    data.reshape(nsub, -1))
        code = {4: "B", 8: "B", 16: "I", 32: "E"}[nbits]
        cols = [("DAT_WTS", "%dE" % nchan), ("DAT_OFFS", "%dE" % (npol * nchan)),
                ("DAT_SCL", "%dE" % (npol * nchan)), ("FLAG", "1B"),
                ("DATA", "%d%s" % (body.shape[1], code))]
        rows = {"DAT_WTS": c.wts, "DAT_OFFS": c.off, "DAT_SCL": c.scl,
                "FLAG": np.arange(nsub, dtype=np.uint8), "DATA": body}
        fits.write(fn, [("FITSTYPE", "PSRFITS"), ("OBS_MODE", "SEARCH")],
                   [("SUBINT", [("NCHAN", nchan)], cols, rows)])
    sub = fits.open(fn)["SUBINT"]
    names = sub.columns.names
    c.rows = np.array(sub.raw_rows(0, nsub))
    c.row_bytes = c.rows.shape[1]
    c.data_off, c.scl_off, c.offs_off, c.wts_off = (
        sub.columns[names.index(k)].offset for k in ("DATA", "DAT_SCL", "DAT_OFFS", "DAT_WTS"))
    c.nbits, c.nchan, c.nsblk, c.npol, c.nsub, c.fn = nbits, nchan, nsblk, npol, nsub, fn
    _CASES[key] = c
    return c


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return tmp_path_factory.mktemp("psrfits_stream")


def _block(c, s0, n, out_code=F32, ld_pad=0, pol0=0, npol_sum=1, scl=True, offs=True, wts=True,
           **override):
    """pdd_psrfits_block through the raw ABI into a 0x5A-filled buffer of
    n + 2 rows; returns (status, decoded [n, nchan], the buffer's bytes were
    left alone outside it)."""
    import torch
    from pypulsar_amd import _lib
    from pypulsar_amd._lib import ptr, stream_ptr
    a = dict(rows=None, nsub=c.nsub, row_bytes=c.row_bytes, data_off=c.data_off,
             scl_off=c.scl_off if scl else -1, offs_off=c.offs_off if offs else -1,
             wts_off=c.wts_off if wts else -1, nbits=c.nbits, nsblk=c.nsblk, nchan=c.nchan,
             npol=c.npol, pol0=pol0, npol_sum=npol_sum, s0=s0, n=n, out_code=out_code,
             ld_out=c.nchan + ld_pad)
    a.update(override)
    es = 1 if out_code == U8 else 4
    ld = max(a["ld_out"], c.nchan)
    buf = torch.full(((n + 2) * ld * es,), 0x5A, dtype=torch.uint8, device="cuda")
    rows = torch.from_numpy(c.rows).cuda()
    status = _lib.lib().pdd_psrfits_block(
        None if override.get("null_rows") else ptr(rows), a["nsub"], a["row_bytes"], a["data_off"],
        a["scl_off"], a["offs_off"], a["wts_off"], a["nbits"], a["nsblk"], a["nchan"], a["npol"],
        a["pol0"], a["npol_sum"], a["s0"], a["n"], a["out_code"],
        None if override.get("null_out") else ptr(buf), a["ld_out"], stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy().reshape(n + 2, ld * es)
    got = host[:n, :c.nchan * es].copy().view(np.uint8 if es == 1 else np.float32)
    untouched = bool((host[n:] == 0x5A).all() and (host[:n, c.nchan * es:] == 0x5A).all())
    if status != 0:
        untouched = bool((host == 0x5A).all())
    return status, got, untouched


def _spans(nsblk, nsub=NSUB):
    return [(0, nsub * nsblk), (1, 1), (nsblk - 1, 2 * nsblk + 2), (nsblk, nsblk)]


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint8 if got.dtype == np.uint8 else np.uint32),
                                  want.view(np.uint8 if want.dtype == np.uint8 else np.uint32))


# (nchan, nsblk): row 0's DATA 16-byte aligned and the later rows not; whole
# 16-channel chunks; no multiple of 16 channels; more chunks than one
SHAPES = [(6, 7), (64, 16), (100, 5), (272, 3)]


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("ld_pad", [0, 5])
@pytest.mark.parametrize("nchan,nsblk", SHAPES)
@pytest.mark.parametrize("nbits", [4, 8, 16, 32])
def test_block_f32(gpu, tmpdir, nbits, nchan, nsblk, ld_pad):
    c = _case(tmpdir, nbits, nchan, nsblk)
    if (nchan, nsblk) == (6, 7):
        assert c.data_off == 144 and (nbits != 8 or c.row_bytes == 186)
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts)
    for s0, n in _spans(nsblk):
        status, got, untouched = _block(c, s0, n, ld_pad=ld_pad)
        assert status == 0
        _same_bits(got, want[s0:s0 + n])
        assert untouched


@pytest.mark.parametrize("ld_pad", [0, 5])
@pytest.mark.parametrize("nchan,nsblk", SHAPES)
@pytest.mark.parametrize("nbits", [4, 8])
def test_block_u8(gpu, tmpdir, nbits, nchan, nsblk, ld_pad):
    c = _case(tmpdir, nbits, nchan, nsblk, unit=True)
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts, out="uint8")
    assert (want == 0).any() and (c.wts == 0).any()
    for s0, n in _spans(nsblk):
        status, got, untouched = _block(c, s0, n, U8, ld_pad, scl=False, offs=False)
        assert status == 0
        _same_bits(got, want[s0:s0 + n])
        assert untouched
    # weights off: the file's own values
    status, got, untouched = _block(c, 0, NSUB * nsblk, U8, ld_pad, scl=False, offs=False, wts=False)
    assert status == 0 and untouched
    _same_bits(got, c.data[:, :, 0, :].reshape(-1, nchan))


@pytest.mark.parametrize("nbits", [4, 8, 16, 32])
def test_block_odd_data_offset(gpu, tmpdir, nbits):
    """A 1-byte column ahead of DATA: data_off is odd, so 16- and 32-bit
    samples straddle every alignment."""
    c = _case(tmpdir, nbits, 100, 5, extra=True)
    assert c.data_off % 2 == 1
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts)
    for s0, n in _spans(5):
        status, got, untouched = _block(c, s0, n, ld_pad=5)
        assert status == 0 and untouched
        _same_bits(got, want[s0:s0 + n])
    # and a shape whose rows would otherwise take the aligned path
    c = _case(tmpdir, nbits, 64, 16, extra=True)
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts)
    status, got, untouched = _block(c, 15, 34)
    assert status == 0 and untouched
    _same_bits(got, want[15:49])


@pytest.mark.parametrize("off_col", ["scl", "offs", "wts"])
@pytest.mark.parametrize("nbits", [8, 16])
def test_block_switches(gpu, tmpdir, nbits, off_col):
    c = _case(tmpdir, nbits, 100, 5)
    kw = {off_col: False}
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts, apply_scales=off_col != "scl",
                      apply_offsets=off_col != "offs", apply_weights=off_col != "wts")
    for s0, n in ((0, NSUB * 5), (4, 12)):
        status, got, untouched = _block(c, s0, n, **kw)
        assert status == 0 and untouched
        _same_bits(got, want[s0:s0 + n])


@pytest.mark.parametrize("npol,pol_type,pol0,npol_sum", [(2, "AABB", 0, 2), (4, "IQUV", 0, 1),
                                                         (4, "AABBCRCI", 2, 1)])
@pytest.mark.parametrize("nbits", [8, 16])
def test_block_polarisations(gpu, tmpdir, nbits, npol, pol_type, pol0, npol_sum):
    c = _case(tmpdir, nbits, 100, 5, npol=npol, pol_type=pol_type)
    want = pso.decode(c.data, nbits, c.scl, c.off, c.wts, pol0=pol0, npol_sum=npol_sum)
    for s0, n in _spans(5):
        status, got, untouched = _block(c, s0, n, pol0=pol0, npol_sum=npol_sum, ld_pad=5)
        assert status == 0 and untouched
        _same_bits(got, want[s0:s0 + n])


def test_block_polarisations_aligned_sum(gpu, tmpdir):
    """The summed form on whole 16-channel chunks (the wide loads of both
    polarisations)."""
    c = _case(tmpdir, 8, 64, 16, npol=2, pol_type="AABB")
    want = pso.decode(c.data, 8, c.scl, c.off, c.wts, npol_sum=2)
    status, got, untouched = _block(c, 3, 50, npol_sum=2)
    assert status == 0 and untouched
    _same_bits(got, want[3:53])


@pytest.mark.parametrize("nchan,nsblk", SHAPES)
@pytest.mark.parametrize("nbits", [4, 8, 16, 32])
def test_block_equals_old_kernel(gpu, tmpdir, nbits, nchan, nsblk):
    """pdd_psrfits_subints(flip=0), transposed, is the new block."""
    import torch
    from pypulsar_amd._lib import call, ptr, stream_ptr
    c = _case(tmpdir, nbits, nchan, nsblk)
    wso = np.stack([c.scl, c.off, c.wts], axis=1).astype(np.float32)   # [nsub][3][nchan]
    rows, wso = torch.from_numpy(c.rows).cuda(), torch.from_numpy(wso).cuda()
    for s0, n in _spans(nsblk):
        old = torch.empty((nchan, n), dtype=torch.float32, device="cuda")
        call("pdd_psrfits_subints", ptr(rows), NSUB, c.row_bytes, c.data_off, nbits, nsblk, nchan,
             ptr(wso), s0, n, 0, ptr(old), n, stream_ptr())
        status, got, _ = _block(c, s0, n)
        assert status == 0
        _same_bits(got, old.t().contiguous().cpu().numpy())


def test_block_refusals(gpu, tmpdir):
    c = _case(tmpdir, 8, 64, 16)
    total = NSUB * 16
    bad = [dict(null_rows=True), dict(null_out=True), dict(nbits=2), dict(nbits=12),
           dict(s0=1, n=total), dict(s0=total, n=1),
           dict(row_bytes=c.data_off + 16 * 64 - 1),              # DATA past the row
           dict(scl_off=c.row_bytes - 4 * 64 + 1), dict(offs_off=c.row_bytes - 4),
           dict(wts_off=c.row_bytes - 4 * 64 + 4),
           dict(pol0=1), dict(npol_sum=2), dict(npol_sum=0),
           dict(ld_out=63), dict(out_code=2)]
    for kw in bad:
        status, _, untouched = _block(c, kw.pop("s0", 3), kw.pop("n", 20), **kw)
        assert status != 0 and untouched, kw
    # the integer form outside its conditions
    for kw in (dict(offs=False), dict(scl=False)):
        status, _, untouched = _block(c, 3, 20, U8, **kw)
        assert status != 0 and untouched, kw
    c2 = _case(tmpdir, 8, 100, 5, npol=2, pol_type="AABB")
    status, _, untouched = _block(c2, 0, 5, U8, scl=False, offs=False, npol_sum=2)
    assert status != 0 and untouched
    c16 = _case(tmpdir, 16, 64, 16)
    status, _, untouched = _block(c16, 0, 5, U8, scl=False, offs=False)
    assert status != 0 and untouched
    # 4-bit spectra of an odd number of samples
    c4 = _case(tmpdir, 4, 6, 7)
    status, _, untouched = _block(c4, 0, 5, nchan=5, ld_out=6)
    assert status != 0 and untouched
    # n == 0: fine, and nothing written
    status, _, untouched = _block(c, 7, 0)
    assert status == 0 and untouched
    from pypulsar_amd import _lib
    assert _lib.lib().pdd_last_error()


# ---------------------------------------------------------------- the stream
C_ST, NSBLK_ST, BLOCK, DS = 64, 96, 1024, 2
NSUB_ST = 37     # 3552 spectra: three whole blocks and a short one (whole subints only)
DMS = np.linspace(0.0, 30.0, 16)


def _stream_file(tmpdir, name, nbits=8, descending=True, seed=1, **kw):
    from pypulsar_amd.formats import psrfits
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 1 << min(nbits, 8), (NSUB_ST, NSBLK_ST, C_ST)).astype(np.uint8)
    if nbits == 16:
        data = rng.integers(-2000, 2000, data.shape).astype(np.int16)
    fn = os.path.join(str(tmpdir), name)
    psrfits.write_search_psrfits(fn, data, band(C_ST, descending), DT, nbits, **kw)
    return fn, data


def _row_chunks(f, block=BLOCK, first=0):
    import torch
    out = []
    for start in range(first * block, f.number_of_samples, block):
        row0, k, _ = f.rows_for(start, block)
        h = torch.empty((k, f.row_bytes), dtype=torch.uint8).pin_memory()
        assert f.read_rows_into(row0, h.numpy()) == k
        out.append(h)
    return out


def _chunks(x, block=BLOCK):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x[i:i + block])).pin_memory()
            for i in range(0, len(x), block)]


def _run(st, chunks, **kw):
    import torch
    got = [(t0, p.cpu().numpy()) for t0, p in st(chunks, **kw)]
    torch.cuda.synchronize()
    st.close()
    return got


def _same(got, want):
    assert len(got) == len(want) and len(got) >= 1
    for (ta, pa), (tb, pb) in zip(got, want):
        assert ta == tb and pa.shape == pb.shape
        np.testing.assert_array_equal(pa.view(np.uint32), pb.view(np.uint32))


def _decoded_stream(fn, zero_dm, rfimask=None, first=0, **kw):
    from pypulsar_amd.formats import psrfits
    from pypulsar_amd.stream import StreamingSweep
    f = psrfits.PsrfitsSearchFile(fn, **kw)
    st = StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm=zero_dm,
                        decoder=f.decoder(), rfimask=rfimask)
    assert st.ov > 0 and st.ov % NSBLK_ST != 0 and st.ov < BLOCK
    assert st.rows is not None and len(st.raw) == 1
    got = _run(st, _row_chunks(f, first=first), start_block=first)
    return f, st, got


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("zero_dm", ["wrap", "int", "float", False])
def test_stream_integer_mode(gpu, tmpdir, zero_dm, descending):
    import torch
    from pypulsar_amd.stream import StreamingSweep
    fn, data = _stream_file(tmpdir, "int%d.fits" % descending, descending=descending)
    f, st, got = _decoded_stream(fn, zero_dm)
    assert f.dtype == "uint8" and st.dtype == torch.uint8 and st.exact == (zero_dm != "float")
    ref = StreamingSweep(DMS, band(C_ST, descending), DT, block=BLOCK, downsamp=DS,
                         zero_dm=zero_dm)
    want = _run(ref, _chunks(data.reshape(-1, C_ST)))
    assert len(want) == 4
    _same(got, want)


def test_stream_4bit(gpu, tmpdir):
    from pypulsar_amd.stream import StreamingSweep
    fn, data = _stream_file(tmpdir, "four.fits", nbits=4, seed=2)
    f, st, got = _decoded_stream(fn, "int")
    assert f.dtype == "uint8" and f.nbits == 4 and st.exact and data.max() == 15
    ref = StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm="int")
    _same(got, _run(ref, _chunks(data.reshape(-1, C_ST))))


def test_stream_zero_weight_channel(gpu, tmpdir):
    from pypulsar_amd.stream import StreamingSweep
    w = np.ones((NSUB_ST, C_ST), dtype=np.float32)
    w[:, 11] = 0
    w[20:, 40] = 0
    fn, data = _stream_file(tmpdir, "wts.fits", seed=3, weights=w)
    f, st, got = _decoded_stream(fn, "wrap")
    assert f.dtype == "uint8" and f.wts_off >= 0
    x = (data * (w[:, None, :] != 0)).astype(np.uint8).reshape(-1, C_ST)
    assert (x[:, 11] == 0).all()
    ref = StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm="wrap")
    _same(got, _run(ref, _chunks(x)))


def test_stream_restart(gpu, tmpdir):
    fn, _ = _stream_file(tmpdir, "int1.fits")
    _, _, full = _decoded_stream(fn, "int")
    _, _, part = _decoded_stream(fn, "int", first=2)
    assert len(full) == 4 and len(part) == 2
    _same(part, full[2:])


@pytest.mark.parametrize("nbits", [8, 16])
def test_stream_float_mode(gpu, tmpdir, nbits):
    import torch
    from pypulsar_amd.stream import StreamingSweep
    rng = np.random.default_rng(4)
    kw = {}
    if nbits == 8:
        kw = dict(scales=rng.uniform(0.5, 2, (NSUB_ST, C_ST)).astype(np.float32),
                  offsets=rng.normal(0, 4, (NSUB_ST, C_ST)).astype(np.float32),
                  weights=(rng.integers(0, 3, (NSUB_ST, C_ST)) / 2).astype(np.float32))
    fn, data = _stream_file(tmpdir, "flt%d.fits" % nbits, nbits=nbits, seed=5, **kw)
    f, st, got = _decoded_stream(fn, "auto")
    assert f.dtype == "float32" and st.dtype == torch.float32 and not st.exact
    one = np.ones((NSUB_ST, C_ST), dtype=np.float32)
    x = pso.decode(data, nbits, kw.get("scales", one), kw.get("offsets", 0 * one),
                   kw.get("weights", one))
    ref = StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm="auto",
                         dtype=torch.float32)
    _same(got, _run(ref, _chunks(x)))


def test_stream_with_mask(gpu, tmpdir):
    from pypulsar_amd.rfi import RFIMask
    from pypulsar_amd.stream import StreamingSweep
    fn, data = _stream_file(tmpdir, "int1.fits")
    rng = np.random.default_rng(6)
    ppi = 300    # intervals straddle block and subint seams
    m = rng.random((-(-NSUB_ST * NSBLK_ST // ppi), C_ST)) < 0.05
    m[:, 9] = True
    m[4, :] = True
    fill = rng.normal(128, 10, C_ST)
    f, st, got = _decoded_stream(fn, "wrap", rfimask=RFIMask(m, ppi, fill))
    ref = StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm="wrap",
                         rfimask=RFIMask(m, ppi, fill))
    want = _run(ref, _chunks(data.reshape(-1, C_ST)))
    _same(got, want)
    plain = _run(StreamingSweep(DMS, f.freqs, DT, block=BLOCK, downsamp=DS, zero_dm="wrap"),
                 _chunks(data.reshape(-1, C_ST)))
    assert any((a[1] != b[1]).any() for a, b in zip(want, plain))


def test_stream_without_decoder_is_unchanged(gpu):
    """decoder=None: the 8-bit chunk stream as before -- three rotating raw
    buffers, no row buffers, and the oracle's one-shot plane bit for bit."""
    from pypulsar_amd.stream import StreamingSweep
    x = np.random.default_rng(7).integers(0, 256, (NSUB_ST * NSBLK_ST, C_ST)).astype(np.uint8)
    freqs = band(C_ST)
    st = StreamingSweep(DMS, freqs, DT, block=BLOCK, downsamp=DS, zero_dm="int", decoder=None)
    assert st.decoder is None and st.rows is None and len(st.raw) == 3
    got = np.concatenate([p for _, p in _run(st, _chunks(x))], axis=1)
    ref = orc.sweep_plane(orc.zdm_int_downsample(x, DS, "int").astype(np.float64),
                          orc.sweep_table(DMS, freqs, DT * DS))
    np.testing.assert_array_equal(got, ref)


def test_read_block_into_and_read_device(gpu, tmpdir):
    """The window reader: any span, through the device, in bounded pieces."""
    from pypulsar_amd.formats import psrfits
    fn, data = _stream_file(tmpdir, "int1.fits")
    f = psrfits.PsrfitsSearchFile(fn)
    x = data.reshape(-1, C_ST)
    out = np.full((500, C_ST), 0x5A, dtype=np.uint8)
    assert f.read_block_into(77, out[:400]) == 400
    np.testing.assert_array_equal(out[:400], x[77:477])
    assert (out[400:] == 0x5A).all()
    assert f.read_block_into(len(x) - 10, out[:400]) == 10
    np.testing.assert_array_equal(out[:10], x[-10:])
    got = f.read_device(5, 1000, piece_bytes=3 * f.row_bytes)   # several pieces
    np.testing.assert_array_equal(got.cpu().numpy(), x[5:1005])
    f.close()


# ---------------------------------------------------------------- the CLIs
CLI_C, CLI_NSBLK, CLI_NSUB = 64, 768, 30
CLI_ARGS = ["--block", "8192", "--downsamp", "2", "--numdms", "32", "--hidm", "60"]


def _observation(descending=True):
    """Gaussian 8-bit noise with one dispersed pulse (DM 40) and a weak
    periodic signal (DM 20, 64 samples)."""
    from pypulsar_amd.delays import delay_from_DM
    N = CLI_NSBLK * CLI_NSUB
    freqs = band(CLI_C, descending)
    rng = np.random.default_rng(71)
    x = rng.normal(100.0, 10.0, (N, CLI_C))
    for dm, amp, times in ((40.0, 14.0, [9000]), (20.0, 4.0, range(13, N, 64))):
        bins = np.round((delay_from_DM(dm, freqs) - delay_from_DM(dm, freqs.max())) / DT)
        for c in range(CLI_C):
            for w in range(4 if dm == 40.0 else 2):
                t = np.asarray(times) + int(bins[c]) + w
                x[t[t < N], c] += amp
    return freqs, np.clip(np.round(x), 0, 255).astype(np.uint8)


def _twins(tmp_path, kind, descending=True):
    """(PSRFITS file, SIGPROC twin): the twin of an integer-mode file is the
    8-bit .fil, that of a float-mode file the float32 .fil of the
    restatement's values; both carry the same start time and band."""
    from pypulsar_amd.formats import filterbank as fbm
    from pypulsar_amd.formats import psrfits, sigproc
    freqs, x = _observation(descending)
    data = x.reshape(CLI_NSUB, CLI_NSBLK, CLI_C)
    rng = np.random.default_rng(72)
    one = np.ones((CLI_NSUB, CLI_C), dtype=np.float32)
    fits_fn = str(tmp_path / ("obs_%s.fits" % kind))
    if kind == "int":
        psrfits.write_search_psrfits(fits_fn, data, freqs, DT, 8)
        twin = x
    elif kind == "scaled":
        scl = rng.uniform(0.5, 2, one.shape).astype(np.float32)
        off = rng.normal(0, 4, one.shape).astype(np.float32)
        psrfits.write_search_psrfits(fits_fn, data, freqs, DT, 8, scl, off)
        twin = pso.decode(data, 8, scl, off, one)
    elif kind == "16bit":
        d16 = (data.astype(np.int16) - 100) * 37
        psrfits.write_search_psrfits(fits_fn, d16, freqs, DT, 16)
        twin = pso.decode(d16, 16, one, 0 * one, one)
    else:
        assert kind == "aabb"
        two = np.stack([data // 2, data - data // 2], axis=2)
        scl = rng.uniform(0.5, 2, (CLI_NSUB, 2 * CLI_C)).astype(np.float32)
        off = rng.normal(0, 4, (CLI_NSUB, 2 * CLI_C)).astype(np.float32)
        psrfits.write_search_psrfits(fits_fn, two, freqs, DT, 8, scl, off, npol=2, pol_type="AABB")
        twin = pso.decode(two, 8, scl, off, one, npol_sum=2)
    f = psrfits.PsrfitsSearchFile(fits_fn)
    assert f.dtype == ("uint8" if kind == "int" else "float32")
    # (64 channels over 300 MHz: every frequency is exact in binary, so the
    # twin's fch1 + foff * arange is DAT_FREQ bit for bit)
    params, hdr = sigproc.make_header(CLI_C, 8 if kind == "int" else 32, DT, float(freqs[0]),
                                      float(freqs[1] - freqs[0]), tstart=f.header["tstart"],
                                      src_raj=123456.789, src_dej=-123456.5)
    f.close()
    # same base name in a directory of its own: the outputs carry the base name
    os.makedirs(str(tmp_path / "twin"), exist_ok=True)
    fil_fn = str(tmp_path / "twin" / ("obs_%s.fil" % kind))
    fbm.write_filterbank(fil_fn, params, hdr, twin)
    return fits_fn, fil_fn


def _text(fn):
    with open(fn) as f:
        return f.read()


def _same_npz(a, b):
    with np.load(a) as za, np.load(b) as zb:
        assert sorted(za.files) == sorted(zb.files) and za.files
        for k in za.files:
            np.testing.assert_array_equal(za[k], zb[k], err_msg=k)


@pytest.mark.parametrize("kind,descending", [("int", True), ("int", False), ("scaled", True),
                                             ("scaled", False), ("16bit", True), ("aabb", True)])
def test_frb_search_equals_twin(gpu, tmp_path, kind, descending):
    from pypulsar_amd.bin import frb_search
    a, b = _twins(tmp_path, kind, descending)
    assert frb_search.main(CLI_ARGS + [a]) == 0
    assert frb_search.main(CLI_ARGS + [b]) == 0
    ta, tb = _text(a[:-5] + ".singlepulse"), _text(b[:-4] + ".singlepulse")
    assert ta == tb and len(ta.splitlines()) > 1


def test_frb_search_group_cutouts_equal_twin(gpu, tmp_path):
    from pypulsar_amd.bin import frb_search
    a, b = _twins(tmp_path, "int")
    for fn in (a, b):
        assert frb_search.main(CLI_ARGS + ["--group", "--cutouts", "2", fn]) == 0
    ba, bb = a[:-5], b[:-4]
    assert _text(ba + ".singlepulse") == _text(bb + ".singlepulse")
    ga, gb = _text(ba + ".spgroups"), _text(bb + ".spgroups")
    assert ga == gb and len(ga.splitlines()) > 1
    _same_npz(ba + "_cutouts.npz", bb + "_cutouts.npz")


def test_frb_search_rfifind_equals_twin(gpu, tmp_path):
    from pypulsar_amd.bin import frb_search
    a, b = _twins(tmp_path, "int")
    for fn in (a, b):
        assert frb_search.main(CLI_ARGS + ["--rfifind", "0.1", fn]) == 0
    ta, tb = _text(a[:-5] + ".singlepulse"), _text(b[:-4] + ".singlepulse")
    assert ta == tb and len(ta.splitlines()) > 1


def test_frb_search_switches_equal_plain_twin(gpu, tmp_path):
    """--noscales --nooffsets --noweights on the float-mode 8-bit file: the
    plain 8-bit values, so the 8-bit twin's candidates."""
    from pypulsar_amd.bin import frb_search
    a, fil = _twins(tmp_path, "scaled")
    os.remove(fil)
    _, b = _twins(tmp_path, "int")
    assert frb_search.main(CLI_ARGS + ["--noscales", "--nooffsets", "--noweights", a]) == 0
    assert frb_search.main(CLI_ARGS + ["--noscales", "--poln", "0", b]) == 0   # noted, ignored
    ta, tb = _text(a[:-5] + ".singlepulse"), _text(b[:-4] + ".singlepulse")
    assert ta == tb and len(ta.splitlines()) > 1


@pytest.mark.parametrize("kind", ["int", "scaled"])
def test_pulsar_search_equals_twin(gpu, tmp_path, kind):
    from pypulsar_amd.bin import pulsar_search
    a, b = _twins(tmp_path, kind)
    args = ["--downsamp", "2", "--numdms", "16", "--hidm", "60"]
    for fn in (a, b):
        assert pulsar_search.main(args + [fn]) == 0
    ta, tb = _text(a[:-5] + ".accelcands"), _text(b[:-4] + ".accelcands")
    assert ta == tb and len(ta.splitlines()) > 1


def test_pulsar_search_fold_equals_twin(gpu, tmp_path):
    from pypulsar_amd.bin import pulsar_search
    a, b = _twins(tmp_path, "int")
    args = ["--downsamp", "2", "--numdms", "16", "--hidm", "60", "--zmax", "4", "--fold", "1",
            "--fold-subbands", "8"]
    for fn in (a, b):
        assert pulsar_search.main(args + [fn]) == 0
    ba, bb = a[:-5], b[:-4]
    assert _text(ba + ".accelcands") == _text(bb + ".accelcands")
    # (the first header line names the input file)
    pa = _text(ba + "_cand1.bestprof").splitlines()[1:]
    pb = _text(bb + "_cand1.bestprof").splitlines()[1:]
    assert pa == pb and len(pa) > 10
    _same_npz(ba + "_cand1.npz", bb + "_cand1.npz")
    _same_npz(ba + "_cand1_subbands.npz", bb + "_cand1_subbands.npz")


@pytest.mark.parametrize("kind", ["int", "scaled"])
def test_rfifind_equals_twin(gpu, tmp_path, kind):
    from pypulsar_amd.bin import rfifind
    from pypulsar_amd.rfi import RFIMask
    a, b = _twins(tmp_path, kind)
    for fn in (a, b):
        assert rfifind.main(["-t", "0.1", "--block", "8192", fn]) == 0
    ma = RFIMask.from_file(a[:-5] + "_rfifind.mask")
    mb = RFIMask.from_file(b[:-4] + "_rfifind.mask")
    np.testing.assert_array_equal(ma.mask, mb.mask)
    assert ma.masked_fraction == mb.masked_fraction
    assert (ma.nint, ma.nchan, ma.ptsperint) == (mb.nint, mb.nchan, mb.ptsperint)
    assert (ma.mjd, ma.dtint, ma.lofreq, ma.df) == (mb.mjd, mb.dtint, mb.lofreq, mb.df)
    assert (ma.time_sig, ma.freq_sig) == (mb.time_sig, mb.freq_sig)
