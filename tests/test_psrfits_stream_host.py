"""The PSRFITS search-file reader on the host (no GPU): row addressing and
raw row reads, the once-per-file mode decision, the open-by-content
dispatcher, the filterbank-like attributes, the fixture writer's unchanged
default bytes, and the stream restatement against the reference's
read_subint (bit for bit)."""
import numpy as np
import pytest

import psrfits_stream_oracle as pso
from conftest import band
from oracle import psrfits_oracle as po

TBIN = 64e-6


def _write(fn, nbits=8, nsub=3, nsblk=96, nchan=16, seed=0, descending=False, **kw):
    from pypulsar_amd.formats import psrfits
    rng = np.random.default_rng(seed)
    npol = kw.get("npol", 1)
    shape = (nsub, nsblk, nchan) if npol == 1 else (nsub, nsblk, npol, nchan)
    if nbits == 16:
        data = rng.integers(-3000, 3000, shape).astype(np.int16)
    else:
        data = rng.integers(0, 16 if nbits == 4 else 256, shape).astype(np.uint8)
    psrfits.write_search_psrfits(fn, data, band(nchan, descending), TBIN, nbits, **kw)
    return data


# ------------------------------------------------------------ rows_for / read_rows_into
def test_rows_for_and_read_rows(tmp_path):
    from pypulsar_amd.formats import fits, psrfits
    fn = str(tmp_path / "a.fits")
    nsblk, block, nsub = 96, 1024, 38       # 3648 samples: 3 blocks and a short one of 576
    _write(fn, nsub=nsub, nsblk=nsblk, nchan=16)
    f = psrfits.PsrfitsSearchFile(fn)
    assert f.number_of_samples == nsub * nsblk
    assert f.rows_for(0, block) == (0, 11, 0)               # samples 0..1023: rows 0..10
    assert f.rows_for(block, block) == (10, 12, 64)         # 1024 = 10*96 + 64 .. 2047 in row 21
    assert f.rows_for(3 * block, block) == (32, 6, 0)       # the last, short block: rows 32..37
    assert f.rows_for(nsub * nsblk, block) == (38, 0, 0)
    # the seam row 10 (samples 960..1055) belongs to both chunks
    r0, k0, _ = f.rows_for(0, block)
    r1, _, _ = f.rows_for(block, block)
    assert r0 + k0 - 1 == r1 == 10
    raw = fits.open(fn)["SUBINT"].raw_rows(0, nsub)
    for start in (0, block, 3 * block):
        row0, k, _ = f.rows_for(start, block)
        out = np.full((k + 1, f.row_bytes), 0x5A, dtype=np.uint8)
        assert f.read_rows_into(row0, out[:k]) == k
        np.testing.assert_array_equal(out[:k], raw[row0:row0 + k])
        assert (out[k] == 0x5A).all()
    # more rows asked than the table has left: whole rows only, none past the end
    out = np.zeros((8, f.row_bytes), dtype=np.uint8)
    assert f.read_rows_into(35, out) == 3
    np.testing.assert_array_equal(out[:3], raw[35:38])
    assert f.read_rows_into(38, out) == 0
    f.close()


def test_read_rows_refusals(tmp_path):
    from pypulsar_amd.formats import psrfits
    fn = str(tmp_path / "a.fits")
    _write(fn, nsub=4)
    f = psrfits.PsrfitsSearchFile(fn)
    wide = np.zeros((4, 2 * f.row_bytes), dtype=np.uint8)
    with pytest.raises(ValueError):
        f.read_rows_into(0, wide[:, ::2])                     # not contiguous
    with pytest.raises(ValueError):
        f.read_rows_into(0, np.zeros((4, f.row_bytes + 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        f.read_rows_into(0, np.zeros((4, f.row_bytes), dtype=np.int8))
    with pytest.raises(ValueError):
        f.read_rows_into(0, [[0] * f.row_bytes])
    with pytest.raises(ValueError):
        f.read_block_into(0, np.zeros((4, 2 * f.nchans), dtype=np.uint8)[:, ::2])
    with pytest.raises(ValueError):
        f.read_block_into(0, np.zeros((4, f.nchans), dtype=np.float32))   # the file is uint8
    f.close()


# ------------------------------------------------------------ mode decision
def test_mode_decision(tmp_path):
    from pypulsar_amd.formats import psrfits
    nsub, nchan = 5, 16
    one = np.ones((nsub, nchan), dtype=np.float32)
    fn = str(tmp_path / "m.fits")

    _write(fn, nsub=nsub)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "uint8"
    _write(fn, nbits=4, nsub=nsub)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "uint8"

    scl = one.copy()
    scl[-1, 7] = 1.5                       # one entry, in the last subint
    _write(fn, nsub=nsub, scales=scl)
    f = psrfits.PsrfitsSearchFile(fn)
    assert f.dtype == "float32" and f.scl_off >= 0
    f = psrfits.PsrfitsSearchFile(fn, apply_scales=False)
    assert f.dtype == "uint8" and f.scl_off == -1

    off = 0 * one
    off[3, 0] = -2.0
    _write(fn, nsub=nsub, offsets=off)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "float32"
    assert psrfits.PsrfitsSearchFile(fn, apply_offsets=False).dtype == "uint8"

    w = one.copy()
    w[2, 5] = 0.5
    _write(fn, nsub=nsub, weights=w)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "float32"
    assert psrfits.PsrfitsSearchFile(fn, apply_weights=False).dtype == "uint8"
    w[2, 5] = 0.0
    w[:, 9] = 0.0
    _write(fn, nsub=nsub, weights=w)
    f = psrfits.PsrfitsSearchFile(fn)
    assert f.dtype == "uint8" and f.wts_off >= 0 and f.scl_off == f.offs_off == -1

    _write(fn, nbits=16, nsub=nsub)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "float32"

    _write(fn, nsub=nsub, npol=2, pol_type="AABB")
    f = psrfits.PsrfitsSearchFile(fn)
    assert (f.dtype, f.pol0, f.npol_sum) == ("float32", 0, 2)
    f = psrfits.PsrfitsSearchFile(fn, poln=1)
    assert (f.dtype, f.pol0, f.npol_sum) == ("uint8", 1, 1)
    with pytest.raises(ValueError):
        psrfits.PsrfitsSearchFile(fn, poln=2)
    # a scale of the polarisation that is not used does not count
    scl2 = np.ones((nsub, 2 * nchan), dtype=np.float32)
    scl2[1, 3] = 2.0                       # polarisation 0
    _write(fn, nsub=nsub, npol=2, pol_type="AABB", scales=scl2)
    assert psrfits.PsrfitsSearchFile(fn, poln=1).dtype == "uint8"
    assert psrfits.PsrfitsSearchFile(fn, poln=0).dtype == "float32"

    _write(fn, nsub=nsub, npol=4, pol_type="IQUV")
    f = psrfits.PsrfitsSearchFile(fn)
    assert (f.dtype, f.pol0, f.npol_sum) == ("uint8", 0, 1)


def test_poln_from_environment(tmp_path, monkeypatch):
    from pypulsar_amd.formats import psrfits
    fn = str(tmp_path / "p.fits")
    _write(fn, npol=2, pol_type="AABB")
    monkeypatch.setenv("PSRFITS_POLN", "1")
    f = psrfits.PsrfitsSearchFile(fn)
    assert (f.pol0, f.npol_sum) == (1, 1)


def test_mode_scan_runs_in_slices(tmp_path, monkeypatch):
    """The scan reads bounded slices: with a bound of one row at a time the
    entry in the last row is still found."""
    from pypulsar_amd.formats import psrfits
    fn = str(tmp_path / "s.fits")
    scl = np.ones((6, 16), dtype=np.float32)
    scl[5, 15] = 3.0
    _write(fn, nsub=6, scales=scl)
    monkeypatch.setattr(psrfits.PsrfitsSearchFile, "_CHECK_BYTES", 1)
    assert psrfits.PsrfitsSearchFile(fn).dtype == "float32"


# ------------------------------------------------------------ open_search_file
def test_open_search_file(tmp_path):
    from pypulsar_amd.formats import filterbank, psrfits, sigproc
    fil = str(tmp_path / "x.fil")
    params, hdr = sigproc.make_header(16, 8, TBIN, 1500.0, -1.0)
    filterbank.write_filterbank(fil, params, hdr, np.zeros((32, 16), dtype=np.uint8))
    f = psrfits.open_search_file(fil)
    assert isinstance(f, filterbank.filterbank)
    f.close()
    # options meant for PSRFITS are noted and ignored for a filterbank
    f = psrfits.open_search_file(fil, apply_scales=False, poln=1)
    assert isinstance(f, filterbank.filterbank)
    f.close()

    dat = str(tmp_path / "x.dat")           # by content, not by extension
    _write(dat)
    f = psrfits.open_search_file(dat, apply_weights=False)
    assert isinstance(f, psrfits.PsrfitsSearchFile) and f.wts_off == -1
    f.close()

    fold = str(tmp_path / "fold.fits")
    _write(fold, primary={"OBS_MODE": "PSR"})
    with pytest.raises(ValueError, match="not a search-mode PSRFITS"):
        psrfits.open_search_file(fold)
    with pytest.raises(ValueError):
        psrfits.open_search_file(str(tmp_path / "missing.fits"))


# ------------------------------------------------------------ attributes
@pytest.mark.parametrize("descending", [True, False])
def test_adapter_attributes(tmp_path, descending):
    from pypulsar_amd import rfi
    from pypulsar_amd.formats import psrfits
    fn = str(tmp_path / "h.fits")
    nchan, nsub, nsblk = 16, 3, 96
    _write(fn, nsub=nsub, nsblk=nsblk, nchan=nchan, descending=descending)
    f = psrfits.PsrfitsSearchFile(fn)
    freqs = band(nchan, descending)
    np.testing.assert_array_equal(f.freqs, freqs)
    assert f.frequencies is f.freqs
    assert (f.nchans, f.nbits, f.packed, f.tsamp) == (nchan, 8, False, TBIN)
    assert f.number_of_samples == nsub * nsblk
    # the STT_* start of the fixture writer: 58850 + (11045 + 0.5) / 86400
    assert f.header["tstart"] == 58850 + (11045 + 0.5) / 86400.0
    assert f.header["foff"] == freqs[1] - freqs[0]
    assert (f.header["foff"] < 0) == descending
    assert f.header["fch1"] == freqs[0]
    assert (f.header["nchans"], f.header["tsamp"], f.header["nbits"]) == (nchan, TBIN, 8)
    h = rfi.file_header(f)
    assert h["mjd"] == f.header["tstart"] and h["tsamp"] == TBIN
    assert h["lofreq"] == freqs.min() and h["df"] == abs(freqs[1] - freqs[0])
    f.close()


def test_tstart_counts_nsuboffs(tmp_path):
    from pypulsar_amd.formats import psrfits
    fn = str(tmp_path / "o.fits")
    _write(fn, nsuboffs=5)
    f = psrfits.PsrfitsSearchFile(fn)
    assert f.header["tstart"] == psrfits.SpectraInfo([fn]).start_MJD[0]


# ------------------------------------------------------------ writer
@pytest.mark.parametrize("nbits", [4, 8, 16, 32])
def test_writer_default_bytes_unchanged(tmp_path, nbits):
    """With the default arguments the fixture writer's file is, byte for byte,
    what it was before it learnt ``npol``: the expected file is built here
    from fits.write directly."""
    from pypulsar_amd.formats import fits, psrfits
    nsub, nsblk, nchan = 2, 6, 8
    rng = np.random.default_rng(nbits)
    freqs = band(nchan)
    scl = rng.uniform(0.5, 2, (nsub, nchan)).astype(np.float32)
    off = rng.normal(0, 1, (nsub, nchan)).astype(np.float32)
    wts = rng.integers(0, 2, (nsub, nchan)).astype(np.float32)
    if nbits == 4:
        data = rng.integers(0, 16, (nsub, nsblk, nchan)).astype(np.uint8)
        flat = data.reshape(nsub, -1)
        body, tform = (flat[:, 0::2] & 15) | ((flat[:, 1::2] & 15) << 4), "%dB" % (nsblk * nchan // 2)
    elif nbits == 8:
        data = rng.integers(0, 256, (nsub, nsblk, nchan)).astype(np.uint8)
        body, tform = data.reshape(nsub, -1), "%dB" % (nsblk * nchan)
    elif nbits == 16:
        data = rng.integers(-999, 999, (nsub, nsblk, nchan)).astype(np.int16)
        body, tform = data.reshape(nsub, -1).astype(">i2"), "%dI" % (nsblk * nchan)
    else:
        data = rng.normal(0, 1, (nsub, nsblk, nchan)).astype(np.float32)
        body, tform = data.reshape(nsub, -1).astype(">f4"), "%dE" % (nsblk * nchan)
    got = str(tmp_path / "got.fits")
    psrfits.write_search_psrfits(got, data, freqs, TBIN, nbits, scl, off, wts)

    cols = [("TSUBINT", "1D"), ("OFFS_SUB", "1D"), ("TEL_AZ", "1E"), ("TEL_ZEN", "1E"),
            ("DAT_FREQ", "%dD" % nchan), ("DAT_WTS", "%dE" % nchan), ("DAT_OFFS", "%dE" % nchan),
            ("DAT_SCL", "%dE" % nchan), ("DATA", tform)]
    rows = {"TSUBINT": np.full(nsub, nsblk * TBIN),
            "OFFS_SUB": (np.arange(nsub) + 0.5) * nsblk * TBIN,
            "TEL_AZ": np.full(nsub, 123.5, dtype=np.float32),
            "TEL_ZEN": np.full(nsub, 21.25, dtype=np.float32),
            "DAT_FREQ": np.tile(freqs, (nsub, 1)), "DAT_WTS": wts, "DAT_OFFS": off,
            "DAT_SCL": scl, "DATA": body}
    p = [("FITSTYPE", "PSRFITS"), ("OBS_MODE", "SEARCH"), ("TELESCOP", "GBT"),
         ("OBSERVER", "pdd"), ("SRC_NAME", "J0000+0000"), ("FRONTEND", "Rcvr1_2"),
         ("BACKEND", "GUPPI"), ("PROJID", "TEST"), ("DATE-OBS", "2020-01-02T03:04:05.500"),
         ("FD_POLN", "LIN"), ("RA", "12:34:56.7"), ("DEC", "-01:23:45.6"),
         ("OBSFREQ", float(np.mean(freqs))), ("OBSNCHAN", nchan),
         ("OBSBW", float(abs(freqs[-1] - freqs[0]) * nchan / max(nchan - 1, 1))),
         ("BMIN", 0.15), ("CHAN_DM", 0.0), ("STT_IMJD", 58850), ("STT_SMJD", 11045),
         ("STT_OFFS", 0.5), ("TRK_MODE", "TRACK")]
    sub = [("TBIN", float(TBIN)), ("NCHAN", nchan), ("NPOL", 1), ("POL_TYPE", "AA+BB"),
           ("NCHNOFFS", 0), ("NSBLK", nsblk), ("NBITS", nbits), ("NSUBOFFS", 0)]
    want = str(tmp_path / "want.fits")
    fits.write(want, p, [("SUBINT", sub, cols, rows)])
    assert open(got, "rb").read() == open(want, "rb").read()


def test_writer_npol(tmp_path):
    from pypulsar_amd.formats import fits, psrfits
    fn = str(tmp_path / "n.fits")
    data = _write(fn, nbits=16, nsub=2, nsblk=5, nchan=6, npol=4, pol_type="IQUV")
    sub = fits.open(fn)["SUBINT"]
    assert (sub.header["NPOL"], sub.header["POL_TYPE"]) == (4, "IQUV")
    assert sub.columns[sub.columns.names.index("DAT_SCL")].repeat == 24
    np.testing.assert_array_equal(np.asarray(sub.data["DATA"]).reshape(2, 5, 4, 6), data)


# ------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nbits", [4, 8, 16, 32])
@pytest.mark.parametrize("applied", [(True, True, True), (False, True, True), (True, False, True),
                                     (True, True, False), (False, False, False)])
def test_restatement_is_read_subint(nbits, applied):
    nsub, nsblk, nchan = 3, 5, 12
    rng = np.random.default_rng(nbits)
    if nbits == 32:
        data = rng.normal(0, 50, (nsub, nsblk, nchan)).astype(np.float32)
    elif nbits == 16:
        data = rng.integers(-30000, 30000, (nsub, nsblk, nchan)).astype(np.int16)
    else:
        data = rng.integers(0, 1 << nbits, (nsub, nsblk, nchan)).astype(np.uint8)
    scl = rng.uniform(0.5, 2, (nsub, nchan)).astype(np.float32)
    off = rng.normal(0, 3, (nsub, nchan)).astype(np.float32)
    wts = rng.integers(0, 3, (nsub, nchan)).astype(np.float32) / 2
    a_s, a_o, a_w = applied
    got = pso.decode(data, nbits, scl, off, wts, apply_scales=a_s, apply_offsets=a_o,
                     apply_weights=a_w)
    assert got.dtype == np.float32 and got.shape == (nsub * nsblk, nchan)
    for i in range(nsub):
        want = po.read_subint(pso.stored(data[i], nbits), nbits, nsblk, nchan, scl[i], off[i],
                              wts[i], a_w, a_s, a_o)
        np.testing.assert_array_equal(got[i * nsblk:(i + 1) * nsblk].view(np.uint32),
                                      np.asarray(want, dtype=np.float32).view(np.uint32))


def test_restatement_sum_and_u8():
    nsub, nsblk, nchan = 2, 3, 4
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, (nsub, nsblk, 2, nchan)).astype(np.uint8)
    scl = rng.uniform(0.5, 2, (nsub, 2 * nchan)).astype(np.float32)
    off = rng.normal(0, 3, (nsub, 2 * nchan)).astype(np.float32)
    wts = rng.integers(0, 2, (nsub, nchan)).astype(np.float32)
    got = pso.decode(data, 8, scl, off, wts, npol_sum=2)
    s, o = scl.reshape(nsub, 2, nchan), off.reshape(nsub, 2, nchan)
    d = data.astype(np.float32)
    want = (((d[:, :, 0] * s[:, None, 0]) + o[:, None, 0])
            + ((d[:, :, 1] * s[:, None, 1]) + o[:, None, 1])) * wts[:, None]
    np.testing.assert_array_equal(got, want.reshape(-1, nchan))
    # unscaled uint8 parts are summed in float32, not in uint8
    got = pso.decode(data, 8, scl, off, wts, npol_sum=2, apply_scales=False, apply_offsets=False,
                     apply_weights=False)
    np.testing.assert_array_equal(got, (d[:, :, 0] + d[:, :, 1]).reshape(-1, nchan))
    u = pso.decode(data, 8, scl, off, wts, pol0=1, out="uint8")
    assert u.dtype == np.uint8
    np.testing.assert_array_equal(u, (data[:, :, 1] * (wts[:, None] != 0)).reshape(-1, nchan))
