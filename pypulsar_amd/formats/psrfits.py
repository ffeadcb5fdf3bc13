"""PSRFITS search-mode reader feeding the device ``Spectra`` (drop-in for
pypulsar's formats/psrfits.py).

Same names and behaviour as the reference: ``PsrfitsFile(fn)`` with
``filename``, ``fits``, ``specinfo``, ``header``, ``nbits``, ``nchan``,
``nsamp_per_subint``, ``nsubints``, ``freqs``/``frequencies``, ``tsamp``;
``read_subint``, ``get_weights``/``get_scales``/``get_offsets``,
``get_spectra``; ``SpectraInfo`` (psrfits.py:186-464) with its ``__str__``;
``unpack_4bit``, ``DATEOBS_to_MJD``, ``is_PSRFITS``, ``debug_mode``.

The data path is the device: ``get_spectra`` copies the needed SUBINT rows
(as stored, big-endian) to the GPU and one HIP kernel
(``pdd_psrfits_subints``) unpacks 4/8/16/32-bit samples, applies
``((data*scales)+offsets)*weights`` in float32 in the reference's order
(psrfits.py:103-106), transposes to ``[chan, time]``, cuts the requested
span and flips an ascending band (psrfits.py:140-183).  ``read_subint``
returns the same kernel's result as a host ``[nsamp, nchan]`` float32 array.

Differences, all where the reference cannot run here: the FITS container is
read by ``formats/fits.py`` (astropy absent); PRESTO's ``psr_utils`` and
``pyslalib`` are replaced by SECPERDAY = 86400 and the SLALIB sla_cldj
calendar formula (``_cldj``); ``get_spectra`` at the exact end of a file
reads only the subints it needs (the reference indexes one past the last
subint there and raises); multi-polarisation data (NPOL > 1 unsummed) is
rejected as in the reference's reshape.

New, for the searches: ``PsrfitsSearchFile`` gives a
search-mode file the attributes and ``read_block_into`` of a ``filterbank``
and streams it as its own SUBINT rows (``rows_for``, ``read_rows_into``),
which ``PsrfitsDecoder`` turns into the stream's time-major uint8 or float32
block on the device (``pdd_psrfits_block``: scales, offsets and weights read
from the rows, one polarisation or AA + BB); ``open_search_file`` returns a
``filterbank`` or a ``PsrfitsSearchFile`` by the file's content.
"""
import os
import re
import warnings

import numpy as np

from . import fits as pyfits

SECPERDAY = 86400.0

date_obs_re = re.compile(r"^(?P<year>[0-9]{4})-(?P<month>[0-9]{2})-"
                         r"(?P<day>[0-9]{2})T(?P<hour>[0-9]{2}):"
                         r"(?P<min>[0-9]{2}):(?P<sec>[0-9]{2}"
                         r"(?:\.[0-9]+)?)$")

debug = True


def unpack_4bit(data):
    """Two 4-bit samples per byte, low nibble first (psrfits.py:37-50).
    Host helper; the device kernel decodes the same order."""
    data = np.asarray(data, dtype=np.uint8)
    return np.dstack([np.bitwise_and(15, data), data >> 4]).flatten()


def _cldj(iy, im, idd):
    """SLALIB sla_cldj: Gregorian calendar date -> Modified Julian Date
    (integer arithmetic with Fortran truncating division).  Returns
    (mjd, status)."""
    iy, im, idd = int(iy), int(im), int(idd)
    if iy < -4699:
        return 0.0, 1
    if im < 1 or im > 12:
        return 0.0, 2
    mtab = [31, 28 + (1 if (iy % 4 == 0 and (iy % 100 != 0 or iy % 400 == 0)) else 0),
            31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    status = 0 if 1 <= idd <= mtab[im - 1] else 3

    def tdiv(a, b):
        q = abs(a) // abs(b)
        return q if (a >= 0) == (b >= 0) else -q
    djm = (tdiv(1461 * (iy - tdiv(12 - im, 10) + 4712), 4)
           + tdiv(306 * ((im + 9) % 12) + 5, 10)
           - tdiv(3 * tdiv(iy - tdiv(12 - im, 10) + 4900, 100), 4)
           + idd - 2399904)
    return float(djm), status


def DATEOBS_to_MJD(dateobs):
    """DATE-OBS string -> (integer MJD, fractional day) (psrfits.py:563-575)."""
    m = date_obs_re.match(dateobs)
    mjd_fracday = (float(m.group("hour")) + (float(m.group("min")) +
                                             (float(m.group("sec")) / 60.0)) / 60.0) / 24.0
    mjd_day, err = _cldj(float(m.group("year")), float(m.group("month")), float(m.group("day")))
    return mjd_day, mjd_fracday


def is_PSRFITS(filename):
    """FITSTYPE == 'PSRFITS' and OBS_MODE == 'SEARCH' (psrfits.py:578-594)."""
    hdus = pyfits.open(filename, mode="readonly")
    primary = hdus["PRIMARY"].header
    try:
        ok = (primary["FITSTYPE"] == "PSRFITS") and (primary["OBS_MODE"] == "SEARCH")
    except KeyError:
        ok = False
    hdus.close()
    return ok


def debug_mode(mode=None):
    global debug
    if mode is None:
        return debug
    debug = bool(mode)


def _sexagesimal_to_deg(s, hours):
    """protractor.convert(s, 'hmsstr'|'dmsstr', 'deg') (utils/astro/protractor.py:19-80):
    [sign]DD:MM[:SS.S], the sign applying to the whole value; NaN if unparsable."""
    m = re.match(r"^(?P<sign>[-+])?(?P<a>\d{2}):(?P<b>\d{2})(?::(?P<c>\d{2}(?:.\d+)?))?$", str(s))
    if m is None:
        warnings.warn("Input is not a valid sexigesimal string: %s" % s)
        return float("nan")
    v = float(m.group("a")) + float(m.group("b")) / 60.0 + float(m.group("c") or 0) / 3600.0
    v = -v if m.group("sign") == "-" else v
    return v * 15.0 if hours else v


class SpectraInfo(object):
    """Header summary of one or more PSRFITS files (psrfits.py:186-464)."""

    def __init__(self, filenames):
        self.filenames = filenames
        self.num_files = len(filenames)
        self.N = 0
        self.user_poln = 0
        self.default_poln = 0
        self.start_MJD = np.empty(self.num_files)
        self.num_subint = np.empty(self.num_files)
        self.start_subint = np.empty(self.num_files)
        self.start_spec = np.empty(self.num_files)
        self.num_pad = np.empty(self.num_files)
        self.num_spec = np.empty(self.num_files)
        self.need_scale = False
        self.need_offset = False
        self.need_weight = False
        self.need_flipband = False

        for ii, fn in enumerate(filenames):
            if not is_PSRFITS(fn):
                raise ValueError("File '%s' does not appear to be PSRFITS!" % fn)
            hdus = pyfits.open(fn, mode="readonly")
            if ii == 0:
                self.hdu_names = [hdu.name for hdu in hdus]
            primary = hdus["PRIMARY"].header
            telescope = primary.get("TELESCOP", "")
            if telescope == "ARECIBO 305m":
                telescope = "Arecibo"
            if ii == 0:
                self.telescope = telescope
            elif telescope != self.telescope[0]:
                warnings.warn("'TELESCOP' values don't match for files 0 and %d!" % ii)
            self.observer = primary["OBSERVER"]
            self.source = primary["SRC_NAME"]
            self.frontend = primary["FRONTEND"]
            self.backend = primary["BACKEND"]
            self.project_id = primary["PROJID"]
            self.date_obs = primary["DATE-OBS"]
            self.poln_type = primary["FD_POLN"]
            self.ra_str = primary["RA"]
            self.dec_str = primary["DEC"]
            self.fctr = primary["OBSFREQ"]
            self.orig_num_chan = primary["OBSNCHAN"]
            self.orig_df = primary["OBSBW"]
            self.beam_FWHM = primary["BMIN"]
            self.chan_dm = primary.get("CHAN_DM", 0.0)
            self.start_MJD[ii] = primary["STT_IMJD"] + (primary["STT_SMJD"] +
                                                        primary["STT_OFFS"]) / SECPERDAY
            track = primary["TRK_MODE"] == "TRACK"
            if ii == 0:
                self.tracking = track
            elif track != self.tracking:
                warnings.warn("'TRK_MODE' values don't match for files 0 and %d" % ii)

            subint = hdus["SUBINT"].header
            self.dt = subint["TBIN"]
            self.num_channels = subint["NCHAN"]
            self.num_polns = subint["NPOL"]
            envval = os.getenv("PSRFITS_POLN")
            if envval is not None:
                ival = int(envval)
                if -1 < ival < self.num_polns:
                    print("Using polarisation %d (from 0-%d) from PSRFITS_POLN." %
                          (ival, self.num_polns - 1))
                    self.default_poln = ival
                    self.user_poln = 1
            self.poln_order = subint["POL_TYPE"]
            if subint["NCHNOFFS"] > 0:
                warnings.warn("first freq channel is not 0 in file %d" % ii)
            self.spectra_per_subint = subint["NSBLK"]
            self.bits_per_sample = subint["NBITS"]
            self.num_subint[ii] = subint["NAXIS2"]
            self.start_subint[ii] = subint["NSUBOFFS"]
            self.time_per_subint = self.dt * self.spectra_per_subint
            self.start_MJD[ii] += (self.time_per_subint * self.start_subint[ii]) / SECPERDAY
            MJDf = self.start_MJD[ii] - self.start_MJD[0]
            if MJDf < 0.0:
                raise ValueError("File %d seems to be from before file 0!" % ii)
            self.start_spec[ii] = (MJDf * SECPERDAY / self.dt + 0.5)

            sh = hdus["SUBINT"]
            names = sh.columns.names
            if "OFFS_SUB" not in names:
                warnings.warn("Can't find the 'OFFS_SUB' column!")
            else:
                col = names.index("OFFS_SUB")
                if ii == 0:
                    self.offs_sub_col = col
                elif self.offs_sub_col != col:
                    warnings.warn("'OFFS_SUB' column changes between files 0 and %d!" % ii)
            if "DATA" not in names:
                warnings.warn("Can't find the 'DATA' column!")
            else:
                col = names.index("DATA")
                if ii == 0:
                    self.data_col = col
                    self.FITS_typecode = sh.columns[self.data_col].format[-1]
                elif self.data_col != col:
                    warnings.warn("'DATA' column changes between files 0 and %d!" % ii)
            if "TEL_AZ" not in names:
                self.azimuth = 0.0
            elif ii == 0:
                self.tel_az_col = names.index("TEL_AZ")
                self.azimuth = sh.data[0]["TEL_AZ"]
            if "TEL_ZEN" not in names:
                self.zenith_ang = 0.0
            elif ii == 0:
                self.tel_zen_col = names.index("TEL_ZEN")
                self.zenith_ang = sh.data[0]["TEL_ZEN"]
            if "DAT_FREQ" not in names:
                warnings.warn("Can't find the channel freq column, 'DAT_FREQ'!")
            else:
                col = names.index("DAT_FREQ")
                freqs = np.atleast_1d(sh.data[0]["DAT_FREQ"]).astype(np.float64)
                if ii == 0:
                    self.freqs_col = col
                    self.df = freqs[1] - freqs[0]
                    self.lo_freq = freqs[0]
                    self.hi_freq = freqs[-1]
                    ftmp = freqs[1:] - freqs[:-1]
                    if np.any((ftmp - self.df)) > 1e-7:  # the reference's test, kept as is
                        warnings.warn("Channel spacing changes in file %d!" % ii)
                else:
                    if np.abs(self.df - (freqs[1] - freqs[0])) > 1e-7:
                        warnings.warn("Channel spacing between files 0 and %d!" % ii)
                    if np.abs(self.lo_freq - freqs[0]) > 1e-7:
                        warnings.warn("Low channel changes between files 0 and %d!" % ii)
                    if np.abs(self.hi_freq - freqs[-1]) > 1e-7:
                        warnings.warn("High channel changes between files 0 and %d!" % ii)
            for key, attr, unit in (("DAT_WTS", "dat_wts_col", 1.0),
                                    ("DAT_OFFS", "dat_offs_col", 0.0),
                                    ("DAT_SCL", "dat_scl_col", 1.0)):
                label = {"DAT_WTS": "weights", "DAT_OFFS": "offsets", "DAT_SCL": "scalings"}[key]
                if key not in names:
                    warnings.warn("Can't find the channel %s column, '%s'!" % (label, key))
                    continue
                col = names.index(key)
                if ii == 0:
                    setattr(self, attr, col)
                elif getattr(self, attr) != col:
                    warnings.warn("'%s' column changes between files 0 and %d!" % (key, ii))
                if np.any(np.atleast_1d(sh.data[0][key]) != unit):
                    if key == "DAT_WTS":
                        self.need_weight = True
                    elif key == "DAT_OFFS":
                        self.need_offset = True
                    else:
                        self.need_scale = True
            self.num_pad[ii] = 0
            self.num_spec[ii] = self.spectra_per_subint * self.num_subint[ii]
            if ii > 0 and self.start_spec[ii] > self.N:
                self.num_pad[ii - 1] = self.start_spec[ii] - self.N
                self.N += self.num_pad[ii - 1]
            self.N += self.num_spec[ii]

        self.ra2000 = _sexagesimal_to_deg(self.ra_str, hours=True)
        self.dec2000 = _sexagesimal_to_deg(self.dec_str, hours=False)
        self.summed_polns = self.poln_order in ("AA+BB", "INTEN")
        self.T = self.N * self.dt
        self.orig_df /= float(self.orig_num_chan)
        self.samples_per_spectra = self.num_polns * self.num_channels
        if self.bits_per_sample < 8:
            self.bytes_per_spectra = self.samples_per_spectra
        else:
            self.bytes_per_spectra = (self.bits_per_sample * self.samples_per_spectra) / 8
        self.samples_per_subint = self.samples_per_spectra * self.spectra_per_subint
        self.bytes_per_subint = self.bytes_per_spectra * self.spectra_per_subint
        if self.hi_freq < self.lo_freq:
            self.hi_freq, self.lo_freq = self.lo_freq, self.hi_freq
            self.df *= -1.0
            self.need_flipband = True
        self.BW = self.num_channels * self.df
        self.mjd = int(self.start_MJD[0])
        self.secs = (self.start_MJD[0] % 1) * SECPERDAY

    def __str__(self):
        """psrfits.py:466-557, same lines."""
        r = ["From the PSRFITS file '%s':" % self.filenames[0],
             "                       HDUs = %s" % ", ".join(self.hdu_names),
             "                  Telescope = %s" % self.telescope,
             "                   Observer = %s" % self.observer,
             "                Source Name = %s" % self.source,
             "                   Frontend = %s" % self.frontend,
             "                    Backend = %s" % self.backend,
             "                 Project ID = %s" % self.project_id,
             "            Obs Date String = %s" % self.date_obs]
        imjd, fmjd = DATEOBS_to_MJD(self.date_obs)
        mjdtmp = "%.14f" % fmjd
        r.append("  MJD start time (DATE-OBS) = %5d.%14s" % (imjd, mjdtmp[2:]))
        r.append("     MJD start time (STT_*) = %19.14f" % self.start_MJD[0])
        r.append("                   RA J2000 = %s" % self.ra_str)
        r.append("             RA J2000 (deg) = %-17.15g" % self.ra2000)
        r.append("                  Dec J2000 = %s" % self.dec_str)
        r.append("            Dec J2000 (deg) = %-17.15g" % self.dec2000)
        r.append("                  Tracking? = %s" % self.tracking)
        r.append("              Azimuth (deg) = %-.7g" % self.azimuth)
        r.append("           Zenith Ang (deg) = %-.7g" % self.zenith_ang)
        r.append("          Polarisation type = %s" % self.poln_type)
        if self.num_polns >= 2 and not self.summed_polns:
            numpolns = "%d" % self.num_polns
        elif self.summed_polns:
            numpolns = "2 (summed)"
        else:
            numpolns = "1"
        r.append("            Number of polns = %s" % numpolns)
        r.append("          Polarisation oder = %s" % self.poln_order)
        r.append("           Sample time (us) = %-17.15g" % (self.dt * 1e6))
        r.append("         Central freq (MHz) = %-17.15g" % self.fctr)
        r.append("          Low channel (MHz) = %-17.15g" % self.lo_freq)
        r.append("         High channel (MHz) = %-17.15g" % self.hi_freq)
        r.append("        Channel width (MHz) = %-17.15g" % self.df)
        r.append("         Number of channels = %d" % self.num_channels)
        if self.chan_dm != 0.0:
            r.append("   Orig Channel width (MHz) = %-17.15g" % self.orig_df)
            r.append("    Orig Number of channels = %d" % self.orig_num_chan)
            r.append("    DM used for chan dedisp = %-17.15g" % self.chan_dm)
        r.append("      Total Bandwidth (MHz) = %-17.15g" % self.BW)
        r.append("         Spectra per subint = %d" % self.spectra_per_subint)
        r.append("            Starting subint = %d" % self.start_subint[0])
        r.append("           Subints per file = %d" % self.num_subint[0])
        r.append("           Spectra per file = %d" % self.num_spec[0])
        r.append("        Time per file (sec) = %-.12g" % (self.num_spec[0] * self.dt))
        r.append("              FITS typecode = %s" % self.FITS_typecode)
        if debug:
            r.append("                DATA column = %d" % self.data_col)
            r.append("            bits per sample = %d" % self.bits_per_sample)
            if self.bits_per_sample < 8:
                spectmp = (self.bytes_per_spectra * self.bits_per_sample) / 8
                subtmp = (self.bytes_per_subint * self.bits_per_sample) / 8
            else:
                spectmp = self.bytes_per_spectra
                subtmp = self.bytes_per_subint
            r.append("          bytes per spectra = %d" % spectmp)
            r.append("        samples per spectra = %d" % self.samples_per_spectra)
            r.append("           bytes per subint = %d" % subtmp)
            r.append("         samples per subint = %d" % self.samples_per_subint)
            r.append("              Need scaling? = %s" % self.need_scale)
            r.append("              Need offsets? = %s" % self.need_offset)
            r.append("              Need weights? = %s" % self.need_weight)
            r.append("        Need band inverted? = %s" % self.need_flipband)
        return "\n".join(r)

    def __getitem__(self, key):
        return getattr(self, key)


class PsrfitsFile(object):
    def __init__(self, psrfitsfn):
        if not os.path.isfile(psrfitsfn):
            raise ValueError("ERROR: File does not exist!\n\t(%s)" % psrfitsfn)
        self.filename = psrfitsfn
        self.fits = pyfits.open(psrfitsfn, mode="readonly", memmap=True)
        self.specinfo = SpectraInfo([psrfitsfn])
        self.header = self.fits[0].header
        self.nbits = self.specinfo.bits_per_sample
        self.nchan = self.specinfo.num_channels
        self.nsamp_per_subint = self.specinfo.spectra_per_subint
        self.nsubints = int(self.specinfo.num_subint[0])
        self.freqs = np.atleast_1d(self.fits["SUBINT"].data[0]["DAT_FREQ"]).astype(np.float64)
        self.frequencies = self.freqs
        self.tsamp = self.specinfo.dt
        sub = self.fits["SUBINT"]
        names = sub.columns.names
        self._row_bytes = int(sub.header["NAXIS1"])
        self._data_off = sub.columns[names.index("DATA")].offset
        if self.nbits not in (4, 8, 16, 32):
            raise ValueError("PSRFITS nbits=%d is not supported (4, 8, 16, 32)" % self.nbits)
        npol = self.specinfo.num_polns
        if npol != 1 and not self.specinfo.summed_polns:
            raise ValueError("multi-polarisation (NPOL=%d) data cannot be reshaped to "
                             "(nsamp, nchan) (psrfits.py:104)" % npol)

    def get_weights(self, isub):
        return self.fits["SUBINT"].data[isub]["DAT_WTS"]

    def get_scales(self, isub):
        return self.fits["SUBINT"].data[isub]["DAT_SCL"]

    def get_offsets(self, isub):
        return self.fits["SUBINT"].data[isub]["DAT_OFFS"]

    def _wso(self, sub0, nsub, apply_weights=True, apply_scales=True, apply_offsets=True):
        """[nsub][3][nchan] float32: scales, offsets, weights (or 1, 0, 1)."""
        out = np.empty((nsub, 3, self.nchan), dtype=np.float32)
        for i in range(nsub):
            isub = sub0 + i
            out[i, 0] = np.asarray(self.get_scales(isub), dtype=np.float32)[:self.nchan] \
                if apply_scales else 1.0
            out[i, 1] = np.asarray(self.get_offsets(isub), dtype=np.float32)[:self.nchan] \
                if apply_offsets else 0.0
            out[i, 2] = np.asarray(self.get_weights(isub), dtype=np.float32)[:self.nchan] \
                if apply_weights else 1.0
        return out

    def _decode(self, sub0, nsub, s0, N, flip, apply_weights=True, apply_scales=True,
                apply_offsets=True):
        """Device [nchan, N] float32: samples s0 .. s0+N-1 of subints
        sub0 .. sub0+nsub-1 (pdd_psrfits_subints)."""
        import torch
        from .. import _lib
        from .._lib import call, ptr, stream_ptr
        _lib.require_gpu()
        if N == 0:
            return torch.empty((self.nchan, 0), dtype=torch.float32, device="cuda")
        rows = np.array(self.fits["SUBINT"].raw_rows(sub0, sub0 + nsub))  # host copy
        raw = torch.from_numpy(rows).pin_memory().cuda(non_blocking=True)
        wso = torch.from_numpy(self._wso(sub0, nsub, apply_weights, apply_scales,
                                         apply_offsets)).cuda()
        out = torch.empty((self.nchan, N), dtype=torch.float32, device="cuda")
        call("pdd_psrfits_subints", ptr(raw), nsub, self._row_bytes, self._data_off, self.nbits,
             self.nsamp_per_subint, self.nchan, ptr(wso), s0, N, int(bool(flip)), ptr(out),
             N, stream_ptr())
        return out

    def read_subint(self, isub, apply_weights=True, apply_scales=True, apply_offsets=True):
        """float32 [nsamp_per_subint, nchan] with scales, offsets and weights
        applied (psrfits.py:67-107), decoded on the device."""
        out = self._decode(isub, 1, 0, self.nsamp_per_subint, False, apply_weights,
                           apply_scales, apply_offsets)
        return out.t().contiguous().cpu().numpy()

    def get_spectra(self, startsamp, N):
        """Device Spectra of samples startsamp .. startsamp+N-1, high
        frequency first (psrfits.py:140-183)."""
        from .spectra import Spectra
        startsub = int(startsamp / self.nsamp_per_subint)
        skip = startsamp - startsub * self.nsamp_per_subint
        endsub = int((startsamp + N) / self.nsamp_per_subint)
        trunc = ((endsub + 1) * self.nsamp_per_subint) - (startsamp + N)
        if trunc < 0:
            raise ValueError("Number of bins to truncate is negative: %d" % trunc)
        # subints actually holding samples (the reference also reads endsub
        # when the span ends on a subint boundary; its samples are cut)
        last = min(endsub, (startsamp + N - 1) // self.nsamp_per_subint) if N > 0 else startsub
        if last >= self.nsubints:
            raise IndexError("samples up to %d requested, file has %d"
                             % (startsamp + N, self.nsubints * self.nsamp_per_subint))
        flip = not self.specinfo.need_flipband
        data = self._decode(startsub, last - startsub + 1, skip, N, flip)
        freqs = self.freqs[::-1] if flip else self.freqs
        return Spectra._from_device(np.array(freqs), self.tsamp, data,
                                    starttime=self.tsamp * startsamp)


class PsrfitsDecoder(object):
    """Device decode of verbatim SUBINT rows into the stream's time-major raw
    block (pdd_psrfits_block): what ``StreamingSweep(decoder=...)`` uses.
    Holds the file's geometry only, no open file."""

    def __init__(self, row_bytes, data_off, scl_off, offs_off, wts_off, nbits, nsblk, nchan,
                 npol, pol0, npol_sum, nsubints, dtype):
        self.row_bytes, self.data_off = int(row_bytes), int(data_off)
        self.scl_off, self.offs_off, self.wts_off = int(scl_off), int(offs_off), int(wts_off)
        self.nbits, self.nsblk, self.nchan = int(nbits), int(nsblk), int(nchan)
        self.npol, self.pol0, self.npol_sum = int(npol), int(pol0), int(npol_sum)
        self.nsubints = int(nsubints)
        self.number_of_samples = self.nsubints * self.nsblk
        self.dtype = np.dtype(dtype)  # uint8 (integer mode) or float32

    @property
    def torch_dtype(self):
        import torch
        return torch.uint8 if self.dtype == np.uint8 else torch.float32

    def rows_for(self, start, n):
        """(row0, nrows, s0): the rows that hold samples [start, start + n)
        (cut at the end of the file) and the offset of ``start`` in the first
        of them."""
        start = int(start)
        n = max(0, min(int(n), self.number_of_samples - start))
        row0 = start // self.nsblk
        s0 = start - row0 * self.nsblk
        if n == 0:
            return row0, 0, s0
        return row0, (start + n - 1) // self.nsblk - row0 + 1, s0

    def max_rows(self, n):
        """Most rows any span of ``n`` samples touches."""
        return (max(int(n), 1) - 1) // self.nsblk + 2

    def decode(self, rows, nrows, s0, n, out, stream=None):
        """Samples [s0, s0 + n) of the ``nrows`` device rows ``rows``
        (uint8 [>= nrows, row_bytes]) -> out[:n] (device [>= n, >= nchan] of
        this decoder's dtype, unit channel stride)."""
        from .. import _lib
        from .._lib import call, ptr, stream_ptr
        assert rows.is_cuda and rows.dtype.itemsize == 1 and rows.is_contiguous()
        assert rows.shape[1] == self.row_bytes and rows.shape[0] >= nrows
        assert out.is_cuda and out.dtype == self.torch_dtype and out.stride(1) == 1
        assert out.shape[0] >= n and out.shape[1] >= self.nchan
        if n:
            call("pdd_psrfits_block", ptr(rows), int(nrows), self.row_bytes, self.data_off,
                 self.scl_off, self.offs_off, self.wts_off, self.nbits, self.nsblk, self.nchan,
                 self.npol, self.pol0, self.npol_sum, int(s0), int(n),
                 _lib.U8 if self.dtype == np.uint8 else _lib.F32, ptr(out), out.stride(0),
                 stream_ptr(stream))
        return out[:n, :self.nchan]


class PsrfitsSearchFile(object):
    """A search-mode PSRFITS file as the search tools read a ``filterbank``:
    ``nchans``, ``freqs`` / ``frequencies`` (DAT_FREQ of row 0, file order),
    ``tsamp``, ``number_of_samples`` (NAXIS2 * NSBLK), ``nbits``, ``packed``
    (False), ``dtype`` ("uint8" or "float32": what the device decode emits),
    ``header`` (tstart, fch1, foff, nchans, tsamp, nbits, ...),
    ``read_block_into`` and ``close``; plus the row interface of the stream:
    ``rows_for``, ``read_rows_into`` and ``decoder()``.

    Polarisations (the project's own rule; PRESTO is absent, parity unpinned):
    NPOL 1 or POL_TYPE AA+BB / INTEN: the one polarisation; AABB / AABBCRCI:
    AA + BB summed after scales and offsets; IQUV: polarisation 0; ``poln=k``
    (or the PSRFITS_POLN environment variable): polarisation k alone.

    Mode, decided once over every row of the file: integer (uint8 samples,
    the file's own values, zeroed where the weight is 0) when nbits is 4 or
    8, one polarisation is used and every applied DAT_SCL is 1, DAT_OFFS 0
    and DAT_WTS 0 or 1; float32 ``((v*scl)+offs)*wts`` otherwise.
    ``apply_*=False`` takes a column out of the test and of the decode."""

    _CHECK_BYTES = 1 << 26  # bound of one slice of the mode scan

    def __init__(self, fn, apply_scales=True, apply_offsets=True, apply_weights=True, poln=None):
        if not os.path.isfile(fn):
            raise ValueError("ERROR: File does not exist!\n\t(%s)" % fn)
        if not is_PSRFITS(fn):
            raise ValueError("File '%s' is not a search-mode PSRFITS file" % fn)
        self.filename = fn
        self.fits = pyfits.open(fn, mode="readonly", memmap=True)
        primary = self.fits["PRIMARY"].header
        sub = self.fits["SUBINT"]
        sh = sub.header
        names = sub.columns.names
        self.nbits = int(sh["NBITS"])
        if self.nbits not in (4, 8, 16, 32):
            raise ValueError("PSRFITS nbits=%d is not supported (4, 8, 16, 32)" % self.nbits)
        self.nchans = self.nchan = int(sh["NCHAN"])
        self.npol = int(sh.get("NPOL", 1))
        self.pol_type = str(sh.get("POL_TYPE", "AA+BB")).strip()
        self.nsblk = self.nsamp_per_subint = int(sh["NSBLK"])
        self.nsubints = int(sh["NAXIS2"])
        self.number_of_samples = self.nsubints * self.nsblk
        self.tsamp = float(sh["TBIN"])
        self.packed = False
        self.row_bytes = int(sh["NAXIS1"])
        self._data_offset = int(sub.data_offset)
        if "DATA" not in names or "DAT_FREQ" not in names:
            raise ValueError("%s: the SUBINT table has no DATA / DAT_FREQ column" % fn)
        col = sub.columns[names.index("DATA")]
        self.data_off = int(col.offset)
        if col.nbytes * 8 != self.nsblk * self.npol * self.nchans * self.nbits:
            raise ValueError("%s: DATA holds %d bytes a row, NSBLK x NPOL x NCHAN x NBITS needs %d "
                             "(a partial last subint is not supported)"
                             % (fn, col.nbytes, self.nsblk * self.npol * self.nchans * self.nbits // 8))
        if self.nbits == 4 and (self.npol * self.nchans) % 2:
            raise ValueError("%s: 4-bit spectra of %d samples do not fill whole bytes"
                             % (fn, self.npol * self.nchans))
        # polarisations
        if poln is None and os.getenv("PSRFITS_POLN") is not None:
            poln = int(os.getenv("PSRFITS_POLN"))
        if poln is not None:
            if not 0 <= int(poln) < self.npol:
                raise ValueError("polarisation %d of a file with %d" % (poln, self.npol))
            self.pol0, self.npol_sum = int(poln), 1
        elif self.npol == 1 or self.pol_type in ("AA+BB", "INTEN", "IQUV"):
            self.pol0, self.npol_sum = 0, 1
        elif self.pol_type in ("AABB", "AABBCRCI") and self.npol >= 2:
            self.pol0, self.npol_sum = 0, 2
        else:
            raise ValueError("%s: POL_TYPE %r with NPOL %d: choose a polarisation (poln)"
                             % (fn, self.pol_type, self.npol))
        # scale, offset and weight columns in use (-1: not applied)
        offs = {}
        for key, want, count in (("DAT_SCL", apply_scales, self.npol * self.nchans),
                                 ("DAT_OFFS", apply_offsets, self.npol * self.nchans),
                                 ("DAT_WTS", apply_weights, self.nchans)):
            offs[key] = -1
            if want and key in names:
                c = sub.columns[names.index(key)]
                if c.code != "E" or c.repeat < count:
                    raise ValueError("%s: column %s is %s, expected %dE" % (fn, key, c.format, count))
                offs[key] = int(c.offset)
        self.scl_off, self.offs_off, self.wts_off = offs["DAT_SCL"], offs["DAT_OFFS"], offs["DAT_WTS"]
        self.freqs = np.atleast_1d(sub.data[0]["DAT_FREQ"]).astype(np.float64) \
            if self.nsubints else np.zeros(self.nchans)
        self.frequencies = self.freqs
        self.is_hifreq_first = bool(len(self.freqs) > 1 and self.freqs[1] < self.freqs[0])
        self.dtype = "uint8" if self._integer_mode() else "float32"
        if self.dtype == "uint8":
            self.scl_off = self.offs_off = -1  # all 1 and 0: the file's own values
        tstart = (primary.get("STT_IMJD", 0) + (primary.get("STT_SMJD", 0) +
                                                primary.get("STT_OFFS", 0.0)) / SECPERDAY
                  + self.tsamp * self.nsblk * sh.get("NSUBOFFS", 0) / SECPERDAY)
        foff = float(self.freqs[1] - self.freqs[0]) if self.nchans > 1 else \
            float(sh.get("CHAN_BW", 1.0))
        self.header = {"tstart": float(tstart), "fch1": float(self.freqs[0]), "foff": foff,
                       "nchans": self.nchans, "tsamp": self.tsamp, "nbits": self.nbits,
                       "nifs": 1, "source_name": str(primary.get("SRC_NAME", "")),
                       "telescope": str(primary.get("TELESCOP", ""))}
        self._f = open(fn, "rb")

    def _integer_mode(self):
        """The mode decision over every row, read through the memmap in
        bounded slices."""
        if self.nbits not in (4, 8) or self.npol_sum != 1:
            return False
        data = self.fits["SUBINT"].data
        lo_c, hi_c = self.pol0 * self.nchans, (self.pol0 + 1) * self.nchans
        step = max(1, self._CHECK_BYTES // max(1, 12 * self.nchans))
        for r0 in range(0, self.nsubints, step):
            part = data[r0:r0 + step]
            if self.scl_off >= 0 and np.any(np.asarray(part["DAT_SCL"]).reshape(
                    len(part), -1)[:, lo_c:hi_c] != 1):
                return False
            if self.offs_off >= 0 and np.any(np.asarray(part["DAT_OFFS"]).reshape(
                    len(part), -1)[:, lo_c:hi_c] != 0):
                return False
            if self.wts_off >= 0:
                w = np.asarray(part["DAT_WTS"]).reshape(len(part), -1)[:, :self.nchans]
                if np.any((w != 0) & (w != 1)):
                    return False
        return True

    def close(self):
        f = self.__dict__.get("_f")
        if f is not None and not f.closed:
            f.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decoder(self):
        return PsrfitsDecoder(self.row_bytes, self.data_off, self.scl_off, self.offs_off,
                              self.wts_off, self.nbits, self.nsblk, self.nchans, self.npol,
                              self.pol0, self.npol_sum, self.nsubints, self.dtype)

    def rows_for(self, start, n):
        """(row0, nrows, s0): the rows that hold samples [start, start + n)
        and the offset of ``start`` in the first of them.  A row on a seam of
        two spans belongs to both."""
        return self.decoder().rows_for(start, n)

    def read_rows_into(self, row0, out):
        """Rows row0 ... as stored into ``out``, a C-contiguous uint8
        [k, NAXIS1] host array (numpy, or a pinned tensor's .numpy()), in one
        contiguous read; returns the number of whole rows read (fewer at the
        end of the table).  Refusals as filterbank.read_block_into."""
        if not isinstance(out, np.ndarray) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("read_rows_into: out must be a C-contiguous numpy array")
        if out.ndim != 2 or out.shape[1] != self.row_bytes or out.dtype != np.uint8:
            raise ValueError("read_rows_into: out must be [k, %d] of uint8, not %s of %s"
                             % (self.row_bytes, out.shape, out.dtype))
        k = max(0, min(out.shape[0], self.nsubints - int(row0)))
        if k == 0:
            return 0
        self._f.seek(self._data_offset + int(row0) * self.row_bytes)
        got = self._f.readinto(memoryview(out.reshape(-1))[:k * self.row_bytes])
        return got // self.row_bytes

    def read_device(self, start, n, out=None, piece_bytes=1 << 28):
        """Samples [start, start + n) decoded on the device into ``out``
        (device [>= n, nchans] of ``dtype``; made here when None): the rows go
        up and are decoded in pieces of at most ``piece_bytes``.  Returns
        out[:n read]."""
        import torch
        from .. import _lib
        _lib.require_gpu()
        dec = self.decoder()
        n = max(0, min(int(n), self.number_of_samples - int(start)))
        if out is None:
            out = torch.empty((n, self.nchans), dtype=dec.torch_dtype, device="cuda")
        per = max(1, piece_bytes // self.row_bytes) * self.nsblk  # samples a piece
        host = None
        done = 0
        while done < n:
            m = min(per, n - done)
            row0, nrows, s0 = dec.rows_for(start + done, m)
            if host is None:
                host = np.empty((dec.max_rows(min(per, n)), self.row_bytes), dtype=np.uint8)
            got = self.read_rows_into(row0, host[:nrows])
            if got != nrows:
                raise IOError("%s: short read, %d of %d rows" % (self.filename, got, nrows))
            dec.decode(torch.from_numpy(host[:nrows]).cuda(), nrows, s0, m, out[done:done + m])
            done += m
        return out[:n]

    def read_block_into(self, startsamp, out):
        """Samples [startsamp, startsamp + len(out)) into ``out``, a
        C-contiguous host array [n, nchans] of ``dtype``; returns the number
        of spectra read (fewer at the end of the file).  Goes through the
        device (rows up, pdd_psrfits_block, block back): for windows -- the
        mask's fill, cut-outs, subband folds -- not for the stream."""
        import torch
        if not isinstance(out, np.ndarray) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("read_block_into: out must be a C-contiguous numpy array")
        if out.ndim != 2 or out.shape[1] != self.nchans or out.dtype != self.dtype:
            raise ValueError("read_block_into: out must be [n, %d] of %s, not %s of %s"
                             % (self.nchans, self.dtype, out.shape, out.dtype))
        n = max(0, min(out.shape[0], self.number_of_samples - int(startsamp)))
        if n:
            torch.from_numpy(out[:n]).copy_(self.read_device(int(startsamp), n))
        return n


def open_search_file(fn, **kw):
    """The input of a search: a ``filterbank`` (SIGPROC) or a
    ``PsrfitsSearchFile``, decided by content (a FITS file starts with
    ``SIMPLE  =``), not by extension.  ``kw``: PsrfitsSearchFile's options
    (apply_scales, apply_offsets, apply_weights, poln), noted and ignored for
    a filterbank.  A FITS file that is not search-mode PSRFITS is refused."""
    if not os.path.isfile(fn):
        raise ValueError("ERROR: File does not exist!\n\t(%s)" % fn)
    with open(fn, "rb") as f:
        magic = f.read(9)
    if magic == b"SIMPLE  =":
        if not is_PSRFITS(fn):
            raise ValueError("%s is a FITS file but not a search-mode PSRFITS file "
                             "(FITSTYPE 'PSRFITS', OBS_MODE 'SEARCH')" % fn)
        return PsrfitsSearchFile(fn, **kw)
    from .filterbank import filterbank
    if any(kw.get(k) is False for k in ("apply_scales", "apply_offsets", "apply_weights")) \
            or kw.get("poln") is not None:
        print("%s is a SIGPROC filterbank: the PSRFITS scale, offset, weight and polarisation "
              "options are ignored" % fn)
    return filterbank(fn)


def write_search_psrfits(fn, data, freqs, tbin, nbits, scales=None, offsets=None, weights=None,
                         primary=None, nsuboffs=0, npol=1, pol_type="AA+BB"):
    """Write a search-mode PSRFITS file (test fixtures and mock data).
    ``data``: [nsub, nsblk, nchan] samples in FILE channel order
    (uint8 0..15 for nbits 4 -- packed low nibble first, uint8 for 8, int16
    for 16, float32 for 32); ``freqs``: the DAT_FREQ column (either order);
    scales/offsets/weights: [nsub, nchan] (defaults 1, 0, 1).  With
    ``npol`` > 1 (``pol_type`` e.g. "AABB", "IQUV") ``data`` is
    [nsub, nsblk, npol, nchan] and scales and offsets are [nsub, npol*nchan]."""
    data = np.asarray(data)
    if npol == 1:
        nsub, nsblk, nchan = data.shape
    else:
        nsub, nsblk, dpol, nchan = data.shape
        if dpol != npol:
            raise ValueError("data holds %d polarisations, npol is %d" % (dpol, npol))
    nper = nsblk * npol * nchan
    if nbits == 4:
        flat = data.reshape(nsub, -1).astype(np.uint8)
        body = (flat[:, 0::2] & 15) | ((flat[:, 1::2] & 15) << 4)
        tform = "%dB" % body.shape[1]
    elif nbits == 8:
        body, tform = data.reshape(nsub, -1).astype(np.uint8), "%dB" % nper
    elif nbits == 16:
        body, tform = data.reshape(nsub, -1).astype(">i2"), "%dI" % nper
    elif nbits == 32:
        body, tform = data.reshape(nsub, -1).astype(">f4"), "%dE" % nper
    else:
        raise ValueError("nbits must be 4, 8, 16 or 32")
    ones = np.ones((nsub, nchan), dtype=np.float32)
    pones = np.ones((nsub, npol * nchan), dtype=np.float32)
    scales = pones if scales is None else np.asarray(scales, dtype=np.float32)
    offsets = 0 * pones if offsets is None else np.asarray(offsets, dtype=np.float32)
    weights = ones if weights is None else np.asarray(weights, dtype=np.float32)
    freqs = np.asarray(freqs, dtype=np.float64)
    cols = [("TSUBINT", "1D"), ("OFFS_SUB", "1D"), ("TEL_AZ", "1E"), ("TEL_ZEN", "1E"),
            ("DAT_FREQ", "%dD" % nchan), ("DAT_WTS", "%dE" % nchan),
            ("DAT_OFFS", "%dE" % (npol * nchan)), ("DAT_SCL", "%dE" % (npol * nchan)),
            ("DATA", tform)]
    rows = {
        "TSUBINT": np.full(nsub, nsblk * tbin), "OFFS_SUB": (np.arange(nsub) + 0.5) * nsblk * tbin,
        "TEL_AZ": np.full(nsub, 123.5, dtype=np.float32),
        "TEL_ZEN": np.full(nsub, 21.25, dtype=np.float32),
        "DAT_FREQ": np.tile(freqs, (nsub, 1)), "DAT_WTS": weights, "DAT_OFFS": offsets,
        "DAT_SCL": scales, "DATA": body,
    }
    p = [("FITSTYPE", "PSRFITS"), ("OBS_MODE", "SEARCH"), ("TELESCOP", "GBT"),
         ("OBSERVER", "pdd"), ("SRC_NAME", "J0000+0000"), ("FRONTEND", "Rcvr1_2"),
         ("BACKEND", "GUPPI"), ("PROJID", "TEST"), ("DATE-OBS", "2020-01-02T03:04:05.500"),
         ("FD_POLN", "LIN"), ("RA", "12:34:56.7"), ("DEC", "-01:23:45.6"),
         ("OBSFREQ", float(np.mean(freqs))), ("OBSNCHAN", nchan),
         ("OBSBW", float(abs(freqs[-1] - freqs[0]) * nchan / max(nchan - 1, 1))),
         ("BMIN", 0.15), ("CHAN_DM", 0.0), ("STT_IMJD", 58850), ("STT_SMJD", 11045),
         ("STT_OFFS", 0.5), ("TRK_MODE", "TRACK")]
    if primary:
        d = dict(p)
        d.update(primary)
        p = list(d.items())
    sub = [("TBIN", float(tbin)), ("NCHAN", nchan), ("NPOL", npol), ("POL_TYPE", pol_type),
           ("NCHNOFFS", 0), ("NSBLK", nsblk), ("NBITS", nbits), ("NSUBOFFS", nsuboffs)]
    pyfits.write(fn, p, [("SUBINT", sub, cols, rows)])
