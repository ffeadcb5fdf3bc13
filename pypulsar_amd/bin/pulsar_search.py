#!/usr/bin/env python
"""pulsar_search.py -- periodicity search of a SIGPROC filterbank or PSRFITS
search-mode file.

New (the reference has no search; it reads PRESTO's ``.fft`` and
``.accelcands`` files, formats/prestofft.py and formats/accelcands.py): the
file -- one that fits on the GPU in one piece -- is optionally zero-DM
filtered (bin/zero_dm_filter.py:30-39, float mode) and downsampled
(spectra.py:329-351), swept over a uniform DM grid (per-DM
Spectra.dedisperse + channel sum, spectra.py:229-260), and every DM row's
power spectrum is whitened (PrestoFFT.deredden, prestofft.py:151-195),
harmonic summed (PrestoFFT.harmonic_sum, :98-113) and searched
(pypulsar_amd.periodicity) in batches of DM rows; only candidates come back to
the host.  They are sifted across DMs and harmonics and written in the
``.accelcands`` layout.  With ``--fold K`` the K strongest sifted candidates
are then folded on the plane (pypulsar_amd.fold: their own DM row and its
neighbours, a search over period and period derivative) and written as
``<base>_cand<k>.bestprof`` and ``<base>_cand<k>.npz``; with
``--fold-subbands NSUB`` each is also folded from the input file itself, at
its own time resolution, into NSUB subbands and its DM refined on a ladder
finer than the grid (pypulsar_amd.subfold): ``<base>_cand<k>_subbands.npz``
holds the phase-versus-frequency image.  With ``--zmax Z`` the
rows are searched for signals that drift up to Z Fourier bins over the
observation (pulsars in binaries; pypulsar_amd.accel): the candidates carry
their ``z``, and a fold starts from their frequency derivative.  With
``--wmax W`` the templates also carry a jerk of up to W bins (``w = fdd T^3``:
tight binaries in long observations; pypulsar_amd.jerk): the ``.accelcands``
names end in ``_JERK_<W>``, ``<base>_jerkcands.npz`` holds every sifted
candidate's ``w`` and second derivative (the ``.accelcands`` layout has no
column for them), and a fold starts from the frequency and its derivative at
the first sample.  With
``--ffa`` the plane is also searched by fast folding (pypulsar_amd.ffa: slow,
narrow pulses that the harmonic sums lose); its sifted candidates go to
``<base>.ffacands`` in the same layout, and ``--fold K`` folds its K strongest
as ``<base>_ffacand<k>``.  A PSRFITS file (recognised by content) goes up as
its own SUBINT rows and is decoded on the device in bounded pieces
(pdd_psrfits_block);
``--noscales``, ``--nooffsets``, ``--noweights`` and ``--poln K`` choose what
the decode applies (ignored, with a note, for a filterbank).  With
``--zaplist FILE`` and / or ``--autozap`` the
Fourier bins of periodic interference -- listed in a PRESTO ``.zaplist``, or
found on the plane as the bins that stand out in (nearly) every DM row
(pypulsar_amd.zap) -- are set to the whitened mean level before the
periodicity or acceleration search.  With ``--sideband`` the same whitened,
zapped powers are also searched for the sideband combs of pulsars in binaries
shorter than the observation (pypulsar_amd.sideband: short FFTs of the power
spectrum); its sifted candidates -- orbital period and the frequency range that
holds the spin frequency -- go to ``<base>.bincands`` and
``<base>_bincands.npz``.  With ``--orbit-follow K`` the K strongest of them are
followed up coherently (pypulsar_amd.orbit): the plane row of the candidate's DM
is demodulated on the device by a bank of circular orbits that covers its
orbital period, frequency range and every orbital phase, each demodulated row is
searched like a DM row, and the sifted candidates -- a spin frequency with the
orbit that collects its power -- go to ``<base>.orbcands`` and
``<base>_orbcands.npz``; with ``--fold N`` the best of each followed candidate
is folded from its demodulated row as ``<base>_orbcand<k>``.

    python -m pypulsar_amd.bin.pulsar_search --lodm 0 --hidm 100 --numdms 256 \\
        --downsamp 2 --sigma 8 -o obs.accelcands obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --fold 3 guppi_obs_0001.fits
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --fold 3 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --fold 3 --fold-subbands 32 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --zmax 50 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --zmax 50 --wmax 100 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --sideband obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --zmax 50 --sideband --sb-maxfft 4096 \\
        --sb-numharm 2 --sb-sigma 7 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --numharm 2 --sideband --orbit-follow 3 \\
        --fold 1 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --rfifind 2.0 obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --autozap obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --zaplist site.zaplist obs.fil
    python -m pypulsar_amd.bin.pulsar_search --numdms 256 --ffa --ffa-pmin 0.5 --ffa-pmax 10 \\
        --fold 3 obs.fil
"""
import optparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def search_file(infile, dms, downsamp=1, zero_dm=False, sigma=6.0, harms=None, flo=1.0,
                nfft=None, row_batch=None, return_plane=False, zmax=0, dz=2, maskfile=None,
                rfifind=None, zaplist=None, autozap=None, file_kw=None, wmax=0, dw=20,
                jerk_workspace_bytes=None, injector=None, sideband=None):
    """(candidate records, sample time of the searched plane); with
    ``return_plane`` also the searched [D, n] float32 device plane (for
    pypulsar_amd.fold): (candidates, sample time, plane).  ``zmax`` > 0: the
    acceleration search (pypulsar_amd.accel.AccelSearch, records of
    ACCEL_CAND_DTYPE) on a z grid of ``dz``; ``harms`` then at most 16.
    ``wmax`` > 0: the jerk search (pypulsar_amd.jerk.JerkSearch, records of
    JERK_CAND_DTYPE) on that z grid (``zmax`` may be 0) and a w grid of ``dw``,
    its row batches bounded by ``jerk_workspace_bytes`` (None: its default).
    ``maskfile`` / ``rfifind``: the cells of that rfifind ``.mask``, or of the
    one made here from the data with intervals of ``rfifind`` seconds (left as
    <base>_rfifind.mask), are replaced by their channel's level first.
    ``zaplist`` (a ``.zaplist`` file name or a ``pypulsar_amd.zap.Zaplist``) /
    ``autozap`` (a ``pypulsar_amd.zap.BirdieFinder``, or True for the default
    one, run on the swept plane; its list is left as <base>.zaplist): the
    Fourier bins of those intervals are set to the whitened mean level in
    every DM row before the search; both: the two lists merged.
    ``file_kw``: open_search_file's keywords (PSRFITS input).
    ``injector``: a ``pypulsar_amd.inject.Injector`` whose signals are added
    to the raw block (at sample 0, before the mask; a packed file's values
    clipped to its bit depth).  ``sideband``: a
    ``pypulsar_amd.sideband.SidebandSearch``, or a dict of its options
    (``sigma_threshold`` defaults to ``sigma``, ``flo`` to ``flo``): every
    batch of whitened, zapped powers of the search above is also searched for
    the sideband combs of binaries shorter than the observation -- no second
    prep, FFT or whitening -- and its records (``sideband.CAND_DTYPE``) are
    appended to the result: (candidates, sample time[, plane], sideband
    candidates)."""
    import torch
    from pypulsar_amd.formats.psrfits import open_search_file
    from pypulsar_amd.periodicity import DEFAULT_HARMS, PeriodicitySearch
    from pypulsar_amd.stream import prologue
    from pypulsar_amd.sweep import DMSweep

    fb = open_search_file(infile, **(file_kw or {}))
    if np.dtype(fb.dtype) == np.uint16:
        raise ValueError("16-bit filterbanks: convert to 8 or 32 bits first")
    assert 64 % downsamp == 0, "the downsampling factor must divide 64"
    C, dt = fb.nchans, fb.tsamp * downsamp
    n = fb.number_of_samples // downsamp * downsamp
    if hasattr(fb, "read_device"):
        # a PSRFITS file: its rows go to the device and are decoded there
        raw = fb.read_device(0, n)
    elif fb.packed:
        # a 1-, 2- or 4-bit file: its bytes go to the device and are unpacked there
        from pypulsar_amd.stream import unpack_bits
        host = np.empty((n, fb.bytes_per_spectrum), dtype=np.uint8)
        got = fb.read_packed_into(0, host)
        assert got == n, "short read: %d of %d spectra" % (got, n)
        raw = unpack_bits(torch.from_numpy(host).cuda(), fb.nbits, C)
    else:
        raw = torch.from_numpy(fb.read_all_samples()[:n * C].reshape(n, C)).cuda()
    if injector is not None:
        injector.apply(raw, 0, vmax=(1 << fb.nbits) - 1 if fb.packed else None)
    if rfifind or maskfile:
        from pypulsar_amd import rfi
        if rfifind:
            from pypulsar_amd.bin.rfifind import ptsperint_for
            finder = rfi.RFIFind(ptsperint_for(rfifind, fb.tsamp))
            mask = finder.mask_from_stats(*finder.stats(raw), **rfi.file_header(fb))
            out = os.path.splitext(infile)[0] + "_rfifind.mask"
            mask.write(out)
            print("rfifind: %.2f%% masked -> %s" % (100.0 * mask.masked_fraction, out))
        else:
            mask = rfi.mask_from_file(maskfile, fb)
        mask.apply(raw, 0)
    fb.close()
    # zero-DM + downsample + corner turn in one pass: [C, n / downsamp] float32
    img = torch.empty((C, n // downsamp), dtype=torch.float32, device=raw.device)
    prologue(raw, n, C, downsamp, "float" if zero_dm else "none", img)
    del raw
    sw = DMSweep(dms, fb.freqs, dt, dtype="f32")
    plane = sw(img, trim=True)
    del img
    if wmax > 0:
        from pypulsar_amd.jerk import DEFAULT_HARMS as JERK_HARMS, JerkSearch
        jkw = {} if jerk_workspace_bytes is None else {"workspace_bytes": jerk_workspace_bytes}
        ps = JerkSearch(sigma, zmax, wmax, dz, dw, harms or JERK_HARMS, flo=flo, **jkw)
    elif zmax > 0:
        from pypulsar_amd.accel import DEFAULT_HARMS as ACCEL_HARMS, AccelSearch
        ps = AccelSearch(sigma, zmax, dz, harms or ACCEL_HARMS, flo=flo)
    else:
        ps = PeriodicitySearch(sigma, harms or DEFAULT_HARMS, flo=flo)
    kw = {}
    if zaplist is not None or autozap is not None:
        from pypulsar_amd import zap as _zap
        zl = _zap.Zaplist()
        if zaplist is not None:
            zl = zaplist if isinstance(zaplist, _zap.Zaplist) else _zap.read_zaplist(zaplist)
        if autozap is not None:
            finder = autozap if isinstance(autozap, _zap.BirdieFinder) else _zap.BirdieFinder()
            nf = PeriodicitySearch.default_nfft(plane.shape[1]) if nfft is None else int(nfft)
            found = finder.find(ps.ps if zmax > 0 or wmax > 0 else ps, plane, dt, nfft=nf)
            out = os.path.splitext(infile)[0] + ".zaplist"
            _zap.write_zaplist(out, found)
            b = found.bins(nf, dt)
            print("autozap: %d intervals, %d of %d bins zapped -> %s" % (
                len(b), int(np.sum(b[:, 1] - b[:, 0] + 1)), nf // 2, out))
            zl = zl.merged(found)
        kw["zap"] = zl
    sb_parts = []
    if sideband is not None:
        from pypulsar_amd import sideband as _sb
        if not isinstance(sideband, _sb.SidebandSearch):
            opts = dict(sideband)
            opts.setdefault("sigma_threshold", sigma)
            opts.setdefault("flo", flo)
            sideband = _sb.SidebandSearch(**opts)
        kw["tap"] = sideband.tap(dms, dt, sb_parts)
    cands = ps(plane, dms, dt, row_batch=row_batch, nfft=nfft, **kw)
    sw.close()
    res = (cands, dt, plane) if return_plane else (cands, dt)
    if sideband is not None:
        res += (_sb.merge(sb_parts),)
    return res


def main(argv=None):
    parser = optparse.OptionParser(prog="pulsar_search.py", usage="%prog [OPTIONS] INFILE",
                                   description="Dedispersion + periodicity search of a SIGPROC "
                                               "filterbank or PSRFITS search-mode file on the "
                                               "GPU.")
    parser.add_option("--lodm", type="float", default=0.0, help="Lowest DM (pc/cc).")
    parser.add_option("--hidm", type="float", default=100.0, help="Highest DM (pc/cc).")
    parser.add_option("--numdms", type="int", default=128, help="Number of DM trials.")
    parser.add_option("--downsamp", type="int", default=1,
                      help="Downsampling factor (divides 64). (Default: 1)")
    parser.add_option("--zero-dm", dest="zero_dm", action="store_true", default=False,
                      help="Apply the zero-DM filter first.")
    parser.add_option("--mask", dest="maskfile", type="string", default=None,
                      help="rfifind .mask file: its cells are replaced by the channel's "
                           "level before anything else. (Default: no mask)")
    parser.add_option("--rfifind", type="float", default=None, metavar="SECONDS",
                      help="Make the mask from the data first, with intervals of SECONDS "
                           "(written to <INFILE base>_rfifind.mask), then search with it.")
    parser.add_option("--zaplist", type="string", default=None, metavar="FILE",
                      help="PRESTO .zaplist of periodic interference: its Fourier bins are set "
                           "to the whitened mean level in every DM row before the periodicity "
                           "or acceleration search.  (The fast-folding search works in the "
                           "time domain and is not affected.)")
    parser.add_option("--autozap", action="store_true", default=False,
                      help="Find the periodic interference on the swept plane first (bins "
                           "whose percentile across DM rows stands out), write it to <INFILE "
                           "base>.zaplist and search with it; with --zaplist the two lists "
                           "are merged.  (Not applied to the fast-folding search.)")
    parser.add_option("--autozap-rows", dest="autozap_rows", type="int", default=33,
                      help="DM rows, evenly spaced, that --autozap uses (at most 64). "
                           "(Default: 33)")
    parser.add_option("--autozap-percent", dest="autozap_percent", type="float", default=50.0,
                      help="Percentile across those rows. (Default: 50, the median)")
    parser.add_option("--autozap-nsig", dest="autozap_nsig", type="float", default=5.0,
                      help="Per-bin false-alarm level of --autozap in sigma. (Default: 5)")
    parser.add_option("-s", "--sigma", type="float", default=6.0,
                      help="Single-trial candidate threshold in sigma. (Default: 6)")
    parser.add_option("--numharm", type="int", default=16,
                      help="Largest number of summed harmonics (1, 2, 4, 8, 16 or 32).")
    parser.add_option("--flo", type="float", default=1.0,
                      help="Lowest searched frequency in Hz. (Default: 1)")
    parser.add_option("--nfft", type="int", default=None,
                      help="FFT length (even; default: next power of two).")
    parser.add_option("--row-batch", type="int", default=None,
                      help="DM rows searched at once (default: bounded by the workspace).")
    parser.add_option("--zmax", type="int", default=0,
                      help="Largest searched drift in Fourier bins over the observation "
                           "(z = fd T^2): the acceleration search; caps --numharm at 16. "
                           "(Default: 0, the periodicity search)")
    parser.add_option("--dz", type="int", default=2,
                      help="Step of the z grid of the acceleration search. (Default: 2)")
    parser.add_option("--wmax", type="int", default=0,
                      help="Largest searched jerk in Fourier bins over the observation "
                           "(w = fdd T^3): the jerk search, on the z grid of --zmax (which may "
                           "be 0); caps --numharm at 16; also writes <base>_jerkcands.npz. "
                           "(Default: 0, no jerk)")
    parser.add_option("--dw", type="int", default=20,
                      help="Step of the w grid of the jerk search. (Default: 20)")
    parser.add_option("--jerk-workspace-gib", dest="jerk_workspace_gib", type="float",
                      default=None, metavar="G",
                      help="Device memory in GiB that bounds a row batch of the jerk search, "
                           "whose whole volume of a row must be resident. (Default: 32)")
    parser.add_option("--sideband", action="store_true", default=False,
                      help="Also search the whitened powers of every DM row for the sideband "
                           "combs of pulsars in binaries shorter than the observation (short "
                           "FFTs of the power spectrum); writes <base>.bincands and "
                           "<base>_bincands.npz.")
    parser.add_option("--sb-minfft", dest="sb_minfft", type="int", default=32,
                      help="Shortest mini FFT of --sideband (a power of two >= 32). (Default: 32)")
    parser.add_option("--sb-maxfft", dest="sb_maxfft", type="int", default=16384,
                      help="Longest mini FFT of --sideband (a power of two <= 16384). "
                           "(Default: 16384)")
    parser.add_option("--sb-numharm", dest="sb_numharm", type="choice",
                      choices=["1", "2", "4", "8"], default="4",
                      help="Largest number of summed harmonics of the comb's spacing (1, 2, 4 "
                           "or 8). (Default: 4)")
    parser.add_option("--sb-shift", dest="sb_shift", type="int", default=2,
                      help="Segments of length L start L >> SHIFT bins apart (0..3). (Default: 2)")
    parser.add_option("--sb-clip", dest="sb_clip", type="float", default=None,
                      help="Whitened powers are clipped here before the mini FFTs (0: no clip). "
                           "(Default: the single-bin threshold of --sb-sigma)")
    parser.add_option("--sb-sigma", dest="sb_sigma", type="float", default=None,
                      help="Single-trial threshold of --sideband in sigma. (Default: --sigma)")
    parser.add_option("--orbit-follow", dest="orbit_follow", type="int", default=0, metavar="K",
                      help="Follow the K strongest sifted candidates of --sideband up with a "
                           "coherent search over a bank of circular orbits: writes "
                           "<base>.orbcands and <base>_orbcands.npz (and, with --fold, "
                           "<base>_orbcand<k>.bestprof and .npz of the demodulated row). "
                           "(Default: 0, off)")
    parser.add_option("--orbit-mismatch", dest="orbit_mismatch", type="float", default=0.05,
                      help="Largest Roemer-delay error between neighbouring templates as a "
                           "fraction of the shortest searched period. (Default: 0.05)")
    parser.add_option("--orbit-xmax", dest="orbit_xmax", type="float", default=None,
                      help="Largest projected semi-major axis of the bank in light-seconds. "
                           "(Default: what lets the comb fit the candidate's frequency range)")
    parser.add_option("--orbit-max-templates", dest="orbit_max_templates", type="int",
                      default=1 << 20,
                      help="A candidate whose bank would be larger is reported and skipped. "
                           "(Default: 1048576)")
    parser.add_option("--orbit-mode", dest="orbit_mode", type="choice",
                      choices=["nearest", "linear"], default="nearest",
                      help="How the demodulated rows are sampled: the nearest sample (drop / "
                           "duplicate) or a linear interpolation. (Default: nearest)")
    parser.add_option("--orbit-sigma", dest="orbit_sigma", type="float", default=None,
                      help="Single-trial threshold of --orbit-follow in sigma. (Default: --sigma)")
    parser.add_option("--fold", type="int", default=0,
                      help="Fold the K strongest sifted candidates on the plane and refine "
                           "period, period derivative and DM; writes <base>_cand<k>.bestprof "
                           "and <base>_cand<k>.npz. (Default: 0, no folding)")
    parser.add_option("--fold-nbins", dest="fold_nbins", type="int", default=64,
                      help="Profile bins of a fold. (Default: 64)")
    parser.add_option("--fold-npart", dest="fold_npart", type="int", default=32,
                      help="Sub-integrations of a fold. (Default: 32)")
    parser.add_option("--fold-dm-halfwidth", dest="fold_dm_halfwidth", type="int", default=2,
                      help="DM trials folded on each side of a candidate's. (Default: 2)")
    parser.add_option("--fold-subbands", dest="fold_subbands", type="int", default=0,
                      metavar="NSUB",
                      help="Also fold the K candidates of --fold from the input file into NSUB "
                           "subbands at the file's own resolution and refine their DM on a "
                           "ladder finer than the grid (the --mask / --rfifind mask applied, the "
                           "zero-DM filter not); writes <base>_cand<k>_subbands.npz. "
                           "(Default: 0, off)")
    parser.add_option("--fold-ndm", dest="fold_ndm", type="int", default=None,
                      help="Entries of the DM ladder of --fold-subbands. "
                           "(Default: --fold-nbins + 1)")
    parser.add_option("--ffa", action="store_true", default=False,
                      help="Also run the fast-folding search for slow pulsars on the plane; "
                           "writes <base>.ffacands (and, with --fold K, "
                           "<base>_ffacand<k>.bestprof and .npz).")
    parser.add_option("--ffa-pmin", dest="ffa_pmin", type="float", default=0.5,
                      help="Shortest fast-folded period in s. (Default: 0.5)")
    parser.add_option("--ffa-pmax", dest="ffa_pmax", type="float", default=10.0,
                      help="Longest fast-folded period in s. (Default: 10)")
    parser.add_option("--ffa-bins-min", dest="ffa_bins_min", type="int", default=250,
                      help="Fewest profile bins of a fast fold. (Default: 250)")
    parser.add_option("--ffa-bins-max", dest="ffa_bins_max", type="int", default=500,
                      help="Most profile bins of a fast fold. (Default: 500)")
    parser.add_option("--ffa-snr", dest="ffa_snr", type="float", default=8.0,
                      help="S/N threshold of a fast-folding candidate. (Default: 8)")
    parser.add_option("--ffa-ducy", dest="ffa_ducy", type="float", default=0.2,
                      help="Largest searched duty cycle. (Default: 0.2)")
    parser.add_option("--ffa-detrend", dest="ffa_detrend", type="float", default=None,
                      help="Length in s of the chunks whose means make the removed baseline. "
                           "(Default: 4 x --ffa-pmax)")
    parser.add_option("--noscales", dest="apply_scales", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_SCL.")
    parser.add_option("--nooffsets", dest="apply_offsets", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_OFFS.")
    parser.add_option("--noweights", dest="apply_weights", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_WTS.")
    parser.add_option("--poln", type="int", default=None, metavar="K",
                      help="PSRFITS input: use polarisation K alone. (Default: the one "
                           "polarisation, AA + BB of AABB data, I of IQUV)")
    parser.add_option("-o", "--outname", default=None,
                      help="Output .accelcands file (default: INFILE with .accelcands).")
    from pypulsar_amd.bin.frb_search import (INJECT_HINT, add_inject_options, file_options,
                                             load_injector)
    add_inject_options(parser)
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("one input file expected")
    options.file_kw = file_options(options)
    if options.inject and options.fold_subbands:
        parser.error("--inject cannot be combined with --fold-subbands: the subband fold reads "
                     "the file again and would not see the signal; " + INJECT_HINT)
    if options.recovery and not options.inject:
        parser.error("--recovery needs --inject SPEC.json")
    injector = load_injector(options.inject, args[0], options.file_kw, parser.error)
    from pypulsar_amd.periodicity import sift, write_accelcands
    if options.zmax < 0 or options.dz < 1:
        parser.error("--zmax must be >= 0 and --dz >= 1")
    if options.wmax < 0 or options.dw < 1:
        parser.error("--wmax must be >= 0 and --dw >= 1")
    accelerated = options.zmax > 0 or options.wmax > 0
    sideband = None
    if options.sideband:
        def pow2(v):
            return v >= 1 and v & (v - 1) == 0
        if not (pow2(options.sb_minfft) and pow2(options.sb_maxfft) and
                32 <= options.sb_minfft <= options.sb_maxfft <= 16384):
            parser.error("--sb-minfft and --sb-maxfft must be powers of two with 32 <= "
                         "--sb-minfft <= --sb-maxfft <= 16384")
        if not 0 <= options.sb_shift <= 3:
            parser.error("--sb-shift must be in 0..3")
        if options.sb_clip is not None and options.sb_clip < 0:
            parser.error("--sb-clip must be >= 0")
        sideband = dict(sigma_threshold=options.sigma if options.sb_sigma is None
                        else options.sb_sigma,
                        minfft=options.sb_minfft, maxfft=options.sb_maxfft,
                        shift=options.sb_shift,
                        harms=tuple(h for h in (1, 2, 4, 8) if h <= int(options.sb_numharm)),
                        clip="auto" if options.sb_clip is None else options.sb_clip)
    if options.orbit_follow < 0 or (options.orbit_follow and not options.sideband):
        parser.error("--orbit-follow K needs K >= 0 and --sideband")
    if options.orbit_mismatch <= 0 or options.orbit_max_templates < 1 or \
            (options.orbit_xmax is not None and options.orbit_xmax <= 0):
        parser.error("--orbit-mismatch, --orbit-xmax and --orbit-max-templates must be > 0")
    if options.fold_subbands < 0 or (options.fold_subbands and options.fold <= 0):
        parser.error("--fold-subbands NSUB needs NSUB >= 0 and --fold K")
    numharm = min(options.numharm, 16) if accelerated else options.numharm
    harms = tuple(h for h in (1, 2, 4, 8, 16, 32) if h <= numharm) or (1,)
    dms = np.linspace(options.lodm, options.hidm, options.numdms)
    finder = None
    if options.autozap:
        from pypulsar_amd.zap import MAX_ROWS, BirdieFinder
        if not 1 <= options.autozap_rows <= MAX_ROWS:
            parser.error("--autozap-rows must be in 1..%d" % MAX_ROWS)
        finder = BirdieFinder(options.autozap_rows, options.autozap_percent,
                              options.autozap_nsig)
    res = search_file(args[0], dms, options.downsamp, options.zero_dm, options.sigma, harms,
                      options.flo, options.nfft, options.row_batch,
                      return_plane=options.fold > 0 or options.ffa or options.orbit_follow > 0,
                      zmax=options.zmax,
                      dz=options.dz,
                      maskfile=options.maskfile, rfifind=options.rfifind,
                      zaplist=options.zaplist, autozap=finder, file_kw=options.file_kw,
                      wmax=options.wmax, dw=options.dw,
                      jerk_workspace_bytes=None if options.jerk_workspace_gib is None
                      else int(options.jerk_workspace_gib * (1 << 30)), injector=injector,
                      sideband=sideband)
    cands = res[0]
    sifted = sift(cands)
    base = os.path.splitext(args[0])[0]
    out = options.outname or base + ".accelcands"
    write_accelcands(sifted, out, basename=os.path.basename(base), zmax=options.zmax,
                     wmax=options.wmax)
    print("%d candidates (%d sifted) -> %s" % (len(cands), len(sifted), out))
    if sideband is not None:
        from pypulsar_amd import sideband as _sb
        bcands = res[-1]
        bsifted = _sb.sift(bcands)
        bout = os.path.splitext(out)[0] + ".bincands"
        _sb.write_bincands(bsifted, bout)
        _sb.write_bincands_npz(bsifted, os.path.splitext(out)[0] + "_bincands.npz")
        print("%d sideband candidates (%d sifted) -> %s" % (len(bcands), len(bsifted), bout))
        if options.orbit_follow > 0:
            osifted = follow_orbits(res[2], dms, res[1], bsifted[:options.orbit_follow],
                                    os.path.splitext(out)[0], args[0], options, max(harms))
    if options.recovery:
        from pypulsar_amd import recovery
        truth = injector.truth()
        n_plane = injector.n_samples // options.downsamp
        T = n_plane * res[1]
        rep = recovery.match_pulsars(truth, cands, T, dms, injector.freqs, injector.dt)
        more = {}
        if sideband is not None:
            more["binaries"] = recovery.match_binaries(truth, bsifted, T, dms, injector.freqs,
                                                       injector.dt)
            if options.orbit_follow > 0:
                more["orbits"] = recovery.match_orbits(truth, osifted, T, dms, injector.freqs,
                                                       injector.dt)
        rout = os.path.splitext(out)[0] + "_recovery.json"
        recovery.write_report(rout, truth, rep, **more)
        print("%d of %d injected pulsars recovered -> %s"
              % (sum(r["found"] for r in rep), len(rep), rout))
        for key, what in (("binaries", "found by the sideband search"),
                          ("orbits", "found by the orbit search")):
            if key in more:
                print("%d of %d injected binaries %s -> %s"
                      % (sum(r["found"] for r in more[key]), len(more[key]), what, rout))
    to_fold = sifted[:options.fold]
    if options.wmax > 0:
        jout = os.path.splitext(out)[0] + "_jerkcands.npz"
        write_jerkcands(sifted, jout)
        print("w and the second derivative of the %d sifted candidates -> %s" % (len(sifted), jout))
        if options.fold > 0:
            to_fold = first_sample_starts(to_fold, res[2].shape[1] * res[1])
    if options.fold > 0:
        folded = fold_candidates(res[2], dms, res[1], to_fold,
                                 os.path.splitext(out)[0], args[0], options.fold_npart,
                                 options.fold_nbins, options.fold_dm_halfwidth)
        if options.fold_subbands:
            fold_subbands(folded, os.path.splitext(out)[0], args[0], options)
    if options.ffa:
        from pypulsar_amd.ffa import FFASearch
        fs = FFASearch(options.ffa_pmin, options.ffa_pmax, options.ffa_bins_min,
                       options.ffa_bins_max, options.ffa_snr, ducy_max=options.ffa_ducy,
                       detrend=options.ffa_detrend)
        fcands = fs(res[2], dms, res[1], row_batch=options.row_batch)
        fsifted = sift(fcands)
        fout = os.path.splitext(out)[0] + ".ffacands"
        write_accelcands(fsifted, fout, basename=os.path.basename(base))
        print("%d FFA candidates (%d sifted) -> %s" % (len(fcands), len(fsifted), fout))
        if options.fold > 0:
            folded = fold_candidates(res[2], dms, res[1], fsifted[:options.fold],
                                     os.path.splitext(out)[0], args[0], options.fold_npart,
                                     options.fold_nbins, options.fold_dm_halfwidth, tag="ffacand")
            if options.fold_subbands:
                fold_subbands(folded, os.path.splitext(out)[0], args[0], options, tag="ffacand")
    return 0


def follow_orbits(plane, dms, dt, bsifted, base, infile, options, numharm):
    """The coherent follow-up of sifted sideband candidates (``--orbit-follow``).
    Per candidate, on the plane row of its DM: a bank of circular orbits
    (pypulsar_amd.orbit.circular_bank) over ``porb +- porb / q`` (the half-bin
    step of its mini spectrum), ``x <= (freq_hi - freq_lo) porb / (4 pi
    freq_lo)`` (the comb's ``2 beta / porb`` Hz must fit the segment; or
    ``--orbit-xmax``) and every phase; the band ``[freq_lo, freq_hi]`` of every
    demodulated row is searched with the stages of ``--numharm`` that reach it
    below the Nyquist frequency, and the bank's steps are set for ``f_top =
    numharm freq_hi`` of the largest of them (at most the Nyquist frequency:
    there is no harmonic above it).  Every demodulated row is transformed zero
    padded to twice the FFT length of the search: once a template has put the
    power into one bin, a spin frequency half way between two bins would lose
    0.6 of it, while a template that leaves a residual modulation can put a
    third of it into a sideband ``1 / porb`` away that falls on a bin -- at half
    bins the carrier keeps at least 0.81 and wins.  A bank above
    ``--orbit-max-templates`` is reported and skipped.  Writes ``<base>.orbcands`` and
    ``<base>_orbcands.npz`` (the sifted candidates of all followed ones) and,
    with ``--fold``, folds the best of each from its demodulated row
    (``<base>_orbcand<k>.bestprof`` / ``.npz``, k the rank of the sideband
    candidate).  Returns the sifted records."""
    from pypulsar_amd import orbit as _orb
    n = plane.shape[1]
    T, nyquist = n * dt, 0.5 / dt
    sigma = options.sigma if options.orbit_sigma is None else options.orbit_sigma
    from pypulsar_amd.periodicity import PeriodicitySearch
    nfft = 2 * (PeriodicitySearch.default_nfft(n) if options.nfft is None else options.nfft)
    kept = []
    for k, c in enumerate(bsifted, 1):
        porb, f_lo, f_hi = float(c["porb"]), float(c["freq_lo"]), float(c["freq_hi"])
        stages = tuple(h for h in (1, 2, 4, 8, 16, 32) if h <= numharm and h * f_lo < nyquist) \
            or (1,)
        x_max = options.orbit_xmax if options.orbit_xmax is not None \
            else (f_hi - f_lo) * porb / (4.0 * np.pi * f_lo)
        try:
            bank = _orb.validate(_orb.circular_bank(porb - porb / float(c["q"]), porb + porb / float(c["q"]),
                                      x_max, min(max(stages) * f_hi, nyquist), T,
                                      options.orbit_mismatch, options.orbit_max_templates))
        except ValueError as e:
            print("orbit follow-up %d (DM %.2f, porb %.5f s) skipped: %s" % (k, c["DM"], porb, e))
            continue
        row = plane[int(c["row"])]
        search = _orb.OrbitSearch(sigma, stages, options.orbit_mode, flo=f_lo, fhi=f_hi)
        s = _orb.sift(search(row, float(c["DM"]), dt, bank, nfft=nfft,
                             plane_row=int(c["row"])), ntemplates=len(bank))
        kept.append(s)
        if not len(s):
            print("orbit follow-up %d (DM %.2f, porb %.5f s): %d templates, no candidate"
                  % (k, c["DM"], porb, len(bank)))
            continue
        b = s[0]
        print("orbit follow-up %d (DM %.2f, porb %.5f s): %d templates, best sigma %.2f  "
              "f %.6f Hz  pb %.5f s  x %.6f lt-s  t0 %.5f s  (%d sifted)"
              % (k, c["DM"], porb, len(bank), b["sigma"], b["freq"], b["pb"], b["x"], b["t0"],
                 len(s)))
        if options.fold > 0:
            demod = _orb.demodulated(row, [b[name] for name in ("pb", "x", "e", "omega", "t0")], dt)
            fold_candidates(demod[None, :], [float(c["DM"])], dt, [(0, float(b["freq"]))], base,
                            infile, options.fold_npart, options.fold_nbins, 0, tag="orbcand",
                            first=k)
    sifted = np.concatenate(kept) if kept else np.empty(0, dtype=_orb.SIFTED_DTYPE)
    _orb.write_orbcands(sifted, base + ".orbcands")
    _orb.write_orbcands_npz(sifted, base + "_orbcands.npz")
    print("%d orbit candidates -> %s" % (len(sifted), base + ".orbcands"))
    return sifted


def write_jerkcands(sifted, fn):
    """``<base>_jerkcands.npz``: per sifted candidate of the jerk search, by
    descending sigma (the order of the ``.accelcands`` file), ``DM``, ``r``,
    ``period`` (s, mid-observation), ``numharm``, ``sigma``, ``z`` and ``w``
    (bins of 1/T), ``fd`` (Hz / s, the mean) and ``fdd`` (Hz / s^2), ``accel``
    (m / s^2) and ``jerk`` (m / s^3)."""
    from pypulsar_amd.accel import C_LIGHT
    cl = sorted(sifted, key=lambda c: -c.sigma)
    col = lambda f, t="f8": np.asarray([f(c) for c in cl], dtype=t)  # noqa: E731
    np.savez(fn, DM=col(lambda c: c.dm), r=col(lambda c: c.r), period=col(lambda c: c.period),
             numharm=col(lambda c: c.numharm, "i4"), sigma=col(lambda c: c.sigma),
             z=col(lambda c: c.z), w=col(lambda c: c.w), fd=col(lambda c: c.fd),
             fdd=col(lambda c: c.fdd), accel=col(lambda c: c.fd * C_LIGHT * c.period),
             jerk=col(lambda c: c.fdd * C_LIGHT * c.period))


def first_sample_starts(sifted, T):
    """Copies of candidates of the jerk search for pypulsar_amd.fold, which
    has no second derivative: their ``fd`` becomes the derivative at the first
    sample, ``fd - fdd T / 2``, and their frequency is set so that the fold
    starts at the first sample's, ``f - fd T / 2 + fdd T^2 / 12`` (``f``,
    ``fd``: the means over the ``T`` seconds)."""
    import copy
    out = []
    for c in sifted:
        f0 = c.freq - 0.5 * c.fd * T + c.fdd * T * T / 12.0
        fd0 = c.fd - 0.5 * c.fdd * T
        s = copy.copy(c)
        s.fd = fd0
        # (Folder starts a candidate with fd != 0 at freq - fd T / 2)
        s.period = 1.0 / (f0 + 0.5 * fd0 * T if fd0 != 0.0 else f0)
        out.append(s)
    return out


def fold_subbands(folded, base, infile, options, tag="cand"):
    """Fold the FoldedCandidates of ``fold_candidates`` from the input file
    into ``options.fold_subbands`` subbands and refine their DM
    (pypulsar_amd.subfold); the mask the search used (--mask, or the
    <base>_rfifind.mask that --rfifind left) is applied.  Writes
    ``<base>_<tag><k>_subbands.npz`` and prints one line per candidate."""
    from pypulsar_amd.formats.psrfits import open_search_file
    from pypulsar_amd.subfold import subfold_from_file, write_subfold
    fb = open_search_file(infile, **(getattr(options, "file_kw", None) or {}))
    mask = None
    maskfile = os.path.splitext(infile)[0] + "_rfifind.mask" if options.rfifind else options.maskfile
    if maskfile:
        from pypulsar_amd import rfi
        mask = rfi.mask_from_file(maskfile, fb)
    folds = subfold_from_file(fb, folded, rfimask=mask, npart=options.fold_npart,
                              nsub=options.fold_subbands, nbins=options.fold_nbins,
                              ndm=options.fold_ndm)
    fb.close()
    for k, sf in enumerate(folds, 1):
        name = "%s_%s%d_subbands.npz" % (base, tag, k)
        write_subfold(name, sf)
        print("%s %d subbands: fold DM %.2f  refined DM %.2f +- %.2f  reduced chi2 %.2f  "
              "sigma %.1f -> %s" % (tag, k, sf.dm_fold, sf.dm, sf.ddm, sf.chi2, sf.sigma, name))
    return folds


def fold_candidates(plane, dms, dt, sifted, base, infile, npart=32, nbins=64, dm_halfwidth=2,
                    tag="cand", first=1):
    """Fold sifted candidates on the plane; writes ``<base>_<tag><k>.bestprof``
    and ``<base>_<tag><k>.npz`` (k from 1, by descending sigma; ``tag``:
    ``cand``, or ``ffacand`` for those of the fast-folding search; ``first``:
    the k of the first one) and prints one line per candidate.  Returns the
    FoldedCandidates."""
    from pypulsar_amd.fold import Folder, write_bestprof
    folded = Folder(npart, nbins)(plane, dms, dt, sifted, dm_halfwidth=dm_halfwidth)
    for k, fc in enumerate(folded, first):
        name = "%s_%s%d" % (base, tag, k)
        write_bestprof(fc, name + ".bestprof", infile=infile, candname=os.path.basename(name))
        np.savez(name + ".npz", subints=fc.subints, subint_counts=fc.subint_counts,
                 chi2_plane=fc.chi2_plane, chi2_vs_dm=fc.chi2_vs_dm, dms=fc.dms,
                 profile=fc.profile, counts=fc.counts, trial=np.asarray(fc.trial),
                 f=fc.f, fd=fc.fd, dm=fc.dm, chi2=fc.chi2, sigma=fc.sigma)
        print("%s %d: DM %.2f  P %.9f ms  fd %.3g Hz/s  reduced chi2 %.2f  sigma %.1f -> %s" % (
            tag, k, fc.dm, 1000.0 * fc.period, fc.fd, fc.chi2, fc.sigma, name + ".bestprof"))
    return folded


if __name__ == "__main__":
    sys.exit(main())
