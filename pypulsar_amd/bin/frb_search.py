#!/usr/bin/env python
"""frb_search.py -- streaming single-pulse search of a SIGPROC filterbank or
PSRFITS search-mode file.

New (the reference has no search; BASELINE config 5 plus its consumer):
blocks of spectra are read into rotating pinned host buffers
(filterbank.read_block_into), copied to the GPU on a copy stream, zero-DM
filtered (bin/zero_dm_filter.py:30-39, float mode), downsampled
(spectra.py:329-351), swept over a uniform DM grid (per-DM
Spectra.dedisperse + channel sum, spectra.py:229-260) and boxcar-searched
(pypulsar_amd.search; boxcar of pulse.py:217-241); only candidates come back
to the host.  The candidates equal those of a one-shot search of the whole
file's DM-time plane.  Output: PRESTO-style ``.singlepulse`` text.

    python -m pypulsar_amd.bin.frb_search --lodm 0 --hidm 1000 --numdms 2048 \\
        --downsamp 2 --threshold 7 -o obs.singlepulse obs.fil
    python -m pypulsar_amd.bin.frb_search --hidm 1000 --numdms 2048 guppi_obs_0001.fits
    python -m pypulsar_amd.bin.frb_search --rfifind 2.0 --numdms 2048 obs.fil
    python -m pypulsar_amd.bin.frb_search --mask obs_rfifind.mask --numdms 2048 obs.fil
    python -m pypulsar_amd.bin.frb_search --group --min-members 3 --min-group-dm 5 obs.fil
    python -m pypulsar_amd.bin.frb_search --cutouts 20 --min-members 3 obs.fil

A PSRFITS file (recognised by content) is streamed as its own SUBINT rows,
decoded on the device (pdd_psrfits_block; formats.psrfits.PsrfitsSearchFile):
``--noscales``, ``--nooffsets``, ``--noweights`` and ``--poln K`` choose what
the decode applies; they are ignored, with a note, for a filterbank.

``--mask`` / ``--rfifind``: the cells of an rfifind ``.mask`` (read, or made in
a first pass over the file: pypulsar_amd.rfi) are replaced on the device by
their channel's level before the zero-DM filter.

``--group``: after the stream ends the merged candidates are grouped across
DM row, time and width on the device (pypulsar_amd.spgroup: one line per
event, not per DM trial) and the kept groups written to ``<out base>.spgroups``;
the ``.singlepulse`` file is the same with or without it.

``--cutouts N`` (implies ``--group``): the frequency-time and DM-time images
(pypulsar_amd.cutout) of the best member of the N strongest kept groups, from
the raw file (masked when a mask is in use; the zero-DM filter is not
applied), go to ``<out base>_cutouts.npz``; the ``.singlepulse`` and
``.spgroups`` files are the same with or without it.

``--inject SPEC.json``: the synthetic bursts and pulsars of the spec
(pypulsar_amd.inject; a pulsar may be in a Keplerian orbit) are added to every raw block on the device, before any
mask; ``--recovery`` matches the candidates to them
(pypulsar_amd.recovery) into ``<out base>_recovery.json``.  Not with
``--cutouts``, which reads the file again: write an injected copy with
``python -m pypulsar_amd.bin.inject`` first.
"""
import optparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _chunks(fb, block, nbuf=4, start_block=0):
    """Pinned [n, nchans] host chunks of the file from block ``start_block``
    on, in rotation (a buffer is reused nbuf chunks later, after its
    asynchronous copy has completed: StreamingSweep keeps at most 2 chunks in
    flight).  A 1-, 2- or 4-bit file is read as it is: packed
    [n, bytes_per_spectrum] uint8 chunks, unpacked on the device.  A PSRFITS
    file yields row chunks: the SUBINT rows [k, NAXIS1] of each block's
    samples as stored (a seam row is read into both chunks), for
    StreamingSweep(decoder=fb.decoder())."""
    import torch
    if hasattr(fb, "read_rows_into"):
        dec = fb.decoder()
        bufs = [torch.empty((dec.max_rows(block), fb.row_bytes), dtype=torch.uint8,
                            pin_memory=True) for _ in range(nbuf)]
        done, i = int(start_block) * block, 0
        while done < fb.number_of_samples:
            h = bufs[i % nbuf]
            row0, nrows, _ = dec.rows_for(done, block)
            got = fb.read_rows_into(row0, h.numpy()[:nrows])
            if got != nrows:
                raise IOError("%s: short read, %d of %d rows" % (fb.filename, got, nrows))
            yield h[:nrows]
            done += block
            i += 1
        return
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16,
           np.dtype(np.float32): torch.float32}[np.dtype(fb.dtype)]
    width = fb.bytes_per_spectrum if fb.packed else fb.nchans
    bufs = [torch.empty((block, width), dtype=tdt, pin_memory=True) for _ in range(nbuf)]
    done, i = int(start_block) * block, 0
    while done < fb.number_of_samples:
        h = bufs[i % nbuf]
        if fb.packed:
            n = fb.read_packed_into(done, h.numpy()[:block])
        else:
            n = fb.read_block_into(done, h.numpy().view(np.dtype(fb.dtype))[:block])
        if n <= 0:
            break
        yield h[:n]
        done += n
        i += 1


def get_mask(infile, fb, maskfile=None, rfifind=None, block=1 << 18, file_kw=None):
    """The pypulsar_amd.rfi.RFIMask of a search: made in a first pass over the
    file with intervals of ``rfifind`` seconds (and left beside it as
    <base>_rfifind.mask), or read from ``maskfile``; None without either."""
    if rfifind:
        from pypulsar_amd.bin.rfifind import find_mask
        mask = find_mask(infile, rfifind, block, file_kw=file_kw)
        out = os.path.splitext(infile)[0] + "_rfifind.mask"
        mask.write(out)
        print("rfifind: %.2f%% masked -> %s" % (100.0 * mask.masked_fraction, out))
        return mask
    if maskfile:
        from pypulsar_amd.rfi import mask_from_file
        return mask_from_file(maskfile, fb, block)
    return None


def search_file(infile, dms, downsamp=2, block=1 << 18, zero_dm=True, threshold=6.0,
                widths=None, detrendlen=1024, debug=False, maskfile=None, rfifind=None,
                rfimask=None, file_kw=None, injector=None):
    """``rfimask``: a mask already made (else ``maskfile`` / ``rfifind``);
    ``file_kw``: open_search_file's keywords (PSRFITS input); ``injector``: a
    ``pypulsar_amd.inject.Injector`` whose signals are added to every raw
    block on the device, before the mask."""
    import torch
    from pypulsar_amd.formats.psrfits import open_search_file
    from pypulsar_amd.search import DEFAULT_WIDTHS, StreamingSearch, merge

    fb = open_search_file(infile, **(file_kw or {}))
    if np.dtype(fb.dtype) == np.uint16:
        raise ValueError("16-bit filterbanks: convert to 8 or 32 bits first")
    tdt = torch.uint8 if np.dtype(fb.dtype) == np.uint8 else torch.float32
    ss = StreamingSearch(dms, fb.freqs, fb.tsamp, block=block, downsamp=downsamp,
                         zero_dm=zero_dm, dtype=tdt, threshold=threshold,
                         widths=widths or DEFAULT_WIDTHS, detrendlen=detrendlen,
                         nbits=fb.nbits if fb.packed else 8, rfimask=rfimask if rfimask is not None else
                         get_mask(infile, fb, maskfile, rfifind, block, file_kw),
                         decoder=fb.decoder() if hasattr(fb, "decoder") else None,
                         injector=injector)
    parts = []  # candidate times are relative to the file start
    for i, c in enumerate(ss(_chunks(fb, block))):
        parts.append(c)
        if debug:
            sys.stderr.write("\rblock %d: %d candidates" % (i, sum(len(p) for p in parts)))
    if debug:
        sys.stderr.write("\n")
    ss.close()
    fb.close()
    return merge(parts)


INJECT_HINT = ("write an injected copy with `python -m pypulsar_amd.bin.inject --spec SPEC.json "
               "-o OUT.fil INFILE` and run on that")


def add_inject_options(parser):
    parser.add_option("--inject", type="string", default=None, metavar="SPEC.json",
                      help="Add the synthetic pulsars and bursts of SPEC.json (a list of "
                           "signals, each with amp or snr; pypulsar_amd.inject) to the data on "
                           "the device, before any mask.  snr is scaled by 1.4826 MAD per "
                           "channel of the file's first 65536 spectra.")
    parser.add_option("--recovery", action="store_true", default=False,
                      help="With --inject: match the candidates to the injected signals and "
                           "write <out base>_recovery.json.")


def load_injector(spec, infile, file_kw=None, error=None):
    """The Injector of --inject SPEC.json for ``infile`` (None without).  A
    spec or a file that cannot be injected (16-bit data, ``snr`` against a
    noise level of 0) is a ValueError, handed to ``error`` (a parser's) if
    given."""
    if not spec:
        return None
    from pypulsar_amd.formats.psrfits import open_search_file
    from pypulsar_amd.inject import injector_for_file
    fb = open_search_file(infile, **(file_kw or {}))
    try:
        if np.dtype(fb.dtype) == np.uint16:
            raise ValueError("--inject: 16-bit data cannot be injected; convert the file to 8 or "
                             "32 bits first")
        return injector_for_file(spec, fb)
    except ValueError as e:
        if error is None:
            raise
        error(str(e))
    finally:
        fb.close()


def file_options(options):
    """open_search_file's keywords from the parsed --noscales / --nooffsets /
    --noweights / --poln options."""
    return dict(apply_scales=options.apply_scales, apply_offsets=options.apply_offsets,
                apply_weights=options.apply_weights, poln=options.poln)


def main(argv=None):
    parser = optparse.OptionParser(prog="frb_search.py", usage="%prog [OPTIONS] INFILE",
                                   description="Streaming dedispersion + single-pulse search "
                                               "of a SIGPROC filterbank or PSRFITS search-mode "
                                               "file on the GPU.")
    parser.add_option("--lodm", type="float", default=0.0, help="Lowest DM (pc/cc).")
    parser.add_option("--hidm", type="float", default=1000.0, help="Highest DM (pc/cc).")
    parser.add_option("--numdms", type="int", default=1024, help="Number of DM trials.")
    parser.add_option("--downsamp", type="int", default=2,
                      help="Downsampling factor (divides 64). (Default: 2)")
    parser.add_option("--block", type="int", default=1 << 18,
                      help="Spectra per streamed block. (Default: 262144)")
    parser.add_option("--no-zero-dm", dest="zero_dm", action="store_false", default=True,
                      help="Skip the zero-DM filter.")
    parser.add_option("--mask", dest="maskfile", type="string", default=None,
                      help="rfifind .mask file: its cells are replaced by the channel's "
                           "level before the zero-DM filter. (Default: no mask)")
    parser.add_option("--rfifind", type="float", default=None, metavar="SECONDS",
                      help="Make the mask in a first pass over the file, with intervals of "
                           "SECONDS (written to <INFILE base>_rfifind.mask), then search "
                           "with it.")
    parser.add_option("-t", "--threshold", type="float", default=6.0,
                      help="Candidate S/N threshold. (Default: 6)")
    parser.add_option("-m", "--maxwidth", type="int", default=150,
                      help="Largest boxcar width in downsampled samples (<= 1025).")
    parser.add_option("-o", "--outname", default=None,
                      help="Output .singlepulse file (default: INFILE with .singlepulse).")
    parser.add_option("--group", action="store_true", default=False,
                      help="Group the candidates across DM, time and width; the kept groups "
                           "go to <out base>.spgroups.")
    parser.add_option("--group-rows", type="int", default=2, metavar="N",
                      help="Candidates up to N DM trials apart can be linked. (Default: 2)")
    parser.add_option("--group-samples", type="int", default=3, metavar="N",
                      help="Candidates whose extents are up to N downsampled samples apart "
                           "can be linked. (Default: 3)")
    parser.add_option("--min-members", type="int", default=1, metavar="N",
                      help="Keep groups of at least N candidates. (Default: 1)")
    parser.add_option("--min-group-dm", type="float", default=None, metavar="DM",
                      help="Drop groups whose best member is below DM. (Default: keep all)")
    parser.add_option("--cutouts", type="int", default=0, metavar="N",
                      help="Cut out the frequency-time and DM-time images of the best member "
                           "of the N strongest kept groups into <out base>_cutouts.npz "
                           "(implies --group).")
    parser.add_option("--cutout-bins", type="int", default=256, metavar="N",
                      help="Time bins of both images. (Default: 256)")
    parser.add_option("--cutout-subbands", type="int", default=None, metavar="N",
                      help="Subbands of the frequency-time image; divides the channels. "
                           "(Default: 256, or all channels if that does not divide them)")
    parser.add_option("--cutout-dms", type="int", default=256, metavar="N",
                      help="Trial DMs of the DM-time image. (Default: 256)")
    parser.add_option("--cutout-dm-half", type="float", default=None, metavar="DM",
                      help="Half-range of the DM-time image's trial DMs. (Default: the "
                           "candidate's DM, at least 10)")
    add_inject_options(parser)
    parser.add_option("--noscales", dest="apply_scales", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_SCL.")
    parser.add_option("--nooffsets", dest="apply_offsets", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_OFFS.")
    parser.add_option("--noweights", dest="apply_weights", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_WTS.")
    parser.add_option("--poln", type="int", default=None, metavar="K",
                      help="PSRFITS input: use polarisation K alone. (Default: the one "
                           "polarisation, AA + BB of AABB data, I of IQUV)")
    parser.add_option("-d", "--debug", action="store_true", default=False)
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("one input file expected")
    file_kw = file_options(options)
    from pypulsar_amd.search import DEFAULT_WIDTHS, write_singlepulse
    widths = tuple(w for w in DEFAULT_WIDTHS if w <= options.maxwidth) or (1,)
    dms = np.linspace(options.lodm, options.hidm, options.numdms)
    if options.cutouts < 0:
        parser.error("--cutouts expects a count")
    if options.inject and options.cutouts:
        parser.error("--inject cannot be combined with --cutouts: the cut-outs read the file "
                     "again and would not see the signal; " + INJECT_HINT)
    if options.recovery and not options.inject:
        parser.error("--recovery needs --inject SPEC.json")
    injector = load_injector(options.inject, args[0], file_kw, parser.error)
    mask = None
    if options.cutouts and (options.maskfile or options.rfifind):
        # (made once: the search and the cut-outs see the same masked data)
        from pypulsar_amd.formats.psrfits import open_search_file
        fb = open_search_file(args[0], **file_kw)
        mask = get_mask(args[0], fb, options.maskfile, options.rfifind, options.block, file_kw)
        fb.close()
    cands = search_file(args[0], dms, options.downsamp, options.block, options.zero_dm,
                        options.threshold, widths, debug=options.debug,
                        maskfile=options.maskfile, rfifind=options.rfifind, rfimask=mask,
                        file_kw=file_kw, injector=injector)
    out = options.outname or os.path.splitext(args[0])[0] + ".singlepulse"
    write_singlepulse(cands, out)
    print("%d candidates -> %s" % (len(cands), out))
    if options.recovery:
        from pypulsar_amd import recovery
        truth = injector.truth()
        rep = recovery.match_bursts(truth, cands, dms, injector.freqs, injector.dt,
                                    options.downsamp)
        rout = os.path.splitext(out)[0] + "_recovery.json"
        recovery.write_report(rout, truth, rep)
        print("%d of %d injected bursts recovered -> %s"
              % (sum(r["found"] for r in rep), len(rep), rout))
    if options.group or options.cutouts:
        from pypulsar_amd.spgroup import SinglePulseGrouper, select, write_groups
        # (the merged list is grouped once; its rows are those of the DM grid)
        _, groups = SinglePulseGrouper(options.group_rows, options.group_samples)(cands, dms=dms)
        kept = select(groups, options.min_members, options.min_group_dm)
        gout = os.path.splitext(out)[0] + ".spgroups"
        write_groups(kept, gout)
        print("%d candidates -> %d groups -> %d kept -> %s"
              % (len(cands), len(groups), len(kept), gout))
    if options.cutouts:
        from pypulsar_amd.cutout import cutouts_from_file, write_cutouts
        from pypulsar_amd.formats.psrfits import open_search_file
        best = kept[np.argsort(-kept["Sigma"], kind="stable")[:options.cutouts]]
        fb = open_search_file(args[0], **file_kw)
        nsub = options.cutout_subbands
        if nsub is None:
            nsub = 256 if fb.nchans % 256 == 0 else fb.nchans
        ft, dmt, jobs = cutouts_from_file(fb, best, options.downsamp, rfimask=mask,
                                          nbin=options.cutout_bins, nsub=nsub,
                                          ndm=options.cutout_dms, dm_half=options.cutout_dm_half)
        fb.close()
        cout = os.path.splitext(out)[0] + "_cutouts.npz"
        write_cutouts(cout, ft, dmt, best, jobs)
        print("%d cut-outs -> %s" % (len(best), cout))
    return 0


if __name__ == "__main__":
    sys.exit(main())
