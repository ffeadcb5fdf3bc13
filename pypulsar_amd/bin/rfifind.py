#!/usr/bin/env python
"""rfifind.py -- find interference in a SIGPROC filterbank or PSRFITS
search-mode file and write a PRESTO ``.mask``.

New (the reference reads ``.mask`` files through PRESTO's rfifind module,
bin/waterfaller.py:28-48, but has nothing that makes one): the file is streamed
through the GPU in blocks, the per (interval, channel) mean, standard
deviation and largest normalised Fourier power are computed on the device
(pypulsar_amd.rfi.RFIFind), the cells are flagged on the host
(pypulsar_amd.rfi.decide) and written as ``BASE_rfifind.mask`` in the layout
of formats/rfifind.py, which ``waterfaller --mask``, ``frb_search --mask`` and
``pulsar_search --mask`` read.

    python -m pypulsar_amd.bin.rfifind -t 2.0 -o obs obs.fil
    python -m pypulsar_amd.bin.rfifind -t 2.0 guppi_obs_0001.fits

A PSRFITS file (recognised by content) is streamed as its own SUBINT rows and
decoded on the device; ``--noscales``, ``--nooffsets``, ``--noweights`` and
``--poln K`` choose what the decode applies (ignored, with a note, for a
filterbank).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def ptsperint_for(seconds, tsamp):
    """Samples of an interval of ``seconds`` (at least 16)."""
    return max(16, int(round(seconds / tsamp)))


def _decoded(fb, chunks, block):
    """The row chunks of a PSRFITS file decoded on the device into
    [n, nchans] blocks (two in rotation: RFIFind.accumulate reads a chunk
    before the one after the next is handed in)."""
    import torch
    dec = fb.decoder()
    rows = [torch.empty((dec.max_rows(block), fb.row_bytes), dtype=torch.uint8, device="cuda")
            for _ in range(2)]
    outs = [torch.empty((block, fb.nchans), dtype=dec.torch_dtype, device="cuda")
            for _ in range(2)]
    for i, chunk in enumerate(chunks):
        _, nrows, s0 = dec.rows_for(i * block, block)
        n = min(block, fb.number_of_samples - i * block)
        r = rows[i % 2]
        r[:nrows].copy_(chunk, non_blocking=True)
        out = dec.decode(r, nrows, s0, n, outs[i % 2])
        # the consumer copies the block on a stream of its own, and the pinned
        # chunk is refilled by the reader: both need the decode to be done
        torch.cuda.current_stream().synchronize()
        yield out


def find_mask(infile, seconds, block=1 << 18, file_kw=None, **kw):
    """The RFIMask of a filterbank or PSRFITS search-mode file, intervals of
    ``seconds``; ``file_kw``: open_search_file's keywords; ``kw``: the
    thresholds of pypulsar_amd.rfi.RFIFind."""
    from pypulsar_amd import rfi
    from pypulsar_amd.bin.frb_search import _chunks
    from pypulsar_amd.formats.psrfits import open_search_file

    fb = open_search_file(infile, **(file_kw or {}))
    if np.dtype(fb.dtype) == np.uint16:
        raise ValueError("16-bit filterbanks: convert to 8 or 32 bits first")
    finder = rfi.RFIFind(ptsperint_for(seconds, fb.tsamp), **kw)
    chunks = _chunks(fb, block)
    if hasattr(fb, "decoder"):
        chunks = _decoded(fb, chunks, block)
    mask = finder.find(chunks, **rfi.file_header(fb))
    fb.close()
    return mask


def main(argv=None):
    parser = argparse.ArgumentParser(prog="rfifind.py",
                                     description="Find RFI in a SIGPROC filterbank or PSRFITS "
                                                 "search-mode file on the GPU and write a "
                                                 "PRESTO .mask file.")
    parser.add_argument("-t", "-time", dest="time", type=float, required=True,
                        help="Seconds per interval.")
    parser.add_argument("-timesig", type=float, default=10.0,
                        help="Rejection threshold of the time-domain statistics, in robust "
                             "sigma. (Default: 10)")
    parser.add_argument("-freqsig", type=float, default=4.0,
                        help="Rejection threshold of the largest Fourier power, in equivalent "
                             "Gaussian sigma. (Default: 4)")
    parser.add_argument("-chansig", type=float, default=6.0,
                        help="Rejection threshold of a channel against its neighbours. "
                             "(Default: 6)")
    parser.add_argument("-chanfrac", type=float, default=0.7,
                        help="Fraction of bad intervals that zaps a channel. (Default: 0.7)")
    parser.add_argument("-intfrac", type=float, default=0.3,
                        help="Fraction of bad channels that zaps an interval. (Default: 0.3)")
    parser.add_argument("--block", type=int, default=1 << 18,
                        help="Spectra per streamed block. (Default: 262144)")
    parser.add_argument("-o", dest="outbase", default=None,
                        help="Output base name: writes BASE_rfifind.mask (default: INFILE "
                             "without its extension).")
    parser.add_argument("--noscales", dest="apply_scales", action="store_false",
                        help="PSRFITS input: do not apply DAT_SCL.")
    parser.add_argument("--nooffsets", dest="apply_offsets", action="store_false",
                        help="PSRFITS input: do not apply DAT_OFFS.")
    parser.add_argument("--noweights", dest="apply_weights", action="store_false",
                        help="PSRFITS input: do not apply DAT_WTS.")
    parser.add_argument("--poln", type=int, default=None, metavar="K",
                        help="PSRFITS input: use polarisation K alone.")
    parser.add_argument("infile")
    options = parser.parse_args(argv)
    file_kw = dict(apply_scales=options.apply_scales, apply_offsets=options.apply_offsets,
                   apply_weights=options.apply_weights, poln=options.poln)
    mask = find_mask(options.infile, options.time, options.block, file_kw=file_kw,
                     time_sig=options.timesig,
                     freq_sig=options.freqsig, chan_sig=options.chansig,
                     chantrigfrac=options.chanfrac, inttrigfrac=options.intfrac)
    base = options.outbase or os.path.splitext(options.infile)[0]
    out = base + "_rfifind.mask"
    mask.write(out)
    print("%d intervals of %d samples x %d channels: %.2f%% masked (%d channels, %d intervals "
          "entirely) -> %s" % (mask.nint, mask.ptsperint, mask.nchan,
                               100.0 * mask.masked_fraction, len(mask.zap_chans()),
                               len(mask.zap_ints()), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
