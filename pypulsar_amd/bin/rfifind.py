#!/usr/bin/env python
"""rfifind.py -- find interference in a SIGPROC filterbank and write a PRESTO
``.mask``.

New (the reference reads ``.mask`` files through PRESTO's rfifind module,
bin/waterfaller.py:28-48, but has nothing that makes one): the file is streamed
through the GPU in blocks, the per (interval, channel) mean, standard
deviation and largest normalised Fourier power are computed on the device
(pypulsar_amd.rfi.RFIFind), the cells are flagged on the host
(pypulsar_amd.rfi.decide) and written as ``BASE_rfifind.mask`` in the layout
of formats/rfifind.py, which ``waterfaller --mask``, ``frb_search --mask`` and
``pulsar_search --mask`` read.

    python -m pypulsar_amd.bin.rfifind -t 2.0 -o obs obs.fil
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def ptsperint_for(seconds, tsamp):
    """Samples of an interval of ``seconds`` (at least 16)."""
    return max(16, int(round(seconds / tsamp)))


def find_mask(infile, seconds, block=1 << 18, **kw):
    """The RFIMask of a filterbank file, intervals of ``seconds``; ``kw``:
    the thresholds of pypulsar_amd.rfi.RFIFind."""
    from pypulsar_amd import rfi
    from pypulsar_amd.bin.frb_search import _chunks
    from pypulsar_amd.formats import filterbank

    fb = filterbank.filterbank(infile)
    if np.dtype(fb.dtype) == np.uint16:
        raise ValueError("16-bit filterbanks: convert to 8 or 32 bits first")
    finder = rfi.RFIFind(ptsperint_for(seconds, fb.tsamp), **kw)
    mask = finder.find(_chunks(fb, block), **rfi.file_header(fb))
    fb.close()
    return mask


def main(argv=None):
    parser = argparse.ArgumentParser(prog="rfifind.py",
                                     description="Find RFI in a SIGPROC filterbank on the GPU "
                                                 "and write a PRESTO .mask file.")
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
    parser.add_argument("infile")
    options = parser.parse_args(argv)
    mask = find_mask(options.infile, options.time, options.block, time_sig=options.timesig,
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
