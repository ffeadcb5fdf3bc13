#!/usr/bin/env python
"""pulsar_search.py -- periodicity search of a SIGPROC filterbank.

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
``.accelcands`` layout.

    python -m pypulsar_amd.bin.pulsar_search --lodm 0 --hidm 100 --numdms 256 \\
        --downsamp 2 --sigma 8 -o obs.accelcands obs.fil
"""
import optparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def search_file(infile, dms, downsamp=1, zero_dm=False, sigma=6.0, harms=None, flo=1.0,
                nfft=None, row_batch=None):
    """(candidate records, sample time of the searched plane)."""
    import torch
    from pypulsar_amd.formats import filterbank
    from pypulsar_amd.periodicity import DEFAULT_HARMS, PeriodicitySearch
    from pypulsar_amd.stream import prologue
    from pypulsar_amd.sweep import DMSweep

    fb = filterbank.filterbank(infile)
    if np.dtype(fb.dtype) == np.uint16:
        raise ValueError("16-bit filterbanks: convert to 8 or 32 bits first")
    assert 64 % downsamp == 0, "the downsampling factor must divide 64"
    C, dt = fb.nchans, fb.tsamp * downsamp
    n = fb.number_of_samples // downsamp * downsamp
    raw = torch.from_numpy(fb.read_all_samples()[:n * C].reshape(n, C)).cuda()
    fb.close()
    # zero-DM + downsample + corner turn in one pass: [C, n / downsamp] float32
    img = torch.empty((C, n // downsamp), dtype=torch.float32, device=raw.device)
    prologue(raw, n, C, downsamp, "float" if zero_dm else "none", img)
    del raw
    sw = DMSweep(dms, fb.freqs, dt, dtype="f32")
    plane = sw(img, trim=True)
    del img
    ps = PeriodicitySearch(sigma, harms or DEFAULT_HARMS, flo=flo)
    cands = ps(plane, dms, dt, row_batch=row_batch, nfft=nfft)
    sw.close()
    return cands, dt


def main(argv=None):
    parser = optparse.OptionParser(prog="pulsar_search.py", usage="%prog [OPTIONS] INFILE",
                                   description="Dedispersion + periodicity search of a SIGPROC "
                                               "filterbank on the GPU.")
    parser.add_option("--lodm", type="float", default=0.0, help="Lowest DM (pc/cc).")
    parser.add_option("--hidm", type="float", default=100.0, help="Highest DM (pc/cc).")
    parser.add_option("--numdms", type="int", default=128, help="Number of DM trials.")
    parser.add_option("--downsamp", type="int", default=1,
                      help="Downsampling factor (divides 64). (Default: 1)")
    parser.add_option("--zero-dm", dest="zero_dm", action="store_true", default=False,
                      help="Apply the zero-DM filter first.")
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
    parser.add_option("-o", "--outname", default=None,
                      help="Output .accelcands file (default: INFILE with .accelcands).")
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("one input filterbank expected")
    from pypulsar_amd.periodicity import sift, write_accelcands
    harms = tuple(h for h in (1, 2, 4, 8, 16, 32) if h <= options.numharm) or (1,)
    dms = np.linspace(options.lodm, options.hidm, options.numdms)
    cands, _ = search_file(args[0], dms, options.downsamp, options.zero_dm, options.sigma, harms,
                           options.flo, options.nfft, options.row_batch)
    sifted = sift(cands)
    base = os.path.splitext(args[0])[0]
    out = options.outname or base + ".accelcands"
    write_accelcands(sifted, out, basename=os.path.basename(base))
    print("%d candidates (%d sifted) -> %s" % (len(cands), len(sifted), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
