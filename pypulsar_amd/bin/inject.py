#!/usr/bin/env python
"""inject.py -- write a copy of a search file with synthetic pulsars and
bursts added on the GPU (pypulsar_amd.inject).

    python -m pypulsar_amd.bin.inject --spec SPEC.json -o out.fil in.fil

SPEC.json is a list of signals (or {"signals": [...], "nbins": B, "seed":
S}), each {"kind": "pulsar", "f", "dm", ...} or {"kind": "burst", "t", "dm",
"width", ...} with the strength as ``amp`` (data units) or ``snr`` (matched
S/N against 1.4826 MAD per channel of the file's first 65536 spectra); a
pulsar with ``pb`` and ``x`` (and optionally ``e``, ``omega``, ``t0``) is in a
Keplerian orbit, and the truth carries the orbit.  8-bit
and 32-bit SIGPROC input gives the same bit depth out under the input's own
header; a PSRFITS file gives a SIGPROC file of its decoded type (8-bit or
float32).  Packed (1-, 2-, 4-bit) and 16-bit input are refused.  The truth
(parameters, matched S/N, arrival sample) goes to ``<out base>_truth.json``.
The file is worked block by block with ``Injector.apply`` at the block's
first sample, so the bytes do not depend on the block length.
"""
import json
import optparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BLOCK = 1 << 16  # spectra per device round trip


def inject_file(infile, outname, spec, block=BLOCK, file_kw=None, seed=None, nbins=None):
    """Write ``outname``; returns the Injector used."""
    import torch
    from pypulsar_amd.formats import sigproc
    from pypulsar_amd.formats.psrfits import open_search_file
    from pypulsar_amd.inject import injector_for_file

    fb = open_search_file(infile, **(file_kw or {}))
    try:
        if fb.packed:
            raise ValueError("inject: %d-bit packed input is not supported (packed output is not "
                             "written); convert the file to 8 bits first" % fb.nbits)
        np_dtype = np.dtype(fb.dtype)
        if np_dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise ValueError("inject: %s input is not supported; convert the file to 8 or 32 "
                             "bits first" % np_dtype)
        kw = {}
        if seed is not None:
            kw["seed"] = seed
        if nbins is not None:
            kw["nbins"] = nbins
        injector = injector_for_file(spec, fb, **kw)
        nchan, N = fb.nchans, int(fb.number_of_samples)
        psrfits = hasattr(fb, "read_device")
        if psrfits:
            foff = float(fb.header["foff"])
            params, header = sigproc.make_header(
                nchan, 8 * np_dtype.itemsize, fb.tsamp, float(fb.header["fch1"]), foff,
                tstart=float(fb.header["tstart"]),
                source_name=fb.header.get("source_name") or "injected")
        else:
            params, header = fb.header_params, fb.header
        tdt = torch.uint8 if np_dtype == np.uint8 else torch.float32
        host = None if psrfits else torch.empty((block, nchan), dtype=tdt, pin_memory=True)
        with open(outname, "wb") as out:
            sigproc.write_header(out, params, header)
            done = 0
            while done < N:
                n = min(block, N - done)
                if psrfits:
                    dev = fb.read_device(done, n)
                else:
                    n = fb.read_block_into(done, host.numpy()[:n])
                    if n <= 0:
                        break
                    dev = host[:n].to("cuda", non_blocking=True)
                injector.apply(dev, done)
                dev.cpu().numpy().tofile(out)
                done += n
    finally:
        fb.close()
    return injector


def main(argv=None):
    parser = optparse.OptionParser(prog="inject.py", usage="%prog --spec SPEC.json -o OUT.fil INFILE",
                                   description="Write a copy of a SIGPROC filterbank or PSRFITS "
                                               "search-mode file with synthetic pulsars and "
                                               "bursts added on the GPU.")
    parser.add_option("--spec", type="string", default=None, help="The JSON list of signals.")
    parser.add_option("-o", "--outname", type="string", default=None, help="Output filterbank file.")
    parser.add_option("--seed", type="int", default=None,
                      help="Seed of the 8-bit dither. (Default: the spec's, else 0)")
    parser.add_option("--nbins", type="int", default=None,
                      help="Bins of the profile tables, a power of two in 64..4096. "
                           "(Default: the spec's, else 1024)")
    parser.add_option("--block", type="int", default=BLOCK,
                      help="Spectra per device round trip. (Default: 65536)")
    from pypulsar_amd.bin.frb_search import file_options
    parser.add_option("--noscales", dest="apply_scales", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_SCL.")
    parser.add_option("--nooffsets", dest="apply_offsets", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_OFFS.")
    parser.add_option("--noweights", dest="apply_weights", action="store_false", default=True,
                      help="PSRFITS input: do not apply DAT_WTS.")
    parser.add_option("--poln", type="int", default=None, metavar="K",
                      help="PSRFITS input: use polarisation K alone.")
    options, args = parser.parse_args(argv)
    if len(args) != 1 or not options.spec or not options.outname:
        parser.error("--spec SPEC.json, -o OUT.fil and one input file are expected")
    if options.block < 1:
        parser.error("--block must be positive")
    try:
        injector = inject_file(args[0], options.outname, options.spec, options.block,
                               file_options(options), options.seed, options.nbins)
    except ValueError as e:
        parser.error(str(e))
    tout = os.path.splitext(options.outname)[0] + "_truth.json"
    with open(tout, "w") as f:
        json.dump(injector.truth(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d signals -> %s, %s" % (len(injector.jobs), options.outname, tout))
    return 0


if __name__ == "__main__":
    sys.exit(main())
