"""Test data of the 1-, 2- and 4-bit filterbank tests.  The oracle of the
device work is the existing 8-bit path on host-unpacked values
(formats/sigproc.py unpack_bits), so there is no NumPy restatement here: only
the seeded values every test shares."""
import numpy as np


def lowbit_data(n, C, nbits, seed):
    """[n, C] uint8 values of ``nbits`` bits, time-major: seeded full-range
    random values with, in rows 0.., an all-zero spectrum, an all-max spectrum
    and spectra whose channel mean is exactly k + 1/2 for every k in
    0 .. 2^nbits - 2 (half the channels k, half k + 1, interleaved): the ties
    of the half-to-even rounding, with k even and, from 2 bits on, odd."""
    assert C % 2 == 0
    vmax = (1 << nbits) - 1
    x = np.random.default_rng(seed).integers(0, vmax + 1, (n, C)).astype(np.uint8)
    ks = list(range(vmax))[:max(0, n - 2)]
    if n > 0:
        x[0] = 0
    if n > 1:
        x[1] = vmax
    for i, k in enumerate(ks):
        x[2 + i] = k + (np.arange(C) + i) % 2
    return x
