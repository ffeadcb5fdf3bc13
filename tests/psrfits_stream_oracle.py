"""NumPy restatement of the PSRFITS stream decode (pdd_psrfits_block and
formats.psrfits.PsrfitsSearchFile), for the tests only.

One polarisation is ``oracle.psrfits_oracle.read_subint`` itself (the
reference's ``((data*scales)+offsets)*weights`` with numpy's float32
promotion).  Two summed polarisations (AABB), the project's own rule:
``(((v0*scl0)+offs0) + ((v1*scl1)+offs1)) * wts`` in float32.  The integer
form: the file's value where the weight is non-zero (or weights are off),
else 0.
"""
import numpy as np

from oracle import psrfits_oracle as po


def stored(values, nbits):
    """One polarisation's [nsblk, nchan] values as read_subint expects its
    ``raw``: packed nibbles for 4 bits (low first), '>i2', '>f4' or uint8."""
    v = np.asarray(values)
    if nbits == 4:
        flat = v.reshape(-1).astype(np.uint8)
        return (flat[0::2] & 15) | ((flat[1::2] & 15) << 4)
    return v.astype({8: np.uint8, 16: ">i2", 32: ">f4"}[nbits])


def one_pol(values, nbits, scales, offsets, weights, apply_scales=True, apply_offsets=True,
            apply_weights=True):
    """read_subint of one polarisation of one subint ([nsblk, nchan])."""
    nsblk, nchan = values.shape
    if nbits == 4 and (nsblk * nchan) % 2:
        # an odd count cannot be packed on its own: the unpacked uint8 values
        # take read_subint's 8-bit branch (unpack_4bit yields the same uint8)
        raw, nb = np.asarray(values, dtype=np.uint8), 8
    else:
        raw, nb = stored(values, nbits), nbits
    return po.read_subint(raw, nb, nsblk, nchan, np.asarray(scales, dtype=np.float32),
                          np.asarray(offsets, dtype=np.float32),
                          np.asarray(weights, dtype=np.float32), apply_weights, apply_scales,
                          apply_offsets)


def decode(data, nbits, scales, offsets, weights, pol0=0, npol_sum=1, apply_scales=True,
           apply_offsets=True, apply_weights=True, out="float32"):
    """data [nsub, nsblk, npol, nchan] (file values), scales / offsets
    [nsub, npol*nchan], weights [nsub, nchan] -> [nsub*nsblk, nchan] of
    ``out`` ("float32" or "uint8"), channels in file order."""
    data = np.asarray(data)
    if data.ndim == 3:
        data = data[:, :, None, :]
    nsub, nsblk, npol, nchan = data.shape
    scales = np.asarray(scales, dtype=np.float32).reshape(nsub, npol, nchan)
    offsets = np.asarray(offsets, dtype=np.float32).reshape(nsub, npol, nchan)
    weights = np.asarray(weights, dtype=np.float32).reshape(nsub, nchan)
    rows = []
    for i in range(nsub):
        if out == "uint8":
            assert nbits <= 8 and npol_sum == 1
            v = np.asarray(data[i, :, pol0, :], dtype=np.uint8)
            rows.append(np.where(weights[i] != 0, v, 0).astype(np.uint8) if apply_weights else v)
        elif npol_sum == 1:
            rows.append(np.asarray(one_pol(data[i, :, pol0, :], nbits, scales[i, pol0],
                                           offsets[i, pol0], weights[i], apply_scales,
                                           apply_offsets, apply_weights), dtype=np.float32))
        else:
            parts = [np.asarray(one_pol(data[i, :, p, :], nbits, scales[i, p], offsets[i, p],
                                        weights[i], apply_scales, apply_offsets, False),
                                dtype=np.float32) for p in (pol0, pol0 + 1)]
            f = parts[0] + parts[1]
            rows.append(f * weights[i] if apply_weights else f)
    return np.concatenate(rows).astype(np.dtype(out), copy=False)
