"""Injection-recovery bookkeeping (host only): the candidates of a search
matched to the truth of ``pypulsar_amd.inject.Injector.truth()``.

Matching windows:

* bursts -- with ``w`` the smeared width of the injected burst (the
  quadrature sum of its FWHM, its scattering time, the largest intra-channel
  smear and one downsampled sample), a candidate matches when its time is
  within ``w`` plus its own boxcar length of the arrival, and its DM within
  ``max(2 DM steps, w / band_delay)``, ``band_delay`` being the delay across
  the band per unit DM: the DM error that moves the band-crossing delay by
  ``w``;
* pulsars -- a candidate matches when, for some ``h <= 16``, its frequency is
  within ``1.5 h / T`` of ``h f`` (a harmonic) or within ``1.5 / T`` of ``f / h``
  (a sub-harmonic), and its DM within ``max(2 DM steps, w / band_delay)`` with
  ``w`` the smeared pulse width in seconds.

The strongest matching candidate is reported; a candidate may be the best
match of several injected signals (two signals closer than the windows are
not told apart)."""
import json
import math

import numpy as np

from . import delays

MAX_HARM = 16


def _dm_step(dms):
    dms = np.asarray(dms, dtype=np.float64)
    return float(np.median(np.diff(dms))) if dms.size > 1 else 0.0


def _band_delay(freqs):
    freqs = np.asarray(freqs, dtype=np.float64)
    return float(delays.delay_from_DM(1.0, freqs.min()) - delays.delay_from_DM(1.0, freqs.max()))


def _smear(sig, freqs, dt):
    freqs = np.asarray(freqs, dtype=np.float64)
    foff = abs(freqs[1] - freqs[0]) if freqs.size > 1 else 0.0
    return float(np.max(np.abs(delays.dm_smear(sig["dm"], foff, freqs))))


def dm_window(width, dms, freqs):
    """max(2 DM steps, the DM error that moves the band-crossing delay by
    ``width`` seconds)."""
    band = _band_delay(freqs)
    return max(2.0 * abs(_dm_step(dms)), width / band if band > 0 else 0.0)


def burst_width(sig, freqs, dt):
    """The smeared width (seconds) of an injected burst at sample time dt."""
    return math.sqrt(sig["width"] ** 2 + sig.get("tau", 0.0) ** 2 + _smear(sig, freqs, dt) ** 2
                     + dt ** 2)


def _field(cands, *names):
    for n in names:
        if n in cands.dtype.names:
            return np.asarray(cands[n], dtype=np.float64)
    raise KeyError("candidates have none of the fields %s" % (names,))


def match_bursts(truth, cands, dms, freqs, dt, downsamp=1):
    """One report per injected burst of ``truth``: found, the strongest
    matching candidate's sigma, DM, time, and its DM and time offsets.
    ``cands``: records with DM, Sigma, Time and Downfact (pypulsar_amd.search
    CAND_DTYPE); ``dt``: the file's sample time, ``downsamp`` the search's."""
    cands = np.asarray(cands)
    dts = dt * downsamp
    out = []
    for k, sig in enumerate(truth):
        if sig.get("kind") != "burst":
            continue
        w = burst_width(sig, freqs, dts)
        ddm = dm_window(w, dms, freqs)
        rep = dict(index=k, kind="burst", t=sig["t"], dm=sig["dm"],
                   matched_snr=sig.get("matched_snr"), found=False, sigma=None, cand_dm=None,
                   cand_time=None, dm_offset=None, time_offset=None, ratio=None,
                   time_window=w, dm_window=ddm)
        if len(cands):
            cdm, ct, cs = _field(cands, "DM"), _field(cands, "Time"), _field(cands, "Sigma", "sigma")
            box = _field(cands, "Downfact") * dts if "Downfact" in cands.dtype.names else 0.0
            ok = (np.abs(cdm - sig["dm"]) <= ddm) & (np.abs(ct - sig["t"]) <= w + box)
            if ok.any():
                i = int(np.flatnonzero(ok)[np.argmax(cs[ok])])
                rep.update(found=True, sigma=float(cs[i]), cand_dm=float(cdm[i]),
                           cand_time=float(ct[i]), dm_offset=float(cdm[i] - sig["dm"]),
                           time_offset=float(ct[i] - sig["t"]))
                if sig.get("matched_snr"):
                    rep["ratio"] = rep["sigma"] / sig["matched_snr"]
        out.append(rep)
    return out


def harmonic_relation(f_cand, f, T, max_harm=MAX_HARM):
    """(label, h, offset in Hz) of the closest relation ``h f`` or ``f / h``
    within its window (1.5 h / T, 1.5 / T), or None.  The fundamental wins a
    tie."""
    best = None
    for h in range(1, max_harm + 1):
        for label, target, tol in (("%d*f" % h if h > 1 else "f", h * f, 1.5 * h / T),
                                   ("f/%d" % h, f / h, 1.5 / T)):
            if h == 1 and label != "f":
                continue
            off = f_cand - target
            if abs(off) <= tol and (best is None or abs(off) / tol < best[3]):
                best = (label, h, off, abs(off) / tol)
        if best is not None and best[1] == 1:
            break
    return None if best is None else best[:3]


def match_pulsars(truth, cands, T, dms, freqs, dt):
    """One report per injected pulsar: found, the strongest matching
    candidate's sigma, DM, frequency, the harmonic relation (``h*f`` or
    ``f/h``, h <= 16) and the frequency offset from it.  ``cands``: records
    with DM, freq and sigma; ``T``: the length of the searched series in
    seconds."""
    cands = np.asarray(cands)
    out = []
    for k, sig in enumerate(truth):
        if sig.get("kind") != "pulsar":
            continue
        w = math.sqrt((sig.get("width", 0.05) / sig["f"]) ** 2 + sig.get("tau", 0.0) ** 2
                      + _smear(sig, freqs, dt) ** 2 + dt ** 2)
        ddm = dm_window(w, dms, freqs)
        rep = dict(index=k, kind="pulsar", f=sig["f"], dm=sig["dm"],
                   matched_snr=sig.get("matched_snr"), found=False, sigma=None, cand_dm=None,
                   cand_freq=None, harmonic=None, dm_offset=None, freq_offset=None,
                   dm_window=ddm, freq_window=1.5 / T)
        best = None
        if len(cands):
            cdm, cf, cs = _field(cands, "DM"), _field(cands, "freq"), _field(cands, "sigma", "Sigma")
            for i in np.flatnonzero(np.abs(cdm - sig["dm"]) <= ddm):
                rel = harmonic_relation(cf[i], sig["f"], T)
                if rel is not None and (best is None or cs[i] > cs[best[0]]):
                    best = (int(i), rel)
        if best is not None:
            i, (label, _, off) = best
            rep.update(found=True, sigma=float(cs[i]), cand_dm=float(cdm[i]), cand_freq=float(cf[i]),
                       harmonic=label, dm_offset=float(cdm[i] - sig["dm"]), freq_offset=float(off))
        out.append(rep)
    return out


def write_report(fn, truth, reports):
    """<base>_recovery.json: the truth and the per-signal reports."""
    with open(fn, "w") as f:
        json.dump(dict(truth=truth, recovery=reports), f, indent=1, sort_keys=True)
        f.write("\n")
