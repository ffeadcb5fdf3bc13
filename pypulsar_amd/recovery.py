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

A pulsar in an orbit (``pb`` in its truth) keeps its apparent frequency
inside ``[f_lo, f_hi]``, so for it the window of the relation ``h f`` widens
to ``[h f_lo - 1.5 h / T, h f_hi + 1.5 h / T]`` and that of ``f / h`` to
``[f_lo / h - 1.5 / T, f_hi / h + 1.5 / T]`` (where an acceleration search
sees it; the report says ``widened``).  The binary searches are graded by

* ``match_binaries`` -- a sideband candidate matches an injected binary when
  its DM is inside the pulsar's DM window, ``[freq_lo, freq_hi]`` intersects
  ``[h f_lo, h f_hi]`` for some ``h <= 16``, and ``porb`` is within ``1.5 porb
  / q`` (its own half-bin grid step, the window the orbit follow-up searches)
  of ``pb / m`` or ``pb m``, ``m <= 4``;
* ``match_orbits`` -- an orbit candidate matches when its frequency is in a
  harmonic relation to ``f`` itself (in the demodulated frame of the right
  orbit the pulsar is at ``f``) and its DM inside the window; the template's
  offsets in ``pb``, ``x`` and orbital phase are reported, not judged.

The strongest matching candidate is reported; a candidate may be the best
match of several injected signals (two signals closer than the windows are
not told apart)."""
import json
import math

import numpy as np

from . import delays

MAX_HARM = 16
MAX_ORBIT_RATIO = 4


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


def harmonic_relation(f_cand, f, T, max_harm=MAX_HARM, half_band=0.0):
    """(label, h, offset in Hz) of the closest relation ``h f`` or ``f / h``
    within its window (1.5 h / T, 1.5 / T), or None.  The fundamental wins a
    tie.  ``half_band``: half the width in Hz of the band that holds the
    apparent frequency of a pulsar in an orbit; the windows widen by ``h
    half_band`` and ``half_band / h``."""
    best = None
    for h in range(1, max_harm + 1):
        for label, target, tol in (("%d*f" % h if h > 1 else "f", h * f,
                                    1.5 * h / T + h * half_band),
                                   ("f/%d" % h, f / h, 1.5 / T + half_band / h)):
            if h == 1 and label != "f":
                continue
            off = f_cand - target
            if abs(off) <= tol and (best is None or abs(off) / tol < best[3]):
                best = (label, h, off, abs(off) / tol)
        if best is not None and best[1] == 1:
            break
    return None if best is None else best[:3]


def has_orbit(sig):
    return sig.get("kind") == "pulsar" and sig.get("pb") is not None


def pulsar_dm_window(sig, dms, freqs, dt):
    """The DM window of an injected pulsar: ``dm_window`` of its smeared
    pulse width in seconds."""
    w = math.sqrt((sig.get("width", 0.05) / sig["f"]) ** 2 + sig.get("tau", 0.0) ** 2
                  + _smear(sig, freqs, dt) ** 2 + dt ** 2)
    return dm_window(w, dms, freqs)


def match_pulsars(truth, cands, T, dms, freqs, dt):
    """One report per injected pulsar: found, the strongest matching
    candidate's sigma, DM, frequency, the harmonic relation (``h*f`` or
    ``f/h``, h <= 16) and the frequency offset from it.  ``cands``: records
    with DM, freq and sigma; ``T``: the length of the searched series in
    seconds.  For a pulsar in an orbit the frequency windows widen by the
    band ``[f_lo, f_hi]`` of its apparent frequency and the report carries
    ``widened``, ``f_lo`` and ``f_hi``."""
    cands = np.asarray(cands)
    out = []
    for k, sig in enumerate(truth):
        if sig.get("kind") != "pulsar":
            continue
        ddm = pulsar_dm_window(sig, dms, freqs, dt)
        rep = dict(index=k, kind="pulsar", f=sig["f"], dm=sig["dm"],
                   matched_snr=sig.get("matched_snr"), found=False, sigma=None, cand_dm=None,
                   cand_freq=None, harmonic=None, dm_offset=None, freq_offset=None,
                   dm_window=ddm, freq_window=1.5 / T)
        half = 0.0
        if has_orbit(sig):
            half = 0.5 * (sig["f_hi"] - sig["f_lo"])
            rep.update(widened=True, f_lo=sig["f_lo"], f_hi=sig["f_hi"])
        best = None
        if len(cands):
            cdm, cf, cs = _field(cands, "DM"), _field(cands, "freq"), _field(cands, "sigma", "Sigma")
            for i in np.flatnonzero(np.abs(cdm - sig["dm"]) <= ddm):
                rel = harmonic_relation(cf[i], sig["f"], T, half_band=half)
                if rel is not None and (best is None or cs[i] > cs[best[0]]):
                    best = (int(i), rel)
        if best is not None:
            i, (label, _, off) = best
            rep.update(found=True, sigma=float(cs[i]), cand_dm=float(cdm[i]), cand_freq=float(cf[i]),
                       harmonic=label, dm_offset=float(cdm[i] - sig["dm"]), freq_offset=float(off))
        out.append(rep)
    return out


def orbit_relation(porb, pb, tol, max_ratio=MAX_ORBIT_RATIO):
    """(label, m, offset in s) of the closest of ``pb / m`` and ``pb m``, m <=
    4, within ``tol`` seconds of ``porb``, or None; ``pb`` itself wins a tie."""
    best = None
    for m in range(1, max_ratio + 1):
        for label, target in (("pb/%d" % m if m > 1 else "pb", pb / m), ("%d*pb" % m, pb * m)):
            if m == 1 and label != "pb":
                continue
            off = porb - target
            if abs(off) <= tol and (best is None or abs(off) < abs(best[2])):
                best = (label, m, off)
        if best is not None and best[1] == 1:
            break
    return best


def match_binaries(truth, bincands, T, dms, freqs, dt):
    """One report per injected pulsar with an orbit, graded against sideband
    candidates (``sideband.BINCAND_DTYPE`` or ``SIFTED_DTYPE`` records): found,
    and of the strongest matching candidate its sigma, DM, ``porb``, the
    relations ``h`` (``[freq_lo, freq_hi]`` meets ``[h f_lo, h f_hi]``; the
    smallest such h) and ``m`` (``porb`` against ``pb / m`` or ``pb m``:
    ``porb_relation``), ``L``, ``q`` and the offset in ``porb``."""
    cands = np.asarray(bincands)
    out = []
    for k, sig in enumerate(truth):
        if not has_orbit(sig):
            continue
        ddm = pulsar_dm_window(sig, dms, freqs, dt)
        rep = dict(index=k, kind="binary", f=sig["f"], dm=sig["dm"], pb=sig["pb"], x=sig["x"],
                   f_lo=sig["f_lo"], f_hi=sig["f_hi"], matched_snr=sig.get("matched_snr"),
                   found=False, sigma=None, cand_dm=None, cand_porb=None, cand_freq_lo=None,
                   cand_freq_hi=None, h=None, m=None, porb_relation=None, L=None, q=None,
                   porb_offset=None, dm_window=ddm)
        best = None
        if len(cands):
            cdm, cs = _field(cands, "DM"), _field(cands, "sigma")
            lo, hi = _field(cands, "freq_lo"), _field(cands, "freq_hi")
            porb, q = _field(cands, "porb"), _field(cands, "q")
            for i in np.flatnonzero(np.abs(cdm - sig["dm"]) <= ddm):
                hs = [h for h in range(1, MAX_HARM + 1)
                      if lo[i] <= h * sig["f_hi"] and hi[i] >= h * sig["f_lo"]]
                rel = orbit_relation(porb[i], sig["pb"], 1.5 * porb[i] / q[i]) if q[i] > 0 else None
                if hs and rel is not None and (best is None or cs[i] > cs[best[0]]):
                    best = (int(i), hs[0], rel)
        if best is not None:
            i, h, (label, m, off) = best
            rep.update(found=True, sigma=float(cs[i]), cand_dm=float(cdm[i]),
                       cand_porb=float(porb[i]), cand_freq_lo=float(lo[i]),
                       cand_freq_hi=float(hi[i]), h=int(h), m=int(m), porb_relation=label,
                       L=int(cands["L"][i]), q=int(cands["q"][i]), porb_offset=float(off))
        out.append(rep)
    return out


def match_orbits(truth, orbcands, T, dms, freqs, dt):
    """One report per injected pulsar with an orbit, graded against orbit
    candidates (``orbit.ORBCAND_DTYPE`` or ``SIFTED_DTYPE`` records): found,
    and of the strongest candidate whose frequency is in a harmonic relation
    to ``f`` (``harmonic_relation``, unwidened) and whose DM is inside the
    window: sigma, DM, frequency, the relation, and the template's offsets in
    ``pb`` (s), ``x`` (light seconds) and orbital phase (``t0 / pb`` mod 1,
    in [-0.5, 0.5) orbits) -- reported, not judged."""
    cands = np.asarray(orbcands)
    out = []
    for k, sig in enumerate(truth):
        if not has_orbit(sig):
            continue
        ddm = pulsar_dm_window(sig, dms, freqs, dt)
        rep = dict(index=k, kind="orbit", f=sig["f"], dm=sig["dm"], pb=sig["pb"], x=sig["x"],
                   matched_snr=sig.get("matched_snr"), found=False, sigma=None, cand_dm=None,
                   cand_freq=None, harmonic=None, freq_offset=None, cand_pb=None, cand_x=None,
                   cand_t0=None, pb_offset=None, x_offset=None, phase_offset=None, dm_window=ddm,
                   freq_window=1.5 / T)
        best = None
        if len(cands):
            cdm, cf, cs = _field(cands, "DM"), _field(cands, "freq"), _field(cands, "sigma")
            for i in np.flatnonzero(np.abs(cdm - sig["dm"]) <= ddm):
                rel = harmonic_relation(cf[i], sig["f"], T)
                if rel is not None and (best is None or cs[i] > cs[best[0]]):
                    best = (int(i), rel)
        if best is not None:
            i, (label, _, off) = best
            cpb, cx, ct0 = (float(cands[n][i]) for n in ("pb", "x", "t0"))
            dphi = (ct0 / cpb - sig.get("t0", 0.0) / sig["pb"] + 0.5) % 1.0 - 0.5
            rep.update(found=True, sigma=float(cs[i]), cand_dm=float(cdm[i]), cand_freq=float(cf[i]),
                       harmonic=label, freq_offset=float(off), cand_pb=cpb, cand_x=cx, cand_t0=ct0,
                       pb_offset=cpb - sig["pb"], x_offset=cx - sig["x"], phase_offset=float(dphi))
        out.append(rep)
    return out


def write_report(fn, truth, reports, **more):
    """<base>_recovery.json: the truth and the per-signal reports; ``more``:
    further reports under keys of their own (``binaries``, ``orbits``)."""
    with open(fn, "w") as f:
        json.dump(dict(truth=truth, recovery=reports, **more), f, indent=1, sort_keys=True)
        f.write("\n")
