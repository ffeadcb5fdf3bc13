"""The comparison rule of the single-pulse search tests, shared by
test_gpu_search.py and test_gpu_search_paths.py (one rule, not two copies):
device candidates against the float64 oracle (oracle/search_oracle.py), per
(row, window of 1024 starts).

* S/N within 1e-4 * max(1, |s|) (the project's bar: f32 prefix sums against
  float64), plus ``snr_extra(w)`` where a test states a further addend;
* (start, width) exact when the oracle's margin between its best and its
  runner-up exceeds 1e-4 |s| (plus the same addend): below that the f32 and
  the float64 arg-max may differ (a near-tie);
* a candidate on one side only is allowed only within that bar of the
  threshold.

check() returns how many windows it excused (near-ties + at-threshold), how
many it compared, so a test can bound the share the exemptions cover, and
the worst S/N error met, |device - oracle| / max(1, |s|), for reports."""


def check(gpu_c, ora, margins, thr, snr_extra=None):
    extra = snr_extra if snr_extra is not None else (lambda w: 0.0)
    og = {(d, t // 1024): (t, w, s, m) for (d, t, w, s), m in zip(ora, margins)}
    gg = {(int(r), int(t) // 1024): (int(t), int(w), float(s))
          for r, t, w, s in zip(gpu_c["row"], gpu_c["Sample"], gpu_c["Downfact"], gpu_c["Sigma"])}
    assert len(gg) == len(gpu_c["row"]), "two device candidates in one (row, window)"
    excused, worst = 0, 0.0
    for k in set(og) | set(gg):
        if k in og and k in gg:
            t, w, s, m = og[k]
            assert abs(gg[k][2] - s) <= 1e-4 * max(1.0, abs(s)) + extra(w), (k, gg[k], og[k])
            worst = max(worst, abs(gg[k][2] - s) / max(1.0, abs(s)))
            if m > 1e-4 * abs(s) + extra(w):
                assert gg[k][:2] == (t, w), (k, gg[k], og[k])
            else:
                excused += 1
        else:  # only allowed at the threshold
            s, w = (og[k][2], og[k][1]) if k in og else (gg[k][2], gg[k][1])
            assert abs(s - thr) <= 1e-4 * abs(thr) + extra(w), (k, s)
            excused += 1
    return excused, len(set(og) | set(gg)), worst
