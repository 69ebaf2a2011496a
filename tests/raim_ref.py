"""Reference of the integrity tests: the section "Fix integrity: residual test and single-satellite exclusion" of
include/gpsacq.h restated in numpy, written from that text and not from the kernels.

  * chi2_tail / chi2_threshold: the closed-form tail for integer degrees of freedom, bisected as the header says;
  * statistic: T(S) at a state with held delays;
  * fix_raim: the model's own steps -- atm_ref.fix_atm for FULL, atm_ref.solve_from over every S \\ {k} from the full solution's
    state, then FINAL's rounds (atm_ref.views at the current state, atm_ref.solve_from from the current state).

Parameters are atm_ref's dict for the atmosphere and dict(sigma_m, threshold=[8], exclude) for the test.
"""
import math

import numpy as np

import atm_ref
import nav_ref
from nav_ref import C, WEEK_MS

NONE, UNCHECKED, PASS, EXCLUDED, FAILED = 0, 1, 2, 3, 4
MAX_DOF = 8
TABLE_1E3 = (10.827566170662733, 13.815510557964274, 16.26623619623813, 18.46682695290317, 20.515005652432876, 22.457744484825323,
             24.321886347856854, 26.12448155837614)


def chi2_tail(d, x):
    h = x / 2
    if d % 2 == 0:
        return math.exp(-h) * sum(h ** j / math.factorial(j) for j in range(d // 2))
    return math.erfc(math.sqrt(h)) + math.exp(-h) * sum(h ** (j + 0.5) / math.gamma(j + 1.5) for j in range((d - 1) // 2))


def chi2_threshold(d, p_fa):
    lo, hi = 0.0, 4000.0
    for _ in range(200):
        mid = (lo + hi) / 2
        if chi2_tail(d, mid) > p_fa:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def params(sigma_m, p_fa=1e-3, exclude=1):
    return dict(sigma_m=float(sigma_m), threshold=[chi2_threshold(d, p_fa) for d in range(1, MAX_DOF + 1)], exclude=int(exclude))


def statistic(xyz, t, w, delay, sel, pos, t_rx, sigma_m):
    """T over the satellites sel (bool) at the state (pos, t_rx) with the delays given"""
    d = pos - atm_ref.turned(xyz[sel], t[sel], t_rx)
    res = C * (t_rx - t[sel]) - delay[sel] - np.sqrt((d * d).sum(1))
    return float((w[sel] * res * res).sum()) / sigma_m ** 2


def _row(ephs, eph_index, tx_ms, tx_frac):
    """what CORRECTED FIX makes of a row before it iterates: satellite states, corrected transmit times as offsets from the
    earliest millisecond ms0, the start t0 of the receive time"""
    tx_ms = np.asarray(tx_ms, np.int64)
    d = nav_ref.fold_ms(tx_ms - int(tx_ms[0]))
    ms0 = int(tx_ms[0]) + int(d.min())
    xyz, t = [], []
    for j, k in enumerate(eph_index):
        pos, dt = nav_ref.sat_state(ephs[k], tx_ms[j], tx_frac[j])
        xyz.append(pos[0])
        t.append(float(d[j] - d.min()) * 1e-3 + tx_frac[j] - dt[0])
    xyz, t = np.array(xyz), np.array(t)
    return xyz, t, ms0, t.mean() + 75e-3


def fix_raim(ephs, eph_index, tx_ms, tx_frac, weight, p, rp):
    """One fix with integrity from the USABLE observations of a row.  Returns atm_ref.fix_atm's dict of the solution that is
    output (for EXCLUDED: the final one, `kept` without the excluded observation, `stages` the steps of every stage run of FULL,
    of the winning candidate and of FINAL) plus raim = dict(status, dof, excluded (index among the observations given, or -1),
    n_candidates, stat_full, stat, threshold), full = fix_atm's own result, and candidates = {k: T_k} of the subset solves that
    converged."""
    w = np.asarray(weight, np.float64)
    full = atm_ref.fix_atm(ephs, eph_index, tx_ms, tx_frac, w, p)
    out = dict(full)
    out["full"] = full
    out["candidates"] = {}
    raim = dict(status=NONE, dof=0, excluded=-1, n_candidates=0, stat_full=0.0, stat=0.0, threshold=0.0)
    out["raim"] = raim
    if full["status"] != atm_ref.FIX_OK:
        return out
    xyz, t, ms0, t0 = _row(ephs, eph_index, tx_ms, tx_frac)
    sigma, thr = rp["sigma_m"], rp["threshold"]
    S = np.array(full["kept"], bool)
    T = statistic(xyz, t, w, full["delay"], S, full["xyz"], full["t_rx"], sigma)
    d = int((S & (w > 0)).sum()) - 4
    raim.update(dof=d, stat_full=T, stat=T)
    if d < 1:
        raim["status"] = UNCHECKED
        return out
    raim["threshold"] = thr[d - 1]
    if T <= thr[d - 1]:
        raim["status"] = PASS
        return out
    raim["status"] = FAILED
    if not rp["exclude"] or d < 2:
        return out
    # EXCLUDE: every subset from the full solution's state, its delays held
    bias0 = C * (t0 - full["t_rx"])
    best = None
    for k in range(len(w)):
        if not (S[k] and w[k] > 0):
            continue
        sub = S.copy()
        sub[k] = False
        st = atm_ref.solve_from(xyz[sub], t[sub], w[sub], full["delay"][sub], t0, full["xyz"], bias0)
        if not st["ok"]:
            continue
        Tk = statistic(xyz, t, w, full["delay"], sub, st["pos"], t0 - st["bias"] / C, sigma)
        if not math.isfinite(Tk):
            continue
        out["candidates"][k] = Tk
        if best is None or Tk < best[0]:
            best = (Tk, k, sub, st)
    raim["n_candidates"] = len(out["candidates"])
    if best is None or best[0] > thr[d - 2]:
        return out
    # FINAL: the rounds over S \ {k} from the winner's state
    Tk, k, sub, st = best
    pos, bias, rms = st["pos"], st["bias"], st["rms"]
    stages = list(full["stages"]) + [st["iterations"]]
    delay = np.array(full["delay"], np.float64)
    t_rx = t0 - bias / C
    if not (p["flags"] == 0 and full["n_masked"] == 0):
        for _ in range(atm_ref.ROUNDS):
            v = atm_ref.views(pos, atm_ref.turned(xyz, t, t_rx), (ms0 % WEEK_MS) * 1e-3 + t_rx, p)
            delay = v["iono"] + v["tropo"]
            st = atm_ref.solve_from(xyz[sub], t[sub], w[sub], delay[sub], t0, pos, bias)
            stages.append(st["iterations"])
            if not st["ok"]:
                out.update(status=atm_ref.FIX_NO_CONVERGE, n_used=int(sub.sum()), kept=sub, iterations=sum(stages), stages=stages)
                out["raim"] = dict(status=NONE, dof=0, excluded=k, n_candidates=0, stat_full=0.0, stat=0.0, threshold=0.0)
                return out
            pos, bias, rms = st["pos"], st["bias"], st["rms"]
            t_rx = t0 - bias / C
    ms, frac = nav_ref.split_time(ms0, t_rx)
    sat = atm_ref.turned(xyz, t, t_rx)
    out.update(n_used=int(sub.sum()), kept=sub, iterations=sum(stages), stages=stages, xyz=pos, rx_ms=int(ms), rx_frac=float(frac), t_rx=t_rx,
               rms=rms, lla=atm_ref.geodetic(pos), sat=sat, delay=delay, dop=atm_ref.dops(pos, sat[sub & (w > 0)]))
    raim.update(status=EXCLUDED, dof=d - 1, excluded=k, stat=statistic(xyz, t, w, delay, sub, pos, t_rx, sigma), threshold=thr[d - 2])
    return out
