"""The snapshot chain of include/gpsacq.h ("Coarse-time fixes", "Cold snapshot fixes" 2, "Aided acquisition" A) evaluated in mpmath
at 40 digits: what coarse_ref, coarse_raim_ref, dop_ref, aided_ref and the kernels k_coarse_fix, k_coarse_exclude, k_doppler_fix,
k_aid_predict and k_aid_instant are measured against in tests/test_snapshot_oracle.py and tests/test_gpu_snapshot_oracle.py.

Written from the header's text and IS-GPS-200, not from the *_ref.py files; orbit, geodesy and view are tests/nav_oracle.py's.
Where the kernels iterate or differentiate, this file does something else:

  * the Doppler fix carries each column's light time from pass to pass; here tau = |R(-Omega tau) p(-tau) - place| / c is solved to
    1e-30 s before anything else is evaluated;
  * velocity and clock drift are nav_oracle.sat_rate's central differences, not the analytic rates;
  * the physical Doppler is a central difference of nav_oracle.truth_tx (the light-time equation itself) over receiver time, and
    owes nothing to the header's range-rate equations;
  * the dilutions come from mp.matrix inverses, not from a Cholesky factor;
  * the coarse-time rows take rho from the truth (c times the true travel time), not from an iterated state.
Only where the header DEFINES a truncated iteration is it followed: the two light-time passes of step A and of the prediction.

Only tests/golden/make_snapshot_oracle.py and the CPU test import this file.  Ephemerides are nav_ref's dicts; times are (ms,
frac) pairs, and frac may be any real number of seconds (nav_oracle folds the whole milliseconds only)."""
from mpmath import mp, mpf

import nav_oracle as orc

mp.dps = 40

C, OMEGA_E = orc.C, orc.OMEGA_E
L1 = mpf("1575.42e6")
WEEK_MS = orc.WEEK_MS
EPS = mpf("1e-30")


def _vec(v):
    return tuple(mpf(x) for x in v)


def _sub(a, b):
    return tuple(a[k] - b[k] for k in range(3))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def _spin(p):
    """Omega_e x p"""
    return (-OMEGA_E * p[1], OMEGA_E * p[0], mpf(0))


def _add(a, b):
    return tuple(a[k] + b[k] for k in range(3))


def _pdop(rows, n):
    """(sqrt of the trace of the position block, the whole inverse) of (H^T H) for rows of n columns"""
    H = mp.matrix([[r[k] for k in range(n)] for r in rows])
    Q = (H.T * H) ** -1
    return mp.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]), Q


# ---- a. the Doppler model ---------------------------------------------------------------------------------------------------------
def doppler_column(eph, place, g, rx_ms):
    """one column of PASS at (place, g) with its light time solved: (doppler_hz that makes res 0, the row h (4), tau)"""
    place = _vec(place)
    tau = mpf("0.075")
    for _ in range(60):
        p = orc.sat_state(eph, rx_ms, -tau)[0]
        new = _norm(_sub(orc.turned(p, -OMEGA_E * tau), place)) / C
        done = abs(new - tau) < EPS
        tau = new
        if done:
            break
    else:
        raise ArithmeticError("light time")
    p = orc.sat_state(eph, rx_ms, -tau)[0]
    v, d = orc.sat_rate(eph, rx_ms, -tau)
    a = -OMEGA_E * tau
    r, vi = orc.turned(p, a), orc.turned(_add(v, _spin(p)), a)
    D = _sub(r, place)
    rng = _norm(D)
    e = tuple(x / rng for x in D)
    w = _sub(vi, _spin(place))
    ew = _dot(e, w)
    pred = (ew + mpf(g)) - C * d
    se = _spin(e)
    h = tuple(-(w[k] - ew * e[k]) / rng + se[k] for k in range(3)) + (mpf(1),)
    return -(L1 / C) * pred, h, tau


def doppler_model(ephs, cols, place, g, rx_ms):
    """(doppler_hz per column of cols, pdop over them, the rows h) at (place, g) and t0 = (rx_ms, 0)"""
    out = [doppler_column(ephs[k], place, g, rx_ms) for k in cols]
    return [o[0] for o in out], _pdop([o[1] for o in out], 4)[0], [o[1] for o in out]


# ---- b. the physical Doppler ------------------------------------------------------------------------------------------------------
H_FD = mpf("0.05")


def physical_doppler(eph, site, ref_ms, t_rx, drift):
    """L1 (d t_tx / d t_rx / (1 + drift) - 1) of a receiver at rest at site whose clock runs fast by drift: truth_tx differenced over
    +-H_FD seconds of RECEIVER time, H_FD / (1 + drift) of true time"""
    dtrue = H_FD / (1 + mpf(drift))
    tt = [orc.truth_tx(eph, site, ref_ms, mpf(t_rx) + sg * dtrue) for sg in (-1, 1)]
    return L1 * ((tt[1] - tt[0]) / (2 * H_FD) - 1)


# ---- c. the coarse-time rows at the truth -----------------------------------------------------------------------------------------
def coarse_row(eph, site, ref_ms, t_rx, tx_ms, tx_frac):
    """step B's h (5) at the truth: the satellite at the uncorrected time (tx_ms, tx_frac), rho = c (receive time - corrected
    transmit time)"""
    site = _vec(site)
    p, cc = orc.sat_state(eph, tx_ms, tx_frac)
    v, d = orc.sat_rate(eph, tx_ms, tx_frac)
    rho = C * (mpf(orc.fold_ms(int(ref_ms) - int(tx_ms))) / 1000 + (mpf(t_rx) - (mpf(tx_frac) - cc)))
    theta = -OMEGA_E * rho / C
    los = _sub(site, orc.turned(p, theta))
    rng = _norm(los)
    u = tuple(x / rng for x in los)
    return u + (mpf(1), -(C * d + _dot(u, orc.turned(v, theta)))), rho - rng


def coarse_dilution(rows):
    """(pdop, cdop) from the 5x5 inverse"""
    pd, Q = _pdop(rows, 5)
    return pd, mp.sqrt(Q[4, 4])


# ---- d. / e. the two light-time passes, the prediction and step A -----------------------------------------------------------------
def two_passes(eph, place, rx_ms, rx_frac):
    """(T = cc - tau', cc, tau') of "Coarse-time fixes" A from place at the instant (rx_ms, rx_frac): two passes, NOT converged"""
    place, rx_frac = _vec(place), mpf(rx_frac)
    tau = mpf("0.075")
    p = orc.sat_state(eph, rx_ms, rx_frac - tau)[0]
    tau = _norm(_sub(orc.turned(p, -OMEGA_E * tau), place)) / C
    p, cc = orc.sat_state(eph, rx_ms, rx_frac - tau)
    tau2 = _norm(_sub(orc.turned(p, -OMEGA_E * tau), place)) / C
    return cc - tau2, cc, tau2


def split(rx_ms, u):
    """FIX's split of rx_ms milliseconds + u seconds: (ms of week, frac as an mpf in [0, 1e-3))"""
    k = int(mp.floor(u * 1000))
    return (int(rx_ms) + k) % WEEK_MS, u - mpf(k) / 1000


def predict(eph, place, rx_ms, rx_frac, fs, step_hz, vel=None):
    """gpsacq_aid_predict's record for one (fix, channel), unrounded: dict(tx_ms, tx_frac, doppler_hz, elev_deg, ca_pos = tx_frac fs,
    lo_pos = doppler_hz / step_hz).  vel: None (at rest) or (vx, vy, vz, drift)"""
    rr, rx_frac = _vec(place), mpf(rx_frac)
    T = two_passes(eph, rr, rx_ms, rx_frac)[0]
    tx_ms, tx_frac = split(rx_ms, rx_frac + T)
    p, cc3 = orc.sat_state(eph, tx_ms, tx_frac)
    v, cd = orc.sat_rate(eph, tx_ms, tx_frac)
    theta = OMEGA_E * (mpf(orc.fold_ms(tx_ms - int(rx_ms))) / 1000 + ((tx_frac - cc3) - rx_frac))
    ri, vi = orc.turned(p, theta), orc.turned(_add(v, _spin(p)), theta)
    D = _sub(ri, rr)
    rng = _norm(D)
    e = tuple(x / rng for x in D)
    vr, drift = ((mpf(0),) * 3, mpf(0)) if vel is None else (_vec(vel[:3]), mpf(vel[3]))
    rho = _dot(e, _sub(vi, _add(vr, _spin(rr)))) + C * drift - C * cd
    doppler = -(L1 / C) * rho
    lat, lon, _ = orc.geodetic(*rr)
    el = orc.view(lat, lon, D)[1] * 180 / mp.pi
    return dict(tx_ms=tx_ms, tx_frac=tx_frac, doppler_hz=doppler, elev_deg=el, ca_pos=tx_frac * mpf(fs), lo_pos=doppler / mpf(step_hz))


def nearbyint(x):
    """to nearest, ties to even"""
    f = mp.floor(x)
    r = x - f
    if r > mpf("0.5") or (r == mpf("0.5") and int(f) % 2):
        return int(f) + 1
    return int(f)


def step_a(ephs, cols, tx_frac, place, rx_ms):
    """step A for the usable columns `cols` (the first is the reference) with code phases tx_frac (one per column of cols) from
    the prior (place, rx_ms): (P, delta, x (unrounded, milliseconds; the reference's is (P_r - f_r) 1e3), N), one entry per column"""
    P = [two_passes(ephs[k], place, rx_ms, 0)[0] for k in cols]
    f = [mpf(float(t)) for t in tx_frac]
    xr = (P[0] - f[0]) * 1000
    Nr = nearbyint(xr)
    delta = mpf(Nr) / 1000 + f[0] - P[0]
    x = [xr] + [(delta + P[j] - f[j]) * 1000 for j in range(1, len(cols))]
    return P, delta, x, [Nr] + [nearbyint(v) for v in x[1:]]
