"""The navigation model of include/gpsacq.h evaluated in mpmath at 40 digits: what the fp64 references (nav_ref, rate_ref,
atm_ref) and the fp64 kernels are measured against in tests/test_nav_oracle.py and tests/test_gpu_nav_oracle.py.

Written from the header's text and IS-GPS-200 (Table 20-IV, Figure 20-4), not from the references.  Where the kernels solve or
differentiate, this file does something else:

  * Kepler's equation by Newton to 1e-35 (the header's fixed point stops at a step of 1e-12: its root is off by at most
    e / (1 - e) 1e-12 rad = 8e-7 m at 2.66e7 m);
  * velocity as a central difference, h = 1e-8 s, of the Table 20-IV position in the corrected time t_k, the clock correction
    held (the header's definition); drift as a central difference of the clock correction in the uncorrected time;
  * lon = atan2(y, x) in (-pi, pi]; lat and alt iterated to 1e-30;
  * the light-time equation solved to 1e-30 s, the clock correction inverted to the same.

Only tests/golden/make_nav_oracle.py and the CPU test import this file (mpmath need not be present where the GPU tests run).
Ephemerides are nav_ref's dicts (floats: every one is taken exactly).  Times are (ms, frac) pairs as in the library.
"""
from mpmath import mp, mpf

mp.dps = 40

MU = mpf("3.986005e14")
OMEGA_E = mpf("7.2921151467e-5")
C = mpf("2.99792458e8")
F_REL = mpf("-4.442807633e-10")
WGS84_A = mpf(6378137)
WGS84_E2 = mpf("0.00669437999014132")
WEEK_MS = 604800000
ATM_IONO, ATM_TROPO = 1, 2
H_RATE = mpf("1e-8")


def fold_ms(d):
    d = int(d)
    if d > WEEK_MS // 2:
        return d - WEEK_MS
    if d < -WEEK_MS // 2:
        return d + WEEK_MS
    return d


def _since(ms, epoch_s, frac):
    """seconds from an epoch (whole seconds of week) to (ms, frac), the millisecond difference folded"""
    return mpf(fold_ms(int(ms) - 1000 * int(epoch_s))) / 1000 + mpf(frac)


def eccentric_anomaly(eph, tk):
    A = mpf(eph["sqrt_a"]) ** 2
    n = mp.sqrt(MU / A ** 3) + mpf(eph["dn"])
    M = mpf(eph["m_0"]) + n * tk
    e = mpf(eph["e"])
    E = M
    for _ in range(200):
        step = (E - e * mp.sin(E) - M) / (1 - e * mp.cos(E))
        E -= step
        if abs(step) < mpf("1e-35"):
            return E
    raise ArithmeticError("Kepler")


def clock_correction(eph, tk, tc):
    return (mpf(eph["a_f0"]) + mpf(eph["a_f1"]) * tc + mpf(eph["a_f2"]) * tc * tc
            + F_REL * mpf(eph["e"]) * mpf(eph["sqrt_a"]) * mp.sin(eccentric_anomaly(eph, tk)) - mpf(eph["t_gd"]))


def position(eph, tk):
    """IS-GPS-200 Table 20-IV at tk seconds of GPS time from t_oe: ECEF at that time"""
    A = mpf(eph["sqrt_a"]) ** 2
    e = mpf(eph["e"])
    E = eccentric_anomaly(eph, tk)
    nu = mp.atan2(mp.sqrt(1 - e * e) * mp.sin(E), mp.cos(E) - e)
    phi = nu + mpf(eph["omega"])
    s2, c2 = mp.sin(2 * phi), mp.cos(2 * phi)
    u = phi + mpf(eph["c_us"]) * s2 + mpf(eph["c_uc"]) * c2
    r = A * (1 - e * mp.cos(E)) + mpf(eph["c_rs"]) * s2 + mpf(eph["c_rc"]) * c2
    inc = mpf(eph["i_0"]) + mpf(eph["c_is"]) * s2 + mpf(eph["c_ic"]) * c2 + mpf(eph["idot"]) * tk
    om = mpf(eph["omega_0"]) + (mpf(eph["omega_dot"]) - OMEGA_E) * tk - OMEGA_E * int(eph["t_oe"])
    xp, yp = r * mp.cos(u), r * mp.sin(u)
    return (xp * mp.cos(om) - yp * mp.cos(inc) * mp.sin(om), xp * mp.sin(om) + yp * mp.cos(inc) * mp.cos(om), yp * mp.sin(inc))


def sat_state(eph, tx_ms, tx_frac):
    """((x, y, z), clock_corr) at the UNCORRECTED satellite time (tx_ms, tx_frac)"""
    tk0 = _since(tx_ms, eph["t_oe"], tx_frac)
    tc = _since(tx_ms, eph["t_oc"], tx_frac)
    dt = clock_correction(eph, tk0, tc)
    return position(eph, tk0 - dt), dt


def sat_rate(eph, tx_ms, tx_frac):
    """((vx, vy, vz), clock_drift): the position's derivative in the corrected time with the clock correction held, and the clock
    correction's derivative in the uncorrected time, both by central differences"""
    tk0 = _since(tx_ms, eph["t_oe"], tx_frac)
    tc = _since(tx_ms, eph["t_oc"], tx_frac)
    tk = tk0 - clock_correction(eph, tk0, tc)
    a, b = position(eph, tk - H_RATE), position(eph, tk + H_RATE)
    v = tuple((b[k] - a[k]) / (2 * H_RATE) for k in range(3))
    drift = (clock_correction(eph, tk0 + H_RATE, tc + H_RATE) - clock_correction(eph, tk0 - H_RATE, tc - H_RATE)) / (2 * H_RATE)
    return v, drift


# ---- geodesy and view -----------------------------------------------------------------------------------------------------
def ecef_of(lat, lon, alt):
    lat, lon, alt = mpf(lat), mpf(lon), mpf(alt)
    N = WGS84_A / mp.sqrt(1 - WGS84_E2 * mp.sin(lat) ** 2)
    return ((N + alt) * mp.cos(lat) * mp.cos(lon), (N + alt) * mp.cos(lat) * mp.sin(lon), (N * (1 - WGS84_E2) + alt) * mp.sin(lat))


def geodetic(x, y, z):
    """(lat, lon, alt) on WGS-84; on the axis (sqrt(x^2 + y^2) <= 1e-6) the header's rule"""
    x, y, z = mpf(x), mpf(y), mpf(z)
    p = mp.sqrt(x * x + y * y)
    if not p > mpf("1e-6"):
        return (-mp.pi / 2 if z < 0 else mp.pi / 2), mpf(0), abs(z) - WGS84_A * mp.sqrt(1 - WGS84_E2)
    lon = mp.atan2(y, x)
    lat = mp.atan(z / (p * (1 - WGS84_E2)))
    alt = mpf(0)
    for _ in range(200):
        N = WGS84_A / mp.sqrt(1 - WGS84_E2 * mp.sin(lat) ** 2)
        new_alt = p / mp.cos(lat) - N
        new_lat = mp.atan(z / (p * (1 - WGS84_E2 * N / (N + new_alt))))
        done = abs(new_alt - alt) < mpf("1e-30") and abs(new_lat - lat) < mpf("1e-30")
        lat, alt = new_lat, new_alt
        if done:
            return lat, lon, alt
    raise ArithmeticError("geodetic")


def turned(s, theta):
    c, sn = mp.cos(theta), mp.sin(theta)
    return (s[0] * c - s[1] * sn, s[0] * sn + s[1] * c, s[2])


def view(lat, lon, d):
    """(az, el, hypot(e, n)) of d = satellite - receiver in the local frame at (lat, lon)"""
    sp, cp, sl, cl = mp.sin(lat), mp.cos(lat), mp.sin(lon), mp.cos(lon)
    e = -sl * d[0] + cl * d[1]
    n = -sp * cl * d[0] - sp * sl * d[1] + cp * d[2]
    u = cp * cl * d[0] + cp * sl * d[1] + sp * d[2]
    h = mp.hypot(e, n)
    return mp.atan2(e, n), mp.atan2(u, h), h


def klobuchar(az, el, lat, lon, tow, atm):
    """(iono_m, census dict): IS-GPS-200 Figure 20-4 as the header writes it; the census names the branches taken"""
    if not atm["flags"] & ATM_IONO or not el > 0:
        return mpf(0), None
    E, phi_u, lam_u = el / mp.pi, lat / mp.pi, lon / mp.pi
    psi = mpf("0.0137") / (E + mpf("0.11")) - mpf("0.022")
    raw = phi_u + psi * mp.cos(az)
    lim = mpf("0.416")
    phi_i = lim if raw > lim else -lim if raw < -lim else raw
    lam_i = lam_u + psi * mp.sin(az) / mp.cos(phi_i * mp.pi)
    phi_m = phi_i + mpf("0.064") * mp.cos((lam_i - mpf("1.617")) * mp.pi)
    t_raw = 43200 * lam_i + mpf(tow)
    t = t_raw - 86400 * mp.floor(t_raw / 86400)
    F = 1 + 16 * (mpf("0.53") - E) ** 3
    a, b = [mpf(v) for v in atm["alpha"]], [mpf(v) for v in atm["beta"]]
    amp_raw = ((a[3] * phi_m + a[2]) * phi_m + a[1]) * phi_m + a[0]
    per_raw = ((b[3] * phi_m + b[2]) * phi_m + b[1]) * phi_m + b[0]
    amp = amp_raw if amp_raw > 0 else mpf(0)
    per = per_raw if per_raw > 72000 else mpf(72000)
    x = 2 * mp.pi * (t - 50400) / per
    day = abs(x) < mpf("1.57")
    out = C * F * (mpf("5e-9") + amp * (1 - x * x / 2 + x ** 4 / 24)) if day else C * F * mpf("5e-9")
    census = dict(day=bool(day), amp_clamped=bool(amp_raw < 0), per_clamped_amp=bool(per_raw < 72000 and amp_raw > 0),
                  phi_hi=bool(raw > lim), phi_lo=bool(raw < -lim), t_below=bool(t_raw < 0), t_above=bool(t_raw >= 86400), x=x)
    return out, census


def saastamoinen(el, lat, alt, atm):
    """(tropo_m, census dict or None)"""
    if not atm["flags"] & ATM_TROPO or not el > 0:
        return mpf(0), None
    if alt < -100 or alt > 10000:
        return mpf(0), dict(h_clamped=False, off=True)
    h = alt if alt > 0 else mpf(0)
    P = mpf("1013.25") * (1 - mpf("2.2557e-5") * h) ** mpf("5.2568")
    T = mpf("288.16") - mpf("6.5e-3") * h
    e = mpf("6.108") * mpf("0.7") * mp.exp((mpf("17.15") * T - 4684) / (T - mpf("38.45")))
    zen = mpf("0.0022768") * P / (1 - mpf("0.00266") * mp.cos(2 * lat) - mpf("0.00028") * h / 1000) + mpf("0.002277") * (1255 / T + mpf("0.05")) * e
    return zen / mp.sin(el), dict(h_clamped=bool(alt < 0), off=False)


def sat_view(eph, tx_ms, tx_frac, rx_xyz, rx_ms, rx_frac, atm):
    """VIEW of one observation from a receiver at rx_xyz at receive time (rx_ms, rx_frac): dict(az, el, iono, tropo, horiz (hypot(e,
    n) over the range), x (Klobuchar's phase or None), census)"""
    s, dt = sat_state(eph, tx_ms, tx_frac)
    theta = OMEGA_E * (mpf(fold_ms(int(tx_ms) - int(rx_ms))) / 1000 + (mpf(tx_frac) - dt - mpf(rx_frac)))
    s = turned(s, theta)
    r = tuple(mpf(v) for v in rx_xyz)
    lat, lon, alt = geodetic(*r)
    d = tuple(s[k] - r[k] for k in range(3))
    az, el, h = view(lat, lon, d)
    tow = mpf(int(rx_ms)) / 1000 + mpf(rx_frac)
    iono, ci = klobuchar(az, el, lat, lon, tow, atm)
    tropo, ct = saastamoinen(el, lat, alt, atm)
    return dict(az=az, el=el, iono=iono, tropo=tropo, horiz=h / mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2), iono_census=ci, tropo_census=ct)


# ---- truth maker ---------------------------------------------------------------------------------------------------------
def truth_tx(eph, rx_xyz, ref_ms, t_rx, atm=None):
    """The uncorrected satellite time, as an offset in seconds from the millisecond ref_ms, that a receiver at rx_xyz reads off
    its replica at receive time ref_ms + t_rx: |R(theta) sat(t_tx) - rx| + D = c (t_rx - t_tx), theta = Omega_e (t_tx - t_rx), D the
    delays of the model (atm) at the true position and receive time or 0; then t_sv - clock_corr(t_sv) = t_tx."""
    r = tuple(mpf(v) for v in rx_xyz)
    t_rx = mpf(t_rx)
    bk = mpf(fold_ms(int(ref_ms) - 1000 * int(eph["t_oe"]))) / 1000
    bc = mpf(fold_ms(int(ref_ms) - 1000 * int(eph["t_oc"]))) / 1000
    if atm is not None:
        lat, lon, alt = geodetic(*r)
        tow = mpf(int(ref_ms) % WEEK_MS) / 1000 + t_rx
    eps = mpf("1e-30")
    t_tx = t_rx - mpf("0.075")
    for _ in range(40):
        s = turned(position(eph, bk + t_tx), OMEGA_E * (t_tx - t_rx))
        d = tuple(s[k] - r[k] for k in range(3))
        rng = mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
        if atm is not None:
            az, el, _ = view(lat, lon, d)
            rng += klobuchar(az, el, lat, lon, tow, atm)[0] + saastamoinen(el, lat, alt, atm)[0]
        new = t_rx - rng / C
        done = abs(new - t_tx) < eps
        t_tx = new
        if done:
            break
    else:
        raise ArithmeticError("light time")
    t_sv = t_tx
    for _ in range(40):
        new = t_tx + clock_correction(eph, bk + t_sv, bc + t_sv)
        done = abs(new - t_sv) < eps
        t_sv = new
        if done:
            return t_sv
    raise ArithmeticError("clock inversion")


def split_time(ref_ms, off):
    """(ms of week, frac in [0, 1e-3) as the nearest double) of ref_ms + off seconds"""
    k = int(mp.floor(off * 1000))
    frac = float(off - mpf(k) / 1000)
    if frac >= 1e-3:  # rounded up to the next millisecond
        k, frac = k + 1, 0.0
    return (int(ref_ms) + k) % WEEK_MS, frac
