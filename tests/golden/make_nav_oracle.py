#!/usr/bin/env python3
"""Generate tests/golden/nav_oracle.npz: ephemerides over the whole field ranges of IS-GPS-200, receiver sites, and what
tests/nav_oracle.py (the header's model in mpmath, 40 digits) says about them.  Seeded and deterministic: a second run writes the
same bytes (tests/test_nav_oracle.py checks that).  Needs mpmath; the tests that read the file need only numpy.

    python tests/golden/make_nav_oracle.py

Every oracle value is stored as the double nearest to it.  Every input the library gets (ephemeris fields, (ms, frac) times, site
coordinates) is a double or an integer stored exactly, and the oracle is evaluated on those very numbers.

Contents (N_EPH = 32, N_SITE = 13, N_FIX_SITE = 11):
  eph_fields [25], eph [32][25]        field names (nav_ref.FIELDS order) and values, quantised by nav_ref.quantise
  state_*  [384]                       eph index, tx_ms, tx_frac -> pos [3], clock, vel [3], drift, E (eccentric anomaly mod 2 pi
                                       in (-pi, pi], for the test's own census), tk; and clock_no_af2 / clock_toc_toe, the clock
                                       correction with a_f2 = 0 and with t_oc = t_oe (the sensitivity preconditions)
  site_xyz [13][3], site_lla [13][3]   ECEF doubles and the oracle's geodetic of exactly those
  atm_alpha / atm_beta [4][4], atm_flags [4]   the four parameter sets
  view_rx_ms / view_rx_frac [13][6], view_tx_ms / view_tx_frac [13][6][12]   receive times and vacuum observations of eph 0..11
  view_out [4][13][6][12][4]           az, el, iono_m, tropo_m per parameter set
  view_excl [4][13][6][12]             bit 0: |el| <= 1e-9; bit 1: el > 0, ionosphere on and ||x| - 1.57| <= 1e-9; bit 2: hypot(e,
                                       n) < 1e-6 of the range (the azimuth is not compared)
  census_names [12], census [4][12]    counts per parameter set over the cases with a delay computed
  fix_site [11], fix_eph [11][12][25], fix_ref_ms / fix_t_rx [11][8]   a constellation and 8 receive instants per site
  fix_vac_ms / fix_vac_frac, fix_atm_ms / fix_atm_frac [11][8][12]     exact observations in vacuum / through set 0's atmosphere
  fix_el [11][8][12], fix_pdop [11][8]  the oracle's elevations (radians) and the PDOP over those at or above the 5-degree mask
  vel_site [2] (rows of fix_site), vel_enu [2][3], vel_ecef [2][3], vel_drift [2], vel_doppler [2][8][12]
                                       Dopplers of a moving receiver with a drifting clock by a central difference of the oracle's
                                       truth_tx over +-0.05 s of receiver time (tests/test_gpu_velocity.py's recipe)

Inputs moved on purpose, and why.  The troposphere is zen / sin(el): its slope in el is 2.4 / sin^2(el) m / rad, 8e7 m / rad at
0.01 degrees, where the 1e-15 rad of fp64 rounding on 2.6e7-m coordinates alone is 8e-8 m, a hundred times DELAY_TOL.  At 3 degrees
the slope is 880 m / rad and 2e-14 rad (a 4e-7-m satellite position) costs 2e-11 m.  So a view row's receive time is stepped on by
97 s until none of its twelve satellites stands between -0.1 and 3.1 degrees.  The azimuth is atan2(e, n): a satellite position good
to 4e-7 m of 2e7 (2e-14 rad) gives 2e-14 / cos(el) rad of azimuth, 1.5e-13 at 83 degrees, above a tenth of ANGLE_TOL; at 70 degrees it
is 6e-14.  So the row is stepped on as well while a satellite stands more than 70 degrees above or below the horizon.  The two rows
at the week's end must stay within a minute of it: SEED is the first one with which they need no step at any site.  The fix cases are redrawn until PDOP < 6, every
elevation keeps 1 degree from the 5-degree mask and every used satellite's |x| keeps 1e-3 from 1.57 at all eight instants.
"""
import io
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import nav_oracle as orc  # noqa: E402
import nav_ref  # noqa: E402
from mpmath import mp, mpf  # noqa: E402

PATH = os.path.join(HERE, "nav_oracle.npz")
SEED = 20819   # the first from 20260 on with which no site's two rows at the week's end need a step (see below)
FIELDS = list(nav_ref.FIELDS)
N_EPH, N_TIMES, N_VIEW_TIMES, N_VIEW_SATS, N_FIX_TIMES = 32, 12, 6, 12, 8
H_FD = 0.05
L1 = mpf("1575.42e6")
MASK = math.radians(5.0)
CENSUS = ("day", "night", "amp_clamped", "amp_free", "per_clamped_amp", "phi_hi", "phi_lo", "phi_free", "t_below", "t_above", "h_clamped",
          "tropo_off")

# alpha / beta codes (field units): the project's default; AMP negative for part of the phi_m range (3.7e-9 + 3e-8 phi_m - ...);
# alpha0 > 0 with PER = 69632 + 32768 phi_m - ... on both sides of 72000; the default with the ionosphere only
ATM_SETS = (((20, 2, -1, -2), (55, 4, -2, -6), 3), ((4, 4, -1, -2), (55, 4, -2, -6), 3), ((20, 2, -1, -2), (34, 2, -1, -1), 3),
            ((20, 2, -1, -2), (55, 4, -2, -6), 1))
ALPHA_EXP, BETA_EXP = (-30, -27, -24, -24), (11, 14, 16, 16)


def atm_sets():
    return [dict(alpha=[math.ldexp(float(c), e) for c, e in zip(a, ALPHA_EXP)], beta=[math.ldexp(float(c), e) for c, e in zip(b, BETA_EXP)], flags=f)
            for a, b, f in ATM_SETS]


def field_range(name):
    _, pieces, signed, exp2, _ = nav_ref.FIELDS[name]
    w = sum(n for _, n in pieces)
    lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
    return math.ldexp(lo, exp2), math.ldexp(hi, exp2)


def draw_eph(rng, k, t_oe, t_oc):
    """every field uniform over its range (the clock terms over their whole fields), then quantised"""
    u = rng.uniform
    eph = dict(week=597, iodc=0x100 | (k + 1), iode2=k + 1, iode3=k + 1, t_oc=int(t_oc), t_oe=int(t_oe),
               t_gd=u(*field_range("t_gd")), a_f0=u(*field_range("a_f0")), a_f1=u(*field_range("a_f1")), a_f2=u(*field_range("a_f2")),
               sqrt_a=u(5100.0, 5200.0), e=u(0.0, 0.03), i_0=u(0.87, 1.05),
               omega_0=u(-math.pi, math.pi), m_0=u(-math.pi, math.pi), omega=u(-math.pi, math.pi),
               dn=u(-1e-8, 1e-8), omega_dot=u(-1e-8, -6e-9), idot=u(-9e-10, 9e-10),
               c_rs=u(-400, 400), c_rc=u(-400, 400), c_us=u(-2e-5, 2e-5), c_uc=u(-2e-5, 2e-5), c_is=u(-5e-7, 5e-7), c_ic=u(-5e-7, 5e-7))
    eph = nav_ref.quantise(eph)
    eph["prn"] = k + 1
    return eph


def eph_row(eph):
    return [float(eph[n]) for n in FIELDS]


def draw_epochs(rng):
    t_oe = 16 * int(rng.integers(0, 604800 // 16))
    t_oc = (t_oe + 16 * int(rng.integers(-450, 451))) % 604800
    return t_oe, t_oc


def make_ephemerides(rng):
    ephs = []
    for k in range(N_EPH):
        t_oe, t_oc = draw_epochs(rng)
        if k in (4, 5, 6):  # t_oc - t_oe of -7200, 0, +7200 s, away from the week's ends
            t_oe = 16 * int(rng.integers(1000, 30000))
            t_oc = t_oe + (-7200, 0, 7200)[k - 4]
        if k == 7:
            t_oe = 0
        if k == 8:
            t_oe, t_oc = 604784, 16
        eph = draw_eph(rng, k, t_oe, t_oc)
        if k == 0:
            eph["e"] = 0.0                                   # e code 0
        if k == 1:
            eph["e"] = nav_ref.quantise(dict(eph, e=0.03))["e"]
        if k == 2:
            eph["a_f2"] = nav_ref.value_of("a_f2", -128)
        if k == 3:
            eph["a_f2"] = nav_ref.value_of("a_f2", 127)
        ephs.append(eph)
    return ephs


def _tx_of(eph, tk_ms):
    """tx_ms at tk_ms whole milliseconds from t_oe"""
    return (1000 * int(eph["t_oe"]) + int(tk_ms)) % orc.WEEK_MS


def state_times(rng, eph):
    """12 (tx_ms, tx_frac): six anywhere within 2 h of t_oe, two either side of the instant where the mean anomaly passes 0 or
    +-pi when that lies within 2 h (else two more anywhere), two between 2 and 3.5 days, two a millisecond inside the fold's ends"""
    n = math.sqrt(nav_ref.MU / eph["sqrt_a"] ** 6) + eph["dn"]
    tk = [int(v) for v in rng.integers(-7_200_000, 7_200_001, 6)]
    cross = [t for t in (-eph["m_0"] / n, (math.pi - eph["m_0"]) / n, (-math.pi - eph["m_0"]) / n) if abs(t) < 6800.0]
    if cross:
        c = int(round(cross[0] * 1000))
        tk += [c - 400_000, c + 400_000]   # e <= 0.03 moves E's crossing by less than 0.03 rad = 210 s from M's
    else:
        tk += [int(v) for v in rng.integers(-7_200_000, 7_200_001, 2)]
    tk += [int(rng.integers(172_800_000, 302_400_000)), -int(rng.integers(172_800_000, 302_400_000))]
    tk += [302_400_000 - 1, -302_400_000 + 1]
    frac = rng.uniform(0.0, 1e-3, len(tk))
    return [(_tx_of(eph, t), float(f)) for t, f in zip(tk, frac)]


def make_states(rng, ephs, out):
    rows = []
    for k, eph in enumerate(ephs):
        no_af2, toc_toe = dict(eph, a_f2=0.0), dict(eph, t_oc=eph["t_oe"])
        for ms, frac in state_times(rng, eph):
            p, dt = orc.sat_state(eph, ms, frac)
            v, drift = orc.sat_rate(eph, ms, frac)
            tk0 = orc._since(ms, eph["t_oe"], frac)
            E = orc.eccentric_anomaly(eph, tk0 - dt)
            E = E - 2 * mp.pi * mp.floor((E + mp.pi) / (2 * mp.pi))
            rows.append((k, ms, frac, [float(c) for c in p], float(dt), [float(c) for c in v], float(drift), float(E), float(tk0),
                         float(orc.sat_state(no_af2, ms, frac)[1]), float(orc.sat_state(toc_toe, ms, frac)[1])))
    out["state_eph"] = np.array([r[0] for r in rows], np.int32)
    out["state_tx_ms"] = np.array([r[1] for r in rows], np.int32)
    out["state_tx_frac"] = np.array([r[2] for r in rows], np.float64)
    out["state_pos"] = np.array([r[3] for r in rows], np.float64)
    out["state_clock"] = np.array([r[4] for r in rows], np.float64)
    out["state_vel"] = np.array([r[5] for r in rows], np.float64)
    out["state_drift"] = np.array([r[6] for r in rows], np.float64)
    out["state_E"] = np.array([r[7] for r in rows], np.float64)
    out["state_tk"] = np.array([r[8] for r in rows], np.float64)
    out["state_clock_no_af2"] = np.array([r[9] for r in rows], np.float64)
    out["state_clock_toc_toe"] = np.array([r[10] for r in rows], np.float64)


def make_sites():
    """[13][3] doubles; the last column of the second result says whether the site takes fixes"""
    rad = math.radians
    anti = nav_ref.ecef_of(rad(-17.0), math.pi, 50.0)
    anti[1] = 0.0
    assert anti[0] < 0
    pole = np.array([0.0, 0.0, nav_ref.WGS84_A * math.sqrt(1 - nav_ref.WGS84_E2) + 250.0])
    sites = [nav_ref.ecef_of(rad(47.3), rad(8.5), 100.0), nav_ref.ecef_of(rad(-60.0), rad(170.0), 100.0), nav_ref.ecef_of(0.0, 0.0, 0.0),
             anti, anti + [0.0, 1.0, 0.0], anti + [0.0, -1.0, 0.0],
             nav_ref.ecef_of(rad(89.9), rad(45.0), 2000.0), nav_ref.ecef_of(rad(-89.9), rad(-120.0), 2800.0), pole,
             nav_ref.ecef_of(rad(30.0), rad(-100.0), 9000.0), nav_ref.ecef_of(rad(-10.0), rad(60.0), -50.0),
             nav_ref.ecef_of(rad(47.3), rad(8.5), -150.0), nav_ref.ecef_of(rad(30.0), rad(-100.0), 12000.0)]
    return np.array(sites, np.float64), [k for k in range(13) if k not in (8, 12)]


def rough_elevation(eph, site, lla, rx_ms):
    """elevation (float, good to 0.01 degrees) of a satellite at rx_ms - 75 ms, for the decisions of this file only"""
    s = orc.position(eph, orc._since(rx_ms, eph["t_oe"], -0.075))
    return float(orc.view(lla[0], lla[1], tuple(s[k] - mpf(site[k]) for k in range(3)))[1])


def make_views(rng, ephs, sites, llas, out):
    sets = atm_sets()
    ephs = ephs[:N_VIEW_SATS]
    n_site = len(sites)
    shape = (n_site, N_VIEW_TIMES)
    rx_ms, rx_frac = np.zeros(shape, np.int32), np.zeros(shape)
    tx_ms, tx_frac = np.zeros(shape + (N_VIEW_SATS,), np.int32), np.zeros(shape + (N_VIEW_SATS,))
    view_out = np.zeros((len(sets),) + shape + (N_VIEW_SATS, 4))
    excl = np.zeros((len(sets),) + shape + (N_VIEW_SATS,), np.uint8)
    census = np.zeros((len(sets), len(CENSUS)), np.int32)
    lo, hi, top = math.radians(-0.1), math.radians(3.1), math.radians(70.0)
    for i in range(n_site):
        # 30 s before the week's end, then 20 s, 4 h, ..., 16 h after it
        for j, base in enumerate([orc.WEEK_MS - 30_000] + [20_000 + 14_400_000 * k for k in range(N_VIEW_TIMES - 1)]):
            ms = (base + int(rng.integers(0, 1000))) % orc.WEEK_MS
            frac = float(rng.uniform(0.0, 1e-3))
            for _ in range(200):
                els = [rough_elevation(e, sites[i], llas[i], ms) for e in ephs]
                if not any(lo < el < hi or abs(el) > top for el in els):
                    break
                if j < 2:  # these two stay where they are: every site is seen 30 s before and 20 s after the week's end
                    raise RuntimeError("site %d's row at the week's end would have to move: take another SEED" % i)
                ms = (ms + 97_000) % orc.WEEK_MS
            else:
                raise RuntimeError("no receive time without a satellite on the horizon")
            rx_ms[i, j], rx_frac[i, j] = ms, frac
            for s, eph in enumerate(ephs):
                tx_ms[i, j, s], tx_frac[i, j, s] = orc.split_time(ms, orc.truth_tx(eph, sites[i], ms, frac))
                for a, atm in enumerate(sets):
                    v = orc.sat_view(eph, tx_ms[i, j, s], tx_frac[i, j, s], sites[i], ms, frac, atm)
                    view_out[a, i, j, s] = [float(v["az"]), float(v["el"]), float(v["iono"]), float(v["tropo"])]
                    ci, ct = v["iono_census"], v["tropo_census"]
                    flag = 1 if abs(v["el"]) <= mpf("1e-9") else 0
                    if ci is not None and abs(abs(ci["x"]) - mpf("1.57")) <= mpf("1e-9"):
                        flag |= 2
                    if v["horiz"] < mpf("1e-6"):
                        flag |= 4
                    excl[a, i, j, s] = flag
                    if ci is not None:
                        hits = dict(day=ci["day"], night=not ci["day"], amp_clamped=ci["amp_clamped"], amp_free=not ci["amp_clamped"],
                                    per_clamped_amp=ci["per_clamped_amp"], phi_hi=ci["phi_hi"], phi_lo=ci["phi_lo"],
                                    phi_free=not (ci["phi_hi"] or ci["phi_lo"]), t_below=ci["t_below"], t_above=ci["t_above"])
                        for name, hit in hits.items():
                            census[a, CENSUS.index(name)] += bool(hit)
                    if ct is not None:
                        census[a, CENSUS.index("h_clamped")] += ct["h_clamped"]
                        census[a, CENSUS.index("tropo_off")] += ct["off"]
    out.update(view_rx_ms=rx_ms, view_rx_frac=rx_frac, view_tx_ms=tx_ms, view_tx_frac=tx_frac, view_out=view_out, view_excl=excl,
               census=census, census_names=np.array(CENSUS), atm_alpha=np.array([s["alpha"] for s in sets]),
               atm_beta=np.array([s["beta"] for s in sets]), atm_flags=np.array([s["flags"] for s in sets], np.int32))


def pdop_of(rx, sats):
    d = np.asarray(rx, np.float64) - np.asarray(sats, np.float64)
    H = np.concatenate([d / np.sqrt((d * d).sum(1))[:, None], np.ones((len(d), 1))], 1)
    return math.sqrt(np.trace(np.linalg.inv(H.T @ H)[:3, :3]))


def fix_geometry(ephs, site, lla, ref_ms, t_rx, atm):
    """per instant: (elevations [12], PDOP over the satellites at or above the mask, smallest | |x| - 1.57 | among them), from the
    vacuum geometry at the true receive time"""
    out = []
    for ms, t in zip(ref_ms, t_rx):
        el, sat, xs = [], [], []
        for eph in ephs:
            tx = orc.split_time(ms, orc.truth_tx(eph, site, ms, t))
            v = orc.sat_view(eph, tx[0], tx[1], site, ms, t, atm)
            el.append(float(v["el"]))
            s, dt = orc.sat_state(eph, tx[0], tx[1])
            sat.append([float(c) for c in s])   # unturned: the turn is 2e-6 rad, nothing to a PDOP
            xs.append(abs(abs(float(v["iono_census"]["x"])) - 1.57) if v["iono_census"] else 1.0)
        el = np.array(el)
        used = el >= MASK
        out.append((el, pdop_of(site, np.array(sat)[used]) if used.sum() >= 4 else 99.0, min(np.array(xs)[used], default=1.0)))
    return out


def make_fixes(rng, sites, llas, fix_sites, out):
    atm = atm_sets()[0]
    n = len(fix_sites)
    fix_eph = np.zeros((n, 12, len(FIELDS)))
    ref_ms, t_rx = np.zeros((n, N_FIX_TIMES), np.int32), np.zeros((n, N_FIX_TIMES))
    vac_ms, atm_ms = np.zeros((n, N_FIX_TIMES, 12), np.int32), np.zeros((n, N_FIX_TIMES, 12), np.int32)
    vac_frac, atm_frac = np.zeros((n, N_FIX_TIMES, 12)), np.zeros((n, N_FIX_TIMES, 12))
    fix_el, fix_pdop = np.zeros((n, N_FIX_TIMES, 12)), np.zeros((n, N_FIX_TIMES))
    constellations = []
    steps = np.array([0, 1, 2, 1000, 5000, 20_000, 60_000, 120_000])
    for f, i in enumerate(fix_sites):
        site, lla = sites[i], llas[i]
        # the second site's instants straddle the end of the week
        first = orc.WEEK_MS - 30_000 if f == 1 else int(rng.integers(0, orc.WEEK_MS - 200_000))
        ms = (first + steps) % orc.WEEK_MS
        t = rng.uniform(0.0, 1e-3, N_FIX_TIMES)
        for _ in range(50):
            ephs = []
            while len(ephs) < 12:
                k = len(ephs)
                t_oe = (16 * ((first // 1000 + int(rng.integers(-7000, 7001))) // 16)) % 604800
                t_oc = (t_oe + 16 * int(rng.integers(-450, 451))) % 604800
                eph = draw_eph(rng, k, t_oe, t_oc)
                if k < 9 and rough_elevation(eph, site, lla, first) < math.radians(10.0):
                    continue
                ephs.append(eph)
            geo = fix_geometry(ephs, site, lla, ms, t, atm)
            if all(g[1] < 6.0 and np.abs(g[0] - MASK).min() >= math.radians(1.0) and g[2] >= 1e-3 for g in geo):
                break
        else:
            raise RuntimeError("no constellation for site %d" % i)
        constellations.append(ephs)
        fix_eph[f] = [eph_row(e) for e in ephs]
        ref_ms[f], t_rx[f] = ms, t
        for j in range(N_FIX_TIMES):
            fix_el[f, j], fix_pdop[f, j] = geo[j][0], geo[j][1]
            for s, eph in enumerate(ephs):
                vac_ms[f, j, s], vac_frac[f, j, s] = orc.split_time(ms[j], orc.truth_tx(eph, site, ms[j], t[j]))
                atm_ms[f, j, s], atm_frac[f, j, s] = orc.split_time(ms[j], orc.truth_tx(eph, site, ms[j], t[j], atm))
    out.update(fix_site=np.array(fix_sites, np.int32), fix_eph=fix_eph, fix_ref_ms=ref_ms, fix_t_rx=t_rx, fix_vac_ms=vac_ms, fix_vac_frac=vac_frac,
               fix_atm_ms=atm_ms, fix_atm_frac=atm_frac, fix_el=fix_el, fix_pdop=fix_pdop)
    return constellations


def make_dopplers(sites, llas, fix_sites, constellations, out):
    """tests/test_gpu_velocity.py's truth: the receiver passes the site at each instant with ENU velocity venu, its sampling clock
    fast by drift; Doppler = L1 (dt_tx / dt_rx - 1) by a central difference over +-H_FD seconds of RECEIVER time"""
    rows = (0, 3)  # rows of fix_site: the mid-latitude site and the one on the antimeridian
    cases = (((30.0, -20.0, 5.0), 2e-6), ((0.0, 0.0, 0.0), 0.0))
    dop = np.zeros((len(rows), N_FIX_TIMES, 12))
    vecef = np.zeros((len(rows), 3))
    for c, (f, (venu, drift)) in enumerate(zip(rows, cases)):
        i = fix_sites[f]
        lat, lon = llas[i][0], llas[i][1]
        sp, cp, sl, cl = mp.sin(lat), mp.cos(lat), mp.sin(lon), mp.cos(lon)
        ve, vn, vu = (mpf(x) for x in venu)
        v = (-sl * ve - sp * cl * vn + cp * cl * vu, cl * ve - sp * sl * vn + cp * sl * vu, cp * vn + sp * vu)
        vecef[c] = [float(x) for x in v]
        dtrue = mpf(H_FD) / (1 + mpf(drift))
        for j in range(N_FIX_TIMES):
            ms, t = int(out["fix_ref_ms"][f, j]), mpf(float(out["fix_t_rx"][f, j]))
            for s, eph in enumerate(constellations[f]):
                tt = [orc.truth_tx(eph, tuple(mpf(sites[i][k]) + v[k] * sg * dtrue for k in range(3)), ms, t + sg * dtrue) for sg in (-1, 1)]
                dop[c, j, s] = float(L1 * ((tt[1] - tt[0]) / (2 * mpf(H_FD)) - 1))
    out.update(vel_site=np.array(rows, np.int32), vel_enu=np.array([c[0] for c in cases]), vel_ecef=vecef, vel_drift=np.array([c[1] for c in cases]),
               vel_doppler=dop)


def build():
    """every array of the fixture, by name"""
    rng = np.random.default_rng(SEED)
    out = {}
    ephs = make_ephemerides(rng)
    out["eph_fields"] = np.array(FIELDS)
    out["eph"] = np.array([eph_row(e) for e in ephs])
    make_states(rng, ephs, out)
    sites, fix_sites = make_sites()
    llas = [orc.geodetic(*s) for s in sites]
    out["site_xyz"] = sites
    out["site_lla"] = np.array([[float(c) for c in lla] for lla in llas])
    make_views(rng, ephs, sites, llas, out)
    constellations = make_fixes(rng, sites, llas, fix_sites, out)
    make_dopplers(sites, llas, fix_sites, constellations, out)
    return out


def to_bytes(arrays):
    """an uncompressed .npz with fixed member times, so that the same arrays always give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


if __name__ == "__main__":
    data = to_bytes(build())
    with open(PATH, "wb") as f:
        f.write(data)
    print("%s: %d bytes" % (PATH, len(data)))
