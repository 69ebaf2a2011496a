"""The fp64 references of the navigation tests (nav_ref, rate_ref, atm_ref) against tests/golden/nav_oracle.npz: the model of
include/gpsacq.h evaluated by tests/nav_oracle.py in mpmath at 40 digits -- Newton for Kepler's equation, central differences for
the rates, atan2(y, x) for the longitude -- over ephemerides drawn from the whole field ranges of IS-GPS-200.

Every case must lie within a TENTH of the project's tolerance, so that what tests/test_gpu_nav_oracle.py measures with the whole
tolerance is the kernel.  Only the project's existing rules exclude a case (|el| <= 1e-9; | |x| - 1.57 | <= 1e-9 for the
ionosphere; the azimuth where hypot(e, n) is below 1e-6 of the range), applied on the oracle's values, counted, at most 2 % per
parameter set.

Measured here (the references against the oracle; pytest -s prints them):
    384 states: position 5.64e-07 m, clock correction 4.34e-19 s, velocity 6.97e-11 m/s, clock drift 8.27e-25 s/s
    geodetic, 13 sites: lat 1.11e-16 rad, lon 2.78e-17 rad, alt 8.17e-10 m
    views, 4 x 936 cases: az 7.59e-14 rad, el 3.16e-14 rad, iono 3.22e-13 m, tropo 5.67e-12 m; none excluded by any rule
    fixes of the oracle's exact observations, 11 sites x 8: plain 3.73e-08 m and 8.41e-17 s, corrected 1.98e-07 m and 5.45e-16 s
    a_f2 = 0 moves 375 of the 384 clock corrections by 1e-10 s or more (at most 3.19e-4 s) and 381 drifts by 1e-13 s/s or more (at
    most 2.13e-9 s/s); t_oc = t_oe moves 372 clock corrections (at most 2.15e-3 s) and 361 drifts (at most 4.26e-9 s/s)
    census over the 347 view cases above the horizon: day 183 / night 164, AMP clamped 0 (162 in set 1), PER clamped with AMP > 0
    253 (set 2), phi_i clamped high 52 / low 25 / not 270, t wrapped from below 56 / from above 98, h clamped 24, troposphere off by
    altitude 53; 589 of the 936 cases of a set are below the horizon; all 13 sites have a row 30 s before and one 20 s after the
    week's end.  The fixture is 260 988 bytes.
"""
import importlib.util
import math
import os

import numpy as np
import pytest

import atm_ref
import nav_ref
import rate_ref
from nav_oracle_data import (ALT_TOL, ANGLE_TOL, CLOCK_TOL, DELAY_TOL, DRIFT_TOL, EXCL_AZ, EXCL_EL, EXCL_X, LATLON_TOL, PATH, POS_TOL, SITE_ANTIMERIDIAN,
                             SITE_POLE, TIME_TOL, VEL_TOL, angle_diff, atm_params, constellation, ephemerides, load)


# ---- 1. the fixture is what its generator writes -----------------------------------------------------------------------------------
def test_fixture_regenerates_byte_for_byte():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_nav_oracle", os.path.join(os.path.dirname(PATH), "make_nav_oracle.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(PATH, "rb") as f:
        committed = f.read()
    assert len(committed) < 300 * 1024
    assert gen.to_bytes(gen.build()) == committed


# ---- 2. what the fixture covers -----------------------------------------------------------------------------------------------------
def test_planted_ephemerides_and_times():
    d, ephs = load(), ephemerides()
    assert len(ephs) == 32 and d["state_eph"].size == 384 and (np.bincount(d["state_eph"]) == 12).all()
    assert ephs[0]["e"] == 0.0 and ephs[1]["e"] == nav_ref.value_of("e", nav_ref.code_of("e", 0.03))
    assert nav_ref.code_of("a_f2", ephs[2]["a_f2"]) == -128 and nav_ref.code_of("a_f2", ephs[3]["a_f2"]) == 127
    assert [ephs[k]["t_oc"] - ephs[k]["t_oe"] for k in (4, 5, 6)] == [-7200, 0, 7200]
    assert ephs[7]["t_oe"] == 0 and (ephs[8]["t_oe"], ephs[8]["t_oc"]) == (604784, 16)
    for eph in ephs:  # every value is a code of its field, and the spread is the whole range
        assert nav_ref.quantise(eph) == eph
    for name, frac in (("a_f2", 0.5), ("a_f1", 0.5), ("a_f0", 0.5), ("t_gd", 0.5), ("e", 0.5)):
        codes = [nav_ref.code_of(name, e[name]) for e in ephs]
        w = nav_ref._width(name)
        span = (1 << w) if name != "e" else nav_ref.code_of("e", 0.03)
        assert max(codes) - min(codes) > frac * span, name
    tk = d["state_tk"].reshape(32, 12)
    assert (np.abs(tk[:, :8]) <= 7200.0).all()
    assert ((np.abs(tk[:, 8:10]) >= 172800.0) & (np.abs(tk[:, 8:10]) <= 302400.0)).all()
    assert (np.abs(tk[:, 10] - 302399.999) < 1.1e-3).all() and (np.abs(tk[:, 11] + 302399.999) < 1.1e-3).all()
    E = d["state_E"].reshape(32, 12)[:, :8]
    census = [int(((E > 0) & (E < 0.1)).sum()), int(((E < 0) & (E > -0.1)).sum()), int((E > math.pi - 0.1).sum()), int((E < -math.pi + 0.1).sum())]
    print("E within 0.1 rad above / below 0, below pi / above -pi: %s" % census)
    assert min(census) >= 3
    # the receive times of the view rows: within a minute of the week's end on either side, then every 4 h
    rx = d["view_rx_ms"].astype(np.int64)
    near = (rx > nav_ref.WEEK_MS - 60_000) | (rx < 60_000)
    print("view rows within a minute of the week's end: %d of %d" % (near.sum(), rx.size))
    assert (rx[:, 0] > nav_ref.WEEK_MS - 60_000).all() and (rx[:, 1] < 60_000).all()  # every site, on both sides of it
    assert len(set((rx // 14_400_000).ravel())) >= 5


def test_sensitivity_preconditions():
    """a_f2 and t_oc each move at least 50 state cases by 1000 x CLOCK_TOL: a kernel without the a_f2 term, or with t_oe for t_oc,
    cannot pass"""
    d = load()
    n_af2 = int((np.abs(d["state_clock"] - d["state_clock_no_af2"]) >= 1000 * CLOCK_TOL).sum())
    n_toc = int((np.abs(d["state_clock"] - d["state_clock_toc_toe"]) >= 1000 * CLOCK_TOL).sum())
    print("state cases moved by 1000 x CLOCK_TOL or more: a_f2 = 0: %d, t_oc = t_oe: %d; largest %.3g s and %.3g s" %
          (n_af2, n_toc, np.abs(d["state_clock"] - d["state_clock_no_af2"]).max(), np.abs(d["state_clock"] - d["state_clock_toc_toe"]).max()))
    assert n_af2 >= 50 and n_toc >= 50
    # the drift: 2 a_f2 t is what the a_f2 term of k_sat_state_rate adds, 2 a_f2 (t - t_k) what t_oe in the place of t_oc would take away
    ephs = ephemerides()
    a_f2 = np.array([ephs[k]["a_f2"] for k in d["state_eph"]])
    toc_ms = np.array([1000 * ephs[k]["t_oc"] for k in d["state_eph"]], np.int64)
    toe_ms = np.array([1000 * ephs[k]["t_oe"] for k in d["state_eph"]], np.int64)
    tc = nav_ref.fold_ms(d["state_tx_ms"].astype(np.int64) - toc_ms) * 1e-3 + d["state_tx_frac"]
    tk = nav_ref.fold_ms(d["state_tx_ms"].astype(np.int64) - toe_ms) * 1e-3 + d["state_tx_frac"]
    d_af2, d_toc = np.abs(2 * a_f2 * tc), np.abs(2 * a_f2 * (tc - tk))
    print("drifts moved by 1000 x DRIFT_TOL or more: a_f2 = 0: %d, t_oc = t_oe: %d; largest %.3g s/s and %.3g s/s" %
          ((d_af2 >= 1000 * DRIFT_TOL).sum(), (d_toc >= 1000 * DRIFT_TOL).sum(), d_af2.max(), d_toc.max()))
    assert (d_af2 >= 1000 * DRIFT_TOL).sum() >= 50 and (d_toc >= 1000 * DRIFT_TOL).sum() >= 50


# which parameter set has to show which branch: the default one the common ones, set 1 the AMP clamp, set 2 the PER clamp
CENSUS_SET = dict(day=0, night=0, amp_free=0, phi_hi=0, phi_lo=0, phi_free=0, t_below=0, t_above=0, h_clamped=0, tropo_off=0, amp_clamped=1,
                  per_clamped_amp=2)


def test_census():
    d = load()
    names = [str(n) for n in d["census_names"]]
    for a in range(4):
        print("set %d: %s" % (a, ", ".join("%s %d" % (n, c) for n, c in zip(names, d["census"][a]))))
    assert sorted(names) == sorted(CENSUS_SET)
    for name, a in CENSUS_SET.items():
        assert d["census"][a][names.index(name)] >= 5, (name, a)
    assert d["census"][1][names.index("amp_free")] >= 5 and d["census"][2][names.index("day")] >= 5  # the clamps are partial
    assert not d["census"][3][names.index("h_clamped")] and not d["census"][3][names.index("tropo_off")]  # ionosphere only
    el = d["view_out"][..., 1]
    print("view cases below the horizon: %d of %d" % ((el[0] <= 0).sum(), el[0].size))
    assert (el[0] <= 0).sum() >= 100 and (el[0] > 0).sum() >= 100
    for a in range(4):
        n = d["view_excl"][a].size
        counts = [int(((d["view_excl"][a] & bit) != 0).sum()) for bit in (EXCL_EL, EXCL_X, EXCL_AZ)]
        print("set %d: excluded by |el|, |x|, azimuth: %s of %d" % (a, counts, n))
        assert max(counts) <= 0.02 * n


# ---- 3. the references against the oracle ------------------------------------------------------------------------------------------
def test_nav_ref_and_rate_ref_against_the_oracle():
    d, ephs = load(), ephemerides()
    worst = np.zeros(4)
    for k, eph in enumerate(ephs):
        sel = d["state_eph"] == k
        pos, dt = nav_ref.sat_state(eph, d["state_tx_ms"][sel], d["state_tx_frac"][sel])
        vel, drift = rate_ref.sat_rate(eph, d["state_tx_ms"][sel], d["state_tx_frac"][sel])
        worst = np.maximum(worst, [np.abs(pos - d["state_pos"][sel]).max(), np.abs(dt - d["state_clock"][sel]).max(),
                                   np.abs(vel - d["state_vel"][sel]).max(), np.abs(drift - d["state_drift"][sel]).max()])
    print("references against the oracle, 384 states: position %.3g m, clock %.3g s, velocity %.3g m/s, drift %.3g s/s" % tuple(worst))
    assert worst[0] <= POS_TOL / 10 and worst[1] <= CLOCK_TOL / 10 and worst[2] <= VEL_TOL / 10 and worst[3] <= DRIFT_TOL / 10


def test_geodetic_against_the_oracle():
    d = load()
    worst = np.zeros(3)
    for xyz, lla in zip(d["site_xyz"], d["site_lla"]):
        got = atm_ref.geodetic(xyz)
        worst = np.maximum(worst, [abs(got[0] - lla[0]), abs(got[1] - lla[1]), abs(got[2] - lla[2])])
    print("atm_ref.geodetic against the oracle, %d sites: lat %.3g rad, lon %.3g rad, alt %.3g m" % ((len(d["site_xyz"]),) + tuple(worst)))
    assert worst[0] <= LATLON_TOL / 10 and worst[1] <= LATLON_TOL / 10 and worst[2] <= ALT_TOL / 10


def test_antimeridian():
    d = load()
    x, y, z = d["site_xyz"][SITE_ANTIMERIDIAN]
    assert y == 0.0 and x < 0
    assert atm_ref.geodetic((x, y, z))[1] == math.pi == d["site_lla"][SITE_ANTIMERIDIAN][1]
    assert atm_ref.geodetic((x, -0.0, z))[1] == math.pi  # (-pi, pi]: the sign of a zero is not a side
    assert d["site_lla"][SITE_ANTIMERIDIAN + 1][1] > 3.14159 and d["site_lla"][SITE_ANTIMERIDIAN + 2][1] < -3.14159  # y = +-1 m
    assert d["site_lla"][SITE_POLE][1] == 0.0 and d["site_lla"][SITE_POLE][0] == math.pi / 2  # the header's axis rule


def test_views_against_the_oracle():
    d, ephs = load(), ephemerides()
    worst = np.zeros((4, 4))
    n_site, n_time, n_sat = d["view_tx_ms"].shape
    for i in range(n_site):
        rx = d["site_xyz"][i]
        for j in range(n_time):
            rx_ms, rx_frac = int(d["view_rx_ms"][i, j]), float(d["view_rx_frac"][i, j])
            tow = rx_ms * 1e-3 + rx_frac
            sat = []
            for s in range(n_sat):
                pos, dt = nav_ref.sat_state(ephs[s], d["view_tx_ms"][i, j, s], d["view_tx_frac"][i, j, s])
                dtx = float(nav_ref.fold_ms(int(d["view_tx_ms"][i, j, s]) - rx_ms)) * 1e-3 + ((d["view_tx_frac"][i, j, s] - dt[0]) - rx_frac)
                sat.append(atm_ref.turned(pos[0], dtx, 0.0))
            for a in range(4):
                v = atm_ref.views(rx, np.array(sat), tow, atm_params(a))
                ref, ex = d["view_out"][a, i, j], d["view_excl"][a, i, j]
                keep = (ex & EXCL_EL) == 0
                err = np.stack([np.where(ex & EXCL_AZ, 0.0, angle_diff(v["az"], ref[:, 0])), np.abs(v["el"] - ref[:, 1]),
                                np.where(ex & EXCL_X, 0.0, np.abs(v["iono"] - ref[:, 2])), np.abs(v["tropo"] - ref[:, 3])])
                worst[a] = np.maximum(worst[a], np.where(keep, err, 0.0).max(axis=1))
                assert ((v["iono"] > 0) == (ref[:, 2] > 0))[keep].all() and ((v["tropo"] > 0) == (ref[:, 3] > 0))[keep].all()
    for a in range(4):
        print("atm_ref.views against the oracle, set %d: az %.3g rad, el %.3g rad, iono %.3g m, tropo %.3g m" % ((a,) + tuple(worst[a])))
    assert (worst[:, :2] <= ANGLE_TOL / 10).all() and (worst[:, 2:] <= DELAY_TOL / 10).all()


def test_reference_fixes_recover_the_sites():
    """A tenth of POS_TOL / TIME_TOL, by reasoning: the satellite positions of the references are good to 4e-7 m (above), the
    ranges round at 4e-9 m, PDOP and TDOP are below 6 by the fixture's construction -- 2.4e-6 m and 8e-15 s; Newton's last step
    below 1e-4 m leaves its square; three rounds leave 5e-8 m of the atmosphere (tests/test_atm.py)."""
    d = load()
    p = atm_params(0)
    worst = np.zeros(4)
    for f, i in enumerate(d["fix_site"]):
        ephs, site = constellation(f), d["site_xyz"][i]
        for j in range(d["fix_ref_ms"].shape[1]):
            ref_ms, t_rx = int(d["fix_ref_ms"][f, j]), float(d["fix_t_rx"][f, j])
            plain = nav_ref.fix(ephs, range(12), d["fix_vac_ms"][f, j], d["fix_vac_frac"][f, j], np.ones(12))
            corr = atm_ref.fix_atm(ephs, range(12), d["fix_atm_ms"][f, j], d["fix_atm_frac"][f, j], np.ones(12), p)
            assert plain["ok"] and corr["status"] == 0, (f, j)
            assert corr["n_masked"] == int((d["fix_el"][f, j] < p["elev_mask"]).sum()) and d["fix_pdop"][f, j] < 6.0
            assert np.abs(d["fix_el"][f, j] - p["elev_mask"]).min() >= math.radians(1.0)
            dt = [abs(float(nav_ref.fold_ms(o["rx_ms"] - ref_ms)) * 1e-3 + (o["rx_frac"] - t_rx)) for o in (plain, corr)]
            worst = np.maximum(worst, [np.abs(plain["xyz"] - site).max(), dt[0], np.abs(corr["xyz"] - site).max(), dt[1]])
    print("reference fixes of the oracle's observations, %d sites x %d: plain %.3g m, %.3g s; corrected %.3g m, %.3g s" %
          ((len(d["fix_site"]), d["fix_ref_ms"].shape[1]) + tuple(worst)))
    assert worst[0] <= POS_TOL / 10 and worst[2] <= POS_TOL / 10 and worst[1] <= TIME_TOL / 10 and worst[3] <= TIME_TOL / 10
