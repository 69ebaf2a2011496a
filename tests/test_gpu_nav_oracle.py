"""The fp64 navigation kernels (k_sat_state, k_sat_state_rate, k_sat_view, k_fix, k_fix_atm, k_vel and the RAIM pair) against
tests/golden/nav_oracle.npz: the model of include/gpsacq.h evaluated to 40 digits by tests/nav_oracle.py -- Newton for Kepler's
equation, central differences for the rates, atan2(y, x) for the longitude, the light-time equation solved to 1e-30 s -- over 32
ephemerides drawn from the whole field ranges of IS-GPS-200 (a_f2 over its 8 bits, t_oc up to 2 h from t_oe, e from 0 to 0.03, t_k
out to the fold at 3.5 days, epochs on both sides of the week's end), 13 sites (the antimeridian with y == 0 and y = +-1 m, both
poles' neighbourhood, the axis, -150 m to 12 km) and four sets of Klobuchar coefficients.  Only numpy reads the fixture here.

The tolerances are the project's, unchanged (tests/nav_oracle_data.py); tests/test_nav_oracle.py shows the fp64 references a
hundred times inside them against the same oracle, so what is measured here is the kernel.  The same file holds the fixture's
preconditions (what a_f2 and t_oc move, the census of Klobuchar's branches, the excluded cases: none).

Which case catches which slip (each checked once by making the slip in a CPU copy of the arithmetic, tests/nav_ref.py and
atm_ref.py, and running that against the fixture; the counts are asserted in tests/test_nav_oracle.py):
    a_f2 term of k_sat_state          test_states: 375 of 384 clocks move by 1e-10 s or more (largest 3.2e-4 s)
    a_f2 term of k_sat_state_rate     test_rates: 381 of 384 drifts move by 1e-13 s/s or more (2 a_f2 t, largest 2.1e-9)
    toc_ms -> toe_ms, either kernel   test_states / test_rates: 372 of 384 clocks move by 1e-10 s or more (largest 2.2e-3 s); the
                                      drift in 361 cases by 1e-13 s/s or more (largest 4.3e-9: t folds elsewhere at the week's ends)
    the PER clamp                     test_views, set 2: 253 cases with PER below 72000 and AMP > 0
    lon on the antimeridian           test_views (site 3, y == 0: every azimuth turns by pi; sites 4 and 5, y = +-1 m: 1.2e-11 rad
                                      of lon from the cancelling sum, 3e-12 rad of azimuth), test_geodetic_of_the_fixes

Measured on an MI355X (pytest -s prints them):
    sat_states, 384 observations: position 5.11e-07 m, clock correction 2.17e-19 s (1 / 63..65: 5.59e-08 / 3.44e-07 m)
    sat_rates, 384 observations: velocity 6.35e-11 m/s, clock drift 8.27e-25 s/s
    sat_views, 936 cases per set, none left out: az 7.37e-14 rad, el 2.55e-14 rad, iono 2.1e-13 / 1.42e-13 / 2.03e-13 / 2.1e-13 m
    (sets 0..3), tropo 9.45e-12 m; worst azimuth at the antimeridian sites 1.9e-14 rad
    fix, 88 rows: position 3.54e-08 m, receive time 7.5e-17 s, 5 iterations; lat 5.44e-15 rad, lon 1.9e-12 rad (89.9 degrees north;
    4.0e-15 elsewhere), alt 3.99e-07 m
    fix_atm, 88 rows: position 1.98e-07 m, receive time 5.46e-16 s, 9..12 iterations, 2..3 masked per row; the plain fix on the same
    observations is 1.66 .. 85.2 m off; fix_raim: the same bytes, every row PASS, largest statistic 1.03e-15
    velocity: 8.27e-4 m/s against a bound of 1.39e-2 (moving receiver, drift 2e-6: drift error 4.24e-12 against 4.63e-11), 2.85e-4
    against 8.94e-3 (at rest on the antimeridian)
    fixes with masked observations: 1.3e-08 m from the site.  The 19 tests take 2.5 s, 1.9 s of them the engine's start.
Each test prints its measured maxima before it asserts."""
import math

import numpy as np
import pytest

import nav_ref
import rate_ref
from nav_helpers import to_records
from nav_oracle_data import (ALT_TOL, ANGLE_TOL, CLOCK_TOL, DELAY_TOL, DRIFT_TOL, EXCL_AZ, EXCL_EL, EXCL_X, LATLON_TOL, POS_TOL, TIME_TOL, VEL_TOL,
                             angle_diff, atm_params, constellation, ephemerides, load)

pytestmark = pytest.mark.gpu

H_FD = 0.05                                                                  # tests/test_gpu_velocity.py's, as the fixture's
PER_SAT = 900.0 ** 2 / nav_ref.C + nav_ref.C * 2e-15 / (2 * H_FD) + 1e-6     # its derived bound per satellite


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def gpu_params(p):
    import gpsacq
    out = np.zeros(1, gpsacq.ATM_PARAMS_DTYPE)
    out["alpha"][0], out["beta"][0], out["elev_mask"], out["flags"] = p["alpha"], p["beta"], p["elev_mask"], p["flags"]
    return out


def _xyz(rec, names=("x", "y", "z")):
    return np.stack([rec[n] for n in names], -1)


def _state_obs():
    import gpsacq
    d = load()
    obs = np.zeros(d["state_eph"].size, gpsacq.OBS_DTYPE)
    obs["eph"], obs["tx_ms"], obs["tx_frac"], obs["valid"], obs["weight"] = d["state_eph"], d["state_tx_ms"], d["state_tx_frac"], 1, 1.0
    return obs


def _first(n):
    """n of the 384 state cases: whole ephemerides from the start, so that the small counts hold the planted ones too"""
    return slice(0, n)


# ---- 1. satellite states and rates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs", [1, 63, 64, 65, 384])
def test_states(eng, n_obs):
    d = load()
    rec = to_records(ephemerides())
    sel = _first(n_obs)
    got = eng.sat_states(rec, _state_obs()[sel])
    dpos = np.abs(_xyz(got) - d["state_pos"][sel]).max()
    dclk = np.abs(got["clock_corr"] - d["state_clock"][sel]).max()
    print("sat_states, %d observations: position %.3g m, clock correction %.3g s" % (n_obs, dpos, dclk))
    assert dpos <= POS_TOL and dclk <= CLOCK_TOL


@pytest.mark.parametrize("n_obs", [1, 63, 64, 65, 384])
def test_rates(eng, n_obs):
    d = load()
    rec = to_records(ephemerides())
    sel = _first(n_obs)
    got = eng.sat_rates(rec, _state_obs()[sel])
    dvel = np.abs(_xyz(got, ("vx", "vy", "vz")) - d["state_vel"][sel]).max()
    ddrift = np.abs(got["clock_drift"] - d["state_drift"][sel]).max()
    print("sat_rates, %d observations: velocity %.3g m/s, clock drift %.3g s/s" % (n_obs, dvel, ddrift))
    assert dvel <= VEL_TOL and ddrift <= DRIFT_TOL


# ---- 2. views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_views(eng, a):
    """one call per parameter set: 78 rows (13 sites x 6 receive times) of the first 12 ephemerides, the fix records filled from
    the sites"""
    import gpsacq
    d = load()
    rec = to_records(ephemerides()[:12])
    n_site, n_time, n_sat = d["view_tx_ms"].shape
    obs = np.zeros((n_site * n_time, n_sat), gpsacq.OBS_DTYPE)
    obs["tx_ms"], obs["tx_frac"] = d["view_tx_ms"].reshape(obs.shape), d["view_tx_frac"].reshape(obs.shape)
    obs["eph"], obs["valid"], obs["weight"] = np.arange(n_sat)[None, :], 1, 1.0
    fix = np.zeros(n_site * n_time, gpsacq.FIX_DTYPE)
    site = np.repeat(d["site_xyz"], n_time, axis=0)
    fix["x"], fix["y"], fix["z"] = site[:, 0], site[:, 1], site[:, 2]
    fix["rx_ms"], fix["rx_frac"] = d["view_rx_ms"].ravel(), d["view_rx_frac"].ravel()
    got = eng.sat_views(rec, obs, fix, gpu_params(atm_params(a)))
    ref = d["view_out"][a].reshape(obs.shape + (4,))
    ex = d["view_excl"][a].reshape(obs.shape)
    keep = (ex & EXCL_EL) == 0
    daz = np.where(keep & ((ex & EXCL_AZ) == 0), angle_diff(got["az"], ref[..., 0]), 0.0)
    dele = np.where(keep, np.abs(got["el"] - ref[..., 1]), 0.0)
    dion = np.where(keep & ((ex & EXCL_X) == 0), np.abs(got["iono_m"] - ref[..., 2]), 0.0)
    dtro = np.where(keep, np.abs(got["tropo_m"] - ref[..., 3]), 0.0)
    print("sat_views, set %d, %d cases (%d left out by the |el| rule, %d by |x|, %d azimuths): az %.3g rad, el %.3g rad, iono %.3g m, tropo %.3g m" %
          (a, obs.size, (~keep).sum(), ((ex & EXCL_X) != 0).sum(), ((ex & EXCL_AZ) != 0).sum(), daz.max(), dele.max(), dion.max(), dtro.max()))
    worst_site = np.abs(angle_diff(got["az"], ref[..., 0])).reshape(n_site, -1).max(axis=1)
    print("    azimuth per site: %s" % " ".join("%.1e" % v for v in worst_site))
    assert daz.max() <= ANGLE_TOL and dele.max() <= ANGLE_TOL and dion.max() <= DELAY_TOL and dtro.max() <= DELAY_TOL
    # no delay below the horizon or with its model off -- zero bytes, not a small number -- and a positive one where the oracle has one
    for name, col in (("iono_m", 2), ("tropo_m", 3)):
        off = keep & (ref[..., col] == 0)
        assert off.sum() >= 100 and not got[name][off].view(np.uint64).any(), name
        assert (got[name][keep & (ref[..., col] > 0)] > 0).all(), name
    assert (ref[..., 1] <= 0).sum() >= 100


# ---- 3. fixes ------------------------------------------------------------------------------------------------------------------
def _fix_batch(which):
    """every fix case in one batch: (records of the 11 constellations, obs [88][12], site per row [88][3], ref_ms [88], t_rx [88])"""
    import gpsacq
    d = load()
    n_site, n_time = d["fix_ref_ms"].shape
    rec = np.concatenate([to_records(constellation(f)) for f in range(n_site)])
    obs = np.zeros((n_site * n_time, 12), gpsacq.OBS_DTYPE)
    obs["tx_ms"], obs["tx_frac"] = d["fix_%s_ms" % which].reshape(obs.shape), d["fix_%s_frac" % which].reshape(obs.shape)
    obs["eph"] = (12 * np.repeat(np.arange(n_site), n_time))[:, None] + np.arange(12)[None, :]
    obs["valid"], obs["weight"] = 1, 1.0
    site = np.repeat(d["site_xyz"][d["fix_site"]], n_time, axis=0)
    lla = np.repeat(d["site_lla"][d["fix_site"]], n_time, axis=0)
    return rec, obs, site, lla, d["fix_ref_ms"].ravel().astype(np.int64), d["fix_t_rx"].ravel()


def _rx_error(fix, ref_ms, t_rx):
    return nav_ref.fold_ms(fix["rx_ms"].astype(np.int64) - ref_ms) * 1e-3 + (fix["rx_frac"] - t_rx)


@pytest.fixture(scope="module")
def plain(eng):
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("vac")
    fix = eng.fix(rec, obs)
    fix.setflags(write=False)
    return fix


def test_plain_fixes_recover_the_sites(plain):
    import gpsacq
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("vac")
    assert (plain["status"] == gpsacq.FIX_OK).all() and (plain["n_used"] == 12).all()
    dpos = np.abs(_xyz(plain) - site).max(axis=1)
    dt = np.abs(_rx_error(plain, ref_ms, t_rx))
    print("fix, %d rows of exact vacuum observations: position %.3g m, receive time %.3g s, rms %.3g m, iterations %d..%d" %
          (len(plain), dpos.max(), dt.max(), plain["rms"].max(), plain["iterations"].min(), plain["iterations"].max()))
    print("    position per site: %s" % " ".join("%.1e" % v for v in dpos.reshape(-1, 8).max(axis=1)))
    assert dpos.max() <= POS_TOL and dt.max() <= TIME_TOL and (plain["iterations"] <= 8).all()


def test_geodetic_of_the_fixes(plain):
    """lat / lon / alt as k_fix writes them, against the oracle's geodetic of the site.  The fix stands within 1e-7 m of the site
    (printed above), which is 1e-11 rad of lon even 11 km from the axis; lon is compared on the circle, the fix of the site with
    y == 0 lands a few nanometres to either side of the antimeridian."""
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("vac")
    dlat, dlon, dalt = np.abs(plain["lat"] - lla[:, 0]), angle_diff(plain["lon"], lla[:, 1]), np.abs(plain["alt"] - lla[:, 2])
    print("lat / lon / alt of the fixes: %.3g rad, %.3g rad, %.3g m" % (dlat.max(), dlon.max(), dalt.max()))
    print("    lon per site: %s" % " ".join("%.1e" % v for v in dlon.reshape(-1, 8).max(axis=1)))
    assert dlat.max() <= LATLON_TOL and dlon.max() <= LATLON_TOL and dalt.max() <= ALT_TOL
    assert (np.abs(plain["lon"]) <= math.pi).all() and (np.abs(plain["lon"][24:48]) > 3.14159).all()  # rows 24..47: the antimeridian sites


def test_corrected_fixes_recover_the_sites(eng):
    import gpsacq
    d = load()
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("atm")
    p = atm_params(0)
    fix, dop = eng.fix_atm(rec, obs, gpu_params(p))
    assert (fix["status"] == gpsacq.FIX_OK).all()
    dpos = np.abs(_xyz(fix) - site).max(axis=1)
    dt = np.abs(_rx_error(fix, ref_ms, t_rx))
    el = d["fix_el"].reshape(-1, 12)
    n_masked = (el < p["elev_mask"]).sum(axis=1)
    print("fix_atm, %d rows of exact observations through the model's atmosphere: position %.3g m, receive time %.3g s, rms %.3g m, "
          "iterations %d..%d, masked %d..%d" % (len(fix), dpos.max(), dt.max(), fix["rms"].max(), fix["iterations"].min(), fix["iterations"].max(),
                                               n_masked.min(), n_masked.max()))
    print("    position per site: %s" % " ".join("%.1e" % v for v in dpos.reshape(-1, 8).max(axis=1)))
    assert np.abs(el - p["elev_mask"]).min() >= math.radians(1.0) and (d["fix_pdop"] < 6.0).all()  # the fixture's own conditions
    assert dpos.max() <= POS_TOL and dt.max() <= TIME_TOL
    assert (dop["n_masked"] == n_masked).all() and (fix["n_used"] == 12 - n_masked).all()
    assert (dop["used_mask"] == ((el >= p["elev_mask"]) << np.arange(12)).sum(axis=1)).all()
    assert n_masked.max() >= 3 and ((el > 0) & (el < p["elev_mask"])).any()  # some are masked with a delay on their path
    # the plain solver on the same observations is metres off: the delays are in them
    off = np.linalg.norm(_xyz(eng.fix(rec, obs)) - site, axis=1)
    print("    the plain fix on the same observations: %.3g .. %.3g m off" % (off.min(), off.max()))
    assert off.min() > 1.0
    # the integrity path on the same rows: the same fix bit for bit, nothing to object to
    rfix, rdop, raim = eng.fix_raim(rec, obs, gpu_params(p), gpsacq.raim_params(3.0))
    print("    fix_raim: statuses %s, largest statistic %.3g" % (sorted(set(raim["status"].tolist())), raim["stat"].max()))
    differ = {n: int((rfix[n] != fix[n]).sum()) for n in fix.dtype.names if (rfix[n] != fix[n]).any()}
    differ.update({n: int((rdop[n] != dop[n]).sum()) for n in dop.dtype.names if (rdop[n] != dop[n]).any()})
    print("    rows in which fix_raim and fix_atm differ, by field: %s" % (differ or "none"))
    assert rfix.tobytes() == fix.tobytes() and rdop.tobytes() == dop.tobytes()
    assert np.isin(raim["status"], (gpsacq.RAIM_PASS, gpsacq.RAIM_UNCHECKED)).all()


# ---- 4. velocity -----------------------------------------------------------------------------------------------------------------
def test_velocity(eng, plain):
    """tests/test_gpu_velocity.py's bound, by its derivation: per satellite rho'^2 / c + c 2e-15 / (2 H_FD) + 1e-6 m/s, times the
    row sums of |(H^T W H)^-1 H^T W| from rate_ref's rows.  The Dopplers are the oracle's truth_tx differenced over +-H_FD seconds
    of receiver time; the satellites the 5-degree mask would drop are left out (a range rate below the horizon reaches 930 m/s)."""
    import gpsacq
    d = load()
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("vac")
    for c, f in enumerate(d["vel_site"]):
        rows = slice(8 * f, 8 * f + 8)
        ob, fx = obs[rows].copy(), plain[rows]
        rate = np.zeros(ob.shape, gpsacq.RATE_OBS_DTYPE)
        rate["doppler_hz"], rate["valid"], rate["weight"] = d["vel_doppler"][c], 1, 1.0
        up = d["fix_el"][f] >= math.radians(5.0)
        ob["valid"], rate["valid"] = up, up
        got = eng.velocity(rec, ob, rate, fx)
        assert (got["status"] == gpsacq.VEL_OK).all() and (got["n_used"] == up.sum(axis=1)).all()
        ephs = constellation(f)
        for k in range(8):
            used = list(np.flatnonzero(up[k]))
            H, _ = rate_ref.vel_rows(ephs, used, ob["tx_ms"][k, used], ob["tx_frac"][k, used], rate["doppler_hz"][k, used], d["site_xyz"][d["fix_site"][f]],
                                     fx["rx_ms"][k], fx["rx_frac"][k])
            g = np.abs(rate_ref.gain(H, np.ones(len(used)))).sum(axis=1)
            err = np.abs(_xyz(got[k], ("vx", "vy", "vz")) - d["vel_ecef"][c]).max()
            derr = abs(got["drift"][k] - d["vel_drift"][c])
            enu = np.abs(_xyz(got[k], ("ve", "vn", "vu")) - d["vel_enu"][c]).max()
            if k in (0, 7):
                print("velocity, site %d row %d, %d satellites: error %.3g m/s (bound %.3g), drift error %.3g (bound %.3g), rms %.3g m/s" %
                      (d["fix_site"][f], k, len(used), err, PER_SAT * g[:3].max(), derr, PER_SAT * g.max() / nav_ref.C, got["rms"][k]))
            assert err <= PER_SAT * g[:3].max() and derr <= PER_SAT * g.max() / nav_ref.C
            assert enu <= math.sqrt(3) * PER_SAT * g[:3].max() + 1e-6


# ---- 5. masks, beside good rows ----------------------------------------------------------------------------------------------------
def test_masks_beside_good_rows(eng, plain):
    """An ephemeris whose t_oe or t_oc is 604800 s or more gives a zero state and is skipped by the fix; so is a NaN or infinite
    tx_frac, in the host and in the device forms (include/gpsacq.h, SATELLITE STATE)."""
    import gpsacq
    import torch
    d = load()
    rec, obs, site, lla, ref_ms, t_rx = _fix_batch("vac")
    rec = np.concatenate([rec[:12], rec[:2]])
    rec["t_oe"][12], rec["t_oc"][13] = 604800, 604800   # codes 37800 of 65535: in the field, past the week
    assert all(eng._lib.gpsacq_ephemeris_valid(rec[k:k + 1].ctypes.data) == 1 for k in (12, 13))  # the issue numbers are fine
    ob = obs[:8].copy()
    ob["eph"][1, 0], ob["eph"][1, 1] = 12, 13
    ob["tx_frac"][2, 2], ob["tx_frac"][2, 3], ob["tx_frac"][2, 4] = float("nan"), float("inf"), float("-inf")
    ob["eph"][5, 11], ob["tx_frac"][5, 7] = 12, float("nan")
    bad = np.zeros(ob.shape, bool)
    bad[1, :2], bad[2, 2:5], bad[5, 11], bad[5, 7] = True, True, True, True
    st, rt, fix = eng.sat_states(rec, ob), eng.sat_rates(rec, ob), eng.fix(rec, ob)
    zero = bytes(32)
    assert all((st[i, j].tobytes() == zero) == bad[i, j] and (rt[i, j].tobytes() == zero) == bad[i, j] for i in range(8) for j in range(12))
    assert list(fix["n_used"]) == [12, 10, 9, 12, 12, 10, 12, 12] and (fix["status"] == gpsacq.FIX_OK).all()
    cleared = ob.copy()
    cleared["valid"][bad] = 0
    cleared["eph"][bad], cleared["tx_frac"][bad] = 0, 0.0
    assert eng.fix(rec, cleared).tobytes() == fix.tobytes()          # skipped, exactly as an observation that is not valid
    good = [0, 3, 4, 6, 7]
    assert fix[good].tobytes() == plain[:8][good].tobytes()          # the rows beside them are what they are alone
    dpos = np.abs(_xyz(fix) - site[:8]).max()
    print("fixes with masked observations: %.3g m from the site" % dpos)
    assert dpos <= POS_TOL and np.abs(_rx_error(fix, ref_ms[:8], t_rx[:8])).max() <= TIME_TOL
    # the device forms
    d_obs = torch.from_numpy(ob.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    buf = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_st, d_rt, d_fix = buf(ob.size * 32), buf(ob.size * 32), buf(8 * gpsacq.FIX_DTYPE.itemsize)
    torch.cuda.synchronize()
    eng.sat_states_device(rec, d_obs.data_ptr(), ob.size, d_st.data_ptr(), sync=True)
    eng.sat_rates_device(rec, d_obs.data_ptr(), ob.size, d_rt.data_ptr(), sync=True)
    eng.fix_device(rec, d_obs.data_ptr(), 8, 12, d_fix.data_ptr(), sync=True)
    assert d_st.cpu().numpy().tobytes() == st.tobytes() and d_rt.cpu().numpy().tobytes() == rt.tobytes()
    assert d_fix.cpu().numpy().tobytes() == fix.tobytes()
    # and the corrected and the integrity paths skip them as well
    p = gpu_params(dict(atm_params(0, elev_mask=-math.pi / 2), flags=0))  # vacuum observations: no delay to take off, nothing for RAIM to object to
    fa, da = eng.fix_atm(rec, ob, p)
    fr, dr, rm = eng.fix_raim(rec, ob, p, gpsacq.raim_params(3.0))
    assert list(fa["n_used"]) == list(fix["n_used"]) == list(fr["n_used"])
    want = [0xFFF & ~sum(1 << j for j in range(12) if bad[i, j]) for i in range(8)]
    assert list(da["used_mask"]) == want and list(dr["used_mask"]) == want and (rm["status"] == gpsacq.RAIM_PASS).all()
    assert np.abs(_xyz(fa) - site[:8]).max() <= POS_TOL and np.abs(_xyz(fr) - site[:8]).max() <= POS_TOL
