"""Atmosphere-corrected fixes on the GPU (gpsacq_sat_views*, gpsacq_fix_atm_batch*) against tests/atm_ref.py, which
tests/test_atm.py checks against its own truth maker.

Tolerances, derived and not measured.  Fixes: position 1e-4 m, receive time 1e-12 s -- tests/test_gpu_fix.py's, by its derivation;
the three rounds leave the model's own residue at 5e-8 m (re-measured in tests/test_atm.py), a condition and not a target.
Views: fp64 on 2.6e7-m coordinates with a few-ulp libm gives angles to ~1e-15 rad, so az and el to 1e-12 rad; delays stay below
100 m above a few degrees of elevation and are smooth in the angles (at most 3e4 m / rad for the troposphere at half a degree),
so 1e-9 m.  DOPs are a 4 x 4 inverse of a matrix with condition below 1e3: 1e-9 relative.  `iterations` may differ by one per
stage run: a step that lands on 1e-4 m is the last for one solver and not for the other, and every stage has its own last step.

The masks are 5 and 17 degrees on the "north" geometry.  nav_helpers' geo["elevation"] (geocentric vertical, one instant) puts
satellite 3 at 16.04 degrees, 0.96 from the 17-degree mask; what is asserted instead is the sharper thing, that the reference's
own geodetic elevations AT THE FIXES USED keep at least 1 degree from the mask (15.95 and 18.69 degrees: the rows with the
17-degree mask lie within 65 ms of each other).
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest

import atm_ref
import nav_ref
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu

POS_TOL, TIME_TOL = 1e-4, 1e-12
ANGLE_TOL, DELAY_TOL, DOP_RTOL = 1e-12, 1e-9, 1e-9
N_FIX = 130


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


def _times(n=N_FIX):
    k = np.arange(n)
    ms = np.where(k < n // 2, k, n // 2 + 1000 * (k - n // 2))
    frac = (0.137e-3 + k * 0.0131e-3) % 1e-3
    return ms.astype(np.int64), frac


@pytest.fixture(scope="module")
def truth():
    """{which: (geometry, ref_ms[n], t_rx[n], obs[n][12])}: observations through the model's atmosphere (both delays on),
    made once and never written to"""
    import gpsacq
    out = {}
    p = atm_ref.params()
    for which, n in (("north", N_FIX), ("south", 8), ("rollover", 66)):
        geo = geometry(which)
        ms, frac = _times(n)
        if which == "rollover":
            ms = np.arange(n, dtype=np.int64) * 3
        ref_ms = (geo["ref_ms"] + ms) % nav_ref.WEEK_MS
        tx_ms, tx_frac = atm_ref.truth_times(geo["ephs"], geo["rx"], ref_ms, frac, p)
        obs = np.zeros(tx_ms.shape, gpsacq.OBS_DTYPE)
        obs["tx_ms"], obs["tx_frac"], obs["eph"], obs["valid"], obs["weight"] = tx_ms, tx_frac, np.arange(12), 1, 1.0
        obs.setflags(write=False)
        out[which] = (geo, ref_ms, frac, obs)
    return out


def _rx_error(fix, ref_ms, t_rx):
    return nav_ref.fold_ms(fix["rx_ms"].astype(np.int64) - ref_ms) * 1e-3 + (fix["rx_frac"] - t_rx)


def _xyz(fix):
    return np.stack([fix["x"], fix["y"], fix["z"]], -1)


_ref_cache = {}


def _ref_fix(geo, row, p, key=None):
    """atm_ref.fix_atm of one OBS_DTYPE row (its usable observations), plus the used_mask it implies"""
    if key is not None and key in _ref_cache:
        return _ref_cache[key]
    u = [s for s in range(len(row)) if row["valid"][s] and 0 <= row["eph"][s] < len(geo["ephs"])]
    ref = atm_ref.fix_atm(geo["ephs"], row["eph"][u], row["tx_ms"][u], row["tx_frac"][u], row["weight"][u], p)
    ref["used_mask"] = sum(1 << u[j] for j in range(len(u)) if ref["kept"][j])
    ref["usable"] = u
    if key is not None:
        _ref_cache[key] = ref
    return ref


def _assert_mask_margin(geo, ref, mask_rad):
    """the reference's own elevations at this fix keep 1 degree from the mask (see the module docstring)"""
    el = atm_ref.view(ref["lla"][0], ref["lla"][1], ref["sat"] - ref["xyz"])[1]
    assert np.abs(el - mask_rad).min() >= math.radians(1.0), np.degrees(el)


# ---- 1. views ----------------------------------------------------------------------------------------------------------------
def _receivers(geo):
    pole = np.array([0.0, 0.0, nav_ref.WGS84_A * math.sqrt(1 - nav_ref.WGS84_E2) + 250.0])  # on the axis: geodetic()'s guard
    return [geo["rx"], nav_ref.ecef_of(*nav_ref.RX_LLA_SOUTH), pole, nav_ref.ecef_of(math.radians(47.3), math.radians(8.5), -50.0),
            nav_ref.ecef_of(math.radians(47.3), math.radians(8.5), -150.0), nav_ref.ecef_of(math.radians(30.0), math.radians(-100.0), 12000.0),
            nav_ref.ecef_of(math.radians(-10.0), math.radians(60.0), 9000.0)]


@pytest.mark.parametrize("n_fix,sats", [(1, 1), (7, 9), (8, 8), (13, 5), (20, 10)])
def test_sat_views_against_reference(eng, truth, n_fix, sats):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    assert n_fix * sats in (1, 63, 64, 65, 200)
    p = atm_ref.params()
    rxs = _receivers(geo)
    ob = obs[60:60 + n_fix][:, :sats].copy()  # rows from both halves of the time grid
    fix = np.zeros(n_fix, gpsacq.FIX_DTYPE)
    for k in range(n_fix):
        fix["x"][k], fix["y"][k], fix["z"][k] = rxs[k % len(rxs)]
        fix["rx_ms"][k], fix["rx_frac"][k] = ref_ms[60 + k], t_rx[60 + k]
    if n_fix == 20:
        fix["status"][11] = gpsacq.FIX_TOO_FEW
        ob["valid"][3, 2] = 0
        fix["lat"][5] = 1.0  # lat / lon / alt of the input are not read
    got = eng.sat_views(to_records(geo["ephs"]), ob, fix, gpu_params(p))
    worst = np.zeros(4)
    n_zenith = 0
    alts = []
    for k in range(n_fix):
        if fix["status"][k] != 0:
            assert got[k].tobytes() == bytes(32 * sats)
            continue
        rx = rxs[k % len(rxs)]
        for s in range(sats):
            if not ob["valid"][k, s]:
                assert got[k, s].tobytes() == bytes(32)
                continue
            pos, dt = nav_ref.sat_state(geo["ephs"][ob["eph"][k, s]], ob["tx_ms"][k, s], ob["tx_frac"][k, s])
            d = float(nav_ref.fold_ms(int(ob["tx_ms"][k, s]) - int(fix["rx_ms"][k]))) * 1e-3 + ((ob["tx_frac"][k, s] - dt[0]) - fix["rx_frac"][k])
            tow = float(fix["rx_ms"][k]) * 1e-3 + fix["rx_frac"][k]
            v = atm_ref.views(rx, atm_ref.turned(pos[0], d, 0.0), tow, p)
            alts.append(v["lla"][2])
            # the model's two discontinuities are not among the cases
            assert abs(float(v["el"])) > 1e-9
            if v["el"] > 0:
                x = atm_ref.klobuchar_x(v["az"], v["el"], v["lla"][0], v["lla"][1], tow, p)[0]
                assert abs(abs(float(x)) - 1.57) > 1e-9
            g = got[k, s]
            daz = abs((g["az"] - float(v["az"]) + math.pi) % (2 * math.pi) - math.pi)
            if abs(float(v["el"])) > math.pi / 2 - 1e-6:
                n_zenith, daz = n_zenith + 1, 0.0
            worst = np.maximum(worst, [daz, abs(g["el"] - float(v["el"])), abs(g["iono_m"] - float(v["iono"])), abs(g["tropo_m"] - float(v["tropo"]))])
            assert (g["iono_m"] > 0) == (v["el"] > 0) and (g["tropo_m"] > 0) == (v["el"] > 0 and -100 <= v["lla"][2] <= 1e4)
    print("n_fix %d sats %d: az %.3g rad, el %.3g rad, iono %.3g m, tropo %.3g m (%d at the zenith skipped)" % ((n_fix, sats) + tuple(worst) + (n_zenith,)))
    assert worst[0] <= ANGLE_TOL and worst[1] <= ANGLE_TOL and worst[2] <= DELAY_TOL and worst[3] <= DELAY_TOL
    if n_fix == 20:
        assert min(alts) < -100 and max(alts) > 1e4 and any(-100 < a < 0 for a in alts)
        assert (got["tropo_m"][4] == 0).all() and (got["tropo_m"][5] == 0).all() and (got["iono_m"][5] > 0).any()  # -150 m and 12 km
        assert abs(got["el"][2]).max() > 0 and (got["tropo_m"][3] > 0).any()  # the pole row is there; -50 m has a troposphere


# ---- 2. fixes recover the truth -------------------------------------------------------------------------------------------
def _check_truth(fix, geo, ref_ms, t_rx, label):
    dpos = np.abs(_xyz(fix) - geo["rx"]).max()
    dt = np.abs(_rx_error(fix, ref_ms, t_rx)).max()
    print("%s: position %.3g m, receive time %.3g s, rms %.3g m, iterations %d..%d" %
          (label, dpos, dt, fix["rms"].max(), fix["iterations"].min(), fix["iterations"].max()))
    assert dpos <= POS_TOL and dt <= TIME_TOL
    return dpos


@pytest.mark.parametrize("weights", ["equal", "x100"])
@pytest.mark.parametrize("sats", [4, 5, 8, 12])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 130])
def test_fix_atm_recovers_truth(eng, truth, n_fix, sats, weights):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    p = atm_ref.params()  # the default 5-degree mask
    ob = obs[:n_fix][:, geo["subsets"][sats]].copy()
    if weights == "x100":  # exact observations: the weights must not move the answer
        ob["weight"][:, sats // 2] = 100.0
    rec = to_records(geo["ephs"])
    fix, dop = eng.fix_atm(rec, ob, gpu_params(p))
    plain = eng.fix(rec, ob)
    assert (fix["status"] == gpsacq.FIX_OK).all()
    _check_truth(fix, geo, ref_ms[:n_fix], t_rx[:n_fix], "n_fix %d sats %d %s" % (n_fix, sats, weights))
    off = np.linalg.norm(_xyz(plain) - geo["rx"], axis=1)
    print("    the plain fix on the same observations: %.3g .. %.3g m off" % (off.min(), off.max()))
    assert (plain["status"] == 0).all() and off.min() > 5.0
    assert (fix["iterations"] <= 8 + 2 * 3).all() and (fix["iterations"] >= plain["iterations"] + 3).all()
    if sats < 12:  # the lowest-PDOP subsets stand above 10 degrees: nothing is masked
        assert (fix["n_used"] == sats).all() and (dop["n_masked"] == 0).all() and (dop["used_mask"] == (1 << sats) - 1).all()
    else:
        for k in sorted({0, n_fix // 2, n_fix - 1}):
            ref = _ref_fix(geo, ob[k], p, key=("truth12", k, weights))
            assert ref["status"] == 0 and ref["n_masked"] == 2
            _assert_mask_margin(geo, ref, p["elev_mask"])
            assert (int(dop["n_masked"][k]), int(dop["used_mask"][k]), int(fix["n_used"][k])) == (ref["n_masked"], ref["used_mask"], ref["n_used"])
        assert (dop["n_masked"] == 2).all() and (fix["n_used"] == 10).all() and len(set(dop["used_mask"])) == 1
    assert (dop["pdop"] > 0.5).all() and (dop["pdop"] < 6.0).all() and (dop["gdop"] > dop["pdop"]).all()


# ---- 3. perturbed observations against the reference solver ------------------------------------------------------------------
@pytest.mark.parametrize("sats,mask_deg", [(5, 5.0), (12, 17.0), (12, 5.0)])
def test_fix_atm_against_reference_solver(eng, truth, sats, mask_deg):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    n = 65  # the first 65 rows: 1 ms apart, so the elevations stand still next to the mask's margin
    p = atm_ref.params(elev_mask=math.radians(mask_deg))
    rng = np.random.default_rng(500 + sats)
    ob = obs[:n][:, geo["subsets"][sats]].copy()
    ms, frac = nav_ref.split_time(ob["tx_ms"], ob["tx_frac"] + rng.uniform(-30e-9, 30e-9, ob.shape))  # tens of metres
    ob["tx_ms"], ob["tx_frac"] = ms, frac
    ob["weight"] = rng.uniform(1.0, 100.0, ob.shape)
    fix, dop = eng.fix_atm(to_records(geo["ephs"]), ob, gpu_params(p))
    worst = np.zeros(4)
    for k in range(n):
        ref = _ref_fix(geo, ob[k], p)
        assert ref["status"] == 0 and fix["status"][k] == 0
        _assert_mask_margin(geo, ref, p["elev_mask"])
        assert (int(fix["n_used"][k]), int(dop["used_mask"][k]), int(dop["n_masked"][k])) == (ref["n_used"], ref["used_mask"], ref["n_masked"])
        assert abs(int(fix["iterations"][k]) - ref["iterations"]) <= len(ref["stages"]), (fix["iterations"][k], ref["stages"])
        dpos = np.abs(_xyz(fix[k]) - ref["xyz"]).max()
        dt = abs(float(nav_ref.fold_ms(int(fix["rx_ms"][k]) - ref["rx_ms"])) * 1e-3 + (fix["rx_frac"][k] - ref["rx_frac"]))
        g = np.array([dop[name][k] for name in ("gdop", "pdop", "hdop", "vdop", "tdop")])
        ddop = np.abs(g / np.array(ref["dop"]) - 1).max()
        used = [j for j in range(len(ref["usable"])) if ref["kept"][j]]
        ddop = max(ddop, abs(dop["pdop"][k] / nav_ref.pdop(ref["xyz"], ref["sat"][used]) - 1))
        worst = np.maximum(worst, [dpos, dt, abs(fix["rms"][k] - ref["rms"]), ddop])
    print("sats %d mask %g: position %.3g m, receive time %.3g s, rms %.3g m, DOP %.3g relative (rms itself %.3g .. %.3g m)" %
          ((sats, mask_deg) + tuple(worst) + (fix["rms"].min(), fix["rms"].max())))
    assert worst[0] <= POS_TOL and worst[1] <= TIME_TOL and worst[2] <= POS_TOL and worst[3] <= DOP_RTOL
    assert fix["rms"].max() > 0.5
    if sats == 12:
        assert (dop["n_masked"] == (3 if mask_deg == 17.0 else 2)).all()  # 15.95 degrees falls to the 17-degree mask, 18.69 stays


# ---- 4. flags and mask -------------------------------------------------------------------------------------------------------
def test_flags_and_mask(eng, truth):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    rec = to_records(geo["ephs"])
    ob = obs[:9][:, geo["subsets"][8]].copy()
    # nothing on, nothing masked: the rounds are skipped and the plain solver's answer comes out
    off = atm_ref.params(flags=0, elev_mask=-math.pi / 2)
    fix, dop = eng.fix_atm(rec, ob, gpu_params(off))
    plain = eng.fix(rec, ob)
    for name in ("status", "n_used", "iterations", "rx_ms"):
        assert (fix[name] == plain[name]).all(), name
    d = np.abs(_xyz(fix) - _xyz(plain)).max()
    print("flags 0, no mask: %.3g m from Engine.fix" % d)
    assert d <= POS_TOL and np.abs(fix["rx_frac"] - plain["rx_frac"]).max() <= TIME_TOL
    assert (dop["n_masked"] == 0).all() and (dop["used_mask"] == 0xFF).all()
    # with all twelve the below-horizon pair is used as well: -pi/2 masks nothing
    f12, d12 = eng.fix_atm(rec, obs[:3].copy(), gpu_params(off))
    assert (f12["n_used"] == 12).all() and (d12["n_masked"] == 0).all() and (f12["iterations"] == eng.fix(rec, obs[:3].copy())["iterations"]).all()
    # only the ionosphere, only the troposphere, both: each against the reference
    for flags in (1, 2, 3):
        p = atm_ref.params(flags=flags)
        fix, dop, views = eng.fix_atm(rec, ob, gpu_params(p), views=True)
        worst = 0.0
        for k in range(len(ob)):
            ref = _ref_fix(geo, ob[k], p)
            assert fix["status"][k] == 0 == ref["status"]
            worst = max(worst, np.abs(_xyz(fix[k]) - ref["xyz"]).max())
        print("flags %d: %.3g m from the reference, %.3g m from the receiver" % (flags, worst, np.abs(_xyz(fix) - geo["rx"]).max()))
        assert worst <= POS_TOL
        assert ((views["iono_m"] > 0) == bool(flags & 1)).all() and ((views["tropo_m"] > 0) == bool(flags & 2)).all()
        if flags != 3:  # the observations carry both delays: half a correction is metres off
            assert np.abs(_xyz(fix) - geo["rx"]).max() > 1.0
    # alpha = beta = 0: the 5-ns floor times F
    p0 = atm_ref.params(alpha=[0.0] * 4, beta=[0.0] * 4, flags=1)
    fix, dop, views = eng.fix_atm(rec, ob, gpu_params(p0), views=True)
    E = views["el"] / math.pi
    floor = nav_ref.C * (1 + 16 * (0.53 - E) ** 3) * 5e-9
    print("alpha = beta = 0: %.3g m from the floor" % np.abs(views["iono_m"] - floor).max())
    assert (fix["status"] == 0).all() and np.abs(views["iono_m"] - floor).max() <= DELAY_TOL and (views["iono_m"] > 1.49).all()


# ---- 5. every path in one batch -----------------------------------------------------------------------------------------------
def test_paths_in_one_batch(eng, truth):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    rec = to_records(geo["ephs"])
    p = atm_ref.params()
    gp = gpu_params(p)
    sel = geo["subsets"][8]
    ob = obs[:65][:, sel + [9, 10]].copy()  # ten columns: the eight best and the two below the horizon
    ob["valid"][:, 8:] = 0
    ob["valid"][3, 3:] = 0                        # three usable
    ob["valid"][7, 3:] = 0                        # three above the mask and one below it: four usable, three left
    ob["valid"][7, 8] = 1
    ob["valid"][12, [2, 5]] = 0                   # holes
    ob["weight"][20, 4] = 0.0                     # a weight-0 satellite
    ob[31, 1:4] = ob[31, 0]                       # four times the same satellite at the same time, nothing else: coplanar
    ob["valid"][31, 4:] = 0
    ob["valid"][40, 9] = 1                        # nine usable, one masked
    ob["valid"][63, :] = 0                        # nothing at all
    bad = [3, 7, 31, 63]
    fix, dop, views = eng.fix_atm(rec, ob, gp, views=True)
    status = np.zeros(65, int)
    status[[3, 7, 63]], status[31] = gpsacq.FIX_TOO_FEW, gpsacq.FIX_NO_CONVERGE
    assert list(fix["status"]) == list(status)
    n_used = np.full(65, 8)
    n_used[[3, 7, 12, 31, 63]] = 3, 3, 6, 4, 0
    assert list(fix["n_used"]) == list(n_used)
    assert dop["n_masked"][7] == 1 and dop["n_masked"][40] == 1 and dop["n_masked"].sum() == 2
    assert dop["used_mask"][7] == 0b111 and dop["used_mask"][40] == 0xFF and dop["used_mask"][12] == 0xFF & ~0b100100
    assert dop["used_mask"][3] == 0b111 and dop["used_mask"][63] == 0 and dop["used_mask"][31] == 0b1111
    assert fix["iterations"][7] > 0 and fix["iterations"][3] == 0  # row 7 ran stage 0 before the mask took its fourth satellite
    for k in bad:  # failed: every double is zero, nothing NaN
        for name in ("rx_frac", "x", "y", "z", "lat", "lon", "alt", "rms"):
            assert fix[name][k] == 0.0, (k, name)
        assert fix["rx_ms"][k] == 0
        assert not any(dop[name][k] for name in ("gdop", "pdop", "hdop", "vdop", "tdop"))
        assert views[k].tobytes() == bytes(32 * 10)
    for rec_ in (fix, dop, views):
        for name in rec_.dtype.names:
            assert np.isfinite(rec_[name].astype(np.float64)).all(), name
    good = [k for k in range(65) if k not in bad]
    _check_truth(fix[good], geo, ref_ms[good], t_rx[good], "the good rows of the mixed batch")
    # the weight-0 satellite is used and in used_mask, but absent from DOP
    assert fix["n_used"][20] == 8 and dop["used_mask"][20] == 0xFF
    ref = _ref_fix(geo, ob[20], p)
    g = np.array([dop[name][20] for name in ("gdop", "pdop", "hdop", "vdop", "tdop")])
    assert np.abs(g / np.array(ref["dop"]) - 1).max() <= DOP_RTOL
    assert dop["pdop"][20] > dop["pdop"][19] * 1.001 and abs(dop["pdop"][21] / dop["pdop"][19] - 1) < 1e-3
    # the neighbours of every bad row, and every other row: what the same rows give when solved alone
    alone = [2, 4, 6, 8, 30, 32, 62, 64, 12, 20, 40]
    f2, d2, v2 = eng.fix_atm(rec, ob[alone].copy(), gp, views=True)
    assert f2.tobytes() == fix[alone].tobytes() and d2.tobytes() == dop[alone].tobytes() and v2.tobytes() == views[alone].tobytes()


# ---- 6. views of fix_atm ------------------------------------------------------------------------------------------------------
def test_views_of_fix_atm_equal_sat_views(eng, truth):
    geo, ref_ms, t_rx, obs = truth["north"]
    rec = to_records(geo["ephs"])
    gp = gpu_params(atm_ref.params())
    ob = obs[:65].copy()
    ob["valid"][5, 2:] = 0  # not OK
    fix, dop, views = eng.fix_atm(rec, ob, gp, views=True)
    assert fix["status"][5] != 0 and views[5].tobytes() == bytes(32 * 12) and views[4].tobytes() != bytes(32 * 12)
    assert eng.sat_views(rec, ob, fix, gp).tobytes() == views.tobytes()
    # masked satellites still have a view; the two below the horizon have no delay
    assert (views["el"][0, [9, 10]] < 0).all() and not views["iono_m"][0, [9, 10]].any() and not views["tropo_m"][0, [9, 10]].any()
    assert (views["iono_m"][0, :9] > 1.0).all() and (views["tropo_m"][0, :9] > 2.0).all()


# ---- 7. device forms ----------------------------------------------------------------------------------------------------------
def test_device_forms_equal_host_forms(eng, truth):
    import gpsacq
    import torch
    geo, _, _, obs = truth["north"]
    rec = to_records(geo["ephs"])
    gp = gpu_params(atm_ref.params())
    ob = obs[:65].copy()
    ob["valid"][7, 1] = 0
    ob["valid"][9, 2:] = 0
    fix, dop, views = eng.fix_atm(rec, ob, gp, views=True)
    assert eng.fix_atm(rec, ob, gp, dop=False).tobytes() == fix.tobytes()  # NULL dop and views in the host form
    buf = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs = torch.from_numpy(ob.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_fix, d_dop, d_views, d_views2 = buf(65 * 80), buf(65 * 48), buf(ob.size * 32), buf(ob.size * 32)
    torch.cuda.synchronize()
    eng.fix_atm_device(rec, d_obs.data_ptr(), 65, 12, gp, d_fix.data_ptr(), d_dop.data_ptr(), d_views.data_ptr(), sync=True)
    t = eng.fix_atm_last_ms()
    assert len(t) == 3 and all(math.isfinite(x) and x >= 0 for x in t)
    assert d_fix.cpu().numpy().tobytes() == fix.tobytes() and d_dop.cpu().numpy().tobytes() == dop.tobytes()
    assert d_views.cpu().numpy().tobytes() == views.tobytes()
    eng.sat_views_device(rec, d_obs.data_ptr(), d_fix.data_ptr(), 65, 12, gp, d_views2.data_ptr(), sync=True)
    assert d_views2.cpu().numpy().tobytes() == views.tobytes()
    # NULL dop and views in the device form
    d_fix2 = buf(65 * 80)
    torch.cuda.synchronize()
    eng.fix_atm_device(rec, d_obs.data_ptr(), 65, 12, gp, d_fix2.data_ptr(), sync=True)
    assert d_fix2.cpu().numpy().tobytes() == fix.tobytes()
    t = eng.fix_atm_last_ms()
    assert all(math.isfinite(x) and x >= 0 for x in t) and t[2] == 0
    # the device forms cannot read the weights: such an observation is skipped, not an error
    ob2 = ob.copy()
    ob2["weight"][3, 0] = float("nan")
    d_obs2 = torch.from_numpy(ob2.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.fix_atm_device(rec, d_obs2.data_ptr(), 65, 12, gp, d_fix2.data_ptr(), d_dop.data_ptr(), sync=True)
    dev, ddop = d_fix2.cpu().numpy().view(gpsacq.FIX_DTYPE), d_dop.cpu().numpy().view(gpsacq.FIX_DOP_DTYPE)
    assert dev["n_used"][3] == 9 and dev["status"][3] == 0 and ddop["used_mask"][3] == 0x9FE and dev[4:].tobytes() == fix[4:].tobytes()


# ---- 8. across the end of the week ------------------------------------------------------------------------------------------
def test_rollover(eng, truth):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["rollover"]
    assert ref_ms.min() < 100 and ref_ms.max() > nav_ref.WEEK_MS - 100
    p = atm_ref.params()
    rec = to_records(geo["ephs"])
    for sats in (4, 12):
        ob = obs[:, geo["subsets"][sats]].copy()
        fix, dop, views = eng.fix_atm(rec, ob, gpu_params(p), views=True)
        assert (fix["status"] == 0).all()
        _check_truth(fix, geo, ref_ms, t_rx, "rollover sats %d" % sats)
        # Klobuchar's time of day is taken across the end of the week: the delays on both sides of it follow the reference
        worst = 0.0
        for k in (0, 32, 33, 34, 65):
            ref = _ref_fix(geo, ob[k], p)
            assert ref["status"] == 0 and ref["used_mask"] == dop["used_mask"][k]
            tow = float(fix["rx_ms"][k]) * 1e-3 + fix["rx_frac"][k]
            v = atm_ref.views(ref["xyz"], ref["sat"], tow, p)
            worst = max(worst, np.abs(views["iono_m"][k] - v["iono"]).max(), np.abs(views["tropo_m"][k] - v["tropo"]).max())
        print("    delays across the rollover: %.3g m from the reference" % worst)
        assert worst <= 1e-6  # the views are those of the GPU's fix, 1e-5 m from the reference's: 3e-4 m / m of troposphere
        assert fix["rx_ms"][0] > nav_ref.WEEK_MS - 200 and fix["rx_ms"][65] < 200


# ---- 9. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(eng, truth):
    import gpsacq
    geo, _, _, obs = truth["north"]
    rec = to_records(geo["ephs"])
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    ob = obs[:4][:, :8].copy()
    gp = gpu_params(atm_ref.params())
    out = np.zeros(4, gpsacq.FIX_DTYPE)
    vw = np.zeros((4, 8), gpsacq.SAT_VIEW_DTYPE)
    ptr = lambda a: a.ctypes.data_as(vp)
    assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, ptr(ob), 4, 8, ptr(gp), ptr(out), None, None) == 0
    ok = out.copy()
    out[:] = 0
    assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, ptr(ob), 4, 8, None, ptr(out), None, None) == 1  # NULL parameters
    assert b"params" in lib.gpsacq_last_error()
    assert lib.gpsacq_sat_views(h, ptr(rec), 12, ptr(ob), ptr(ok), 4, 8, None, ptr(vw)) == 1
    assert lib.gpsacq_fix_atm_batch_device(h, ptr(rec), 12, ptr(ob), 4, 8, None, ptr(out), None, None, 1) == 1
    for sats in (0, 13, -1):
        assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, ptr(ob), 2, sats, ptr(gp), ptr(out), None, None) == 1
        assert b"sats_per_fix" in lib.gpsacq_last_error()
        assert lib.gpsacq_sat_views(h, ptr(rec), 12, ptr(ob), ptr(ok), 2, sats, ptr(gp), ptr(vw)) == 1
    for name, value in (("elev_mask", math.pi / 2), ("elev_mask", -math.pi / 2 - 1e-9), ("elev_mask", float("nan")), ("elev_mask", float("inf")),
                        ("flags", 4), ("flags", -1), ("alpha", float("nan")), ("beta", float("inf"))):
        bad = gp.copy()
        if name in ("alpha", "beta"):
            bad[name][0, 2] = value
        else:
            bad[name] = value
        for call in (lambda: eng.fix_atm(rec, ob, bad), lambda: eng.sat_views(rec, ob, ok, bad)):
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                call()
            assert ei.value.code == 1, (name, value)
        assert lib.gpsacq_fix_atm_batch_device(h, ptr(rec), 12, ptr(ob), 4, 8, ptr(bad), ptr(out), None, None, 1) == 1
    edge = gp.copy()
    edge["elev_mask"] = -math.pi / 2  # the lower end is in range
    assert (eng.fix_atm(rec, ob, edge, dop=False)["status"] == 0).all()
    assert lib.gpsacq_fix_atm_batch(None, ptr(rec), 12, ptr(ob), 4, 8, ptr(gp), ptr(out), None, None) == 1
    assert lib.gpsacq_fix_atm_batch(h, None, 12, ptr(ob), 4, 8, ptr(gp), ptr(out), None, None) == 1
    assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, None, 4, 8, ptr(gp), ptr(out), None, None) == 1
    assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, ptr(ob), 4, 8, ptr(gp), None, None, None) == 1
    assert lib.gpsacq_fix_atm_batch(h, ptr(rec), 12, ptr(ob), 0, 8, ptr(gp), ptr(out), None, None) == 1
    assert lib.gpsacq_sat_views(h, ptr(rec), 12, ptr(ob), None, 4, 8, ptr(gp), ptr(vw)) == 1
    assert lib.gpsacq_sat_views(h, ptr(rec), 12, ptr(ob), ptr(ok), 4, 8, ptr(gp), None) == 1
    for bad_w in (float("nan"), -1.0, float("inf")):  # a bad weight in the host forms
        b = ob.copy()
        b["weight"][3, 5] = bad_w
        for call in (lambda: eng.fix_atm(rec, b, gp), lambda: eng.sat_views(rec, b, ok, gp)):
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                call()
            assert ei.value.code == 1 and "weight" in str(ei.value)
    assert not out.view(np.uint8).any() and not vw.view(np.uint8).any()  # nothing was launched, nothing written
    fresh = gpsacq.Engine(4.092e6, 5.456e6, 5000.0)
    try:
        with pytest.raises(gpsacq.GpsAcqError):
            fresh.fix_atm_last_ms()  # no call made on this engine
    finally:
        fresh.close()


# ---- 10. velocity ------------------------------------------------------------------------------------------------------------
def test_velocity_takes_corrected_fix(eng, truth):
    import gpsacq
    geo, _, _, obs = truth["north"]
    rec = to_records(geo["ephs"])
    ob = obs[:5][:, geo["subsets"][8]].copy()
    fix = eng.fix_atm(rec, ob, gpu_params(atm_ref.params()), dop=False)
    ro = np.zeros(ob.shape, gpsacq.RATE_OBS_DTYPE)
    ro["valid"], ro["weight"] = 1, 1.0
    vel = eng.velocity(rec, ob, ro, fix)
    assert (vel["status"] == gpsacq.VEL_OK).all() and (vel["n_used"] == 8).all()
