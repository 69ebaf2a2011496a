"""Satellite states and batched position fixes on the GPU (gpsacq_sat_states*, gpsacq_fix_batch*) against tests/nav_ref.py.

Tolerances, derived and not measured (position 1e-4 m, receive time 1e-12 s, clock correction 1e-13 s): a satellite position is
~50 fp64 operations on magnitudes of 2.7e7 m, ~1.5e-7 m of rounding; the subsets used here have PDOP 2.55 / 2.19 / 1.74 / 1.08
(4 / 5 / 8 / 12 satellites of the northern receiver; 2.16 .. 1.01 for the southern one, 2.32 .. 1.04 at the week's end --
tests/test_ephemeris.py asserts every one is below 6), so a fix stays under 1e-6 m; the orbit-time argument (up to 1e4 s) is
good to 2e-12 s, 1e-8 m at 4 km/s; both solvers apply a last step below 1e-4 m of a quadratically convergent iteration, which
leaves far less than the rounding.  The truth maker keeps every time as an offset below a millisecond from the fix's own
reference millisecond (1e-19 s).  rms is a weighted mean of residuals that are each good to the same ~1e-6 m, so 1e-4 m as well
where two solvers are compared pass for pass (against the truth it is only printed: it belongs to the residuals the last step was
made from, which are of that step's size).
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest

import nav_ref
from nav_helpers import geometry, to_record, to_records, truth_obs

pytestmark = pytest.mark.gpu

POS_TOL, TIME_TOL, CLOCK_TOL = 1e-4, 1e-12, 1e-13
N_FIX = 130


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def _times(n=N_FIX):
    """receive times: the first half 1 ms apart, the second 1 s apart, each with its own sub-millisecond part"""
    k = np.arange(n)
    ms = np.where(k < n // 2, k, n // 2 + 1000 * (k - n // 2))
    frac = (0.137e-3 + k * 0.0131e-3) % 1e-3
    return ms.astype(np.int64), frac


@pytest.fixture(scope="module")
def truth():
    """{which: (geometry, ref_ms[N_FIX], t_rx[N_FIX], obs[N_FIX][12])}, made once and never written to"""
    out = {}
    for which, n in (("north", N_FIX), ("south", 8), ("rollover", 66)):
        geo = geometry(which)
        ms, frac = _times(n)
        if which == "rollover":  # 1 ms apart, from 100 ms before the end of the week to 65 ms... the fixes' satellites straddle it
            ms = np.arange(n, dtype=np.int64) * 3
        ref_ms = (geo["ref_ms"] + ms) % nav_ref.WEEK_MS
        obs = truth_obs(geo, ref_ms, frac)
        obs.setflags(write=False)
        out[which] = (geo, ref_ms, frac, obs)
    return out


def _rx_error(fix, ref_ms, t_rx):
    return nav_ref.fold_ms(fix["rx_ms"].astype(np.int64) - ref_ms) * 1e-3 + (fix["rx_frac"] - t_rx)


def _check_against_truth(fix, geo, ref_ms, t_rx, n_used, label):
    import gpsacq
    assert (fix["status"] == gpsacq.FIX_OK).all() and (fix["n_used"] == n_used).all()
    assert ((fix["rx_frac"] >= 0) & (fix["rx_frac"] < 1e-3)).all() and ((fix["rx_ms"] >= 0) & (fix["rx_ms"] < nav_ref.WEEK_MS)).all()
    dpos = np.abs(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"]).max()
    dt = np.abs(_rx_error(fix, ref_ms, t_rx)).max()
    print("%s: position %.3g m, receive time %.3g s, rms %.3g m, iterations %d..%d" %
          (label, dpos, dt, fix["rms"].max(), fix["iterations"].min(), fix["iterations"].max()))
    assert dpos <= POS_TOL and dt <= TIME_TOL and (fix["iterations"] <= 8).all()
    assert fix["rms"].max() < 0.01  # the residuals the last step was made from: of that step's size, not those of the answer
    return dpos, dt


# ---- 1. satellite states ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def state_case():
    """200 observations over 15 ephemerides: the constellation from t_oe - 2 h to t_oe + 2 h, one at e = 0.03, and the week
    crossover both ways (t_oe = 16 s seen from 604 790 s; t_oe = 604 784 s seen from 10 s).  Reference computed once."""
    import gpsacq
    ephs = list(geometry()["ephs"])
    ephs.append(nav_ref.quantise(dict(ephs[3], e=0.03)))
    ephs.append(nav_ref.quantise(dict(ephs[4], t_oe=16, t_oc=16)))
    ephs.append(nav_ref.quantise(dict(ephs[5], t_oe=604784, t_oc=604784)))
    assert abs(ephs[12]["e"] - 0.03) < 1e-9
    rng = np.random.default_rng(41)
    n = 200
    obs = np.zeros(n, gpsacq.OBS_DTYPE)
    obs["eph"] = np.arange(n) % 15
    obs["valid"], obs["weight"] = 1, 1.0
    obs["tx_ms"] = 1000 * nav_ref.T_OE + np.linspace(-7200e3, 7200e3, n).astype(np.int64)
    obs["tx_ms"][obs["eph"] == 13] = 604_790_000 + np.arange((obs["eph"] == 13).sum()) * 700
    obs["tx_ms"][obs["eph"] == 14] = 10_000 + np.arange((obs["eph"] == 14).sum()) * 700
    obs["tx_frac"] = rng.uniform(0, 1e-3, n)
    xyz, dt = np.zeros((n, 3)), np.zeros(n)
    for k in range(n):
        p, c = nav_ref.sat_state(ephs[obs["eph"][k]], obs["tx_ms"][k], obs["tx_frac"][k])
        xyz[k], dt[k] = p[0], c[0]
    # the crossover pairs are 26 s from their epochs, not a week
    assert np.abs(np.linalg.norm(xyz, axis=1) - 2.656e7).max() < 9e5
    obs.setflags(write=False)
    return to_records(ephs), obs, xyz, dt


@pytest.mark.parametrize("n_obs", [1, 63, 64, 65, 200])
def test_sat_states_against_reference(eng, state_case, n_obs):
    rec, obs, xyz, dt = state_case
    st = eng.sat_states(rec, obs[:n_obs])
    dpos = np.abs(np.stack([st["x"], st["y"], st["z"]], 1) - xyz[:n_obs]).max()
    dclk = np.abs(st["clock_corr"] - dt[:n_obs]).max()
    print("n_obs %d: position %.3g m, clock correction %.3g s" % (n_obs, dpos, dclk))
    assert dpos <= POS_TOL and dclk <= CLOCK_TOL
    if n_obs == 200:  # the special ephemerides are among them
        assert {12, 13, 14} <= set(obs["eph"])
        assert np.abs(dt).max() > 1e-4  # a_f0 up to 5e-4 s: the correction is not a small number checked loosely


# ---- 2. fixes recover the truth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["equal", "x100"])
@pytest.mark.parametrize("sats", [4, 5, 8, 12])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 130])
def test_fix_recovers_truth(eng, truth, n_fix, sats, weights):
    geo, ref_ms, t_rx, obs = truth["north"]
    ob = obs[:n_fix][:, geo["subsets"][sats]].copy()
    if weights == "x100":  # exact observations: the weights must not move the answer
        ob["weight"] = np.random.default_rng(sats).uniform(1.0, 100.0, ob.shape)
    fix = eng.fix(to_records(geo["ephs"]), ob)
    _check_against_truth(fix, geo, ref_ms[:n_fix], t_rx[:n_fix], sats, "n_fix %d sats %d %s" % (n_fix, sats, weights))
    if n_fix == 130:
        assert len(set(fix["rx_ms"])) == 130 and len(set(fix["rx_frac"])) > 100  # both parts of the receive time move


def test_fix_across_the_end_of_the_week(eng, truth):
    geo, ref_ms, t_rx, obs = truth["rollover"]
    assert ref_ms.min() < 100 and ref_ms.max() > nav_ref.WEEK_MS - 100
    straddle = (obs["tx_ms"].max(1) - obs["tx_ms"].min(1)) > nav_ref.WEEK_MS // 2
    assert straddle.any() and not straddle.all()  # some rows hold transmit times from both sides of the rollover
    for sats in (4, 12):
        fix = eng.fix(to_records(geo["ephs"]), obs[:, geo["subsets"][sats]].copy())
        _check_against_truth(fix, geo, ref_ms, t_rx, sats, "rollover sats %d" % sats)


# ---- 3. perturbed observations against the reference solver ------------------------------------------------------------------
@pytest.mark.parametrize("sats", [5, 12])
def test_fix_against_reference_solver(eng, truth, sats):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    n = 65
    rng = np.random.default_rng(300 + sats)
    ob = obs[40:40 + n][:, geo["subsets"][sats]].copy()  # rows from both halves of the time grid
    ms, frac = nav_ref.split_time(ob["tx_ms"], ob["tx_frac"] + rng.uniform(-30e-9, 30e-9, ob.shape))
    ob["tx_ms"], ob["tx_frac"] = ms, frac
    ob["weight"] = rng.uniform(1.0, 100.0, ob.shape)
    fix = eng.fix(to_records(geo["ephs"]), ob)
    assert (fix["status"] == gpsacq.FIX_OK).all() and (fix["n_used"] == sats).all()
    worst = np.zeros(3)
    for k in range(n):
        ref = nav_ref.fix(geo["ephs"], ob["eph"][k], ob["tx_ms"][k], ob["tx_frac"][k], ob["weight"][k])
        assert ref["ok"]
        dpos = np.abs(np.array([fix["x"][k], fix["y"][k], fix["z"][k]]) - ref["xyz"]).max()
        dt = abs(float(nav_ref.fold_ms(int(fix["rx_ms"][k]) - ref["rx_ms"])) * 1e-3 + (fix["rx_frac"][k] - ref["rx_frac"]))
        worst = np.maximum(worst, [dpos, dt, abs(fix["rms"][k] - ref["rms"])])
        assert abs(int(fix["iterations"][k]) - ref["iterations"]) <= 1
    print("sats %d: position %.3g m, receive time %.3g s, rms %.3g m (rms itself %.3g .. %.3g m)" %
          (sats, worst[0], worst[1], worst[2], fix["rms"].min(), fix["rms"].max()))
    assert worst[0] <= POS_TOL and worst[1] <= TIME_TOL and worst[2] <= POS_TOL
    assert fix["rms"].max() > 0.5  # 30 ns of noise is metres of residual: the weights mattered
    off = np.abs(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"]).max(1)
    assert off.max() > 1.0 and off.max() < 200.0


# ---- 4. masks and failures, beside good fixes --------------------------------------------------------------------------------
def test_masks_and_failures_in_one_batch(eng, truth):
    import gpsacq
    geo, ref_ms, t_rx, obs = truth["north"]
    sel = geo["subsets"][8]
    ephs = list(geo["ephs"]) + [dict(geo["ephs"][sel[0]], iode3=200)]  # index 12: the same orbit, but not a valid ephemeris
    rec = to_records(ephs)
    assert not gpsacq.ephemeris_valid(rec[12]) and gpsacq.ephemeris_valid(rec[0])
    ob = obs[:9][:, sel].copy()
    good = eng.fix(rec, ob)  # the nine rows untouched: what the good rows must still give
    ob["valid"][1, [2, 5]] = 0                       # two masked: six left
    ob["eph"][2, 0], ob["eph"][2, 7] = 13, -1        # two indices out of range: six left
    ob["eph"][3, 0] = 12                             # an invalid ephemeris: seven left
    ob["valid"][4, 3:] = 0                           # three usable
    ob[5, 1:4] = ob[5, 0]                            # four times the same satellite at the same time, nothing else
    ob["valid"][5, 4:] = 0
    ob["valid"][6, :] = 0                            # nothing at all
    fix = eng.fix(rec, ob)
    assert list(fix["status"]) == [0, 0, 0, 0, gpsacq.FIX_TOO_FEW, gpsacq.FIX_NO_CONVERGE, gpsacq.FIX_TOO_FEW, 0, 0]
    assert list(fix["n_used"]) == [8, 6, 6, 7, 3, 4, 0, 8, 8]
    assert fix[[0, 7, 8]].tobytes() == good[[0, 7, 8]].tobytes()  # the neighbours of the bad rows: unaffected, bit for bit
    ok = [0, 1, 2, 3, 7, 8]
    for left in ([0, 1, 3, 4, 6, 7], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7]):  # what rows 1, 2, 3 keep: PDOP 2.08, 1.98, 1.88
        assert nav_ref.pdop(geo["rx"], geo["sat_xyz"][[sel[k] for k in left]]) < 6.0
    _check_against_truth(fix[ok], geo, ref_ms[ok], t_rx[ok], fix["n_used"][ok], "masked rows")
    for k in (4, 5, 6):  # failed: every double is zero, nothing NaN
        for name in ("rx_frac", "x", "y", "z", "lat", "lon", "alt", "rms"):
            assert fix[name][k] == 0.0, (k, name)
        assert fix["rx_ms"][k] == 0
    for name in fix.dtype.names:
        assert np.isfinite(fix[name].astype(np.float64)).all(), name
    # a masked observation gives a zero state
    st = eng.sat_states(rec, ob[:7])
    assert st[1, 2].tobytes() == bytes(32) and st[2, 0].tobytes() == bytes(32) and st[3, 0].tobytes() == bytes(32) and st[6].tobytes() == bytes(32 * 8)
    assert abs(math.hypot(st["x"][1, 0], st["y"][1, 0], st["z"][1, 0]) - 2.656e7) < 6e5


def test_argument_errors(eng, truth):
    import gpsacq
    geo, _, _, obs = truth["north"]
    rec = to_records(geo["ephs"])
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    ob = obs[:4][:, :8].copy()
    out = np.zeros(4, gpsacq.FIX_DTYPE)
    st = np.zeros(32, gpsacq.SAT_STATE_DTYPE)
    p = lambda a: a.ctypes.data_as(vp)
    for sats in (0, 13, -1):
        assert lib.gpsacq_fix_batch(h, p(rec), 12, p(ob), 2, sats, p(out)) == 1
    assert b"sats_per_fix" in lib.gpsacq_last_error()
    assert lib.gpsacq_fix_batch(None, p(rec), 12, p(ob), 4, 8, p(out)) == 1
    assert lib.gpsacq_fix_batch(h, None, 12, p(ob), 4, 8, p(out)) == 1
    assert lib.gpsacq_fix_batch(h, p(rec), 12, None, 4, 8, p(out)) == 1
    assert lib.gpsacq_fix_batch(h, p(rec), 12, p(ob), 4, 8, None) == 1
    assert lib.gpsacq_fix_batch(h, p(rec), 0, p(ob), 4, 8, p(out)) == 1
    assert lib.gpsacq_sat_states(h, None, 12, p(ob), 32, p(st)) == 1
    assert lib.gpsacq_sat_states(h, p(rec), 12, None, 32, p(st)) == 1
    assert lib.gpsacq_sat_states(h, p(rec), 12, p(ob), 32, None) == 1
    assert lib.gpsacq_fix_batch_device(h, p(rec), 12, None, 4, 8, None, 1) == 1
    assert lib.gpsacq_sat_states_device(h, p(rec), 12, None, 32, None, 1) == 1
    for bad in (float("nan"), -1.0, float("inf")):
        b = ob.copy()
        b["weight"][3, 5] = bad
        for call in (eng.fix, eng.sat_states):
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                call(rec, b)
            assert ei.value.code == 1 and "weight" in str(ei.value)
    assert not out.view(np.uint8).any()  # nothing was launched, nothing written
    with pytest.raises(gpsacq.GpsAcqError) as ei:
        eng.fix(rec, obs[:2].copy().reshape(1, 24))  # 24 per row
    assert ei.value.code == 1


# ---- 5. device forms ---------------------------------------------------------------------------------------------------------
def test_device_forms_equal_host_forms(eng, truth):
    import gpsacq
    import torch
    geo, _, _, obs = truth["north"]
    rec = to_records(geo["ephs"])
    ob = obs[:65][:, geo["subsets"][8]].copy()
    ob["valid"][7, 1] = 0
    ob["valid"][9, 2:] = 0
    host_fix = eng.fix(rec, ob)
    host_st = eng.sat_states(rec, ob)
    d_obs = torch.from_numpy(ob.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_fix = torch.full((65 * gpsacq.FIX_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((ob.size * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.fix_device(rec, d_obs.data_ptr(), 65, 8, d_fix.data_ptr(), sync=False)
    eng.sat_states_device(rec, d_obs.data_ptr(), ob.size, d_st.data_ptr(), sync=True)  # same stream: both are done
    assert d_fix.cpu().numpy().tobytes() == host_fix.tobytes()
    assert d_st.cpu().numpy().tobytes() == host_st.tobytes()
    # the device forms cannot read the weights: such an observation is skipped, not an error
    ob2 = ob.copy()
    ob2["weight"][3, 0] = float("nan")
    d_obs2 = torch.from_numpy(ob2.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.fix_device(rec, d_obs2.data_ptr(), 65, 8, d_fix.data_ptr(), sync=True)
    dev = d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE)
    assert dev["n_used"][3] == 7 and dev["status"][3] == 0 and dev[4:].tobytes() == host_fix[4:].tobytes()
    sat_ms, fix_ms = eng.fix_last_ms()
    assert sat_ms > 0 and fix_ms > 0


# ---- 6. geodetic output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["north", "south"])
def test_geodetic_output(eng, truth, which):
    geo, ref_ms, t_rx, obs = truth[which]
    n = 8
    fix = eng.fix(to_records(geo["ephs"]), obs[:n][:, geo["subsets"][8]].copy())
    _check_against_truth(fix, geo, ref_ms[:n], t_rx[:n], 8, which)
    lat, lon, alt = geo["lla"]
    dlat, dlon, dalt = np.abs(fix["lat"] - lat).max(), np.abs(fix["lon"] - lon).max(), np.abs(fix["alt"] - alt).max()
    print("%s: lat %.3g rad, lon %.3g rad, alt %.3g m" % (which, dlat, dlon, dalt))
    assert dlat <= 1e-10 and dlon <= 1e-10 and dalt <= 1e-4
    if which == "south":
        assert math.degrees(fix["lat"][0]) < -59.9 and math.degrees(fix["lon"][0]) > 169.9
