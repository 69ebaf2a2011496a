"""Coarse-time fixes on the CPU: the reference of the GPU tests (tests/coarse_ref.py, written from "Coarse-time fixes: positions
from code phases alone" of include/gpsacq.h) against the truth maker of tests/nav_ref.py, the model's own invariants, and the
host-side argument checks of the C ABI.  No device is needed.

The truth's code phases are exact, so the reference must give the receiver back to the solver's own stopping step (POS_TOL, the
figure of tests/test_gpu_fix.py).  The times cannot be held to TIME_TOL of the four-state tests: the fifth unknown is observed only
through the satellites' motion (cdop ~ 1e-3 s per metre with eight satellites), which magnifies the 1e-7 m rounding of a range.  What
the reference reaches against the truth is MEASURED here and written down as RX_TIME_WORST and COARSE_S_WORST; the test asserts that
the measurement stays below them, and tests/test_gpu_coarse.py allows two fp64 evaluations of the same model -- which differ in
operation order only -- ten times that.
Measured (this file, the six cases of test_reference_recovers_the_truth, 78 fixes): position <= 3.7e-8 m, receive time and
coarse_s <= 6.3e-11 s (the 8 satellites at the week's end, cdop 1.9e-3 s/m; 1e-11 s elsewhere), rounding margin >= 0.26 ms, 3-4
passes.
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_ref
import nav_ref
from coarse_helpers import phases, priors, rx_error, times, truth_s
from nav_helpers import geometry

pytestmark = pytest.mark.usefixtures("hip_artifacts")  # the records' layouts and the host-side checks come from the library

POS_TOL = 1e-4            # metres: tests/test_gpu_fix.py's figure, the solver's own stopping step
RX_TIME_WORST = 7e-11     # seconds: the reference's receive time against the truth, measured 6.3e-11 (see above)
COARSE_S_WORST = 7e-11    # seconds: the same for the fifth unknown, measured 6.3e-11
MARGIN_MIN_MS = 0.05      # a case whose whole milliseconds were rounded closer than this is no test of the solver


def sets_of(geo):
    return {"8": geo["subsets"][8], "up": [k for k in range(12) if geo["elevation"][k] > 0]}


def make_case(which, name, n, seed, km=30.0, secs=30.0):
    """(geo, sel, ref_ms, t_rx, obs, truth tx_ms, prior) of n receive times"""
    geo = geometry(which)
    sel = sets_of(geo)[name] if isinstance(name, str) else list(name)
    ms, t_rx = times(n)
    ref_ms = (geo["ref_ms"] + ms) % nav_ref.WEEK_MS
    obs, tx_ms = phases(geo, sel, ref_ms, t_rx)
    return geo, sel, ref_ms, t_rx, obs, tx_ms, priors(geo, ref_ms, seed, km, secs)


# ---- 1. the reference against the truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8", "up"])
@pytest.mark.parametrize("which", ["north", "south", "rollover"])
def test_reference_recovers_the_truth(which, name):
    n = 30 if which == "rollover" else 6
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, name, n, seed=11)
    if which == "rollover":  # the receive times, and with +-30 s the priors, lie on both sides of the end of the week
        assert ref_ms.min() < 200 and ref_ms.max() > nav_ref.WEEK_MS - 200
        assert prior["rx_ms"].min() < 31_000 and prior["rx_ms"].max() > nav_ref.WEEK_MS - 31_000
    ref = coarse_ref.coarse_fix(geo["ephs"], obs, prior)
    assert all(r["status"] == coarse_ref.FIX_OK and r["n_used"] == len(sel) and r["ref"] == 0 and r["flags"] == 0 for r in ref)
    margin = min(r["margin"] for r in ref)
    dpos = max(np.abs(r["xyz"] - geo["rx"]).max() for r in ref)
    dt = np.abs(rx_error([r["rx_ms"] for r in ref], [r["rx_frac"] for r in ref], ref_ms, t_rx)).max()
    s_true = truth_s(ref, tx_ms, prior)
    ds = np.abs(np.array([r["coarse_s"] for r in ref]) - s_true).max()
    its = [r["iterations"] for r in ref]
    print("%s %s (%d satellites): position %.3g m, receive time %.3g s, coarse_s %.3g s (|s| %.4g s), margin %.3g ms, passes %d..%d, cdop %.3g s/m" %
          (which, name, len(sel), dpos, dt, ds, np.abs(s_true).max(), margin, min(its), max(its), max(r["cdop"] for r in ref)))
    assert margin >= MARGIN_MIN_MS
    assert dpos <= POS_TOL
    assert dt <= RX_TIME_WORST and ds <= COARSE_S_WORST
    assert np.abs(s_true).min() > 29.9 and max(its) <= 8  # the priors were 30 s off, and the whole of it came out of the solve
    # the whole milliseconds are the truth's up to one common integer
    for i, r in enumerate(ref):
        d = nav_ref.fold_ms(tx_ms[i] - prior["rx_ms"][i]) - r["N"]
        assert len(set(d.tolist())) == 1, (i, d)


def test_the_fifth_unknown_is_needed():
    """the same rows with s held at 0: a prior 30 s off puts every satellite 100 km from where it was, and the four-state fix
    lands kilometres away or nowhere"""
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 4, seed=11)
    held = coarse_ref.coarse_fix(geo["ephs"], obs, prior, hold_s=True)
    off = [np.linalg.norm(r["xyz"] - geo["rx"]) if r["status"] == coarse_ref.FIX_OK else np.inf for r in held]
    print("s held at 0: position error", ["%.3g" % v for v in off])
    assert min(off) > 1e3


# ---- 2. the invariant: the four-state fix on obs_out ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["north", "rollover"])
def test_four_state_fix_on_obs_out_is_the_coarse_fix(which):
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, "8", 5, seed=23)
    rng = np.random.default_rng(5)
    obs["tx_frac"] = (obs["tx_frac"] + rng.uniform(-100e-9, 100e-9, obs.shape)) % 1e-3  # 30 m of noise: a fix with residuals
    obs["weight"] = rng.uniform(0.3, 1.0, obs.shape)
    worst = 0.0
    for i, r in enumerate(coarse_ref.coarse_fix(geo["ephs"], obs, prior)):
        assert r["status"] == coarse_ref.FIX_OK and r["rms"] > 1.0
        cols = sorted(r["obs_out"])
        four = nav_ref.fix(geo["ephs"], [sel[k] for k in cols], [r["obs_out"][k][0] for k in cols], [r["obs_out"][k][1] for k in cols],
                           obs["weight"][i, cols])
        assert four["ok"]
        dt = abs(float(nav_ref.fold_ms(four["rx_ms"] - r["rx_ms"])) * 1e-3 + four["rx_frac"] - r["rx_frac"])
        worst = max(worst, np.abs(four["xyz"] - r["xyz"]).max())
        assert dt < 1e-3 / nav_ref.C * 10  # the same place in light time
    print("%s: four-state fix on obs_out against the coarse fix: %.3g m" % (which, worst))
    assert worst <= 1e-3  # ten stopping steps


# ---- 3. a false peak -------------------------------------------------------------------------------------------------------------
def test_a_false_peak_sets_inconsistent():
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 4, seed=31)
    clean = coarse_ref.coarse_fix(geo["ephs"], obs, prior)
    bad = obs.copy()
    bad["tx_frac"][:, 3] = (bad["tx_frac"][:, 3] + 0.3e-3) % 1e-3
    flagged = coarse_ref.coarse_fix(geo["ephs"], bad, prior)
    print("rms clean %.3g m, with a peak 0.3 ms off %.3g .. %.3g m" % (max(r["rms"] for r in clean), min(r["rms"] for r in flagged), max(r["rms"] for r in flagged)))
    assert all(r["status"] == 0 and r["flags"] == 0 for r in clean)
    assert all(r["status"] == 0 and r["flags"] == coarse_ref.INCONSISTENT and r["rms"] > 5e3 for r in flagged)
    five = coarse_ref.coarse_fix(geo["ephs"], bad[:, :5], prior)  # no satellite to spare: nothing to judge by
    assert all(r["flags"] == 0 for r in five)


# ---- 4. peaks into observations ------------------------------------------------------------------------------------------------
def test_coarse_obs_arithmetic():
    import gpsacq
    fs = 5.456e6
    pk = np.zeros((2, 6), gpsacq.PEAK_DTYPE)
    pk["snr"] = [[30, 24.99, 25, np.nan, 40, 40], [26, 26, 26, 26, 26, -1]]
    pk["ca_shift"] = [[0, 100, 5455, 7, 5456, -1], [1, 2728, 5455, 5000, 4, 9]]
    valid, eph, frac, weight = coarse_ref.coarse_obs(pk, fs, 25.0)
    assert valid.tolist() == [[True, False, True, False, False, False], [True, True, True, True, True, False]]
    assert eph[1].tolist() == [0, 1, 2, 3, 4, 0] and weight[1].tolist() == [1, 1, 1, 1, 1, 0]
    assert frac[0, 2] == 5455 / fs and frac[1, 1] == 0.5e-3 and ((frac >= 0) & (frac < 1e-3)).all()
    # a code position cut to whole samples is the truth's fraction to within a sample
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 3, seed=1)
    pk = np.zeros(obs.shape, gpsacq.PEAK_DTYPE)
    pk["snr"], pk["ca_shift"] = 100.0, np.floor(obs["tx_frac"] * fs)
    _, _, frac, _ = coarse_ref.coarse_obs(pk, fs, 25.0)
    assert (np.abs(frac - obs["tx_frac"]) < 1.0 / fs).all()


# ---- 5. the host side of the C ABI ---------------------------------------------------------------------------------------------
def test_records_and_default_params():
    import gpsacq
    assert gpsacq.COARSE_PRIOR_DTYPE.itemsize == 32 and gpsacq.COARSE_PARAMS_DTYPE.itemsize == 16 and gpsacq.COARSE_INFO_DTYPE.itemsize == 40
    p = gpsacq.coarse_params()
    assert p["rms_max_m"][0] == 2.99792458e8 / 1.023e6 and abs(p["rms_max_m"][0] - 293.05) < 0.005 and p["reserved"][0] == 0
    assert gpsacq.coarse_params(rms_max_m=50.0)["rms_max_m"][0] == 50.0
    assert gpsacq.load_library().gpsacq_coarse_default_params(None) == 1
    pr = gpsacq.coarse_prior([1.0, 2.0, 3.0], 604_799_999, n_fix=3)
    assert pr.shape == (3,) and pr["y"].tolist() == [2.0] * 3 and pr["rx_ms"].tolist() == [604_799_999] * 3
    pr = gpsacq.coarse_prior(np.arange(6.0).reshape(2, 3), [5, 6])
    assert pr["z"].tolist() == [2.0, 5.0] and pr["rx_ms"].tolist() == [5, 6]


def test_argument_errors_without_an_engine():
    import gpsacq
    lib = gpsacq.load_library()
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 2, seed=1)
    from nav_helpers import to_records
    rec = to_records(geo["ephs"])
    fix, info = np.zeros(2, gpsacq.FIX_DTYPE), np.zeros(2, gpsacq.COARSE_INFO_DTYPE)
    out, pk = np.zeros_like(obs), np.zeros(obs.shape, gpsacq.PEAK_DTYPE)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpsacq_coarse_fix_batch(None, p(rec), 12, p(obs), p(prior), 2, 8, None, p(fix), p(info), p(out)) == 1
    assert lib.gpsacq_coarse_fix_batch_device(None, p(rec), 12, p(obs), p(prior), 2, 8, None, p(fix), p(info), None, 1) == 1
    assert lib.gpsacq_coarse_obs(None, p(pk), 2, 8, 25.0, p(out)) == 1
    assert lib.gpsacq_coarse_obs_device(None, p(pk), 2, 8, 25.0, p(out), 1) == 1
    assert lib.gpsacq_coarse_fix_peaks_device(None, p(rec), 12, p(pk), 2, 8, 25.0, p(prior), None, None, p(fix), p(info), None, 1) == 1
    assert lib.gpsacq_coarse_last_ms(None, None, None) == 1
    assert not fix.view(np.uint8).any() and not info.view(np.uint8).any() and not out.view(np.uint8).any()
