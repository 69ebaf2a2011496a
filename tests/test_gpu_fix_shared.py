"""k_fix and k_fix_atm run ONE Newton iteration (csrc/nav_device.hpp's newton()): with no delays asked for (flags = 0) and an
elevation mask of -pi / 2, which drops nothing, gpsacq_fix_atm_batch is stage 0 alone and must give what gpsacq_fix_batch gives.

Integers equal; position, receive time and rms within tests/test_gpu_fix.py's tolerances (derived there: two fp64 solvers
compared pass for pass on the same observations).  Not bytes: the two kernels are different inlining contexts, so the compiler
may fuse multiply-adds differently.  Rows of 4 (the fewest usable) and 12 (the full row) satellites; 63, 64 and 65 fixes lie
either side of the wave boundary.  The observations carry 30 ns of noise and unequal weights, so every pass has work to do."""
import math

import numpy as np
import pytest

import nav_ref
from nav_helpers import geometry, to_records, truth_obs

pytestmark = pytest.mark.gpu

POS_TOL, TIME_TOL = 1e-4, 1e-12  # tests/test_gpu_fix.py's, derived in its docstring
N_MAX = 65


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def noisy_obs():
    """(geometry, obs[N_MAX][12]) of the northern receiver, 1 ms apart, made once and never written to"""
    geo = geometry("north")
    k = np.arange(N_MAX)
    obs = truth_obs(geo, (geo["ref_ms"] + k) % nav_ref.WEEK_MS, (0.137e-3 + k * 0.0131e-3) % 1e-3).copy()
    rng = np.random.default_rng(77)
    obs["tx_ms"], obs["tx_frac"] = nav_ref.split_time(obs["tx_ms"], obs["tx_frac"] + rng.uniform(-30e-9, 30e-9, obs.shape))
    obs["weight"] = rng.uniform(1.0, 100.0, obs.shape)
    obs.setflags(write=False)
    return geo, obs


@pytest.mark.parametrize("sats", [4, 5, 12])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65])
def test_fix_atm_without_atmosphere_is_fix(eng, noisy_obs, n_fix, sats):
    import gpsacq
    geo, obs = noisy_obs
    rec = to_records(geo["ephs"])
    ob = obs[:n_fix][:, geo["subsets"][sats]].copy()
    plain = eng.fix(rec, ob)
    atm, dop = eng.fix_atm(rec, ob, gpsacq.atm_params(flags=0, elev_mask=-math.pi / 2))
    assert (plain["status"] == gpsacq.FIX_OK).all() and (plain["n_used"] == sats).all() and (plain["iterations"] >= 3).all()
    for name in ("status", "n_used", "iterations", "rx_ms"):
        assert np.array_equal(plain[name], atm[name]), name
    assert (dop["used_mask"] == (1 << sats) - 1).all() and (dop["n_masked"] == 0).all()
    dpos = max(np.abs(plain[c] - atm[c]).max() for c in "xyz")
    dt = np.abs(plain["rx_frac"] - atm["rx_frac"]).max()  # rx_ms is equal
    drms = np.abs(plain["rms"] - atm["rms"]).max()
    dalt = np.abs(plain["alt"] - atm["alt"]).max()
    dll = max(np.abs(plain[c] - atm[c]).max() for c in ("lat", "lon"))
    print("n_fix %d sats %d: position %.3g m, receive time %.3g s, rms %.3g m, alt %.3g m, lat / lon %.3g rad (rms itself up to %.3g m)"
          % (n_fix, sats, dpos, dt, drms, dalt, dll, plain["rms"].max()))
    assert dpos <= POS_TOL and dt <= TIME_TOL and drms <= POS_TOL
    assert dalt <= POS_TOL and dll <= 1e-10  # test_gpu_fix.py's bounds on the geodetic output
    if sats > 4:
        assert plain["rms"].max() > 0.5  # the noise is metres of residual: the solve was not a trivial one
