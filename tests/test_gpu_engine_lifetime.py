"""The engine's own plumbing, seen through gpsacq.Engine: what the *_last_ms calls say before anything ran and about a stage
that did not run, and scratch that grows, is reused and is given back (csrc/gpsacq_engine.hpp: Scratch<T>, Stages<N>).

Free device memory is not read anywhere here: the card is shared, and the figure belongs to every process on it.  That no
buffer leaks follows from the engine's members freeing themselves."""
import numpy as np
import pytest

import nav_ref
from nav_helpers import geometry, to_records, truth_obs

pytestmark = pytest.mark.gpu

ENGINE = (4.092e6, 5.456e6, 5000.0)
ERR_ARG = 1  # GPSACQ_ERR_ARG
N_CHANS = 4


def _last_ms_methods(eng):
    return sorted(n for n in dir(eng) if n.endswith("_last_ms"))


def _peaks(n_fix, seed=0):
    """non-trivial peaks [n_fix][N_CHANS]: snr on both sides of the default threshold, every code phase different"""
    import gpsacq
    rng = np.random.default_rng(seed)
    pk = np.zeros((n_fix, N_CHANS), gpsacq.PEAK_DTYPE)
    pk["snr"] = np.where(np.arange(n_fix * N_CHANS).reshape(n_fix, N_CHANS) % 3 == 1, 11.5, 80.0 + rng.random((n_fix, N_CHANS)) * 40)
    pk["lo_shift"] = rng.integers(-36, 37, (n_fix, N_CHANS))
    pk["ca_shift"] = rng.integers(0, 5456, (n_fix, N_CHANS))
    pk["max_pwr"] = 1e6 * (1 + rng.random((n_fix, N_CHANS)))
    return pk


@pytest.fixture(scope="module")
def fix_case():
    """ephemerides and exact observations [3][4] of the synthetic constellation (tests/nav_helpers.py), made once, read-only"""
    geo = geometry("north")
    ref_ms = (geo["ref_ms"] + np.arange(3, dtype=np.int64)) % nav_ref.WEEK_MS
    obs = truth_obs(geo, ref_ms, np.array([0.137e-3, 0.150e-3, 0.163e-3]))[:, geo["subsets"][8]][:, :N_CHANS].copy()
    obs.setflags(write=False)
    return to_records(geo["ephs"]), obs


def test_last_ms_before_any_call():
    import gpsacq
    with gpsacq.Engine(*ENGINE) as eng:
        names = _last_ms_methods(eng)
        assert len(names) >= 11 and "fix_atm_last_ms" in names and "track_iq8_last_ms" in names
        for name in names:
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                getattr(eng, name)()
            assert ei.value.code == ERR_ARG, name


def test_stage_that_did_not_run_reads_zero(fix_case):
    import gpsacq
    import torch
    zeros = np.zeros((2, N_CHANS), gpsacq.PEAK_DTYPE)
    with gpsacq.Engine(*ENGINE) as eng:
        eng.coarse_obs(zeros)
        obs_ms, fix_ms = eng.coarse_last_ms()
        assert fix_ms == 0.0 and obs_ms >= 0.0
    with gpsacq.Engine(*ENGINE) as eng:
        eng.coarse_obs(zeros, fine=np.zeros(zeros.shape, gpsacq.FINE_DTYPE))
        refine_ms, obs_ms = eng.refine_last_ms()
        assert refine_ms == 0.0 and obs_ms >= 0.0
    with gpsacq.Engine(*ENGINE) as eng:
        eng.rate_obs_fine(zeros, np.zeros(zeros.shape, gpsacq.DOPFINE_DTYPE))
        fine_dop_ms, rate_obs_ms, doppler_fix_ms = eng.doppler_last_ms()
        assert fine_dop_ms == 0.0 and doppler_fix_ms == 0.0 and rate_obs_ms >= 0.0
    rec, obs = fix_case
    with gpsacq.Engine(*ENGINE) as eng:
        eng.sat_rates(rec, obs[:2])  # records no events: neither half of the velocity timers has run
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.velocity_last_ms()
        assert ei.value.code == ERR_ARG
        d_obs = torch.from_numpy(obs[:2].copy().view(np.uint8).reshape(-1)).to("cuda:0")
        d_fix = torch.zeros(2 * gpsacq.FIX_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.fix_atm_device(rec, d_obs.data_ptr(), 2, N_CHANS, gpsacq.atm_params(), d_fix.data_ptr())
        sat_state_ms, fix_atm_ms, sat_view_ms = eng.fix_atm_last_ms()
        assert sat_view_ms == 0.0 and sat_state_ms >= 0.0 and fix_atm_ms >= 0.0


def test_scratch_grows_and_is_reused(fix_case):
    import gpsacq
    import torch
    rec, obs = fix_case
    eng = gpsacq.Engine(*ENGINE)
    try:
        for n_fix in (1, 3, 2):  # grow, grow again, reuse
            pk = _peaks(n_fix, seed=n_fix)
            got = eng.coarse_obs(pk)
            assert 0 < int(got["valid"].sum()) < got.size  # snr on both sides of the threshold
            d_pk = torch.from_numpy(pk.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            d_obs = torch.full((pk.size * gpsacq.OBS_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.coarse_obs_device(d_pk.data_ptr(), n_fix, N_CHANS, d_obs.data_ptr())
            assert d_obs.cpu().numpy().tobytes() == got.tobytes()
            fix = eng.fix(rec, obs[:n_fix].copy())  # its upload shares d_nav_obs with the other host-buffer forms
            with gpsacq.Engine(*ENGINE) as fresh:
                assert fresh.coarse_obs(pk).tobytes() == got.tobytes()
                assert fresh.fix(rec, obs[:n_fix].copy()).tobytes() == fix.tobytes()
    finally:
        eng.close()
    with gpsacq.Engine(*ENGINE) as again:  # a closed engine gave everything back: the next one works
        pk = _peaks(2, seed=7)
        assert again.coarse_obs(pk)["valid"].any()
