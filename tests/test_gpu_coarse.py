"""Coarse-time fixes on the GPU (gpsacq_coarse_obs*, gpsacq_coarse_fix_batch*, gpsacq_coarse_fix_peaks_device) against
tests/coarse_ref.py, the numpy restatement of "Coarse-time fixes: positions from code phases alone" of include/gpsacq.h.

Tolerances.  Position: POS_TOL = 1e-4 m, the solver's stopping step, as in tests/test_gpu_fix.py.  Times (receive time, coarse_s):
ten times what tests/test_coarse.py measured of the reference against the truth (RX_TIME_WORST, COARSE_S_WORST) -- two fp64
evaluations of one model differ in operation order only, and cdop magnifies the rounding of a range into the fifth unknown.  Those
constants were measured with eight and more satellites, cdop <= CDOP_MEASURED = 1.9e-3 s/m; a row whose own cdop is larger (five
or six satellites) is allowed that much more, in proportion, because the error IS cdop times the range rounding.  bias_m = c (s -
(rx - t0)) is held to c times the two time tolerances.  pdop and cdop: 1e-9 relative.  obs_out: whole milliseconds equal, tx_frac
within 1e-12 s of (the reference's tx_frac + the difference of the two coarse_s): the transmit times are t0 + T_k + s, so whatever
separates the two s separates them, and what is left is the split's rounding.
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_ref
import nav_ref
from coarse_helpers import block_times, phases, priors, rx_error, synth_sats
from nav_helpers import geometry, to_records
from test_coarse import COARSE_S_WORST, POS_TOL, RX_TIME_WORST, make_case

pytestmark = pytest.mark.gpu

TIME_TOL, S_TOL = 10 * RX_TIME_WORST, 10 * COARSE_S_WORST
CDOP_MEASURED = 1.9e-3
FS, FC = 5.456e6, 4.092e6


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


def compare(fix, info, oo, ref, obs, label):
    """every record of a batch against the reference's rows; prints the measured maxima"""
    n = len(ref)
    assert fix["status"].tolist() == [r["status"] for r in ref], label
    assert fix["n_used"].tolist() == [r["n_used"] for r in ref] and info["ref"].tolist() == [r["ref"] for r in ref], label
    assert info["flags"].tolist() == [r["flags"] for r in ref], label
    assert all(abs(int(fix["iterations"][i]) - ref[i]["iterations"]) <= 1 for i in range(n)), (label, fix["iterations"], [r["iterations"] for r in ref])
    worst = dict(pos=0.0, rx=0.0, s=0.0, b=0.0, dop=0.0, frac=0.0, rms=0.0)
    for i, r in enumerate(ref):
        if r["status"] != coarse_ref.FIX_OK:  # every double 0, rx_ms 0, no observation out
            assert fix[i].tobytes()[16:] == bytes(64) and fix["rx_ms"][i] == 0 and info[i].tobytes()[8:] == bytes(32), (label, i)
            assert oo[i].tobytes() == bytes(32 * oo.shape[1]), (label, i)
            continue
        scale = max(1.0, r["cdop"] / CDOP_MEASURED)
        dpos = np.abs(np.array([fix["x"][i], fix["y"][i], fix["z"][i]]) - r["xyz"]).max()
        drx = abs(float(nav_ref.fold_ms(int(fix["rx_ms"][i]) - r["rx_ms"])) * 1e-3 + (fix["rx_frac"][i] - r["rx_frac"]))
        ds = info["coarse_s"][i] - r["coarse_s"]
        db = abs(info["bias_m"][i] - r["bias_m"])
        ddop = max(abs(info["pdop"][i] / r["pdop"] - 1), abs(info["cdop"][i] / r["cdop"] - 1)) if r["pdop"] > 0 else max(info["pdop"][i], info["cdop"][i])
        assert dpos <= POS_TOL, (label, i, dpos)
        assert drx <= TIME_TOL * scale and abs(ds) <= S_TOL * scale, (label, i, drx, ds, scale)
        assert db <= nav_ref.C * (TIME_TOL + S_TOL) * scale, (label, i, db)
        assert ddop <= 1e-9, (label, i, ddop, info["pdop"][i], r["pdop"], info["cdop"][i], r["cdop"])
        assert abs(fix["lat"][i] - r["lat"]) <= 1e-10 and abs(fix["lon"][i] - r["lon"]) <= 1e-10 and abs(fix["alt"][i] - r["alt"]) <= 2 * POS_TOL
        assert 0 <= fix["rx_frac"][i] < 1e-3 and 0 <= fix["rx_ms"][i] < nav_ref.WEEK_MS
        if fix["iterations"][i] == r["iterations"]:  # rms belongs to the residuals the last step was made from
            worst["rms"] = max(worst["rms"], abs(fix["rms"][i] - r["rms"]))
            assert abs(fix["rms"][i] - r["rms"]) <= POS_TOL + 1e-9 * r["rms"], (label, i, fix["rms"][i], r["rms"])
        for k in range(oo.shape[1]):
            if k not in r["obs_out"]:
                assert oo[i, k].tobytes() == bytes(32), (label, i, k)
                continue
            ms, frac = r["obs_out"][k]
            assert oo["valid"][i, k] == 1 and oo["eph"][i, k] == obs["eph"][i, k] and oo["weight"][i, k] == obs["weight"][i, k] and oo["reserved"][i, k] == 0
            assert 0 <= oo["tx_frac"][i, k] < 1e-3
            dfrac = float(nav_ref.fold_ms(int(oo["tx_ms"][i, k]) - ms)) * 1e-3 + (oo["tx_frac"][i, k] - frac) - ds
            if 1e-8 < frac < 1e-3 - 1e-8:  # away from the millisecond's edge the two splits cannot differ
                assert oo["tx_ms"][i, k] == ms, (label, i, k)
            assert abs(dfrac) <= 1e-12, (label, i, k, dfrac)
            worst["frac"] = max(worst["frac"], abs(dfrac))
        worst.update(pos=max(worst["pos"], dpos), rx=max(worst["rx"], drx / scale), s=max(worst["s"], abs(ds) / scale), b=max(worst["b"], db / scale),
                     dop=max(worst["dop"], ddop))
    print("%s: position %.3g m, receive time %.3g s, coarse_s %.3g s, bias %.3g m, dop %.3g rel, obs_out frac %.3g s, rms %.3g m" %
          (label, worst["pos"], worst["rx"], worst["s"], worst["b"], worst["dop"], worst["frac"], worst["rms"]))


# ---- 1. the wave boundary ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """130 rows of the northern receiver's eight satellites, priors 30 km / +-30 s off, and the reference of them, made once"""
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 130, seed=7)
    ref = coarse_ref.coarse_fix(geo["ephs"], obs, prior)
    assert min(r["margin"] for r in ref) >= 0.05 and all(r["status"] == 0 for r in ref)
    obs.setflags(write=False)
    return geo, ref_ms, t_rx, obs, prior, ref, to_records(geo["ephs"])


@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 130])
def test_wave_boundary(eng, batch, n_fix):
    geo, ref_ms, t_rx, obs, prior, ref, rec = batch
    fix, info, oo = eng.coarse_fix(rec, obs[:n_fix], prior[:n_fix])
    compare(fix, info, oo, ref[:n_fix], obs, "n_fix %d" % n_fix)
    dpos = np.abs(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"]).max()
    dt = np.abs(rx_error(fix["rx_ms"], fix["rx_frac"], ref_ms[:n_fix], t_rx[:n_fix])).max()
    print("n_fix %d against the truth: position %.3g m, receive time %.3g s, passes %d..%d" % (n_fix, dpos, dt, fix["iterations"].min(), fix["iterations"].max()))
    assert dpos <= POS_TOL and dt <= TIME_TOL + RX_TIME_WORST
    assert (np.abs(info["coarse_s"]) > 29.9).all()


# ---- 2. row shapes -------------------------------------------------------------------------------------------------------------
def shaped_rows(which, sats, seed):
    """seven rows of `sats` columns: untouched; column 0 not valid; weights in [0.3, 1] over 30 m of noise; a weight-0
    observation; tx_frac = 1e-3 and NaN; four usable; nothing usable"""
    geo = geometry(which)
    up = [k for k in range(12) if geo["elevation"][k] > 0]
    sel = {12: list(range(12)), 6: nav_ref.best_subset(geo["rx"], geo["sat_xyz"], up, 6)[0]}.get(sats) or geo["subsets"][sats]
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, sel, 7, seed=seed)
    rng = np.random.default_rng(seed)
    obs["valid"][1, 0] = 0
    obs["tx_frac"][2] = (obs["tx_frac"][2] + rng.uniform(-100e-9, 100e-9, sats)) % 1e-3
    obs["weight"][2] = rng.uniform(0.3, 1.0, sats)
    obs["weight"][3, 1] = 0.0
    obs["tx_frac"][3, 1] = (obs["tx_frac"][3, 1] + 0.4e-3) % 1e-3  # what a weight of 0 must keep out of the fix
    obs["tx_frac"][4, 0], obs["tx_frac"][4, 2] = 1e-3, np.nan
    obs["valid"][5, 4:] = 0
    obs["valid"][6, :] = 0
    return geo, obs, prior


@pytest.mark.parametrize("sats", [5, 6, 8, 12])
def test_row_shapes(eng, sats):
    import gpsacq
    geo, obs, prior = shaped_rows("north", sats, 40 + sats)
    ref = coarse_ref.coarse_fix(geo["ephs"], obs, prior)
    fix, info, oo = eng.coarse_fix(to_records(geo["ephs"]), obs, prior)
    assert info["ref"].tolist() == [0, 1, 0, 0, 1, 0, -1]
    assert fix["n_used"].tolist() == [sats, sats - 1, sats, sats, sats - 2, 4, 0]
    assert fix["status"][5] == gpsacq.FIX_TOO_FEW and fix["status"][6] == gpsacq.FIX_TOO_FEW and fix["status"][0] == 0
    if sats >= 7:
        assert (fix["status"][:5] == 0).all() and (info["flags"][:5] == 0).all()
        assert fix["rms"][2] > 1.0 and fix["rms"][3] < 0.01  # the weights mattered; the weight-0 observation, 120 km off, did not
    for name in fix.dtype.names:
        assert np.isfinite(fix[name].astype(np.float64)).all(), name
    compare(fix, info, oo, ref, obs, "north, %d per row" % sats)


@pytest.mark.parametrize("which", ["rollover", "south"])
def test_other_geometries(eng, which):
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, "8", 30 if which == "rollover" else 6, seed=11)
    if which == "rollover":  # t0 on either side of the end of the week
        assert prior["rx_ms"].min() < 31_000 and prior["rx_ms"].max() > nav_ref.WEEK_MS - 31_000
    ref = coarse_ref.coarse_fix(geo["ephs"], obs, prior)
    fix, info, oo = eng.coarse_fix(to_records(geo["ephs"]), obs, prior)
    compare(fix, info, oo, ref, obs, which)
    assert (fix["status"] == 0).all()
    assert np.abs(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"]).max() <= POS_TOL


# ---- 3. the invariant ----------------------------------------------------------------------------------------------------------
def test_four_state_fix_on_obs_out(eng):
    geo, obs, prior = shaped_rows("north", 8, 48)
    rec = to_records(geo["ephs"])
    fix, info, oo = eng.coarse_fix(rec, obs, prior)
    four = eng.fix(rec, oo)
    ok = fix["status"] == 0
    assert ok.sum() == 5 and (four["status"][ok] == 0).all() and (four["n_used"][ok] == fix["n_used"][ok]).all()
    d = np.abs(np.stack([four[k][ok] - fix[k][ok] for k in "xyz"])).max()
    dt = np.abs(nav_ref.fold_ms(four["rx_ms"][ok].astype(np.int64) - fix["rx_ms"][ok]) * 1e-3 + (four["rx_frac"][ok] - fix["rx_frac"][ok])).max()
    print("gpsacq_fix_batch on obs_out against the coarse fix: %.3g m, %.3g s (rms of the noisy row %.3g m)" % (d, dt, fix["rms"][2]))
    assert d <= 1e-3 and dt <= 1e-3 / nav_ref.C * 10
    assert (four["status"][~ok] == 1).all()  # nothing came out of the rows that failed


# ---- 4. device forms -----------------------------------------------------------------------------------------------------------
def test_device_forms(eng):
    import gpsacq
    import torch
    geo, obs, prior = shaped_rows("north", 8, 48)
    rec = to_records(geo["ephs"])
    n, m = obs.shape
    host = eng.coarse_fix(rec, obs, prior)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs, d_prior = dev(obs), dev(prior)
    d_fix, d_info, d_out = fill(n * 80), fill(n * 40), fill(n * m * 32)
    d_fix2, d_info2 = fill(n * 80), fill(n * 40)
    torch.cuda.synchronize()
    eng.coarse_fix_device(rec, d_obs.data_ptr(), d_prior.data_ptr(), n, m, d_fix.data_ptr(), d_info.data_ptr(), d_out.data_ptr(), sync=False)
    eng.coarse_fix_device(rec, d_obs.data_ptr(), d_prior.data_ptr(), n, m, d_fix2.data_ptr(), d_info2.data_ptr(), None, sync=True)
    assert d_fix.cpu().numpy().tobytes() == host[0].tobytes() and d_info.cpu().numpy().tobytes() == host[1].tobytes()
    assert d_out.cpu().numpy().tobytes() == host[2].tobytes()
    assert d_fix2.cpu().numpy().tobytes() == host[0].tobytes() and d_info2.cpu().numpy().tobytes() == host[1].tobytes()  # obs_out NULL
    obs_ms, fix_ms = eng.coarse_last_ms()
    assert fix_ms > 0
    # peaks -> observations: the numpy line, then the chain against its two halves
    pk = np.zeros((n, m), gpsacq.PEAK_DTYPE)
    pk["snr"], pk["ca_shift"] = 60.0, np.floor(np.nan_to_num(obs["tx_frac"]) * FS)
    pk["snr"][1, 0], pk["ca_shift"][3, 1], pk["ca_shift"][4, 2], pk["ca_shift"][5, 4:] = 24.0, 5456, -1, -1  # [4, 0] is 5456 already
    po = eng.coarse_obs(pk, snr_min=25.0)
    valid, eph, frac, weight = coarse_ref.coarse_obs(pk, FS, 25.0)
    assert (po["valid"] == valid).all() and (po["eph"] == eph).all() and (po["tx_frac"] == frac).all() and (po["weight"] == weight).all()
    assert not po["tx_ms"].any() and not po["reserved"].any() and po[~valid].tobytes() == bytes(32 * int((~valid).sum()))
    assert valid.sum() == n * m - 1 - 1 - 2 - 4
    d_pk = dev(pk)
    d_po, d_fix3, d_info3, d_out3 = fill(n * m * 32), fill(n * 80), fill(n * 40), fill(n * m * 32)
    d_fix4, d_info4, d_out4 = fill(n * 80), fill(n * 40), fill(n * m * 32)
    torch.cuda.synchronize()
    eng.coarse_obs_device(d_pk.data_ptr(), n, m, d_po.data_ptr(), snr_min=25.0, sync=False)
    eng.coarse_fix_device(rec, d_po.data_ptr(), d_prior.data_ptr(), n, m, d_fix3.data_ptr(), d_info3.data_ptr(), d_out3.data_ptr(), sync=True)
    assert d_po.cpu().numpy().tobytes() == po.tobytes()
    eng.coarse_fix_peaks_device(rec, d_pk.data_ptr(), n, m, d_prior.data_ptr(), d_fix4.data_ptr(), d_info4.data_ptr(), d_obs_ptr=None,
                                d_obs_out_ptr=d_out4.data_ptr(), snr_min=25.0, sync=True)
    assert d_fix4.cpu().numpy().tobytes() == d_fix3.cpu().numpy().tobytes() and d_info4.cpu().numpy().tobytes() == d_info3.cpu().numpy().tobytes()
    assert d_out4.cpu().numpy().tobytes() == d_out3.cpu().numpy().tobytes()
    chain = d_fix4.cpu().numpy().view(gpsacq.FIX_DTYPE)
    assert chain["status"].tolist()[:5] == [0] * 5 and chain["n_used"].tolist() == [8, 7, 8, 7, 6, 4, 8]
    obs_ms, fix_ms = eng.coarse_last_ms()
    assert obs_ms > 0 and fix_ms > 0
    # argument errors launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out = [np.zeros(n, gpsacq.FIX_DTYPE), np.zeros(n, gpsacq.COARSE_INFO_DTYPE), np.zeros((n, m), gpsacq.OBS_DTYPE)]
    ob = np.ascontiguousarray(obs)
    for sats in (0, 13):
        assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), p(prior), n, sats, None, p(out[0]), p(out[1]), p(out[2])) == 1
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), None, n, m, None, p(out[0]), p(out[1]), p(out[2])) == 1
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), p(prior), n, m, None, p(out[0]), None, p(out[2])) == 1
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), p(prior), n, m, None, p(out[0]), p(out[1]), p(ob)) == 1
    bad = gpsacq.coarse_params(rms_max_m=0.0)
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), p(prior), n, m, p(bad), p(out[0]), p(out[1]), p(out[2])) == 1
    assert b"rms_max_m" in lib.gpsacq_last_error()
    late = prior.copy()
    late["rx_ms"][2] = nav_ref.WEEK_MS
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(ob), p(late), n, m, None, p(out[0]), p(out[1]), p(out[2])) == 1
    w = ob.copy()
    w["weight"][0, 3] = -1.0
    assert lib.gpsacq_coarse_fix_batch(h, p(rec), 12, p(w), p(prior), n, m, None, p(out[0]), p(out[1]), p(out[2])) == 1
    assert lib.gpsacq_coarse_obs(h, p(pk), n, 13, 25.0, p(out[2])) == 1 and lib.gpsacq_coarse_obs(h, p(pk), n, m, float("nan"), p(out[2])) == 1
    assert not any(a.view(np.uint8).any() for a in out)
    # the device form cannot read the prior: a row whose prior names no instant has nothing usable
    d_late = dev(late)
    torch.cuda.synchronize()
    eng.coarse_fix_device(rec, d_obs.data_ptr(), d_late.data_ptr(), n, m, d_fix2.data_ptr(), d_info2.data_ptr(), None, sync=True)
    got = d_fix2.cpu().numpy().view(gpsacq.FIX_DTYPE)
    assert got["status"][2] == gpsacq.FIX_TOO_FEW and got["n_used"][2] == 0 and got[[0, 1, 3]].tobytes() == host[0][[0, 1, 3]].tobytes()


# ---- 5. a false peak -----------------------------------------------------------------------------------------------------------
def test_a_false_peak_sets_inconsistent(eng):
    import gpsacq
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 4, seed=31)
    rec = to_records(geo["ephs"])
    clean = eng.coarse_fix(rec, obs, prior)
    bad = obs.copy()
    bad["tx_frac"][:, 3] = (bad["tx_frac"][:, 3] + 0.3e-3) % 1e-3
    fix, info, _ = eng.coarse_fix(rec, bad, prior)
    print("rms with a peak 0.3 ms off: %.3g .. %.3g m" % (fix["rms"].min(), fix["rms"].max()))
    assert (clean[0]["status"] == 0).all() and (clean[1]["flags"] == 0).all()
    assert (fix["status"] == 0).all() and (info["flags"] == gpsacq.COARSE_INCONSISTENT).all() and (fix["rms"] > 5e3).all()
    loose = eng.coarse_fix(rec, bad, prior, params=gpsacq.coarse_params(rms_max_m=1e5))
    assert (loose[1]["flags"] == 0).all() and loose[0].tobytes() == fix.tobytes()


# ---- 6. end to end: generated blocks, search, coarse fix ----------------------------------------------------------------------
def test_end_to_end_from_search_peaks(eng):
    import gpsacq
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, spb, spm = 4, gpsacq.BLOCK_BYTES * 8, FS / 1000.0
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3  # the receive time of the first sample of block 0
    sats, dops = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.2)
    bits = eng.generate(n_blocks * gpsacq.BLOCK_BYTES, sats, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = [(b, s[0] - 1) for b in range(n_blocks) for s in sats]
    _, peaks = eng.search(bits, tasks=tasks, want_cells=False)
    peaks = peaks.reshape(n_blocks, len(sel))
    # first the search alone: every code phase within one sample of the truth's code position at its block's first sample
    blk_ms, blk_frac = block_times(ref_ms, ref_frac, n_blocks, spb, FS)
    truth = np.stack([nav_ref.truth_tx(e, geo["rx"], blk_ms, blk_frac) for e in ephs], 1)  # offsets from blk_ms
    want = (truth % 1e-3) * FS
    off = (peaks["ca_shift"] - want + spm / 2) % spm - spm / 2
    print("snr %.0f .. %.0f, code phase against the truth %.2f .. %.2f samples" % (peaks["snr"].min(), peaks["snr"].max(), off.min(), off.max()))
    assert (peaks["snr"] >= gpsacq.THRESHOLD).all() and (np.abs(off) <= 1.0).all()
    assert (np.abs(peaks["lo_shift"] - np.rint(dops * 40000 / FS)[None, :]) <= 1).all()
    # then the fix, from a prior 30 km / 20 s off
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    obs = eng.coarse_obs(peaks)
    fix, info, oo = eng.coarse_fix(to_records(ephs), obs, prior)
    assert (fix["status"] == 0).all() and (fix["n_used"] == 8).all() and (info["flags"] == 0).all()
    # the worst a sample per range can do: |G_pos|_2 sqrt(8) c / fs, G the position rows of (H^T H)^-1 H^T at the truth
    exact, _ = phases(geo, sel, blk_ms, blk_frac)
    H = coarse_ref.coarse_fix(geo["ephs"], exact, prior)[0]["H"]
    G = np.linalg.solve(H.T @ H, H.T)[:3]
    bound = np.linalg.norm(G, 2) * np.sqrt(8.0) * nav_ref.C / FS
    err = np.linalg.norm(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"], axis=1)
    dt = np.abs(rx_error(fix["rx_ms"], fix["rx_frac"], blk_ms, blk_frac))
    print("position error %s m (bound %.0f m), receive time error %s s, rms %s m" % (np.round(err, 1), bound, dt, np.round(fix["rms"], 1)))
    assert (err <= bound).all()
