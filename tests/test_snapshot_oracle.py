"""The fp64 references of the snapshot chain (coarse_ref, coarse_raim_ref, dop_ref, aided_ref) against
tests/golden/snapshot_oracle.npz: "Coarse-time fixes", "Cold snapshot fixes" 2 and "Aided acquisition" A of include/gpsacq.h evaluated
by tests/snapshot_oracle.py in mpmath at 40 digits, on the fix cases of tests/golden/nav_oracle.npz: 11 sites (the antimeridian
with y == 0 and y = +-1 m, 89.9 degrees north and south, -50 m to 9 km), constellations drawn over the whole field ranges of
IS-GPS-200 (a_f2 over its 8 bits, t_oc up to 2 h from t_oe, e up to 0.03), 8 instants each, the second site's on both sides of the
week's end.  No GPU, no engine.

coarse_ref, coarse_raim_ref and dop_ref must lie within a QUARTER of the tolerances tests/test_gpu_snapshot_oracle.py gives the
kernels, aided_ref.predict within a TENTH, so that what the GPU test measures is the kernel.  The fixture's preconditions are
asserted here (the GPU test relies on them): at least 8 columns at fix_el >= 5 degrees per row; step A's rounding margin for the
priors 30 km / 30 s off and for the Doppler-made ones; the near-tie rows; the prediction cases within 1e-6 of a rounding tie
(counted, at most 2 %, left out of the integer comparison only).

Which case catches which slip: each slip is made once in a CPU copy of the reference arithmetic and run against the fixture; a row
counts where the result leaves the GPU tolerance.  Every slip must be caught on at least a quarter of the rows and on at least one
row of every site; the counts are asserted as measured.
    Doppler fix, c d dropped from pred            88 of 88 rows
    Doppler fix, 2 a_f2 t dropped from d          88 of 88
    Doppler fix, t_oc read as t_oe in d           88 of 88
    Doppler fix, (-Omega y, Omega x, 0) flipped   88 of 88
    Doppler fix, tau held at 75 ms                88 of 88
    coarse fix, theta with the wrong sign         88 of 88
    coarse fix, h[4] without c d                  88 of 88 by cdop (beyond 1e-9 relative); the place survives in every row
    prediction, one light-time pass               176 of 176 fix rows
    prediction, cc left out of T                  176 of 176

Measured here (pytest -s prints them):
    columns at fix_el >= 5 degrees per row: 9 .. 10, column 0 among them in every row; step A's smallest margin from 30 km / 30 s: 0.21 ms
    (masked and all twelve); from the Doppler places made with rx_ms +-20 s off (3.67 .. 16.5 km from the site): 0.365 ms
    near-tie rows: 12 at 6 sites, 3.66e-5 .. 6.09e-5 ms from the tie, the other columns' margin >= 0.0667 ms; coarse_ref on the wrong side
    2.83e4 .. 7.15e4 m of rms
    predictions: none of 2124 within 1e-6 of a rounding tie (code or Doppler); 434 below 5 degrees, the closest 2.36 degrees from it;
    298 of the B rows' and all 12 of the last row's off the Doppler grid
    coarse_ref, masked / all twelve: place 1.06e-7 / 5.69e-8 m, receive time and coarse_s 0.129 / 0.0851 of their tolerance, pdop / cdop
    5.25e-14 / 4.06e-14 relative, lat 6.44e-15 rad, lon 1.52e-12 rad, alt 4.26e-7 m, obs_out frac 1.78e-15 s, 3..4 passes
    coarse_raim_ref: 88 EXCLUDED with the moved column, place 7.36e-8 m; largest statistic of the clean rows 2.28e-10
    dop_ref on the model Dopplers: place 5.76e-7 m, drift 1.65e-19, pdop 4.77e-12 relative (8.42e3 .. 1.59e4 m per m/s), rms 2.7e-8 m/s,
    lat 6.43e-14 rad, lon 2.12e-11 rad, alt 3.33e-7 m, 5..6 steps; on the physical ones (model minus physical at most 4.74e-3 m/s)
    0.934 .. 20.2 m from the site, at most 0.503 of the bound
    aided_ref.predict, 177 x 12: tx_frac 4.2e-16 s, doppler_hz 1.38e-10 Hz, elev_deg 1.14e-12 degrees, every ca_center and lo_center
    equal; the oracle's A rows against the truth: code phase 2.05e-9 s, 0.995 of cc (range rate / c + drift); Doppler on the drift-0
    instants 0.0122 Hz against (L1 / c) PER_SAT = 0.0142 Hz
    the slips move the place by: no c d 2.26e3 .. 1.37e4 m; no a_f2 28.4 .. 169 m; t_oc as t_oe 16.5 .. 124 m; receiver term flipped: no
    row converges to a consistent fix; tau held 1.78 .. 7.94 m; theta's sign 0.0868 .. 69.6 m; h[4] without c d: the place within
    1.45e-7 m, cdop 1.34e-4 .. 2e-3 relative; one light-time pass 2.39e-8 .. 6.03e-8 s of tx_frac; no cc 7.45e-4 .. 9.79e-4 s
    The fixture is 154 910 bytes and takes 35 s to make; without the regeneration this file runs in 11 s.
"""
import contextlib
import importlib.util
import math
import os

import numpy as np
import pytest

import aided_ref
import coarse_raim_ref
import coarse_ref
import dop_ref
import nav_ref
import raim_ref
import snapshot_oracle_data as sod
from snapshot_oracle_data import (AID_DOPPLER_TOL, AID_ELEV_TOL, AID_FRAC_TOL, ALT_TOL, CDOP_MEASURED, DOP_ALT_TOL, DOP_PDOP_REL, DOP_REL_TOL,
                                  DOP_RMS_TOL, DRIFT_TOL, EDGE, FIX_OK, FRAC_TOL, INCONSISTENT, LATLON_TOL, MARGIN_MIN_MS, PATH, PLACE_TOL, POS_TOL,
                                  RX_TOL, S_TOL, TIE_CAP, angle_diff, load, rows)

GEN_STEP_HZ, GEN_KMAX, GEN_FS, GEN_SPM = 5.456e6 / 40000, 36, 5.456e6, 5456   # hard-coded in tests/golden/make_snapshot_oracle.py
N_SITES = 11


# ---- 1. the fixture is what its generator writes -----------------------------------------------------------------------------------
def test_fixture_regenerates_byte_for_byte():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_snapshot_oracle", os.path.join(os.path.dirname(PATH), "make_snapshot_oracle.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(PATH, "rb") as f:
        committed = f.read()
    print("the fixture is %d bytes" % len(committed))
    assert len(committed) < 300 * 1024
    assert (gen.STEP_HZ, gen.KMAX, gen.FS, gen.SPM) == (GEN_STEP_HZ, GEN_KMAX, GEN_FS, GEN_SPM)
    assert gen.to_bytes(gen.build()) == committed


def test_fixture_is_under_the_cap_and_carries_its_engine():
    d = load()
    assert os.path.getsize(PATH) < 300 * 1024
    assert sod.engine_grid() == (GEN_FS, GEN_SPM, GEN_STEP_HZ, GEN_KMAX)


# ---- 2. the references' results, made once -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coarse():
    """coarse_ref on the code phases alone from the priors 30 km / +-30 s off: {masked: rows}"""
    return {m: coarse_ref.coarse_fix(sod.all_ephs(), sod.phase_obs(m), sod.priors(1)) for m in (True, False)}


@pytest.fixture(scope="module")
def doppler():
    """dop_ref on the model Dopplers at the true rx_ms"""
    return dop_ref.doppler_fix(sod.all_ephs(), sod.phase_obs(True), sod.rate_obs("model"), rows()["ref_ms"])


def coarse_errors(ref, masked):
    """per row: place, receive time over its tolerance, coarse_s over its tolerance, pdop / cdop relative, lat, lon, alt -- [n][7]"""
    d, r = load(), rows()
    orc = d["coarse_dop"].reshape(88, 2, 2)[:, 0 if masked else 1]
    out = np.full((len(ref), 7), np.inf)
    for i, x in enumerate(ref):
        if x["status"] != FIX_OK:
            continue
        scale = max(1.0, x["cdop"] / CDOP_MEASURED)
        dt = abs(float(sod.rx_error(x["rx_ms"], x["rx_frac"], [i])[0]))
        s_true = (int(sod.fold_ms(r["vac_ms"][i, x["ref"]] - sod.priors(1)["rx_ms"][i])) - int(x["N"][x["ref"]])) * 1e-3
        out[i] = [np.abs(x["xyz"] - r["site"][i]).max(), dt / (RX_TOL * scale), abs(x["coarse_s"] - s_true) / (S_TOL * scale),
                  max(abs(x["pdop"] / orc[i, 0] - 1), abs(x["cdop"] / orc[i, 1] - 1)), abs(x["lat"] - r["lla"][i, 0]),
                  float(angle_diff(x["lon"], r["lla"][i, 1])), abs(x["alt"] - r["lla"][i, 2])]
    return out


def coarse_caught(err):
    """rows a coarse-fix result leaves the GPU tolerance in"""
    return (err[:, 0] > POS_TOL) | (err[:, 1] > 1) | (err[:, 2] > 1) | (err[:, 3] > DOP_REL_TOL)


def doppler_errors(ref):
    """per row: place, drift, pdop relative, rms -- [n][4]"""
    d, r = load(), rows()
    out = np.full((len(ref), 4), np.inf)
    for i, x in enumerate(ref):
        if x["status"] == FIX_OK and x["flags"] == 0:
            out[i] = [np.linalg.norm(x["xyz"] - r["site"][i]), abs(x["drift"] - sod.drifts()[i]), abs(x["pdop"] / d["dop_pdop"].reshape(88, 2)[i, 0] - 1), x["rms"]]
    return out


def doppler_caught(err):
    return (err[:, 0] > PLACE_TOL) | (err[:, 1] > DRIFT_TOL) | (err[:, 2] > DOP_PDOP_REL) | (err[:, 3] > DOP_RMS_TOL)


# ---- 3. preconditions ----------------------------------------------------------------------------------------------------------------
def test_columns_and_margins(coarse):
    r = rows()
    n_up = r["up"].sum(axis=1)
    print("columns at fix_el >= 5 degrees per row: %d .. %d; column 0 among them in every row: %s" % (n_up.min(), n_up.max(), bool(r["up"][:, 0].all())))
    assert n_up.min() >= 8 and r["up"][:, 0].all()
    for m in (True, False):
        margin = min(x["margin"] for x in coarse[m])
        print("step A from 30 km / 30 s, %s: smallest margin %.3g ms" % ("masked" if m else "all twelve", margin))
        assert margin >= MARGIN_MIN_MS
    site = load()["fix_site"]
    pr = sod.priors(1)
    off = sod.fold_ms(pr["rx_ms"].astype(np.int64) - r["ref_ms"])
    assert set(off.tolist()) == {-30000, 30000}
    wk = pr["rx_ms"][8:16].astype(np.int64)   # the second site: t0 on both sides of the week's end
    assert wk.min() < 200_000 and wk.max() > sod.WEEK_MS - 200_000 and len(site) == N_SITES


def test_doppler_made_priors(doppler):
    """the chain's CPU form: dop_ref with rx_ms +-20 s off, its place as coarse_ref's prior"""
    r = rows()
    rx_ms = (r["ref_ms"] + np.where(np.arange(88) % 2 == 0, 20000, -20000)) % sod.WEEK_MS
    dop = dop_ref.doppler_fix(sod.all_ephs(), sod.phase_obs(True), sod.rate_obs("model"), rx_ms)
    assert all(x["status"] == FIX_OK and x["flags"] == 0 for x in dop)
    place = np.array([x["xyz"] for x in dop])
    dist = np.linalg.norm(place - r["site"], axis=1)
    ref = coarse_ref.coarse_fix(sod.all_ephs(), sod.phase_obs(True), sod.coarse_prior(place, rx_ms))
    margin = min(x["margin"] for x in ref)
    pos = max(np.abs(x["xyz"] - r["site"][i]).max() for i, x in enumerate(ref))
    print("Doppler places with rx_ms +-20 s off: %.3g .. %.3g km from the site; coarse_ref from them: margin %.3g ms, place %.3g m" %
          (dist.min() / 1e3, dist.max() / 1e3, margin, pos))
    assert dist.min() >= 1e3 and margin >= MARGIN_MIN_MS and all(x["status"] == FIX_OK for x in ref) and pos <= POS_TOL / 4


def test_near_tie_rows():
    d, r = load(), rows()
    T = len(d["tie_site"])
    assert len(set(d["tie_site"].tolist())) >= 4 and T == 2 * len(set(d["tie_site"].tolist()))
    assert (np.bincount(d["tie_side"]) == T // 2).all()
    obs, prior, row = sod.tie_case()
    gaps, margins = [], []
    for t in range(T):
        up = np.flatnonzero(r["up"][row[t]])
        k = int(d["tie_col"][t])
        assert k in up and k != up[0]
        x = d["tie_x"][t]
        gaps.append(abs(abs(x[k] - math.floor(x[k])) - 0.5))
        margins.append(min(0.5 - abs(x[c] - d["tie_N"][t, c]) for c in up[1:] if c != k))
        off = d["tie_N"][t, up] - sod.fold_ms(r["vac_ms"][row[t], up] - int(d["tie_rx_ms"][t]))
        wrong = off != off[0]
        assert (wrong.sum() == 0) if d["tie_side"][t] else (wrong.sum() == 1 and wrong[list(up).index(k)]), (t, off)
        assert np.linalg.norm(d["tie_xyz"][t] - r["site"][row[t]]) <= 100e3
        assert abs(int(sod.fold_ms(int(d["tie_rx_ms"][t]) - r["ref_ms"][row[t]]))) <= 30000
    print("near-tie rows: %d at %d sites; distance from the tie %.3g .. %.3g ms; the other columns' margin >= %.3g ms" %
          (T, T // 2, min(gaps), max(gaps), min(margins)))
    assert 1e-5 <= min(gaps) and max(gaps) <= 1e-4 and min(margins) >= 0.05
    # the reference rounds as the oracle does and meets what the GPU test asks of the kernel
    ref = coarse_ref.coarse_fix(sod.all_ephs(), obs, prior)
    for t, x in enumerate(ref):
        up = np.flatnonzero(r["up"][row[t]])
        dn = x["N"][up] - d["tie_N"][t, up]
        assert len(set(dn.tolist())) == 1 and x["status"] == FIX_OK, (t, dn)
        if d["tie_side"][t]:
            assert x["flags"] == 0 and np.abs(x["xyz"] - r["site"][row[t]]).max() <= POS_TOL / 4
        else:
            assert x["flags"] == INCONSISTENT and x["rms"] > 5e3, (t, x["rms"])
    print("    coarse_ref on them: rms on the wrong side %.3g .. %.3g m" % (min(x["rms"] for x in ref if x["flags"]), max(x["rms"] for x in ref)))


def test_prediction_ties_and_flags():
    d = load()
    code, dop = sod.pred_integer_cases()
    n = code.size
    print("prediction cases within 1e-6 of a rounding tie: code %d, Doppler %d of %d" % ((~code).sum(), (~dop).sum(), n))
    assert (~code).sum() <= TIE_CAP * n and (~dop).sum() <= TIE_CAP * n
    lo = np.rint(d["pred_lo_pos"])
    off = np.abs(lo) > GEN_KMAX
    print("predictions off the Doppler grid: %d in the A rows, %d in the B rows, %d of 12 in the last row" % (off[0:-1:2].sum(), off[1:-1:2].sum(), off[-1].sum()))
    assert off[-1].all() and not off[0:-1:2].any() and (np.abs(np.abs(d["pred_lo_pos"]) - (GEN_KMAX + 0.5)) >= 1e-6).all()
    low = d["pred_elev_deg"] < 5.0
    print("predictions below 5 degrees: %d of %d; closest elevation to the mask %.3g degrees" % (low.sum(), n, np.abs(d["pred_elev_deg"] - 5.0).min()))
    assert low.sum() >= 100 and np.abs(d["pred_elev_deg"] - 5.0).min() > 1e3 * AID_ELEV_TOL
    r = rows()
    assert (low[0:-1:2] == ~r["up"]).all()   # the A rows: the oracle's two elevations agree about the mask


# ---- 4. the references against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False])
def test_coarse_ref_against_the_oracle(coarse, masked):
    r = rows()
    ref = coarse[masked]
    assert all(x["status"] == FIX_OK and x["flags"] == 0 for x in ref)
    err = coarse_errors(ref, masked).max(axis=0)
    its = [x["iterations"] for x in ref]
    frac = 0.0
    for i, x in enumerate(ref):
        s_true = (int(sod.fold_ms(r["vac_ms"][i, x["ref"]] - sod.priors(1)["rx_ms"][i])) - int(x["N"][x["ref"]])) * 1e-3
        for k, (ms, fr) in x["obs_out"].items():
            if EDGE <= r["vac_frac"][i, k] <= 1e-3 - EDGE:
                assert ms == r["vac_ms"][i, k], (i, k)
            dfrac = float(sod.fold_ms(ms - r["vac_ms"][i, k])) * 1e-3 + (fr - r["vac_frac"][i, k]) - (x["coarse_s"] - s_true)
            frac = max(frac, abs(dfrac))
    print("coarse_ref, %s, 88 rows: place %.3g m, receive time %.3g of its tolerance, coarse_s %.3g of its, pdop / cdop %.3g relative, lat %.3g rad, "
          "lon %.3g rad, alt %.3g m, obs_out frac %.3g s, passes %d..%d" % (("masked" if masked else "all twelve",) + tuple(err) + (frac, min(its), max(its))))
    assert err[0] <= POS_TOL / 4 and err[1] <= 0.25 and err[2] <= 0.25 and err[3] <= DOP_REL_TOL / 4
    assert err[4] <= LATLON_TOL / 4 and err[5] <= LATLON_TOL / 4 and err[6] <= ALT_TOL / 4 and frac <= FRAC_TOL / 4


def test_coarse_raim_ref_against_the_oracle(coarse):
    r = rows()
    ephs, prior, rp = sod.all_ephs(), sod.priors(1), raim_ref.params(sod.SIGMA_EXACT)
    clean = coarse_raim_ref.coarse_fix_raim(ephs, sod.phase_obs(True), prior, rp)
    assert all(x["raim"]["status"] in (sod.RAIM_PASS, sod.RAIM_UNCHECKED) for x in clean)
    assert all(np.array_equal(x["out"]["xyz"], c["xyz"]) for x, c in zip(clean, coarse[True]))
    obs, col = sod.raim_case()
    got = coarse_raim_ref.coarse_fix_raim(ephs, obs, prior, rp)
    assert [x["raim"]["status"] for x in got] == [sod.RAIM_EXCLUDED] * 88 and [x["raim"]["excluded"] for x in got] == col.tolist()
    pos = max(np.abs(x["out"]["xyz"] - r["site"][i]).max() for i, x in enumerate(got))
    for i, x in enumerate(got):
        assert set(x["out"]["obs_out"]) == set(np.flatnonzero(r["up"][i])) - {int(col[i])}
        assert all(ms == r["vac_ms"][i, k] for k, (ms, fr) in x["out"]["obs_out"].items() if EDGE <= r["vac_frac"][i, k] <= 1e-3 - EDGE)
    print("coarse_raim_ref, one code phase 0.3 ms off per row: 88 EXCLUDED with that column, place %.3g m; largest statistic of the clean rows %.3g" %
          (pos, max(x["raim"]["stat"] for x in clean)))
    assert pos <= POS_TOL / 4


def test_dop_ref_against_the_oracle(doppler):
    d, r = load(), rows()
    assert all(x["status"] == FIX_OK and x["flags"] == 0 for x in doppler)
    err = doppler_errors(doppler).max(axis=0)
    lla = np.array([[abs(x["lat"] - r["lla"][i, 0]), float(angle_diff(x["lon"], r["lla"][i, 1])), abs(x["alt"] - r["lla"][i, 2])] for i, x in enumerate(doppler)]).max(axis=0)
    its = [x["iterations"] for x in doppler]
    pd = d["dop_pdop"][..., 0]
    print("dop_ref on the model Dopplers, 88 rows: place %.3g m, drift %.3g, pdop %.3g relative (%.3g .. %.3g m per m/s), rms %.3g m/s, lat %.3g rad, "
          "lon %.3g rad, alt %.3g m, %d..%d steps" % (tuple(err[:3]) + (pd.min(), pd.max(), err[3]) + tuple(lla) + (min(its), max(its))))
    assert err[0] <= PLACE_TOL / 4 and err[1] <= DRIFT_TOL / 4 and err[2] <= DOP_PDOP_REL / 4 and err[3] <= DOP_RMS_TOL / 4
    assert lla[0] <= LATLON_TOL / 4 and lla[1] <= LATLON_TOL / 4 and lla[2] <= DOP_ALT_TOL / 4


def test_physical_dopplers_against_the_model():
    """test 5's bound on the CPU: dop_ref on the physical Dopplers lands within sum_k |G[:3, k]|_inf |diff_k| + 1e-3 m of the site"""
    d, r = load(), rows()
    ephs, obs = sod.all_ephs(), sod.phase_obs(True)
    got = dop_ref.doppler_fix(ephs, obs, sod.rate_obs("phys"), r["ref_ms"])
    dist, bound = physical_bound(ephs, obs, np.array([x["xyz"] for x in got]))
    diff = np.abs(d["dop_diff"].reshape(88, 12)[r["up"]])
    print("model minus physical Doppler: at most %.3g m/s; dop_ref on the physical ones: %.3g .. %.3g m from the site, at most %.3g of the bound" %
          (diff.max(), dist.min(), dist.max(), (dist / bound).max()))
    assert all(x["status"] == FIX_OK and x["flags"] == 0 for x in got) and (dist <= bound).all()


def physical_bound(ephs, obs, place):
    """(distance of place [88][3] to the site, the bound sum_k |G[:3, k]|_inf |diff_k| + 1e-3), G = (H^T H)^-1 H^T of dop_ref.rows at the
    site"""
    d, r = load(), rows()
    use = obs["valid"] != 0
    tau = np.full(use.shape, 75e-3)
    pos, g = r["site"].copy(), sod.C * sod.drifts()
    for _ in range(3):
        rr, vi, dd = dop_ref.satellites(ephs, obs["eph"].astype(np.int64), use, r["ref_ms"], tau)
        H, _, _, rng = dop_ref.rows(rr, vi, dd, np.zeros(use.shape), pos, g)
        tau = np.where(use, rng / sod.C, tau)
    bound = np.zeros(88)
    for i in range(88):
        h = H[i, use[i]]
        G = np.linalg.solve(h.T @ h, h.T)
        bound[i] = (np.abs(G[:3]).max(axis=0) * np.abs(d["dop_diff"].reshape(88, 12)[i, use[i]])).sum() + 1e-3
    return np.linalg.norm(place - r["site"], axis=1), bound


def circ_ms(a_ms, a_frac, b_ms, b_frac):
    """(a - b) in seconds across the millisecond's edge"""
    return sod.fold_ms(np.asarray(a_ms, np.int64) - b_ms) * 1e-3 + (np.asarray(a_frac) - b_frac)


def test_aided_ref_against_the_oracle():
    d = load()
    fx, vel = sod.pred_fix(), sod.pred_vel()
    R = len(fx)
    worst, ints = np.zeros(3), [0, 0]
    code, dop = sod.pred_integer_cases()
    for f in range(N_SITES):
        sel = np.flatnonzero(d["pred_site"] == f)
        got = aided_ref.predict(sod.constellation(f), fx[sel], vel[sel], 12, GEN_FS, GEN_SPM, GEN_STEP_HZ, GEN_KMAX)
        for a, rw in zip(sel, got):
            for s, p in enumerate(rw):
                want = (sod.AID_LOW if d["pred_elev_deg"][a, s] < 5.0 else 0) | (sod.AID_OFF_GRID if abs(np.rint(d["pred_lo_pos"][a, s])) > GEN_KMAX else 0)
                assert p["flags"] == want, (a, s, p["flags"], want)
                dfrac = abs(((p["tx_frac"] - d["pred_tx_frac"][a, s] + 0.5e-3) % 1e-3) - 0.5e-3)
                worst = np.maximum(worst, [dfrac, abs(p["doppler_hz"] - d["pred_doppler_hz"][a, s]), abs(p["elev_deg"] - d["pred_elev_deg"][a, s])])
                if code[a, s]:
                    assert p["ca_center"] == int(np.rint(d["pred_ca_pos"][a, s])) % GEN_SPM, (a, s)
                    ints[0] += 1
                if dop[a, s]:
                    assert p["lo_center"] == int(np.rint(d["pred_lo_pos"][a, s])), (a, s)
                    ints[1] += 1
    print("aided_ref.predict, %d fix rows x 12: tx_frac %.3g s, doppler_hz %.3g Hz, elev_deg %.3g degrees; %d ca_center and %d lo_center equal" %
          ((R,) + tuple(worst) + tuple(ints)))
    assert worst[0] <= AID_FRAC_TOL / 10 and worst[1] <= AID_DOPPLER_TOL / 10 and worst[2] <= AID_ELEV_TOL / 10
    # the physical halves of the A rows: the code phase IS the truth's, the Doppler of a clock without drift the physical one
    r = rows()
    a_rows = np.arange(0, R - 1, 2)
    dfrac = np.abs(circ_ms(d["pred_tx_ms"][a_rows], d["pred_tx_frac"][a_rows], r["vac_ms"], r["vac_frac"]))
    bound = sod.code_phase_bound()
    still = (r["j"] % 2 == 1)
    ddop = np.abs(d["pred_doppler_hz"][a_rows][still] - d["dop_phys"].reshape(88, 12)[still])
    print("    the oracle's A rows against the truth: code phase %.3g s, at most %.3g of cc (range rate / c + drift) (that bound: up to %.3g s); "
          "Doppler on the drift-0 instants %.3g Hz (bound %.3g)" % (dfrac.max(), (dfrac / (bound + AID_FRAC_TOL / 10)).max(), bound.max(), ddop.max(),
                                                                   sod.L1 / sod.C * sod.PER_SAT))
    assert (dfrac <= bound + AID_FRAC_TOL / 10).all() and ddop.max() <= sod.L1 / sod.C * sod.PER_SAT


# ---- 5. what each case catches -----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def patched(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


def verdict(label, caught, per_site, want):
    """print and assert one slip's count: at least a quarter of the rows, one row of every site, and the count as measured"""
    n = len(caught)
    sites = np.add.reduceat(caught.astype(int), np.arange(0, n, per_site))
    print("%-46s caught in %d of %d rows, per site %s" % (label, caught.sum(), n, sites.tolist()))
    assert caught.sum() >= n / 4 and (sites >= 1).all() and caught.sum() == want, (label, int(caught.sum()))


def _d_from(other):
    """coarse_ref._states with the clock drift taken from the ephemerides `other`"""
    true_states = coarse_ref._states

    def states(ephs, eph_index, use, ms, frac, rates=False):
        out = true_states(ephs, eph_index, use, ms, frac, rates)
        return out[:3] + (true_states(other, eph_index, use, ms, frac, True)[3],) if rates else out
    return states


DOPPLER_SLIPS = ("no c d", "no a_f2", "t_oc as t_oe", "receiver term flipped", "tau held")


@pytest.mark.parametrize("slip,want", zip(DOPPLER_SLIPS, (88, 88, 88, 88, 88)))
def test_doppler_slips(slip, want):
    ephs, r = sod.all_ephs(), rows()
    true_rows, true_sats = dop_ref.rows, dop_ref.satellites
    om = dop_ref.OMEGA_E
    if slip == "no c d":
        ctx = patched(dop_ref, "rows", lambda rr, vi, d, dop, pos, g: true_rows(rr, vi, 0.0 * d, dop, pos, g))
    elif slip == "no a_f2":
        ctx = patched(coarse_ref, "_states", _d_from([dict(e, a_f2=0.0) for e in ephs]))
    elif slip == "t_oc as t_oe":
        ctx = patched(coarse_ref, "_states", _d_from([dict(e, t_oc=e["t_oe"]) for e in ephs]))
    elif slip == "receiver term flipped":
        spin = lambda pos: np.stack([-om * pos[:, 1], om * pos[:, 0], np.zeros(len(pos))], -1)[:, None, :]
        ctx = patched(dop_ref, "rows", lambda rr, vi, d, dop, pos, g: true_rows(rr, vi + 2.0 * spin(pos), d, dop, pos, g))
    else:
        ctx = patched(dop_ref, "satellites", lambda e, idx, use, rx_ms, tau: true_sats(e, idx, use, rx_ms, np.full(tau.shape, 75e-3)))
    with ctx:
        got = dop_ref.doppler_fix(ephs, sod.phase_obs(True), sod.rate_obs("model"), r["ref_ms"])
    err = doppler_errors(got)
    fin = np.isfinite(err[:, 0])
    print("    %s: place %.3g .. %.3g m off, drift up to %.3g" % (slip, err[fin, 0].min() if fin.any() else np.nan, err[fin, 0].max() if fin.any() else np.nan,
                                                               err[fin, 1].max() if fin.any() else np.nan))
    verdict("Doppler fix, " + slip, doppler_caught(err), 8, want)


def slipped_rows(theta_sign, with_cd):
    """a copy of coarse_ref._rows with theta's sign and the c d of h[4] to choose"""
    def _rows(ephs, eph_index, use, tx_frac, N, rx_ms, pos, b, s):
        k, frac = coarse_ref.split(tx_frac + s[:, None])
        ms = (rx_ms[:, None] + N + k) % coarse_ref.WEEK_MS
        p, cc, v, d = coarse_ref._states(ephs, eph_index, use, ms, frac, rates=True)
        rho = coarse_ref.C * (cc - (N * 1e-3 + tx_frac)) - b[:, None]
        th = theta_sign * coarse_ref.OMEGA_E * rho / coarse_ref.C
        los = pos[:, None, :] - coarse_ref.turn(p, th)
        rng = np.sqrt((los * los).sum(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            u = los / rng[..., None]
        hs = -((coarse_ref.C * d if with_cd else 0.0) + (u * coarse_ref.turn(v, th)).sum(-1))
        H = np.concatenate([u, np.ones(use.shape + (1,)), hs[..., None]], axis=-1)
        return H, rho - rng, ms, frac
    return _rows


def test_the_copy_of_the_rows_is_the_reference(coarse):
    with patched(coarse_ref, "_rows", slipped_rows(-1.0, True)):
        got = coarse_ref.coarse_fix(sod.all_ephs(), sod.phase_obs(True), sod.priors(1))
    assert all(np.array_equal(a["xyz"], b["xyz"]) and a["cdop"] == b["cdop"] for a, b in zip(got, coarse[True]))


@pytest.mark.parametrize("slip,sign,with_cd,want", [("theta with the wrong sign", 1.0, True, 88), ("h[4] without c d", -1.0, False, 88)])
def test_coarse_slips(slip, sign, with_cd, want):
    with patched(coarse_ref, "_rows", slipped_rows(sign, with_cd)):
        got = coarse_ref.coarse_fix(sod.all_ephs(), sod.phase_obs(True), sod.priors(1))
    err = coarse_errors(got, True)
    fin = np.isfinite(err[:, 0])
    print("    %s: place %.3g .. %.3g m off, pdop / cdop %.3g .. %.3g relative; the place alone leaves its tolerance in %d rows" %
          (slip, err[fin, 0].min(), err[fin, 0].max(), err[fin, 3].min(), err[fin, 3].max(), (err[:, 0] > POS_TOL).sum()))
    if not with_cd:
        assert (err[:, 3] > DOP_REL_TOL).sum() == want   # cdop alone shows it
    verdict("coarse fix, " + slip, coarse_caught(err), 8, want)


def predicted_code(eph, fix, passes, with_cc):
    """a copy of aided_ref.predict_one's LIGHT TIME and CODE with the number of passes and the cc of T to choose: (tx_ms, tx_frac)"""
    rr = np.array([float(fix["x"]), float(fix["y"]), float(fix["z"])])
    rx_ms, rx_frac = int(fix["rx_ms"]), float(fix["rx_frac"])
    tau, cc = 75e-3, 0.0
    for _ in range(passes):
        ms, frac = nav_ref.split_time(rx_ms, rx_frac + -tau)
        p, dt = nav_ref.sat_state(eph, int(ms), float(frac))
        tau = float(np.linalg.norm(rr - aided_ref._turn(p[0], -nav_ref.OMEGA_E * tau))) / nav_ref.C
        cc = float(dt[0])
    ms, tx_frac = nav_ref.split_time(rx_ms, rx_frac + ((cc if with_cc else 0.0) - tau))
    return int(ms), float(tx_frac)


@pytest.mark.parametrize("slip,passes,with_cc,want", [("as written", 2, True, 0), ("one light-time pass", 1, True, 176), ("cc left out of T", 2, False, 176)])
def test_prediction_slips(slip, passes, with_cc, want):
    d = load()
    fx = sod.pred_fix()[:-1]
    worst = np.zeros(len(fx))
    for a in range(len(fx)):
        ephs = sod.constellation(int(d["pred_site"][a]))
        got = [predicted_code(e, fx[a], passes, with_cc) for e in ephs]
        worst[a] = np.abs(circ_ms([g[0] for g in got], [g[1] for g in got], d["pred_tx_ms"][a], d["pred_tx_frac"][a])).max()
    print("    %s: tx_frac %.3g .. %.3g s off" % (slip, worst.min(), worst.max()))
    caught = worst > AID_FRAC_TOL
    if want == 0:
        assert not caught.any()
    else:
        verdict("prediction, " + slip, caught, 16, want)
