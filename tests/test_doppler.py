"""tests/dop_ref.py, the reference of "Cold snapshot fixes: fine Doppler and a Doppler-only position solver" of include/gpsacq.h,
checked on the CPU before the kernels are held against it (tests/test_gpu_doppler.py): the estimator on hand-made (I, Q)
sequences and on a noise-free capture whose Doppler is known, the solver on exact Dopplers of the three geometries, its rows
against central differences, its failure modes; and the structs, exports and defaults of the library through ctypes."""
import ctypes
import math

import numpy as np
import pytest

import dop_ref
import nav_ref
import refine_ref
import track_ref
from nav_helpers import geometry

FS, FC, SPM = 5.456e6, 4.092e6, 5456
T = SPM / FS
DRIFT = 2e-6


# ---- the library's side, without a GPU -------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("hip_artifacts")
def test_structs_exports_defaults():
    import gpsacq
    lib = gpsacq.load_library()
    assert (gpsacq.DOPFINE_PARAMS_DTYPE.itemsize, gpsacq.DOPFINE_DTYPE.itemsize, gpsacq.DOPPLER_FIX_PARAMS_DTYPE.itemsize,
            gpsacq.DOPPLER_FIX_DTYPE.itemsize) == (24, 72, 16, 88)
    for name in ("gpsacq_dopfine_default_params", "gpsacq_doppler_fix_default_params", "gpsacq_fine_doppler", "gpsacq_fine_doppler_device",
                 "gpsacq_rate_obs_fine", "gpsacq_rate_obs_fine_device", "gpsacq_doppler_fix_batch", "gpsacq_doppler_fix_batch_device",
                 "gpsacq_cold_fix_device", "gpsacq_doppler_last_ms"):
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    p = np.full(1, 0xA5, np.uint8).repeat(24).view(gpsacq.DOPFINE_PARAMS_DTYPE)
    assert lib.gpsacq_dopfine_default_params(p.ctypes.data_as(ctypes.c_void_p)) == 0
    assert (int(p["blocks"][0]), int(p["min_segments"][0]), float(p["snr_min"][0]), float(p["coherence_min"][0])) == (16, 2, 25.0, 0.0)
    q = np.full(1, 0xA5, np.uint8).repeat(16).view(gpsacq.DOPPLER_FIX_PARAMS_DTYPE)
    assert lib.gpsacq_doppler_fix_default_params(q.ctypes.data_as(ctypes.c_void_p)) == 0
    assert (float(q["rms_max_mps"][0]), float(q["reserved"][0])) == (dop_ref.RMS_MAX_MPS, 0.0)
    assert lib.gpsacq_dopfine_default_params(None) == 1 and lib.gpsacq_doppler_fix_default_params(None) == 1
    # the Python helpers and their checks
    d = gpsacq.dopfine_params(blocks=3, min_segments=5, snr_min=-1.0, coherence_min=0.25)
    assert (int(d["blocks"][0]), int(d["min_segments"][0]), float(d["snr_min"][0]), float(d["coherence_min"][0])) == (3, 5, -1.0, 0.25)
    for bad in (dict(blocks=0), dict(blocks=65), dict(blocks=2.5), dict(min_segments=1), dict(snr_min=float("nan")), dict(snr_min=float("inf")),
                dict(coherence_min=-0.1), dict(coherence_min=float("nan"))):
        with pytest.raises(ValueError):
            gpsacq.dopfine_params(**bad)
    with pytest.raises(TypeError):
        gpsacq.dopfine_params(spacing=1)
    assert float(gpsacq.doppler_fix_params(5.0)["rms_max_mps"][0]) == 5.0
    assert (gpsacq.DOPFINE_NO_HIT, gpsacq.DOPFINE_SHORT, gpsacq.DOPFINE_NO_POWER, gpsacq.DOPFINE_FEW, gpsacq.DOPFINE_WEAK) == (
        dop_ref.NO_HIT, dop_ref.SHORT, dop_ref.NO_POWER, dop_ref.FEW, dop_ref.WEAK)
    assert gpsacq.DOPPLER_INCONSISTENT == dop_ref.INCONSISTENT


# ---- the estimator on hand-made (I, Q) -------------------------------------------------------------------------------------------
def turning(n, cycles_per_segment, radius=4000, phase0=0.3):
    a = 2 * math.pi * (phase0 + cycles_per_segment * np.arange(n))
    return [(int(round(radius * math.cos(x))), int(round(radius * math.sin(x)))) for x in a]


def test_a_constant_turn_and_data_bits():
    """z^2 turning by an eighth of a cycle per segment (z itself by a sixteenth) is df = 1 / (16 T), and z turning by an eighth is
    1 / (8 T): the angle of the lag product is 4 pi df T.  I and Q are rounded to integers, each off by at most 0.5: the angle of z
    by at most 0.5 sqrt(2) / radius, that of z^2 by twice and that of a lag product by four times that"""
    n, radius = 117, 4000
    bound = 4 * (0.5 * math.sqrt(2) / radius) / (4 * math.pi * T)
    iq = turning(n, 1.0 / 16, radius)
    rec = dop_ref.record(iq, n, SPM, FS, FC, lo_rate=3221225472, ca_rate=805306368)
    print("df %.6f Hz, wanted %.6f, bound of the rounding %.4f; coherence %.9f" % (rec["df_hz"], 1 / (16 * T), bound, rec["coherence"]))
    assert rec["flags"] == 0 and abs(rec["df_hz"] - 1 / (16 * T)) <= bound and rec["coherence"] > 0.999999
    assert rec["doppler_hz"] == ((3221225472.0 * FS) / 4294967296.0 - FC) + rec["df_hz"] and abs(rec["doppler_hz"] - rec["df_hz"]) < 1e-6
    assert abs(dop_ref.record(turning(n, 1.0 / 8, radius), n, SPM, FS, FC, 1, 2)["df_hz"] - 1 / (8 * T)) <= bound
    # the other way round, and the record of the same turn under data bits: every second run of 20 segments negated
    neg = dop_ref.record(turning(n, -1.0 / 16, radius), n, SPM, FS, FC, 3221225472, 805306368)
    assert abs(neg["df_hz"] + 1 / (16 * T)) <= bound
    flipped = [(-i, -q) if (s // 20) % 2 else (i, q) for s, (i, q) in enumerate(iq)]
    assert flipped != iq and dop_ref.record(flipped, n, SPM, FS, FC, 3221225472, 805306368) == rec


def test_no_power_few_and_weak():
    z = dop_ref.record([(0, 0)] * 21, 21, SPM, FS, FC, 1, 2)
    assert z["flags"] == dop_ref.NO_POWER and (z["coherence"], z["df_hz"], z["doppler_hz"]) == (0.0, 0.0, 0.0) and z["power"] == 0
    # re == 0 and im == 0 with mag > 0: a quarter turn of z^2 forth and back
    q = dop_ref.record([(100, 0), (71, 71), (100, 0)], 3, SPM, FS, FC, 1, 2)
    assert q["mag"] > 0 and (q["re"], q["im"]) == (0, 0) and q["flags"] == dop_ref.NO_POWER
    one = dop_ref.record([(300, -400)], 21, SPM, FS, FC, 1, 2)
    assert one["flags"] == dop_ref.SHORT | dop_ref.FEW | dop_ref.NO_POWER and (one["re"], one["im"], one["mag"], one["power"]) == (0, 0, 0, 250000)
    assert not dop_ref.usable(one) and not dop_ref.usable(z)
    none = dop_ref.record([], 21, SPM, FS, FC, 1, 2)
    assert none["flags"] == dop_ref.SHORT | dop_ref.FEW | dop_ref.NO_POWER and none["power"] == 0
    # the gate just below and just above a record's own coherence
    iq = turning(21, 0.01, 500) + [(0, 0), (350, 10)]
    r = dop_ref.record(iq, 23, SPM, FS, FC, 1, 2)
    assert 0 < r["coherence"] < 1
    assert dop_ref.record(iq, 23, SPM, FS, FC, 1, 2, coherence_min=r["coherence"])["flags"] == 0
    assert dop_ref.record(iq, 23, SPM, FS, FC, 1, 2, coherence_min=np.nextafter(r["coherence"], 1.0))["flags"] == dop_ref.WEAK


def test_lag_sums_at_the_overflow_bound():
    """spm = 8184 with 64 blocks is the largest of the usual rates the text admits; with |I| = |Q| = spm in every segment each of
    the 311 lag terms of re (or im) and mag is 4 spm^4, the most it can be"""
    spm, blocks = 8184, 64
    assert blocks * 160000 * spm ** 3 < 2 ** 63 <= blocks * 160000 * 9700 ** 3
    n = blocks * 40000 // spm
    same_sign = dop_ref.record([(spm, spm)] * n, n, spm, 8.184e6, 2e6, 1, 2)
    assert same_sign["re"] == same_sign["mag"] == (n - 1) * 4 * spm ** 4 < 2 ** 63 and same_sign["im"] == 0 and same_sign["coherence"] == 1.0
    assert same_sign["power"] == n * 2 * spm ** 2 and same_sign["df_hz"] == 0.0
    # a quarter turn of z per segment: z^2 turns by a half, re is as negative as it can be
    quarter = dop_ref.record([((spm, spm), (-spm, spm), (-spm, -spm), (spm, -spm))[s % 4] for s in range(n)], n, spm, 8.184e6, 2e6, 1, 2)
    assert quarter["re"] == -(n - 1) * 4 * spm ** 4 >= -2 ** 63 and quarter["im"] == 0 and abs(abs(quarter["df_hz"]) - 250.0) < 1e-9


# ---- the estimator on a noise-free capture ---------------------------------------------------------------------------------------
def clean_capture(n_samples, prn, doppler_hz, code_phase_samples, carrier_phase):
    """sign(cos(2 pi (fc + D) n / fs + phi) * chip), one satellite, no noise, in float64; the code runs at 1.023e6 (1 + D / L1)"""
    m = np.arange(n_samples, dtype=np.float64)
    idx = np.floor((m + code_phase_samples) * (refine_ref.CPS * (1.0 + doppler_hz / refine_ref.L1) / FS)).astype(np.int64) % 1023
    chip = 1.0 - 2.0 * track_ref.chips(prn)[idx]
    y = chip * np.cos(2.0 * np.pi * (((FC + doppler_hz) / FS * m + carrier_phase) % 1.0))
    return np.packbits((y < 0.0).astype(np.uint8), bitorder="little")


# The worst error of doppler_hz test_known_dopplers measured over its five offsets (three blocks, 20 lag products, no noise):
# +4.05, +2.54, +0.29, -2.37 and -3.51 Hz at -60, -40, 0, +40 and +60 Hz.  It grows with the offset, some 7 % of it: without noise
# the hard-limited signal keeps its third harmonic, which meets the third harmonic of the two-bit replica in a term that turns the
# other way, -3 df at a ninth of the amplitude, and pulls the angle of the squares back.  Noise at the usual level (sigma 1 against
# an amplitude of 0.2) linearises the limiter and takes that term away: tests/test_gpu_doppler.py measures the noisy case.  The
# test asserts three times this figure.
KNOWN_DOPPLER_WORST_HZ = 4.054


def test_known_dopplers():
    """A satellite 40 Hz above a bin centre reads df_hz = +37.6, one 40 Hz below -37.5: the sign of the text, and its size up to what
    a noise-free 1-bit capture costs.  Measured: worst 4.054 Hz at -60 Hz (see KNOWN_DOPPLER_WORST_HZ above)."""
    lo_shift, prn, ca_shift = 9, 21, 1500
    centre = lo_shift * FS / 40000
    ok, lo_rate, _ = refine_ref.nco_words(lo_shift, FC, FS)
    replica = lo_rate * FS / 4294967296.0 - FC  # what the truncated NCO word really runs at
    worst = 0.0
    for off in (-60.0, -40.0, 0.0, 40.0, 60.0):
        bits = clean_capture(3 * 40000 + 64, prn, centre + off, ca_shift + 0.2, 0.377)
        rec = dop_ref.fine_doppler(bits, 5120, [(0, prn - 1)], [(100.0, lo_shift, ca_shift, 0.0)], SPM, FC, FS, blocks=3)[0]
        assert rec["flags"] == 0 and rec["segments"] == 3 * 40000 // SPM and rec["coherence"] > 0.9
        err = rec["doppler_hz"] - (centre + off)
        print("offset %+5.1f Hz: df_hz %+9.4f, doppler_hz off by %+.4f Hz, coherence %.6f" % (off, rec["df_hz"], err, rec["coherence"]))
        assert abs(rec["df_hz"] - (centre + off - replica)) == pytest.approx(abs(err), abs=1e-9)
        if off:
            assert rec["df_hz"] * off > 0
        worst = max(worst, abs(err))
    print("worst %.4f Hz; KNOWN_DOPPLER_WORST_HZ %.4f" % (worst, KNOWN_DOPPLER_WORST_HZ))
    assert worst <= 3 * KNOWN_DOPPLER_WORST_HZ


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def exact_case(which, k, drift=DRIFT, t_rx=0.25):
    """geo's k best satellites seen at ref_ms + t_rx: OBS_DTYPE / RATE_OBS_DTYPE rows [1][k] with the exact Dopplers (the central
    difference of the truth's transmit times over a second, as coarse_helpers.synth_sats forms them) of a receiver at rest
    whose clock runs fast by `drift`"""
    import gpsacq
    geo = geometry(which)
    sel = geo["subsets"][k]
    obs = np.zeros((1, k), gpsacq.OBS_DTYPE)
    ro = np.zeros((1, k), gpsacq.RATE_OBS_DTYPE)
    for j, s in enumerate(sel):
        t = nav_ref.truth_tx(geo["ephs"][s], geo["rx"], geo["ref_ms"], np.array([t_rx - 0.5, t_rx + 0.5]))
        obs[0, j] = (s, 1, 0, 0, 0.0, 1.0)
        ro[0, j] = (1, 0, 0, dop_ref.L1 * ((t[1] - t[0]) - 1.0) - dop_ref.L1 * drift, 1.0)
    rx_ms = np.array([(geo["ref_ms"] + int(t_rx * 1000)) % nav_ref.WEEK_MS])
    return geo, obs, ro, rx_ms


@pytest.mark.usefixtures("hip_artifacts")
@pytest.mark.parametrize("which", ["north", "south", "rollover"])
@pytest.mark.parametrize("k", [8, 5])
def test_exact_dopplers_recover_the_place(which, k):
    """no prior of place at all; the prototype's worst was 35 m"""
    geo, obs, ro, rx_ms = exact_case(which, k)
    r = dop_ref.doppler_fix(geo["ephs"], obs, ro, rx_ms)[0]
    assert r["status"] == dop_ref.FIX_OK and r["n_used"] == k and r["flags"] == 0
    err = float(np.linalg.norm(r["xyz"] - geo["rx"]))
    print("%s, %d satellites: %d steps, %.1f m from the truth, drift off by %.2e, rms %.2e m/s, pdop %.0f m per m/s" %
          (which, k, r["iterations"], err, r["drift"] - DRIFT, r["rms"], r["pdop"]))
    assert err <= 100.0 and abs(r["drift"] - DRIFT) <= 1e-9 and 4 <= r["iterations"] <= 8
    assert r["prior"] == tuple(r["xyz"]) and r["pdop"] > 0
    assert abs(np.linalg.norm(nav_ref.ecef_of(r["lat"], r["lon"], r["alt"]) - r["xyz"])) < 1e-3


@pytest.mark.usefixtures("hip_artifacts")
def test_rows_against_central_differences():
    geo, obs, ro, rx_ms = exact_case("north", 8)
    use = np.ones(obs.shape, bool)
    tau = np.full(obs.shape, 70e-3)
    r, vi, d = dop_ref.satellites(geo["ephs"], obs["eph"].astype(np.int64), use, rx_ms, tau)
    pos = (geo["rx"] + np.array([30e3, -20e3, 10e3]))[None, :]
    g = np.array([123.0])
    H, _, pred0, _ = dop_ref.rows(r, vi, d, ro["doppler_hz"], pos, g)
    step = 10.0  # metres: pred is smooth over kilometres, and 10 m keeps the rounding of a 1e3 m/s prediction at 1e-12 / 20
    worst = 0.0
    for a in range(3):
        e = np.zeros((1, 3))
        e[0, a] = step
        hi, lo = dop_ref.rows(r, vi, d, ro["doppler_hz"], pos + e, g)[2], dop_ref.rows(r, vi, d, ro["doppler_hz"], pos - e, g)[2]
        num = (hi - lo) / (2 * step)
        worst = max(worst, float(np.abs(num - H[..., a]).max() / np.abs(H[..., a]).max()))
    num_g = (dop_ref.rows(r, vi, d, ro["doppler_hz"], pos, g + 1.0)[2] - dop_ref.rows(r, vi, d, ro["doppler_hz"], pos, g - 1.0)[2]) / 2.0
    print("analytic rows against central differences: worst %.2e of the largest entry" % worst)
    assert worst < 1e-6 and np.abs(num_g - 1.0).max() < 1e-9 and (H[..., 3] == 1.0).all()


@pytest.mark.usefixtures("hip_artifacts")
def test_too_few_failed_rows_and_inconsistent():
    geo, obs, ro, rx_ms = exact_case("north", 8)
    ephs = geo["ephs"]
    three = dop_ref.doppler_fix(ephs, obs[:, :3], ro[:, :3], rx_ms)[0]
    assert three["status"] == dop_ref.FIX_TOO_FEW and three["n_used"] == 3 and three["iterations"] == 0 and all(math.isnan(v) for v in three["prior"])
    # every way a column drops out, one at a time from eight: seven are left; all at once: TOO_FEW
    cut = [("valid", obs, 0), ("valid", ro, 0), ("eph", obs, 12), ("eph", obs, -1), ("doppler_hz", ro, float("nan")), ("weight", ro, float("inf")),
           ("weight", ro, -1.0)]
    for f, which, v in cut:
        o2, r2 = obs.copy(), ro.copy()
        (o2 if which is obs else r2)[f][0, 2] = v
        got = dop_ref.doppler_fix(ephs, o2, r2, rx_ms)[0]
        assert got["status"] == dop_ref.FIX_OK and got["n_used"] == 7, (f, v)
    assert dop_ref.doppler_fix(ephs, obs, ro, rx_ms, eph_valid=[k != obs["eph"][0, 0] for k in range(12)])[0]["n_used"] == 7
    for bad_ms in (-1, nav_ref.WEEK_MS):
        got = dop_ref.doppler_fix(ephs, obs, ro, np.array([bad_ms]))[0]
        assert got["status"] == dop_ref.FIX_TOO_FEW and got["n_used"] == 0 and all(math.isnan(v) for v in got["prior"])
    # all weights zero: nothing to solve
    r0 = ro.copy()
    r0["weight"] = 0.0
    got = dop_ref.doppler_fix(ephs, obs, r0, rx_ms)[0]
    assert got["status"] == dop_ref.FIX_NO_CONVERGE and got["n_used"] == 8 and all(math.isnan(v) for v in got["prior"])
    # one Doppler pulled by 200 Hz among eight: a fix, flagged, and no prior; among four there is nothing to judge it by
    r2 = ro.copy()
    r2["doppler_hz"][0, 5] += 200.0
    got = dop_ref.doppler_fix(ephs, obs, r2, rx_ms)[0]
    print("200 Hz on one of eight: rms %.2f m/s, %.0f km from the truth" % (got["rms"], np.linalg.norm(got["xyz"] - geo["rx"]) / 1e3))
    assert got["status"] == dop_ref.FIX_OK and got["flags"] == dop_ref.INCONSISTENT and got["rms"] > dop_ref.RMS_MAX_MPS
    assert all(math.isnan(v) for v in got["prior"])
    four = dop_ref.doppler_fix(ephs, obs[:, [0, 3, 5, 7]], r2[:, [0, 3, 5, 7]], rx_ms)[0]
    assert four["status"] == dop_ref.FIX_OK and four["flags"] == 0 and four["rms"] < 1e-3
