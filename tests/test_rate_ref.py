"""Carrier observables and velocity on the host: the models of include/gpsacq.h ("Carrier observables", "Velocity and clock drift")
as tests/rate_ref.py states them, checked against themselves in independent ways -- the prefix sum against a forward simulation of
the carrier NCO, the kernel's chunk / run / scan indexing lane by lane, the analytic satellite velocity against a central difference
of nav_ref's positions -- plus struct sizes and exports.  Needs the library, no GPU."""
import os
import subprocess

import numpy as np
import pytest

import nav_ref
import obs_ref
import rate_ref
from nav_helpers import geometry

pytestmark = pytest.mark.usefixtures("hip_artifacts")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gpsacq_track_nominal_word_iq8", "gpsacq_rate_observables", "gpsacq_rate_observables_device", "gpsacq_sat_rates",
               "gpsacq_sat_rates_device", "gpsacq_vel_batch", "gpsacq_vel_batch_device", "gpsacq_pvt_track_device", "gpsacq_velocity_last_ms")


def test_struct_sizes_and_exports(tmp_path):
    """no padding anywhere: every size is the sum of its fields.  gpsacq_vel's fields -- two int32 and EIGHT doubles (ECEF and ENU
    velocity, drift, rms) -- come to 72 bytes, not the 64 first written down for it; all the fields are kept."""
    import gpsacq
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_rate_obs) == 32 && sizeof(gpsacq_sat_rate) == 32 && sizeof(gpsacq_vel) == 72, "sizes");\n'
                   '_Static_assert(offsetof(gpsacq_rate_obs, adr) == 8 && offsetof(gpsacq_rate_obs, doppler_hz) == 16 && offsetof(gpsacq_rate_obs, weight) == 24, "no padding");\n'
                   '_Static_assert(offsetof(gpsacq_vel, vx) == 8 && offsetof(gpsacq_vel, ve) == 32 && offsetof(gpsacq_vel, drift) == 56 && offsetof(gpsacq_vel, rms) == 64, "no padding");\n'
                   '_Static_assert(sizeof(gpsacq_obs) == 32 && sizeof(gpsacq_sat_state) == 32 && sizeof(gpsacq_fix) == 80 && sizeof(gpsacq_track_record) == 40, "the old structs keep their size");\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert (gpsacq.RATE_OBS_DTYPE.itemsize, gpsacq.SAT_RATE_DTYPE.itemsize, gpsacq.VEL_DTYPE.itemsize) == (32, 32, 72)
    for dt in (gpsacq.RATE_OBS_DTYPE, gpsacq.SAT_RATE_DTYPE, gpsacq.VEL_DTYPE):  # packed: every field follows the one before
        assert sum(dt[n].itemsize for n in dt.names) == dt.itemsize
    assert gpsacq.RATE_OBS_DTYPE.names == ("valid", "reserved", "adr", "doppler_hz", "weight")
    assert gpsacq.VEL_DTYPE.names == ("status", "n_used", "vx", "vy", "vz", "ve", "vn", "vu", "drift", "rms")
    assert (gpsacq.VEL_OK, gpsacq.VEL_TOO_FEW, gpsacq.VEL_NO_FIX, gpsacq.VEL_SINGULAR) == (0, 1, 2, 3)
    lib = gpsacq.load_library()
    for name in NEW_SYMBOLS:
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", gpsacq.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert " T %s\n" % name in out, name
    for name in ("rate_observables", "rate_observables_device", "sat_rates", "velocity", "pvt_track_device", "nominal_word_iq8", "velocity_last_ms"):
        assert callable(getattr(gpsacq.Engine, name))


def _channel(seed, n, spm, nom_word=None, span=40000, sign=0):
    rec, ch, _ = obs_ref.fabricate(seed, n, spm)
    nom = int(4.092e6 / (spm * 1000.0) * 2 ** 32) if nom_word is None else nom_word
    return rate_ref.walk_lo_rate(rec, seed + 1, nom, span, sign), ch, nom


@pytest.mark.parametrize("spm,n", [(2800, 1), (2800, 300), (5456, 1000), (16368, 257)])
def test_prefix_sum_follows_the_nco(spm, n):
    """over ANY run of epochs the low 32 bits of A plus (samples) * nom_word advance as lo_phase does: lo_rate = nom_word + d mod
    2^32, so the identity holds epoch by epoch whatever the rate does; checked from record 0 and between two inner epochs"""
    rec, ch, nom = _channel(7 * spm + n, n, spm)
    nxt = int(ch["next_sample"][0])
    acc = rate_ref.carrier_acc(rec["sample"], rec["lo_rate"], nxt, nom)
    ph = rate_ref.nco_phase_walk(rec["sample"], rec["lo_rate"], nxt, lo_phase0=0x9E3779B9)
    ends = [int(s) for s in rec["sample"]] + [nxt]
    assert len(acc) == n + 1 and acc[0] == 0
    for t in range(n + 1):
        assert (acc[t] + (ends[t] - ends[0]) * nom) & 0xFFFFFFFF == (ph[t] - ph[0]) & 0xFFFFFFFF, t
    a, b = n // 3, n - n // 4
    assert (acc[b] - acc[a] + (ends[b] - ends[a]) * nom) & 0xFFFFFFFF == (ph[b] - ph[a]) & 0xFFFFFFFF
    if n > 2:
        assert len(set(rec["lo_rate"])) > 2  # the rate did move


@pytest.mark.parametrize("case", ["walk", "negative", "wrapped"])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_lane_indexing_equals_the_recursion(n, case):
    """k_carrier_acc's chunk / run / scan / carry indexing, restated lane by lane, against the plain recursion; with every d_t
    negative and with a two's-complement nominal word (a negative carrier) as well"""
    nom = {"walk": None, "negative": None, "wrapped": (-123456789) & 0xFFFFFFFF}[case]
    rec, ch, nom = _channel(31 * n + len(case), n, 2800, nom_word=nom, sign=-1 if case == "negative" else 0)
    nxt = int(ch["next_sample"][0])
    plain = rate_ref.carrier_acc(rec["sample"], rec["lo_rate"], nxt, nom)
    lanes = rate_ref.carrier_acc_lanes(rec["sample"], rec["lo_rate"], nxt, nom)
    assert lanes == plain and None not in lanes
    if case == "negative" and n:
        assert all(plain[t + 1] < plain[t] for t in range(n))
    # a different wave shape gives the same numbers: nothing in the result depends on the chunking
    assert rate_ref.carrier_acc_lanes(rec["sample"], rec["lo_rate"], nxt, nom, lanes=8, run=3) == plain


@pytest.mark.parametrize("W", [1, 2, 1024, 65536])
@pytest.mark.parametrize("spm", [2800, 5456])
def test_constant_rate_doppler_is_exact(spm, W):
    """(lo_rate - nom_word) fs / 2^32 exactly when W is a power of two: D = W d, and W cancels in binary floating point"""
    n, fs = 100, spm * 1000.0
    rec, ch, _ = obs_ref.fabricate(3, n, spm)
    nom = int(4.092e6 / fs * 2 ** 32)
    for d in (12345, -777777, 1):
        rec["lo_rate"] = (nom + d) & 0xFFFFFFFF
        nxt = int(ch["next_sample"][0])
        acc = rate_ref.carrier_acc(rec["sample"], rec["lo_rate"], nxt, nom)
        R = int(rec["sample"][n // 2]) + 17
        adr, dop = rate_ref.rate_observation(rec["sample"], rec["lo_rate"], nxt, acc, nom, R, W, fs)
        assert dop == np.float64(d) * np.float64(fs) / np.float64(2 ** 32)
        assert adr == (R - int(rec["sample"][0])) * d


def test_rate_observation_edges():
    spm, n, W = 2800, 50, 1000
    rec, ch, nom = _channel(11, n, spm)
    s0, nxt = int(rec["sample"][0]), int(ch["next_sample"][0])
    acc = rate_ref.carrier_acc(rec["sample"], rec["lo_rate"], nxt, nom)
    obs = lambda R, w=W: rate_ref.rate_observation(rec["sample"], rec["lo_rate"], nxt, acc, nom, R, w, spm * 1000.0)
    assert obs(s0 + W // 2) is not None and obs(s0 + W // 2 - 1) is None      # R_a at record 0's sample, one before it
    assert obs(nxt - 1 - W + W // 2) is not None and obs(nxt - W + W // 2) is None  # R_b = next_sample - 1, next_sample
    assert obs(nxt - 1, 1) is None and obs(nxt - 2, 1) is not None            # W = 1: R_b = R + 1
    assert obs(3, 1000) is None                                               # R_a negative
    assert rate_ref.rate_observation(rec["sample"][:0], rec["lo_rate"][:0], nxt, [0], nom, s0 + 5, 1, 2.8e6) is None
    # adr at an epoch boundary is the tabulated value
    assert obs(int(rec["sample"][7]))[0] == acc[7]


# ---- analytic satellite velocity ---------------------------------------------------------------------------------------------
def test_analytic_velocity_against_a_central_difference():
    """rounding: one ulp of 2.6e7 m is 3.7e-9 m, a few of them over 0.02 s come to <= 1e-6 m/s; truncation: jerk 9e-5 m/s^3 x
    (0.01 s)^2 / 6 = 1.5e-9 m/s.  Bound 1e-5 m/s: a missing Omega-dot term or harmonic derivative costs metres per second."""
    h, worst = 0.01, 0.0
    tk = np.array([-3000.0, 0.0, 600.0, 1234.5678, 7000.0])
    for eph in geometry("north")["ephs"]:
        num = (nav_ref.position(eph, tk + h) - nav_ref.position(eph, tk - h)) / (2 * h)
        ana = rate_ref.velocity_at(eph, tk)
        worst = max(worst, float(np.abs(num - ana).max()))
        speed = np.linalg.norm(ana, axis=1)
        assert ((speed > 2500) & (speed < 3500)).all()  # ECEF speed of a GPS satellite
    print("analytic velocity against the central difference: worst %.3g m/s" % worst)
    assert worst < 1e-5


def test_clock_drift_against_a_central_difference():
    """the clock correction is ~5e-4 s; its ulp 1e-19 s over 0.02 s is 5e-18 s/s, and the relativistic term's third derivative
    (4.4e-10 * 0.02 * 5153 * (1.46e-4)^3 = 1.4e-19 s/s^3) times h^2 / 6 is nothing.  Bound 1e-15 s/s; the terms themselves are
    a_f1 ~ 1e-11 and the relativistic rate ~ 7e-12."""
    h, worst = 0.01, 0.0
    tk = np.array([-3000.0, 0.0, 600.0, 1234.5678, 7000.0])
    for eph in geometry("north")["ephs"]:
        eph = dict(eph, a_f2=3e-20)  # the constellation's a_f2 is 0: give the term something to do
        num = (nav_ref.clock_correction(eph, tk + h, tk + 5 + h) - nav_ref.clock_correction(eph, tk - h, tk + 5 - h)) / (2 * h)
        ana = rate_ref.clock_drift(eph, tk, tk + 5)
        worst = max(worst, float(np.abs(num - ana).max()))
        assert (np.abs(ana - eph["a_f1"]) > 1e-13).any()  # the relativistic rate is in
    print("clock drift against the central difference: worst %.3g s/s" % worst)
    assert worst < 1e-15


# ---- the velocity model ------------------------------------------------------------------------------------------------------
def test_velocity_model_recovers_a_moving_receiver():
    """the first-order model against nav_ref's truth maker, on the CPU alone: Dopplers L1 (dt_tx / dt_rx - 1) of a receiver
    moving at (250, 100, -50) m/s ENU with a clock drift of 2e-6, the 8-satellite subset.  Neglected terms are of order
    rho'^2 / c <= 900^2 / 3e8 = 2.7 mm/s per satellite, times the subset's gain."""
    geo = geometry("north")
    lat, lon, _ = geo["lla"]
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    venu, drift, h = np.array([250.0, 100.0, -50.0]), 2e-6, 0.05
    E = np.array([[-np.sin(lon), np.cos(lon), 0], [-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)],
                  [np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)]])
    v = E.T @ venu
    t0 = 0.3217e-3
    dop, ms, frac = [], [], []
    for eph in ephs:
        # the receiver clock reads t0 + tau when true time is t0 + tau / (1 + drift); it stands at rx + v * (true time - t0)
        tt = [nav_ref.truth_tx(eph, geo["rx"] + v * (s * h / (1 + drift)), geo["ref_ms"], np.array([t0 + s * h / (1 + drift)]))[0] for s in (-1, 0, 1)]
        dop.append(rate_ref.L1 * ((tt[2] - tt[0]) / (2 * h) - 1.0))
        m, f = nav_ref.split_time(geo["ref_ms"], np.array([tt[1]]))
        ms.append(int(m[0])), frac.append(float(f[0]))
    H, y = rate_ref.vel_rows(ephs, list(range(8)), np.array(ms), np.array(frac), np.array(dop), geo["rx"], geo["ref_ms"], t0)
    x = np.linalg.solve(H.T @ H, H.T @ y)
    g = np.abs(rate_ref.gain(H, np.ones(8))).sum(axis=1).max()
    err = np.abs(x[:3] - v).max()
    print("moving receiver: velocity error %.3g m/s, drift error %.3g, gain %.2f, bound %.3g m/s" % (err, x[3] / nav_ref.C - drift, g, 2.7e-3 * g))
    assert err < 2.7e-3 * g and abs(x[3] / nav_ref.C - drift) < 2.7e-3 * g / nav_ref.C


@pytest.mark.parametrize("drift", [0.0, 2e-6, -2e-6])
@pytest.mark.parametrize("venu", [(0.0, 0.0, 0.0), (30.0, -20.0, 5.0), (250.0, 100.0, -50.0)])
def test_velocity_model_over_the_truth_grid(venu, drift):
    """the grid of tests/test_gpu_velocity.py::test_velocity_recovers_the_truth through rate_ref's own solver: the same receivers,
    the 4, 5, 8 and 12 satellite subsets with the same unequal weights and the same masked satellite, the same bound -- per
    satellite 900^2 / c + c 2e-15 / 0.1 + 1e-6 = 2.71e-3 m/s, times the subset's ||(H^T W H)^-1 H^T W||_inf.  Worst over the
    grid: velocity 3.0e-3 m/s against 8.1e-3 (4 satellites, standing still, drift 2e-6), c * drift 4.1e-3 m/s against 8.1e-3
    (4 satellites, standing still, drift -2e-6)."""
    geo = geometry("north")
    lat, lon, _ = geo["lla"]
    E = np.array([[-np.sin(lon), np.cos(lon), 0], [-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)],
                  [np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)]])
    v = E.T @ np.asarray(venu)
    h, t0 = 0.05, 0.3217e-3
    per_sat = 900.0 ** 2 / nav_ref.C + nav_ref.C * 2e-15 / (2 * h) + 1e-6
    dop, ms, frac = [], [], []
    for eph in geo["ephs"]:
        tt = [nav_ref.truth_tx(eph, geo["rx"] + v * (s * h / (1 + drift)), geo["ref_ms"], np.array([t0 + s * h / (1 + drift)]))[0] for s in (-1, 0, 1)]
        dop.append(rate_ref.L1 * ((tt[2] - tt[0]) / (2 * h) - 1.0))
        m, f = nav_ref.split_time(geo["ref_ms"], np.array([tt[1]]))
        ms.append(int(m[0])), frac.append(float(f[0]))
    dop, ms, frac = np.array(dop), np.array(ms), np.array(frac)
    rng = np.random.default_rng(11)
    for k in (4, 5, 8, 12):
        sel = list(geo["subsets"][k])
        w = dict(zip(sel, rng.uniform(0.5, 2.0, len(sel))))
        if k >= 8:
            sel.remove(sel[2])
        H, y = rate_ref.vel_rows(geo["ephs"], sel, ms[sel], frac[sel], dop[sel], geo["rx"], geo["ref_ms"], t0)
        ww = np.array([w[j] for j in sel])
        x = np.linalg.solve(H.T @ (ww[:, None] * H), H.T @ (ww * y))
        g = np.abs(rate_ref.gain(H, ww)).sum(axis=1)
        err, cerr = np.abs(x[:3] - v).max(), abs(x[3] - nav_ref.C * drift)
        print("venu %s drift %g, %2d satellites: velocity error %.3g m/s (bound %.3g), c * drift error %.3g m/s (bound %.3g)"
              % (venu, drift, len(sel), err, per_sat * g[:3].max(), cerr, per_sat * g.max()))
        assert err <= per_sat * g[:3].max() and cerr <= per_sat * g.max()
