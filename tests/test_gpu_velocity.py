"""Carrier observables and velocity on the GPU (gpsacq_rate_observables*, gpsacq_sat_rates*, gpsacq_vel_batch*,
gpsacq_pvt_track_device; csrc/obs_kernels.hip, csrc/nav_kernels.hip) against tests/rate_ref.py, the models of include/gpsacq.h in
Python integers and float64.

1. fabricated records, byte for byte (doppler_hz included: one fp64 product and one fp64 quotient on both sides), the edges of
   every channel, the device forms, pvt_track_device against its parts, argument errors;
2. sat_rates against the analytic reference;
3. truth recovery of velocity() without a capture, the device against the reference solver, the failure statuses.

The figures themselves are printed before the assertions (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest

import nav_ref
import obs_ref
import rate_ref
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu
MAX_EPOCHS = 1024
COUNTS = [1000, 0, 65, 129, 1, 63, 64, 1000, 129, 65, 64, 63]
NEGATIVE, WRAPPED = 5, 7  # the channel whose every d_t is negative; the one with a two's-complement nominal word


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1. fabricated records ---------------------------------------------------------------------------------------------------
_pools = {}


def pool(spm):
    """12 fabricated channels at spm samples per millisecond, made once and never written to: records [12][1024] whose lo_rate
    walks around each channel's nominal word (the rows past each count filled with 0xFF bytes, which no kernel may read),
    n_epochs, chans, nom_words, tags, and the reference's A_t per channel."""
    import gpsacq
    if spm in _pools:
        return _pools[spm]
    rec = np.full((12, MAX_EPOCHS), 0xFF, np.uint8).repeat(40, axis=1).view(gpsacq.TRACK_RECORD_DTYPE)
    chans = np.zeros(12, gpsacq.TRACK_CHAN_DTYPE)
    tags = np.zeros(12, gpsacq.TIME_TAG_DTYPE)
    nom = np.zeros(12, np.uint32)
    rng = np.random.default_rng(spm + 1)
    for c, n in enumerate(COUNTS):
        r, ch, _ = obs_ref.fabricate(100 * spm + c, n, spm, prn=c + 1)
        # an NCO word is cycles per sample mod 1: at 2800 samples per millisecond 4.092 MHz is more than one cycle per sample
        word = ((-int(0.21 * 2 ** 32)) if c == WRAPPED else int(4.092e6 / (spm * 1000.0) * 2 ** 32) + 1000 * c) & 0xFFFFFFFF
        rec[c, :n] = rate_ref.walk_lo_rate(r, 7 * spm + c, word, 40000, sign=-1 if c == NEGATIVE else 0)
        chans[c] = ch[0]
        chans["lo_nom"][c] = np.array([word << 32], np.uint64).view(np.int64)[0]
        nom[c] = word
        tags[c] = (int(rng.integers(0, 6000)), int(rng.integers(0, obs_ref.WEEK_MS)), c, 1)
    tags[3]["valid"] = 0  # a rate observation needs no time tag
    ne = np.array(COUNTS, np.int32)
    for a in (rec, chans, tags, ne, nom):
        a.setflags(write=False)
    _pools[spm] = (rec, ne, chans, nom, tags)
    return _pools[spm]


def _take(spm, cols):
    return tuple(a[cols].copy() for a in pool(spm))


def _compare(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if got.tobytes() == ref.tobytes():
        return
    bad = np.argwhere(got.view(np.uint8).reshape(got.shape + (32,)) != ref.view(np.uint8).reshape(ref.shape + (32,)))
    i, c = bad[0][:2]
    raise AssertionError("%s: %d rate observations differ, first at [%d][%d]: %r != %r" % (what, len({(a, b) for a, b, _ in bad}), i, c, got[i, c], ref[i, c]))


@pytest.mark.parametrize("avg", ["1", "2", "spm", "20spm+1"])
@pytest.mark.parametrize("step", ["1", "spm", "7spm+3"])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_chans", [1, 4, 12])
@pytest.mark.parametrize("spm", [2800, 5456])
def test_fabricated_records_byte_for_byte(eng, spm, n_chans, n_fix, step, avg):
    rx_step = {"1": 1, "spm": spm, "7spm+3": 7 * spm + 3}[step]
    W = {"1": 1, "2": 2, "spm": spm, "20spm+1": 20 * spm + 1}[avg]
    cols = list(range(n_chans)) if n_chans > 1 else [(n_fix + rx_step + W) % 12]
    rec, ne, chans, nom, _ = _take(spm, cols)
    starts = [int(rec["sample"][c, 0]) for c in range(len(cols)) if ne[c] > 0]
    # the first instants have R_a before some channel's record 0; with step 1 start where the long window has just become whole
    first = max(0, (min(starts) if starts else 1000) - 3 + (W // 2 if rx_step == 1 else 0))
    fs = 5.456e6  # the engine's, whatever spm the records were fabricated at
    got = eng.rate_observables(rec, ne, chans, first, rx_step, n_fix, W, nom_words=nom)
    ref = rate_ref.rate_observables(rec, ne, chans, nom, first, rx_step, n_fix, W, fs)
    _compare(got, ref, "spm %d n_chans %d n_fix %d step %s W %s" % (spm, n_chans, n_fix, step, avg))
    assert got[got["valid"] == 0].tobytes() == bytes(32 * int((got["valid"] == 0).sum()))
    assert (got["weight"][got["valid"] == 1] == 1.0).all()
    if n_chans == 12:
        assert not got["valid"][:, 1].any()  # no epochs
        if n_fix == 257 and step == "spm" and W <= spm:
            assert got["valid"][:, 0].sum() >= 240 and got["valid"][:, 3].sum() >= 100  # no tag, still observed
            v = got["valid"][:, NEGATIVE] == 1
            assert v.sum() >= 40 and (got["doppler_hz"][v, NEGATIVE] < 0).all() and (np.diff(got["adr"][v, NEGATIVE]) < 0).all()
            assert got["valid"][:, WRAPPED].sum() >= 240
        if step == "7spm+3" and n_fix == 257:
            assert not got["valid"][150:].any()  # past the end of every channel


def test_default_nominal_words_are_the_one_bit_rule(eng):
    rec, ne, chans, nom, _ = _take(5456, list(range(12)))
    first = int(rec["sample"][0, 0]) + 100
    assert rate_ref.nominal_words(chans) == [int(w) for w in nom]
    a = eng.rate_observables(rec, ne, chans, first, 5456, 40, 64)
    b = eng.rate_observables(rec, ne, chans, first, 5456, 40, 64, nom_words=nom)
    assert a.tobytes() == b.tobytes() and a["valid"].sum() > 200


@pytest.mark.parametrize("W", [1, 2, 1001])
@pytest.mark.parametrize("spm", [2800, 5456])
def test_edges_of_every_channel(eng, spm, W):
    """per channel: R_a one before record 0's sample and exactly on it; R_b at next_sample - 1, at next_sample and past it"""
    rec, ne, chans, nom, _ = _take(spm, list(range(12)))
    for c in range(12):
        n = int(ne[c])
        if n == 0:
            continue
        s0, nxt = int(rec["sample"][c, 0]), int(chans["next_sample"][c])
        cases = ((s0 + W // 2 - 1, [0, 1, 1]), (nxt - 1 - W + W // 2 - 1, [1, 1, 0, 0]))
        for first, want in cases:
            if first < 0:  # a one-epoch channel at the very start of the stream, shorter than the window
                continue
            got = eng.rate_observables(rec, ne, chans, first, 1, len(want), W, nom_words=nom)
            _compare(got, rate_ref.rate_observables(rec, ne, chans, nom, first, 1, len(want), W, 5.456e6), "channel %d at %d" % (c, first))
            if nxt - s0 > W + 4:  # the channel is longer than the window: both ends can be met separately
                assert list(got["valid"][:, c]) == want, (c, first, W)


def test_device_forms_equal_host_form(eng):
    import gpsacq
    import torch
    rec, ne, chans, nom, tags = _take(5456, list(range(12)))
    ephs = to_records(geometry("north")["ephs"])
    first, step, n_fix, W = int(rec["sample"][0, 0]) + 3000, 3 * 5456 + 1, 130, 5000
    host = eng.rate_observables(rec, ne, chans, first, step, n_fix, W, nom_words=nom)
    assert host["valid"].sum() > 300
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_rate, d_rate2, d_obs, d_obs2 = fill(host.size * 32), fill(host.size * 32), fill(host.size * 32), fill(host.size * 32)
    d_fix, d_fix2, d_fix3 = (fill(n_fix * gpsacq.FIX_DTYPE.itemsize) for _ in range(3))
    d_vel, d_vel2 = fill(n_fix * gpsacq.VEL_DTYPE.itemsize), fill(n_fix * gpsacq.VEL_DTYPE.itemsize)
    torch.cuda.synchronize()
    eng.rate_observables_device(d_rec.data_ptr(), MAX_EPOCHS, ne, chans, first, step, n_fix, W, d_rate.data_ptr(), nom_words=nom, sync=False)
    eng.fix_track_device(ephs, d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, d_fix.data_ptr(), d_obs_ptr=d_obs.data_ptr(), sync=False)
    eng.pvt_track_device(ephs, d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, W, d_fix2.data_ptr(), d_vel.data_ptr(),
                         d_obs_ptr=d_obs2.data_ptr(), d_rate_obs_ptr=d_rate2.data_ptr(), nom_words=nom, sync=False)
    eng.pvt_track_device(ephs, d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, W, d_fix3.data_ptr(), d_vel2.data_ptr(),
                         nom_words=nom, sync=True)  # observations in engine scratch
    assert d_rate.cpu().numpy().tobytes() == host.tobytes()
    assert d_rate2.cpu().numpy().tobytes() == host.tobytes()
    obs = d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 12)
    fix = d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE)
    assert d_obs2.cpu().numpy().tobytes() == obs.tobytes()
    assert d_fix2.cpu().numpy().tobytes() == fix.tobytes() and d_fix3.cpu().numpy().tobytes() == fix.tobytes()
    vel = eng.velocity(ephs, obs, host, fix)
    assert d_vel.cpu().numpy().tobytes() == vel.tobytes() and d_vel2.cpu().numpy().tobytes() == vel.tobytes()
    # rows of fabricated times: a fix that failed gives NO_FIX, and whatever came out is the same on both paths
    assert ((vel["status"] == gpsacq.VEL_NO_FIX) == (fix["status"] != gpsacq.FIX_OK)).all()
    t = eng.velocity_last_ms()
    assert len(t) == 4 and all(x > 0 for x in t)


def test_argument_errors_leave_the_output_untouched(eng):
    import gpsacq
    import torch
    rec, ne, chans, nom, tags = _take(2800, list(range(12)))
    ephs = to_records(geometry("north")["ephs"])
    lib, h = eng._lib, eng._h
    out = np.full(8 * 12 * 32, 0xA5, np.uint8)
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_out, d_obs, d_fix, d_vel = fill(8 * 12 * 32), fill(8 * 12 * 32), fill(8 * 80), fill(8 * 72)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ok = dict(rec=_p(rec), mx=MAX_EPOCHS, ne=_p(ne), ch=_p(chans), nw=_p(nom), nc=12, first=1000, step=2800, n_fix=8, W=100)
    short = np.array(ne)
    short[4] = MAX_EPOCHS + 1
    negative = np.array(ne)
    negative[1] = -1
    bad = [dict(rec=None), dict(ne=None), dict(ch=None), dict(nw=None), dict(nc=0), dict(nc=13), dict(nc=-1), dict(step=0), dict(n_fix=0), dict(W=0),
           dict(ne=_p(short)), dict(ne=_p(negative)), dict(mx=999), dict(first=(1 << 64) - 5, step=1)]
    for change in bad:
        a = dict(ok, **change)
        args = (a["mx"], a["ne"], a["ch"], a["nw"], a["nc"], a["first"], a["step"], a["n_fix"], a["W"])
        assert lib.gpsacq_rate_observables(h, a["rec"], *args, _p(out)) == 1, change
        d = None if a["rec"] is None else d_rec.data_ptr()
        assert lib.gpsacq_rate_observables_device(h, d, *args, d_out.data_ptr(), 1) == 1, change
        assert lib.gpsacq_pvt_track_device(h, _p(ephs), 12, d, a["mx"], a["ne"], a["ch"], _p(tags), a["nw"], a["nc"], a["first"], a["step"], a["n_fix"],
                                           a["W"], d_obs.data_ptr(), d_out.data_ptr(), d_fix.data_ptr(), d_vel.data_ptr(), 1) == 1, change
    args = (ok["mx"], ok["ne"], ok["ch"], ok["nw"], ok["nc"], ok["first"], ok["step"], ok["n_fix"], ok["W"])
    assert lib.gpsacq_rate_observables(h, ok["rec"], *args, None) == 1
    assert lib.gpsacq_rate_observables_device(h, d_rec.data_ptr(), *args, None, 1) == 1
    pvt = lambda eph, n_eph, tg, fx, vl: lib.gpsacq_pvt_track_device(h, eph, n_eph, d_rec.data_ptr(), ok["mx"], ok["ne"], ok["ch"], tg, ok["nw"], 12, 1000, 2800, 8,
                                                                     100, d_obs.data_ptr(), d_out.data_ptr(), fx, vl, 1)
    assert pvt(None, 12, _p(tags), d_fix.data_ptr(), d_vel.data_ptr()) == 1
    assert pvt(_p(ephs), 0, _p(tags), d_fix.data_ptr(), d_vel.data_ptr()) == 1
    assert pvt(_p(ephs), 12, None, d_fix.data_ptr(), d_vel.data_ptr()) == 1
    assert pvt(_p(ephs), 12, _p(tags), None, d_vel.data_ptr()) == 1
    assert pvt(_p(ephs), 12, _p(tags), d_fix.data_ptr(), None) == 1
    # velocity: a NULL row, a row length outside 1 .. 12, no fixes
    vel_out = np.full(8 * 72, 0xA5, np.uint8)
    obs = np.zeros((8, 12), gpsacq.OBS_DTYPE)
    robs = np.zeros((8, 12), gpsacq.RATE_OBS_DTYPE)
    fixes = np.zeros(8, gpsacq.FIX_DTYPE)
    for a in ((None, _p(robs), _p(fixes), 8, 12), (_p(obs), None, _p(fixes), 8, 12), (_p(obs), _p(robs), None, 8, 12), (_p(obs), _p(robs), _p(fixes), 0, 12),
              (_p(obs), _p(robs), _p(fixes), 8, 0), (_p(obs), _p(robs), _p(fixes), 8, 13)):
        assert lib.gpsacq_vel_batch(h, _p(ephs), 12, *a, _p(vel_out)) == 1, a
    assert lib.gpsacq_vel_batch(h, _p(ephs), 12, _p(obs), _p(robs), _p(fixes), 8, 12, None) == 1
    robs["weight"][2, 3] = -1.0
    assert lib.gpsacq_vel_batch(h, _p(ephs), 12, _p(obs), _p(robs), _p(fixes), 8, 12, _p(vel_out)) == 1
    eng.synchronize()
    assert (out == 0xA5).all() and (vel_out == 0xA5).all()
    for d in (d_out, d_obs, d_fix, d_vel):
        assert (d.cpu().numpy() == 0xA5).all()
    with pytest.raises(gpsacq.GpsAcqError) as ei:
        eng.rate_observables(rec, ne, chans, 1000, 2800, 8, 0, nom_words=nom)
    assert ei.value.code == 1 and "avg_samples" in str(ei.value)
    with pytest.raises(ValueError):
        eng.rate_observables(rec, ne[:5], chans, 1000, 1, 8, 1)
    # and the same arguments, unbroken, work
    assert lib.gpsacq_rate_observables(h, ok["rec"], *args, _p(out)) == 0 and not (out == 0xA5).all()


# ---- 2. satellite velocity and clock drift -----------------------------------------------------------------------------------
def test_sat_rates_against_the_reference(eng):
    """1e-7 m/s: the Kepler stop of 1e-12 rad times the orbital speed 3.9e3 m/s is 4e-9 m/s, fp64 rounding of 3e3 m/s values
    through ~50 operations below that; 1e-16 s/s: the drift is ~1e-11, its ulp 1.6e-27, the Kepler stop moves the relativistic rate
    (7e-12 s/s) by 1e-12 of itself."""
    import gpsacq
    geo = geometry("north")
    ephs = to_records(geo["ephs"])
    rng = np.random.default_rng(5)
    n = 200
    obs = np.zeros((n, 12), gpsacq.OBS_DTYPE)
    obs["eph"] = np.arange(12)[None, :]
    obs["valid"], obs["weight"] = 1, 1.0
    obs["tx_ms"] = geo["ref_ms"] + rng.integers(-3_000_000, 3_000_000, (n, 12))
    obs["tx_frac"] = rng.uniform(0, 1e-3, (n, 12))
    got = eng.sat_rates(ephs, obs)
    worst = np.zeros(2)
    for j, eph in enumerate(geo["ephs"]):
        v, cd = rate_ref.sat_rate(eph, obs["tx_ms"][:, j], obs["tx_frac"][:, j])
        dv = np.abs(np.stack([got["vx"][:, j], got["vy"][:, j], got["vz"][:, j]], 1) - v).max()
        worst = np.maximum(worst, [dv, np.abs(got["clock_drift"][:, j] - cd).max()])
    print("sat_rates against the reference: velocity %.3g m/s, clock drift %.3g s/s" % tuple(worst))
    assert worst[0] <= 1e-7 and worst[1] <= 1e-16
    speed = np.sqrt(got["vx"] ** 2 + got["vy"] ** 2 + got["vz"] ** 2)
    assert ((speed > 2500) & (speed < 3500)).all()
    # the positions next to them are untouched by the new kernel: sat_states still what nav_ref says
    st = eng.sat_states(ephs, obs[:4])
    p, _ = nav_ref.sat_state(geo["ephs"][3], obs["tx_ms"][:4, 3], obs["tx_frac"][:4, 3])
    assert np.abs(np.stack([st["x"][:, 3], st["y"][:, 3], st["z"][:, 3]], 1) - p).max() < 1e-4
    # masks: invalid observation, invalid ephemeris, bad index
    masked = obs[:3].copy()
    masked["valid"][0, 2] = 0
    masked["eph"][1, 4] = 12
    masked["eph"][2, 5] = -1
    broken = ephs.copy()
    broken["iode3"][7] += 1
    got = eng.sat_rates(broken, masked)
    zero = bytes(32)
    assert got[0, 2].tobytes() == zero and got[1, 4].tobytes() == zero and got[2, 5].tobytes() == zero
    assert all(got[k, 7].tobytes() == zero for k in range(3))
    assert sum(got[k, j].tobytes() == zero for k in range(3) for j in range(12)) == 6


# ---- 3. truth recovery -----------------------------------------------------------------------------------------------------------
H_FD = 0.05          # half the span of the truth's central difference, seconds
PER_SAT = 900.0 ** 2 / nav_ref.C + nav_ref.C * 2e-15 / (2 * H_FD) + 1e-6   # see test_velocity_recovers_the_truth
_truth = {}


def _enu_matrix(lat, lon):
    return np.array([[-math.sin(lon), math.cos(lon), 0.0], [-math.sin(lat) * math.cos(lon), -math.sin(lat) * math.sin(lon), math.cos(lat)],
                     [math.cos(lat) * math.cos(lon), math.cos(lat) * math.sin(lon), math.sin(lat)]])


def truth(eng, venu, drift):
    """65 receive instants 100 ms apart of a receiver that passes geometry("north")'s position at each of them with ENU velocity
    venu and a sampling clock fast by `drift`: observations (nav_ref.truth_tx at the instant), the device's fixes of them, and the
    Dopplers L1 (dt_tx / dt_rx - 1) by a central difference over +-H_FD seconds of RECEIVER time, the receiver moved accordingly."""
    import gpsacq
    key = (tuple(venu), drift)
    if key in _truth:
        return _truth[key]
    geo = geometry("north")
    n = 65
    v = _enu_matrix(geo["lla"][0], geo["lla"][1]).T @ np.asarray(venu, np.float64)
    ref_ms = geo["ref_ms"] + 100 * np.arange(n)
    t0 = 0.3217e-3
    obs = np.zeros((n, 12), gpsacq.OBS_DTYPE)
    rate = np.zeros((n, 12), gpsacq.RATE_OBS_DTYPE)
    dtrue = H_FD / (1.0 + drift)  # true seconds in H_FD seconds of the receiver's clock
    for j, eph in enumerate(geo["ephs"]):
        t = [nav_ref.truth_tx(eph, geo["rx"][:, None] + v[:, None] * (s * dtrue) * np.ones(n), ref_ms, np.full(n, t0 + s * dtrue)) for s in (-1, 0, 1)]
        ms, frac = nav_ref.split_time(ref_ms, t[1])
        obs["tx_ms"][:, j], obs["tx_frac"][:, j], obs["eph"][:, j] = ms, frac, j
        rate["doppler_hz"][:, j] = rate_ref.L1 * ((t[2] - t[0]) / (2 * H_FD) - 1.0)
    obs["valid"], obs["weight"], rate["valid"], rate["weight"] = 1, 1.0, 1, 1.0
    fix = eng.fix(to_records(geo["ephs"]), obs)
    assert (fix["status"] == 0).all()
    assert np.abs(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"]).max() < 1e-3
    for a in (obs, rate, fix):
        a.setflags(write=False)
    _truth[key] = (geo, v, obs, rate, fix)
    return _truth[key]


@pytest.mark.parametrize("drift", [0.0, 2e-6, -2e-6])
@pytest.mark.parametrize("venu", [(0.0, 0.0, 0.0), (30.0, -20.0, 5.0), (250.0, 100.0, -50.0)])
def test_velocity_recovers_the_truth(eng, venu, drift):
    """The model is first order, so the bound is derived, not measured.  Per satellite the right-hand side is off by at most
        rho'^2 / c            <= 900^2 / 3e8             = 2.7e-3 m/s   the neglected second-order terms
      + c 2e-15 / (2 H_FD)    = 3e8 * 2e-15 / 0.1        = 6e-6  m/s   nav_ref.truth_tx is good to 1e-15 s, twice, over 0.1 s
      + range jerk H_FD^2 / 6 <= 2e-3 * 0.0025 / 6       < 1e-6  m/s   the central difference of the truth
    = PER_SAT = 2.71e-3 m/s, and the solution by at most PER_SAT times the subset's ||(H^T W H)^-1 H^T W||_inf (row sums of absolute
    values), computed here from rate_ref's rows; c * drift by the same.  On the CPU rate_ref's own solver on the same grid
    (tests/test_rate_ref.py::test_velocity_model_over_the_truth_grid, which prints every case) shows at worst 3.0e-3 m/s of velocity
    against a bound of 8.1e-3 (4 satellites, standing still, drift 2e-6) and 4.1e-3 m/s of c * drift against 8.1e-3 (4 satellites,
    standing still, drift -2e-6): the common part of the neglected terms, c drift^2 and the like, goes into the clock.  An MI355X
    shows the same figures to three digits."""
    import gpsacq
    geo, v, obs, rate, fix = truth(eng, venu, drift)
    ephs = to_records(geo["ephs"])
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in (4, 5, 8, 12):
        sel = geo["subsets"][k]
        o, r = obs.copy(), rate.copy()
        o["valid"] = 0
        o["valid"][:, sel] = 1
        r["weight"][:, sel] = rng.uniform(0.5, 2.0, len(sel))  # unequal weights, the same in every row
        used = list(sel)
        if k >= 8:  # one masked satellite: its rate observation is not valid
            r["valid"][:, sel[2]] = 0
            used.remove(sel[2])
        H, _ = rate_ref.vel_rows(geo["ephs"], used, obs["tx_ms"][0, used], obs["tx_frac"][0, used], rate["doppler_hz"][0, used], geo["rx"], fix["rx_ms"][0], fix["rx_frac"][0])
        g = np.abs(rate_ref.gain(H, r["weight"][0, used])).sum(axis=1)
        for n_fix in (1, 64, 65):
            got = eng.velocity(ephs, o[:n_fix], r[:n_fix], fix[:n_fix])
            assert (got["status"] == gpsacq.VEL_OK).all() and (got["n_used"] == len(used)).all()
            err = np.abs(np.stack([got["vx"], got["vy"], got["vz"]], 1) - v).max()
            derr = np.abs(got["drift"] - drift).max()
            enu = np.abs(np.stack([got["ve"], got["vn"], got["vu"]], 1) - np.asarray(venu)).max()
            worst = max(worst, err / (PER_SAT * g[:3].max()))
            if n_fix == 65:
                print("venu %s drift %g, %2d satellites: velocity error %.3g m/s (bound %.3g), drift error %.3g (bound %.3g), rms %.3g m/s"
                      % (venu, drift, len(used), err, PER_SAT * g[:3].max(), derr, PER_SAT * g.max() / nav_ref.C, got["rms"].max()))
            assert err <= PER_SAT * g[:3].max() and derr <= PER_SAT * g.max() / nav_ref.C
            assert enu <= math.sqrt(3) * PER_SAT * g[:3].max() + 1e-6  # a rotation of the ECEF error (the fix's lat / lon are good to 1e-10 rad)
    print("worst velocity error over bound: %.2f" % worst)


def test_device_against_the_reference_solver(eng):
    """perturbed Dopplers (a model that no longer fits): the device's least squares against numpy's, within 1e-7 m/s -- the
    normal matrix of unit vectors has a condition number below 1e3, fp64 leaves 1e-13 relative of velocities up to 1e3 m/s; the
    satellite states on both sides differ by the 4e-9 m/s of test_sat_rates_against_the_reference."""
    import gpsacq
    geo, v, obs, rate, fix = truth(eng, (250.0, 100.0, -50.0), 2e-6)
    ephs = to_records(geo["ephs"])
    rng = np.random.default_rng(3)
    r = rate[:12].copy()
    r["doppler_hz"] += rng.uniform(-50, 50, r.shape)
    r["weight"] = rng.uniform(0.25, 4.0, r.shape)
    o = obs[:12].copy()
    o["valid"][3, [0, 5]] = 0
    r["valid"][4, [1, 2, 7]] = 0
    got = eng.velocity(ephs, o, r, fix[:12])
    worst = np.zeros(3)
    for k in range(12):
        ref = rate_ref.velocity(geo["ephs"], o[k], r[k], fix[k])
        assert got["status"][k] == ref["status"] == gpsacq.VEL_OK and got["n_used"][k] == ref["n_used"]
        worst = np.maximum(worst, [np.abs(np.array([got["vx"][k], got["vy"][k], got["vz"][k]]) - ref["v"]).max(),
                                   abs(got["drift"][k] - ref["drift"]) * nav_ref.C, abs(got["rms"][k] - ref["rms"])])
        assert np.abs(np.array([got["ve"][k], got["vn"][k], got["vu"][k]]) - ref["enu"]).max() <= 1e-7
    print("against the reference solver, 12 rows: velocity %.3g m/s, c * drift %.3g m/s, rms %.3g m/s" % tuple(worst))
    assert (worst <= 1e-7).all() and got["rms"].min() > 1.0  # 50 Hz is 9.5 m/s: the residuals show it
    assert got["n_used"][3] == 10 and got["n_used"][4] == 9


def test_failed_rows_are_all_zero(eng):
    import gpsacq
    geo, v, obs, rate, fix = truth(eng, (30.0, -20.0, 5.0), 0.0)
    ephs = to_records(geo["ephs"])
    o, r, f = obs[:6].copy(), rate[:6].copy(), fix[:6].copy()
    o["valid"][0, 3:] = 0                       # three satellites
    r["valid"][1, :9] = 0                       # three rate observations
    f["status"][2] = gpsacq.FIX_NO_CONVERGE     # no fix
    f["status"][3] = gpsacq.FIX_TOO_FEW
    o[4, :] = o[4, 0]                           # twelve times the same satellite: rows of the normal matrix all alike
    r[4, :] = r[4, 0]
    got = eng.velocity(ephs, o, r, f)
    assert list(got["status"]) == [gpsacq.VEL_TOO_FEW, gpsacq.VEL_TOO_FEW, gpsacq.VEL_NO_FIX, gpsacq.VEL_NO_FIX, gpsacq.VEL_SINGULAR, gpsacq.VEL_OK]
    assert list(got["n_used"]) == [3, 3, 0, 0, 12, 12]
    for k in range(5):
        assert got[k].tobytes()[8:] == bytes(64), k
        assert rate_ref.velocity(geo["ephs"], o[k], r[k], f[k])["status"] == got["status"][k]


# ---- 4. the whole chain --------------------------------------------------------------------------------------------------------
FS, FC, SPM = 5.456e6, 4.092e6, 5456
N_BYTES = int(20 * FS) // 8
R_STAR = int(19.5 * FS)
TOW0 = 64898
BIT0_MS = (TOW0 - 1) * 6000
REF_MS, REF_FRAC = BIT0_MS + 18_275, 0.3217e-3   # the receive time at R*
AVG = int(0.5 * FS)                              # half a second of samples: R_b of R* is 19.75 s, inside the capture
LAMBDA = nav_ref.C / rate_ref.L1                 # 0.1903 m


@pytest.fixture(scope="module")
def chain(eng):
    """tests/test_gpu_observables.py's 20-s scenario by its recipe (stationary receiver, Dopplers consistent with the geometry at
    R*), built here once: capture, channels, decode, then pvt_track_device at 501 instants a millisecond apart around R*"""
    import gpsacq
    import torch
    geo = geometry("north")
    sel = geo["subsets"][5]
    ephs = [geo["ephs"][k] for k in sel]
    sats, nav = [], []
    amps = np.linspace(0.15, 0.2, len(sel))
    for j, eph in enumerate(ephs):
        t = nav_ref.truth_tx(eph, geo["rx"], REF_MS, np.array([REF_FRAC - 0.5, REF_FRAC, REF_FRAC + 0.5]))
        dop = rate_ref.L1 * ((t[2] - t[0]) - 1.0)
        cp = ((REF_MS - BIT0_MS) + t[1] * 1e3) * FS / (1000.0 * (1.0 + dop / rate_ref.L1)) - R_STAR
        sats.append((int(eph["prn"]), float(amps[j]), float(dop), float(cp), 0.1 + 0.17 * j))
        nav.append(1 - 2 * nav_ref.encode_stream(eph, TOW0, ids=(1, 2, 3, 4, 5)).astype(np.int8))
    nav = np.array(nav)
    d_bits = torch.zeros(N_BYTES, dtype=torch.uint8, device="cuda:0")
    d_peaks = torch.zeros(32 * gpsacq.PEAK_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.generate_device(d_bits.data_ptr(), N_BYTES, sats, noise_sigma=1.0, seed=77, nav=nav)
    eng.search_device(d_bits.data_ptr(), 32, d_peaks.data_ptr())
    peaks = d_peaks.cpu().numpy().view(gpsacq.PEAK_DTYPE)
    prns = [s[0] for s in sats]
    assert all(peaks["snr"][p - 1] > 25 for p in prns), peaks["snr"]
    chans = np.concatenate([eng.track_start(p, peaks[p - 1], (p - 1) * gpsacq.BLOCK_BYTES * 8) for p in prns])
    max_epochs = 20100
    d_prompt = torch.zeros(5 * max_epochs * 2, dtype=torch.int32, device="cuda:0")
    d_rec = torch.zeros(5 * max_epochs * 40, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ne = eng.track_device(d_bits.data_ptr(), N_BYTES, chans, 0, max_epochs, d_prompt.data_ptr(), d_rec.data_ptr())
    prompt = d_prompt.cpu().numpy().reshape(5, max_epochs, 2)
    tags, recs, fails = [], [], 0
    for c, prn in enumerate(prns):
        n = int(ne[c])
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=int(chans["epoch"][c]) - n + 1000)
        sf, _ = gpsacq.nav_subframes(bits)
        assert len(sf) >= 3, (prn, len(bits), len(sf))
        fails += gpsacq.nav_subframes(bits[int(sf["bit_offset"][0]):])[1]
        recs.append(gpsacq.ephemeris(sf, prn))
        tags.append(gpsacq.time_tag(sf[0], e0, c))
    tags, recs = np.concatenate(tags), np.concatenate(recs)
    n_fix, first = 501, R_STAR - 250 * SPM
    fill = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    d_fix, d_vel, d_obs, d_rate = fill(n_fix * 80), fill(n_fix * 72), fill(n_fix * 5 * 32), fill(n_fix * 5 * 32)
    torch.cuda.synchronize()
    eng.pvt_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, AVG, d_fix.data_ptr(), d_vel.data_ptr(),
                         d_obs_ptr=d_obs.data_ptr(), d_rate_obs_ptr=d_rate.data_ptr())
    out = dict(geo=geo, ephs=ephs, sats=sats, chans=chans, ne=ne, n_fix=n_fix, first=first, parity_failures=fails,
               records=d_rec.cpu().numpy().view(gpsacq.TRACK_RECORD_DTYPE).reshape(5, max_epochs),
               obs=d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 5), rate=d_rate.cpu().numpy().view(gpsacq.RATE_OBS_DTYPE).reshape(n_fix, 5),
               fix=d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE), vel=d_vel.cpu().numpy().view(gpsacq.VEL_DTYPE), capture=d_bits.cpu().numpy(),
               kernel_ms=eng.observables_last_ms() + eng.fix_last_ms() + eng.velocity_last_ms())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_chain_rate_observations_equal_the_reference(chain):
    import gpsacq
    assert (chain["chans"]["status"] == gpsacq.TRACK_OK).all() and chain["parity_failures"] == 0
    nom = rate_ref.nominal_words(chain["chans"])
    ref = rate_ref.rate_observables(chain["records"], chain["ne"], chain["chans"], nom, chain["first"], SPM, chain["n_fix"], AVG, FS)
    _compare(chain["rate"], ref, "whole chain")
    print("kernel ms (code_pos, observe, sat_state, fix, carrier_acc, observe_rate, sat_state_rate, vel): %s" % (chain["kernel_ms"],))
    valid = chain["rate"]["valid"].all(axis=1)
    # R_b = R + 250 ms reaches the end of the records a little before 250 ms past R*; every instant up to R* is whole
    assert valid[:251].all() and not valid[-1] and 251 <= valid.sum() < 501
    # the channels end within a millisecond of each other: a row with four rate observations left still has a velocity
    assert ((chain["vel"]["status"] == gpsacq.VEL_OK) == ((chain["rate"]["valid"].sum(axis=1) >= 4) & (chain["fix"]["status"] == gpsacq.FIX_OK))).all()
    assert (chain["vel"]["n_used"][chain["vel"]["status"] == gpsacq.VEL_OK] == chain["rate"]["valid"].sum(axis=1)[chain["vel"]["status"] == gpsacq.VEL_OK]).all()


def test_chain_doppler_and_velocity_at_r_star(chain):
    """A lock-and-sign check, not a precision claim.  A Costas loop that decodes subframes without a parity failure keeps its
    phase within a quarter cycle of the signal, so the phase difference over the 0.5 s window is within half a cycle: 1 Hz.  A wrong
    sign is kHz.  The velocity of the stationary receiver is then below 1 Hz x 0.1903 m times the subset's ||(H^T H)^-1 H^T||_inf,
    computed here; a missing Omega_e x r is hundreds of m/s.  The same scenario on the CPU before any GPU run -- a numpy capture by the
    generator's law with its own noise (test_track_ref.make_capture), tests/c/track_model.c started at each satellite's search bin,
    the library's host NAV decode and time tags, obs_ref, nav_ref's solver, rate_ref: no parity failure, Doppler errors -0.006 /
    -0.011 / -0.011 / 0.046 / 0.054 Hz, |v| 0.014 m/s at R* (bound 0.571, gain 3.00), at most 0.052 m/s (mean 0.016) over the 500
    complete instants: the model alone stays 18 times under the Doppler bound and 40 times under the velocity bound.  Measured on
    an MI355X by this test: Doppler errors -0.004 / -0.008 / 0.028 / -0.057 / 0.025 Hz, |v| 0.020 m/s at R*, at most 0.046 m/s
    (mean 0.016) over the 500 complete instants."""
    import gpsacq
    row = 250
    assert chain["first"] + row * SPM == R_STAR
    rate, vel, fix, obs = chain["rate"], chain["vel"], chain["fix"], chain["obs"]
    err = [float(rate["doppler_hz"][row, c]) - s[2] for c, s in enumerate(chain["sats"])]
    print("Doppler error at R*: %s Hz" % ["%.3f" % e for e in err])
    H, _ = rate_ref.vel_rows(chain["ephs"], list(range(5)), obs["tx_ms"][row], obs["tx_frac"][row], rate["doppler_hz"][row],
                             (fix["x"][row], fix["y"][row], fix["z"][row]), int(fix["rx_ms"][row]), float(fix["rx_frac"][row]))
    g = np.abs(rate_ref.gain(H, np.ones(5))).sum(axis=1).max()
    ok = vel["status"] == gpsacq.VEL_OK
    speed = np.sqrt(vel["vx"] ** 2 + vel["vy"] ** 2 + vel["vz"] ** 2)
    print("|v| at R*: %.4f m/s (bound %.3f, gain %.2f), drift %.3e, rms %.4f m/s; over the %d complete instants: max %.4f, mean %.4f m/s"
          % (speed[row], LAMBDA * g, g, vel["drift"][row], vel["rms"][row], ok.sum(), speed[ok].max(), speed[ok].mean()))
    assert vel["status"][row] == gpsacq.VEL_OK and vel["n_used"][row] == 5
    assert max(abs(e) for e in err) < 1.0
    assert speed[row] < 1.0 * LAMBDA * g


def test_gps_track_prints_velocities(chain, tmp_path):
    """the front end on the same capture: without GPSACQ_VELOCITY no line changes; with it a vel line follows the fixes whose
    half-second window lies inside the records"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "cap.bin"
    chain["capture"].tofile(path)
    exe = os.path.join(root, "gnss-gps-sdr_amd", "bin", "gps_track")
    env = {k: v for k, v in os.environ.items() if k != "GPSACQ_VELOCITY"}
    plain = subprocess.run([exe, str(path), str(FC), str(FS)], capture_output=True, text=True, timeout=120, env=env)
    with_v = subprocess.run([exe, str(path), str(FC), str(FS)], capture_output=True, text=True, timeout=120, env=dict(env, GPSACQ_VELOCITY="1"))
    assert plain.returncode == 0 and with_v.returncode == 0, plain.stderr + with_v.stderr
    assert "vel " not in plain.stdout
    lines = with_v.stdout.splitlines(keepends=True)
    assert "".join(l for l in lines if not l.startswith("vel ")) == plain.stdout
    vels = [l.split() for l in lines if l.startswith("vel ")]
    fixes = [l for l in lines if l.startswith("fix ")]
    assert len(fixes) >= 18 and len(fixes) - 2 <= len(vels) <= len(fixes), with_v.stdout
    for k, l in enumerate(lines):  # a vel line follows its own fix line
        if l.startswith("vel "):
            assert lines[k - 1].startswith("fix ") and lines[k - 1].split()[2] == l.split()[2]
    worst = 0.0
    for f in vels[2:]:  # the loops have settled after the first seconds
        d = dict(zip(f[1::2], f[2::2]))
        worst = max(worst, math.sqrt(float(d["ve"]) ** 2 + float(d["vn"]) ** 2 + float(d["vu"]) ** 2))
        assert int(d["n_used"]) >= 5 and abs(float(d["drift"])) < 1e-7, f
    print("gps_track: %d vel lines, worst |v| %.3f m/s" % (len(vels), worst))
    assert worst < 5.0  # a stationary receiver; a sign or frame error is hundreds of m/s


# ---- 5. one multi-bit IQ case ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("if_hz,mode", [(300e3, 1), (-250e3, 2)])
def test_multibit_doppler_needs_the_nominal_word(if_hz, mode):
    """tests/test_gpu_track_iq.py's +-IF scenario at its shortest (2.8 MHz, 4 satellites, 1.5 s), as a real IF and as complex
    baseband with a negative carrier: with nominal_word_iq8 every locked channel reads its generator Doppler within 1 Hz; with
    lo_nom's word -- the START word of a multi-bit channel -- it would read about 0 Hz for every satellite"""
    import gpsacq
    fs, secs = 2.8e6, 1.5
    rng = np.random.default_rng(int(if_hz) % 1000 + mode)
    prns = rng.choice(np.arange(1, 33), 4, replace=False)
    sats = [(int(p), float(rng.uniform(0.12, 0.2)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, fs / 1000)), float(rng.uniform(0, 1))) for p in prns]
    n = int(secs * fs) - 5
    with gpsacq.Engine(0.7e6, fs, 5000.0, device=0) as eng:
        iq = eng.generate_iq8(n, sats, if_hz=if_hz, scale=16.0, signed=True, seed=11)
        mix = eng.fc - if_hz if mode == 1 else -if_hz
        inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=mix, fs=fs, total_samples=n, multibit=mode)
        p = eng.track_params_iq8(eng.iq8_rms(iq[:2 * 400000], inp))
        pk = np.zeros(4, gpsacq.PEAK_DTYPE)
        pk["snr"] = 100.0
        pk["lo_shift"] = [int(round(s[2] * 40000 / fs)) for s in sats]
        pk["ca_shift"] = [int(round(s[3])) % eng.num_lags for s in sats]
        ch = np.concatenate([eng.track_start_iq8(inp, s[0], pk[k], 0, params=p) for k, s in enumerate(sats)])
        _, rec, ne = eng.track_iq8(iq, inp, ch, records=True, params=p)
        word = eng.nominal_word_iq8(inp)
        f0 = if_hz  # the satellite-free carrier of the raw capture
        assert word == int(round(f0 / fs * 2 ** 32)) & 0xFFFFFFFF and (mode == 1 or word >> 31)  # the complex case is a negative carrier
        R, W = int(1.25 * fs), int(0.4 * fs)
        got = eng.rate_observables(rec, ne, ch, R, 1, 1, W, nom_words=[word] * 4)
        wrong = eng.rate_observables(rec, ne, ch, R, 1, 1, W)
    ref = rate_ref.rate_observables(rec, ne, ch, [word] * 4, R, 1, 1, W, fs)
    assert got.tobytes() == ref.tobytes()
    locked = ch["status"] == gpsacq.TRACK_OK
    err = [float(got["doppler_hz"][0, c]) - sats[c][2] for c in range(4)]
    print("IF %g mode %d: Doppler error %s Hz, locked %s; with lo_nom's word: %s Hz" % (if_hz, mode, ["%.3f" % e for e in err], list(locked),
                                                                                      ["%.1f" % v for v in wrong["doppler_hz"][0]]))
    assert locked.sum() >= 3 and got["valid"][0, locked].all()
    assert all(abs(err[c]) < 1.0 for c in range(4) if locked[c])
    assert all(abs(float(wrong["doppler_hz"][0, c])) < 400.0 for c in range(4) if locked[c])  # the start word is the hit's bin: within half a bin
