"""Signal quality per observation on the GPU (gpsacq_quality_observables*, gpsacq_fix_quality_track_device;
csrc/quality_kernels.hip) against tests/quality_ref.py, the model of include/gpsacq.h in Python integers: every field of the info
record byte for byte except cn0_dbhz, which goes through log10 and is held to 1e-9 dB.

1. crafted records: every chunk boundary of k_quality_acc, windows of 1, 20 and 1024 epochs, values at the edge of the no-wrap
   bound and past it, a lock ratio and a C/N0 exactly on their thresholds, instants before, inside, between and past the records;
2. the in-out observation, host and device forms;
3. the chain to fixes, raw and smoothed, and a gated channel against the same row without it;
4. two satellites 10 dB apart and a channel on noise, on a capture made with numpy by the generator's law (so that the CPU model
   of the channels gives the same records, and the constants below were measured with it);
5. the gps_track front end.

The figures themselves are printed before the assertions (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quality_ref as qr
import smooth_ref
from nav_helpers import geometry, to_records, truth_obs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 64 * 4  # SMOOTH_BLOCK * SMOOTH_RUN of csrc/smooth_launch.hpp: the epochs of one pass of k_quality_acc's wave
CN0_TOL_DB = 1e-9


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def _compare(got, ref, what):
    """every field but cn0_dbhz byte for byte, cn0_dbhz to CN0_TOL_DB"""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    worst = float(np.abs(got["cn0_dbhz"] - ref["cn0_dbhz"]).max()) if got.size else 0.0
    a, b = got.copy(), ref.copy()
    a["cn0_dbhz"], b["cn0_dbhz"] = 0, 0
    if a.tobytes() != b.tobytes():
        size = got.dtype.itemsize
        bad = np.argwhere((a.view(np.uint8).reshape(a.shape + (size,)) != b.view(np.uint8).reshape(b.shape + (size,))).any(axis=-1))
        i, c = bad[0]
        raise AssertionError("%s: %d records differ, first at [%d][%d]: %r != %r" % (what, len(bad), i, c, got[i, c], ref[i, c]))
    assert worst <= CN0_TOL_DB, (what, worst)
    return worst


# ---- 1. crafted records -----------------------------------------------------------------------------------------------------
N_EPOCHS = (0, 1, CH - 1, CH, CH + 1, 2 * CH + 3, 2 * CH + 3, 2 * CH + 3, 2 * CH + 3, CH + 1, 1, 2 * CH + 3)
EDGE, WRAP, EXACT, NO_TAG, MIXED = 6, 7, 8, 9, 11   # the channels with a purpose of their own
_crafted = []


def crafted():
    """twelve channels of epochs about 100 samples long: random prompt sums, and
    channel 6: +-(2^21 - 1) on both arms, the edge of the no-wrap bound;   channel 7: +-(2^26 - 1), past it;
    channel 8: ip = +-2, qp = +-1 -- N / D = 3 / 5 and snr = 4, lin = 4000 exactly, in every window;
    channel 9: a tag that is not valid;   channel 11: stretches of nothing, of power in QP alone, of a constant IP alone.
    Made once and never written to."""
    import gpsacq
    if _crafted:
        return _crafted[0]
    rng = np.random.default_rng(2024)
    max_epochs = max(N_EPOCHS) + 2
    rec = np.zeros((12, max_epochs), gpsacq.TRACK_RECORD_DTYPE)
    chans = np.zeros(12, gpsacq.TRACK_CHAN_DTYPE)
    tags = np.zeros(12, gpsacq.TIME_TAG_DTYPE)
    ne = np.array(N_EPOCHS, np.int32)
    for c, n in enumerate(N_EPOCHS):
        length = rng.integers(95, 106, n)
        start = 1000 + 37 * c
        rec["sample"][c, :n] = start + np.concatenate([[0], np.cumsum(length)[:-1]]) if n else 0
        chans["next_sample"][c] = start + int(length.sum())
        sign = np.where(rng.integers(0, 2, n) > 0, 1, -1)
        ip, qp = sign * rng.integers(1500, 2500, n), rng.integers(-700, 701, n)
        if c == EDGE:
            ip, qp = sign * ((1 << 21) - 1), np.where(rng.integers(0, 2, n) > 0, 1, -1) * ((1 << 21) - 1)
            qp[100:400] //= 7
        elif c == WRAP:
            ip, qp = sign * ((1 << 26) - 1), np.where(rng.integers(0, 2, n) > 0, 1, -1) * ((1 << 26) - 1)
            qp[::3] = 12345
        elif c == EXACT:
            ip, qp = sign * 2, np.where(rng.integers(0, 2, n) > 0, 1, -1)
        elif c == MIXED:
            ip[40:80], qp[40:80] = 0, 0
            ip[120:160] = 0
            ip[200:300], qp[200:300] = -1800, 0
        rec["ip"][c, :n], rec["qp"][c, :n] = ip, qp
        rec["ip"][c, n:], rec["qp"][c, n:] = 0x5A5A5A5A, -0x5A5A5A5A   # never read
        tags[c] = (0, 0, c, 0 if c == NO_TAG else 1)
    for a in (rec, chans, tags, ne):
        a.setflags(write=False)
    _crafted.append((rec, ne, chans, tags))
    return _crafted[0]


def _instants(rec, chans):
    """(first_rx_sample, rx_step, n_fix): several instants per epoch from before record 0; a step of about an epoch that runs past
    every next_sample; a step of a dozen epochs; many blocks of instants across the first chunk boundary"""
    end = int(chans["next_sample"].max())
    return ((900, 7, 300), (990, 103, (end + 500 - 990) // 103 + 1), (1000, 1237, 65), (int(rec["sample"][5, CH]) - 9000, 33, 1025))


PARAMS = (dict(epochs=1, min_epochs=1),
          dict(epochs=20, min_epochs=5, lock_num=3, lock_den=5, cn0_min_lin=4000.0, cn0_ref_lin=4000.0),
          dict(epochs=1024, min_epochs=300, require_lock=0),
          dict(epochs=20, min_epochs=20, cn0_min_lin=float(np.nextafter(4000.0, np.inf)), cn0_ref_lin=1e6, cn0_cap_dbhz=-7.5))


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_crafted_records_byte_for_byte(eng, k):
    import gpsacq
    rec, ne, chans, tags = crafted()
    params = gpsacq.quality_params(**PARAMS[k])
    p = qr.par(params)
    worst, seen = 0.0, 0
    for first, step, n_fix in _instants(rec, chans):
        info = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=params)
        ref = qr.quality(rec, ne, chans, tags, first, step, n_fix, params)
        what = "params %s instants (%d, %d, %d)" % (PARAMS[k], first, step, n_fix)
        worst = max(worst, _compare(info, ref, what))
        R = first + step * np.arange(n_fix)
        for c in range(12):
            usable = (R >= int(rec["sample"][c, 0])) & (R < int(chans["next_sample"][c])) if ne[c] and tags["valid"][c] else np.zeros(n_fix, bool)
            assert (info["epochs"][:, c] > 0).tolist() == usable.tolist(), (what, c)
            assert info[:, c][~usable].tobytes() == bytes(48 * int((~usable).sum()))   # INVALID: 48 zero bytes
        seen |= int(np.bitwise_or.reduce(info["flags"].ravel()))
        assert (info["epochs"] <= p["epochs"]).all()
        assert (((info["flags"] & qr.SHORT) != 0) == ((info["epochs"] > 0) & (info["epochs"] < p["min_epochs"]))).all()
        # one channel on its own: the same column
        one = eng.quality(rec[5:6], ne[5:6], chans[5:6], tags[5:6], first, step, n_fix, params=params)
        assert one.tobytes() == info[:, 5:6].tobytes(), what
        ex = info[:, EXACT][(info["epochs"][:, EXACT] >= p["min_epochs"])]
        if k == 1 and ex.size:   # on both thresholds: locked, not gated, weight exactly 1
            assert (ex["lin"] == 4000.0).all() and ((ex["flags"] & qr.UNLOCKED) == 0).all() and (ex["weight"] == 1.0).all()
        if k == 3 and ex.size:   # the gate one ulp above: weight 0
            assert (ex["lin"] == 4000.0).all() and (ex["weight"] == 0.0).all()
            sat = info[(info["flags"] & qr.SATURATED) != 0]
            assert sat.size == 0 or (sat["cn0_dbhz"] == -7.5).all()
    print("params %s: cn0_dbhz within %.3g dB of the reference; flags seen 0x%x" % (PARAMS[k], worst, seen))
    # every flag occurs: a window of one epoch is never SHORT, and one of 1024 epochs is never FULL here, nor free of noise or power
    want = (0x0F, 0x1F, qr.UNLOCKED | qr.SHORT, 0x1F)[k]
    assert seen & want == want and (k == 2 or seen == want)
    if k == 2:   # the sums of the +-(2^26 - 1) channel do wrap, and the answer is still the model's
        n = int(ne[WRAP])
        assert sum(abs(int(v)) for v in rec["ip"][WRAP, :n]) ** 2 > qr.M64


# ---- 2. the in-out observation, host and device forms -------------------------------------------------------------------------
_fab = []


def fabricated():
    """smooth_ref.fabricate_case: twelve channels a tracking call could have left (one without epochs, one without a tag, two with an
    unlocked stretch), with ephemerides for the chain; made once and never written to"""
    if not _fab:
        arrays = smooth_ref.fabricate_case(5456 + 12, 5456, 12, 600)
        for a in arrays:
            a.setflags(write=False)
        _fab.append(arrays)
    return _fab[0]


def test_in_out_observation_and_device_forms(eng):
    import gpsacq
    import torch
    rec, ne, chans, tags, nom = fabricated()
    first, step, n_fix = int(rec["sample"][0, 0]) - 3 * 5456, 5456 + 1, 700
    params = gpsacq.quality_params(epochs=50)
    obs = eng.observables(rec, ne, chans, tags, first, step, n_fix)
    info = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=params)
    _compare(info, qr.quality(rec, ne, chans, tags, first, step, n_fix, params), "fabricated case")
    out, info2 = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=params, obs=obs)
    assert info2.tobytes() == info.tobytes()
    assert ((obs["valid"] != 0) == (info["epochs"] > 0)).all()   # valid and usable coincide
    assert out.tobytes() == qr.apply_weights(obs, info).tobytes()
    back = out.copy()
    back["weight"] = obs["weight"]
    assert back.tobytes() == obs.tobytes() and out.tobytes() != obs.tobytes()   # nothing but weights moved, and some did
    w = out["weight"][obs["valid"] != 0]
    assert (w == 0).any() and (w == 1).any()
    unl = (info["flags"] & qr.UNLOCKED) != 0
    assert unl[:, 0].sum() >= 30 and (out["weight"][unl] == 0).all()   # the stretch with the power in QP
    # an observation with valid == 0 is not written, whatever it holds
    junk = obs.copy()
    junk[obs["valid"] == 0] = (7, 0, 9, 11, 0.25, 3.0)
    out3, _ = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=params, obs=junk)
    assert out3[obs["valid"] == 0].tobytes() == junk[obs["valid"] == 0].tobytes() and out3[obs["valid"] != 0].tobytes() == out[obs["valid"] != 0].tobytes()
    # params None is the defaults
    assert eng.quality(rec, ne, chans, tags, first, step, n_fix).tobytes() == eng.quality(rec, ne, chans, tags, first, step, n_fix, params=gpsacq.quality_params()).tobytes()
    # device forms
    max_epochs = rec.shape[1]
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_info, d_info2 = fill(info.size * 48), fill(info.size * 48)
    d_obs = torch.from_numpy(obs.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.quality_device(d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_info.data_ptr(), params=params, sync=False)
    eng.quality_device(d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_info2.data_ptr(), d_obs_ptr=d_obs.data_ptr(), params=params, sync=True)
    assert d_info.cpu().numpy().tobytes() == info.tobytes() and d_info2.cpu().numpy().tobytes() == info.tobytes()
    assert d_obs.cpu().numpy().tobytes() == out.tobytes()
    t = eng.quality_last_ms()
    print("kernel ms (quality_acc, quality_out): %s" % (t,))
    assert len(t) == 2 and all(x > 0 for x in t)
    with pytest.raises(TypeError):
        eng.quality(rec, ne, chans, tags, first, step, n_fix, obs=obs[:5])
    lib, h, p = eng._lib, eng._h, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpsacq_quality_observables(h, p(rec), max_epochs, p(ne), p(chans), p(tags), 12, first, step, n_fix, None, None, None) == 1   # no info
    assert lib.gpsacq_quality_observables(h, p(rec), max_epochs, p(ne), p(chans), None, 12, first, step, n_fix, None, None, p(info2)) == 1  # no tags
    assert lib.gpsacq_quality_observables_device(h, d_rec.data_ptr(), max_epochs, p(ne), p(chans), p(tags), 13, first, step, n_fix, None, None, d_info.data_ptr(), 1) == 1
    assert lib.gpsacq_quality_last_ms(None, None, None) == 1


# ---- 3. the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True], ids=["raw", "smoothed"])
def test_chain_equals_its_steps(eng, smooth):
    import gpsacq
    import torch
    rec, ne, chans, tags, nom = fabricated()
    ephs = to_records(geometry("north")["ephs"])
    first, step, n_fix = int(rec["sample"][0, 0]) + 3000, 5456 + 1, 500
    max_epochs = rec.shape[1]
    qp = gpsacq.quality_params(epochs=100)
    sp = gpsacq.smooth_params(window=100) if smooth else None
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    n_obs = n_fix * 12
    d_obs, d_info, d_fix = fill(n_obs * 32), fill(n_obs * 48), fill(n_fix * 80)
    s_obs, s_info, s_fix, d_fix2 = fill(n_obs * 32), fill(n_obs * 48), fill(n_fix * 80), fill(n_fix * 80)
    torch.cuda.synchronize()
    where = (d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix)
    eng.fix_quality_track_device(ephs, *where, d_fix.data_ptr(), d_obs_ptr=d_obs.data_ptr(), d_info_ptr=d_info.data_ptr(), quality_params=qp,
                                 smooth_params=sp, nom_words=nom, sync=False)
    eng.fix_quality_track_device(ephs, *where, d_fix2.data_ptr(), quality_params=qp, smooth_params=sp, nom_words=nom, sync=False)   # engine scratch
    if smooth:
        eng.smooth_observables_device(*where, s_obs.data_ptr(), params=sp, nom_words=nom, sync=False)
    else:
        eng.observables_device(*where, s_obs.data_ptr(), sync=False)
    eng.quality_device(*where, s_info.data_ptr(), d_obs_ptr=s_obs.data_ptr(), params=qp, sync=False)
    eng.fix_device(ephs, s_obs.data_ptr(), n_fix, 12, s_fix.data_ptr(), sync=True)
    obs = d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 12)
    assert obs.tobytes() == s_obs.cpu().numpy().tobytes() and d_info.cpu().numpy().tobytes() == s_info.cpu().numpy().tobytes()
    assert d_fix.cpu().numpy().tobytes() == s_fix.cpu().numpy().tobytes() and d_fix2.cpu().numpy().tobytes() == s_fix.cpu().numpy().tobytes()
    # and the steps are the host forms
    host = eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix, params=sp, nom_words=nom, info=False) if smooth else \
        eng.observables(rec, ne, chans, tags, first, step, n_fix)
    hout, hinfo = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=qp, obs=host)
    assert obs.tobytes() == hout.tobytes() and d_info.cpu().numpy().tobytes() == hinfo.tobytes()
    assert (obs["weight"][obs["valid"] != 0] == 0).any() and (obs["weight"] == 1).any()
    assert all(x > 0 for x in eng.quality_last_ms())
    lib, h, p = eng._lib, eng._h, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    if smooth:   # smoothing needs the nominal words, and its parameters are checked
        args = (p(ephs), 12, d_rec.data_ptr(), max_epochs, p(ne), p(chans), p(tags))
        rest = (12, first, step, n_fix)
        assert lib.gpsacq_fix_quality_track_device(h, *args, None, *rest, p(sp), p(qp), None, None, d_fix.data_ptr(), 1) == 1
        bad = gpsacq.smooth_params(window=0)
        assert lib.gpsacq_fix_quality_track_device(h, *args, p(np.asarray(nom, np.uint32)), *rest, p(bad), p(qp), None, None, d_fix.data_ptr(), 1) == 1
        assert lib.gpsacq_fix_quality_track_device(h, *args, p(np.asarray(nom, np.uint32)), *rest, p(sp), p(qp), None, None, None, 1) == 1
        eng.synchronize()
        assert d_fix.cpu().numpy().tobytes() == s_fix.cpu().numpy().tobytes()


def test_gated_channel_is_a_channel_left_out(eng):
    """eight satellites of the fix tests' geometry at their true transmit times, the one on channel 3 pushed 30 m off; its records
    hold the power in QP, so the estimate gates it to weight 0: the fixes are those of the same rows with that observation's valid = 0,
    to the tolerances of tests/test_gpu_fix.py, and not those of the rows at full weight"""
    import gpsacq
    from test_gpu_fix import POS_TOL, TIME_TOL, _rx_error, _times
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = to_records(geo["ephs"])
    n_fix = 20
    ms, frac = _times(n_fix)
    ref_ms = geo["ref_ms"] + ms
    obs = truth_obs(geo, ref_ms, frac)[:, sel].copy()
    obs["tx_frac"][:, 3] += 1e-7
    rec = np.zeros((8, 60), gpsacq.TRACK_RECORD_DTYPE)
    rec["sample"] = 5000 + 1000 * np.arange(60)
    rec["ip"], rec["qp"] = 2000 * (-1) ** np.arange(60), 37
    rec["ip"][3], rec["qp"][3] = 37, 2000
    chans = np.zeros(8, gpsacq.TRACK_CHAN_DTYPE)
    chans["next_sample"] = 65000
    tags = np.zeros(8, gpsacq.TIME_TAG_DTYPE)
    tags["valid"] = 1
    ne = np.full(8, 60, np.int32)
    weighted, info = eng.quality(rec, ne, chans, tags, 30000, 1500, n_fix, obs=obs)
    assert (info["epochs"] >= 20).all() and (weighted["weight"][:, 3] == 0).all() and (np.delete(weighted["weight"], 3, axis=1) == 1).all()
    assert ((info["flags"][:, 3] & qr.UNLOCKED) != 0).all()
    without = obs.copy()
    without["valid"][:, 3] = 0
    a, b, full = eng.fix(ephs, weighted), eng.fix(ephs, without), eng.fix(ephs, obs)
    assert (a["status"] == gpsacq.FIX_OK).all() and (b["status"] == gpsacq.FIX_OK).all()
    xyz = lambda f: np.stack([f["x"], f["y"], f["z"]], 1)
    dpos, dt = np.abs(xyz(a) - xyz(b)).max(), np.abs(_rx_error(a, ref_ms, frac) - _rx_error(b, ref_ms, frac)).max()
    moved = np.linalg.norm(xyz(full) - xyz(b), axis=1).min()
    print("gated against left out: position %.3g m, receive time %.3g s; at full weight the fix lies %.2f m away" % (dpos, dt, moved))
    assert dpos <= POS_TOL and dt <= TIME_TOL and moved > 1.0
    assert np.abs(xyz(b) - geo["rx"]).max() <= POS_TOL


# ---- 4. physical: two satellites 10 dB apart and a channel on noise --------------------------------------------------------------
def test_two_satellites_ten_db_apart_and_one_absent():
    """quality_ref.physical_case on the GPU: the channels' records give the reference's info, and the assertions of
    quality_ref.physical_check hold with the constants measured on the CPU model's records (tests/test_quality.py), where the seed
    was also checked to keep the absent PRN below the gate"""
    import gpsacq
    buf, p, chans = qr.physical_case()
    with gpsacq.Engine(0.5115e6, qr.PHYS_FS, 5000.0) as eng:
        inp = eng.iq8_input(signed=True, remove_dc=False, fs=qr.PHYS_FS, multibit=1)
        _, rec, ne = eng.track_iq8(buf, inp, chans, first_sample=0, max_epochs=1600, records=True, params=p)
        tags = np.zeros(3, gpsacq.TIME_TAG_DTYPE)
        tags["valid"] = 1
        params = gpsacq.quality_params(epochs=qr.PHYS_WINDOW)
        first, step, n_fix = qr.physical_instants(chans)
        info = eng.quality(rec, ne, chans, tags, first, step, n_fix, params=params)
        # the noise-only channel with every epoch as a window's last: one instant on each record's first sample is not an
        # arithmetic sequence, so instants half a nominal period apart, of which every epoch holds at least one
        n2 = int(ne[2])
        start, half = int(rec["sample"][2, 0]), 1023
        m = (int(chans["next_sample"][2]) - 1 - start) // half + 1
        dense = eng.quality(rec[2:3], ne[2:3], chans[2:3], tags[2:3], start, half, m, params=params)[:, 0]
    _compare(info, qr.quality(rec, ne, chans, tags, first, step, n_fix, params), "physical capture")
    assert (chans["status"][:2] == gpsacq.TRACK_OK).all()
    t = np.searchsorted(rec["sample"][2, :n2], start + half * np.arange(m), side="right") - 1
    _, pick = np.unique(t, return_index=True)
    assert len(pick) == n2
    every = dense[pick]
    ref_every = np.zeros(n2, gpsacq.QUALITY_INFO_DTYPE)
    for k, r in enumerate(qr.channel_series(rec["ip"][2, :n2], rec["qp"][2, :n2], qr.par(params))):
        for name, v in r.items():
            ref_every[name][k] = v
    _compare(every[:, None], ref_every[:, None], "noise-only channel at every epoch")
    qr.physical_check(info, every, int(chans["status"][2]), n2, gpsacq.TRACK_LOST)


# ---- 5. the front end ---------------------------------------------------------------------------------------------------------
def test_gps_track_prints_cn0_lines(tmp_path):
    """gps_track on a 3-s capture of three satellites: with GPSACQ_QUALITY=1 one cn0 line per whole second with every channel's PRN,
    dB-Hz and flags; every other line is what the same binary prints without the variable (tests/test_host.py holds no expectation
    of gps_track's output; the lines both runs share are those tests/test_gpu_track.py::test_gps_track_cli reads)"""
    import gpsacq
    fs, fc = 5.456e6, 4.092e6
    sats = [(4, 0.18, 1500.0, 700.0, 0.0), (11, 0.16, -2000.0, 2500.0, 0.3), (26, 0.2, 300.0, 4100.0, 0.6)]
    with gpsacq.Engine(fc, fs, 5000.0) as e:
        buf = e.generate(int(3.2 * fs) // 8, sats, seed=2)
    path = tmp_path / "cap.bin"
    buf.tofile(path)
    exe = os.path.join(ROOT, "gnss-gps-sdr_amd", "bin", "gps_track")
    env = {k: v for k, v in os.environ.items() if k not in ("GPSACQ_QUALITY", "GPSACQ_SMOOTH_MS", "GPSACQ_VELOCITY", "GPSACQ_INPUT")}
    plain = subprocess.run([exe, str(path), str(fc), str(fs)], capture_output=True, text=True, timeout=60, env=env)
    zero = subprocess.run([exe, str(path), str(fc), str(fs)], capture_output=True, text=True, timeout=60, env=dict(env, GPSACQ_QUALITY="0"))
    qual = subprocess.run([exe, str(path), str(fc), str(fs)], capture_output=True, text=True, timeout=60, env=dict(env, GPSACQ_QUALITY="1"))
    assert plain.returncode == 0 and qual.returncode == 0 and zero.returncode == 0, plain.stderr + qual.stderr
    assert "cn0 " not in plain.stdout and zero.stdout == plain.stdout
    assert [l for l in qual.stdout.splitlines() if not l.startswith("cn0 ")] == plain.stdout.splitlines()
    chan_prns = [int(l.split()[3]) for l in plain.stdout.splitlines() if l.startswith("chan ")]
    assert {4, 11, 26} <= set(chan_prns), plain.stdout
    lines = [l.split() for l in qual.stdout.splitlines() if l.startswith("cn0 ")]
    print("\n".join(" ".join(l) for l in lines))
    assert [int(l[2]) for l in lines] == [1, 2, 3]
    for l in lines:
        assert l[3::6] == ["PRN"] * len(l[3::6]) and l[5::6] == ["dbhz"] * len(l[5::6]) and l[7::6] == ["flags"] * len(l[7::6])
        got = {int(prn): (float(db), int(fl)) for prn, db, fl in zip(l[4::6], l[6::6], l[8::6])}
        assert {4, 11, 26} <= set(got) <= set(chan_prns)
        if int(l[2]) >= 2:   # past the pull-in.  Amplitude 0.16 .. 0.2 of the noise is 42 .. 44 dB-Hz before the limiter: far above the floor
            for prn in (4, 11, 26):
                assert 35.0 < got[prn][0] < 60.0 and got[prn][1] == qr.FULL, (prn, got[prn])
