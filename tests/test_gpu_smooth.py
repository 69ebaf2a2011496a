"""Carrier-smoothed observables on the GPU (gpsacq_smooth_observables*, gpsacq_fix_smooth_track_device; csrc/smooth_kernels.hip)
against tests/smooth_ref.py, the model of include/gpsacq.h in Python integers: obs and info byte for byte.

1. fabricated records over spm x n_chans x n_fix x window x step, with per-epoch noise on ca_rate, a planted code slip, an unlocked
   stretch, a channel without epochs, an invalid tag, instants before record 0 and past next_sample, both spectrum senses,
   lock_epochs = 0 and jump = 0; the device forms; argument errors;
2. the 20-s five-satellite capture of tests/test_gpu_velocity.py (its recipe restated here): instants 1 ms apart from second 2 to
   the end of the records, window 1000; the chain to fixes; gps_track with GPSACQ_SMOOTH_MS.

The figures themselves are printed before the assertions (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nav_ref
import obs_ref
import rate_ref
import smooth_ref
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu
N_EPOCHS = 600


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_cases = {}


def case(spm, n_chans):
    """smooth_ref.fabricate_case, made once per (spm, n_chans) and never written to, with the reference's cache for it"""
    key = (spm, n_chans)
    if key not in _cases:
        arrays = smooth_ref.fabricate_case(spm + n_chans, spm, n_chans, N_EPOCHS)
        for a in arrays:
            a.setflags(write=False)
        _cases[key] = (arrays, {})
    return _cases[key]


def _compare(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if got.tobytes() == ref.tobytes():
        return
    size = got.dtype.itemsize
    bad = np.argwhere((got.view(np.uint8).reshape(got.shape + (size,)) != ref.view(np.uint8).reshape(ref.shape + (size,))).any(axis=-1))
    i, c = bad[0]
    raise AssertionError("%s: %d records differ, first at [%d][%d]: %r != %r" % (what, len(bad), i, c, got[i, c], ref[i, c]))


def _options(k):
    """the parameter sets the fabricated cases rotate through: both spectrum senses, lock_epochs = 0, jump = 0"""
    return dict(invert=k % 2, lock_epochs=0 if k % 3 == 2 else 20, jump=0 if k % 4 == 3 else smooth_ref.DEFAULTS["jump"])


def _first(rec, spm, step):
    """with step 1 the instants straddle the boundary between epochs 299 and 300 of channel 0; otherwise the first three instants lie
    before record 0 of every channel"""
    return int(rec["sample"][0, 300]) - 500 if step == 1 else int(rec["sample"][0, 0]) - 3 * step


@pytest.mark.parametrize("step", ["1", "spm", "7spm+3"])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("n_chans", [1, 4, 12])
@pytest.mark.parametrize("spm", [2800, 5456])
def test_fabricated_records_byte_for_byte(eng, spm, n_chans, n_fix, step):
    import gpsacq
    (rec, ne, chans, tags, nom), cache = case(spm, n_chans)
    rx_step = {"1": 1, "spm": spm, "7spm+3": 7 * spm + 3}[step]
    first = _first(rec, spm, rx_step)
    opt = _options([1, 63, 64, 65, 257, 1025].index(n_fix) + (0 if step == "1" else 1 if step == "spm" else 2))
    for window in (1, 2, 64, n_fix + 7):
        params = gpsacq.smooth_params(window=window, **opt)
        obs, info = eng.smooth_observables(rec, ne, chans, tags, first, rx_step, n_fix, params=params, nom_words=nom)
        robs, rinfo = smooth_ref.smooth_observables(rec, ne, chans, tags, nom, first, rx_step, n_fix, params, cache=cache)
        what = "spm %d n_chans %d n_fix %d step %s window %d %s" % (spm, n_chans, n_fix, step, window, opt)
        _compare(obs, robs, what + " obs")
        _compare(info, rinfo, what + " info")
        raw = eng.observables(rec, ne, chans, tags, first, rx_step, n_fix)
        assert (raw["valid"] == obs["valid"]).all()
        unl = (info["flags"] & gpsacq.SMOOTH_UNLOCKED) != 0
        assert obs[unl].tobytes() == raw[unl].tobytes() and not info["window"][unl].any()
        assert obs[obs["valid"] == 0].tobytes() == bytes(32 * int((obs["valid"] == 0).sum()))
        assert info[obs["valid"] == 0].tobytes() == bytes(24 * int((obs["valid"] == 0).sum()))
        if window == 1:  # a window of one instant is the raw observation
            assert obs.tobytes() == raw.tobytes() and not info["corr"].any()
        if n_chans >= 4:
            assert not obs["valid"][:, 1].any() and not obs["valid"][:, n_chans - 1].any()  # no epochs; an invalid tag
    flags = info["flags"]
    if step == "spm" and n_fix == 1025:
        assert not obs["valid"][:3].any() and not obs["valid"][-300:].any()  # before record 0, past next_sample
        assert info["corr"][:, 0].any() and (info["corr"][:, 0] < 0).any() and (info["corr"][:, 0] > 0).any()
        if opt["lock_epochs"]:  # pull-in (t < 19) and the stretch with the power in QP
            assert ((flags[:, 0] & gpsacq.SMOOTH_UNLOCKED) != 0).sum() >= 60
            assert ((flags[:, 0] & gpsacq.SMOOTH_RESET) != 0).sum() >= (3 if opt["jump"] else 2)
        else:
            assert not (flags & gpsacq.SMOOTH_UNLOCKED).any()
            assert ((flags[:, 0] & gpsacq.SMOOTH_RESET) != 0).sum() == (2 if opt["jump"] else 1)


def test_correction_carries_the_position_over_the_epoch_boundary(eng):
    """instants a code period apart that start on an epoch's first sample, and a code rate noisy enough to move the epochs' ends
    by a sample: P is just past 0 or just short of 1023 chips, and the correction carries P~ over the boundary both ways -- tx_ms one
    more and one less than the raw observation's, also across the end of the week"""
    import gpsacq
    spm, n = 5456, 400
    rec, ch, nom = smooth_ref.fabricate_coherent(77, n, spm, noise=100000, first_sample=30 * spm, epoch0=500)
    ne = np.array([n], np.int32)
    first, n_fix = int(rec["sample"][200]), 150
    params = gpsacq.smooth_params(window=50, lock_epochs=0, jump=0)
    for ms in (1000, obs_ref.WEEK_MS - 60):
        tags = np.zeros(1, gpsacq.TIME_TAG_DTYPE)
        tags[0] = (700, ms, 0, 1)
        obs, info = eng.smooth_observables(rec[None], ne, ch, tags, first, spm, n_fix, params=params, nom_words=[nom])
        robs, rinfo = smooth_ref.smooth_observables(rec[None], ne, ch, tags, [nom], first, spm, n_fix, params)
        _compare(obs, robs, "epoch boundary obs")
        _compare(info, rinfo, "epoch boundary info")
        raw = eng.observables(rec[None], ne, ch, tags, first, spm, n_fix)
        moved = (obs["tx_ms"].astype(np.int64) - raw["tx_ms"] + obs_ref.WEEK_MS // 2) % obs_ref.WEEK_MS - obs_ref.WEEK_MS // 2
        print("tag ms %d: tx_ms one more than raw at %d instants, one less at %d" % (ms, (moved == 1).sum(), (moved == -1).sum()))
        assert set(np.unique(moved)) == {-1, 0, 1} and obs["valid"].all()
    assert (np.diff(obs["tx_ms"][:, 0].astype(np.int64)) < 0).any()  # the week did end inside the batch


def test_device_forms_equal_host_form(eng):
    import gpsacq
    import torch
    (rec, ne, chans, tags, nom), cache = case(5456, 12)
    ephs = to_records(geometry("north")["ephs"])
    first, step, n_fix = int(rec["sample"][0, 0]) + 3000, 5456 + 1, 700
    params = gpsacq.smooth_params(window=100)
    host, hinfo = eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix, params=params, nom_words=nom)
    assert host["valid"].sum() > 3000 and ((hinfo["flags"] & gpsacq.SMOOTH_FULL) != 0).sum() > 2000
    assert eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix, params=params, nom_words=nom, info=False).tobytes() == host.tobytes()
    # the default nominal words are the 1-bit rule, the default parameters those of smooth_params()
    a = eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix)
    b = eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix, params=gpsacq.smooth_params(), nom_words=rate_ref.nominal_words(chans))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    max_epochs = rec.shape[1]
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs, d_obs2, d_obs3 = fill(host.size * 32), fill(host.size * 32), fill(host.size * 32)
    d_info, d_info2 = fill(host.size * 24), fill(host.size * 24)
    d_fix, d_fix2 = fill(n_fix * gpsacq.FIX_DTYPE.itemsize), fill(n_fix * gpsacq.FIX_DTYPE.itemsize)
    torch.cuda.synchronize()
    kw = dict(params=params, nom_words=nom)
    eng.smooth_observables_device(d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_obs.data_ptr(), d_info.data_ptr(), sync=False, **kw)
    eng.smooth_observables_device(d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_obs2.data_ptr(), None, sync=False, **kw)
    eng.fix_smooth_track_device(ephs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_fix.data_ptr(), d_obs_ptr=d_obs3.data_ptr(),
                                d_info_ptr=d_info2.data_ptr(), sync=False, **kw)
    eng.fix_smooth_track_device(ephs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, step, n_fix, d_fix2.data_ptr(), sync=True, **kw)
    for d in (d_obs, d_obs2, d_obs3):
        assert d.cpu().numpy().tobytes() == host.tobytes()
    for d in (d_info, d_info2):
        assert d.cpu().numpy().tobytes() == hinfo.tobytes()
    fix = eng.fix(ephs, host)
    assert d_fix.cpu().numpy().tobytes() == fix.tobytes() and d_fix2.cpu().numpy().tobytes() == fix.tobytes()
    t = eng.smooth_last_ms()
    assert len(t) == 4 and all(x > 0 for x in t)
    eng.smooth_observables(rec, ne, chans, tags, first, step, n_fix, params=gpsacq.smooth_params(lock_epochs=0), nom_words=nom)
    t = eng.smooth_last_ms()
    assert t[0] < 0.05 and all(x > 0 for x in t[1:])  # k_lock_acc did not run
    assert eng.observables_last_ms()[0] > 0 and eng.velocity_last_ms()[0] > 0  # k_code_pos and k_carrier_acc keep their getters


def test_argument_errors_leave_the_output_untouched(eng):
    import gpsacq
    import torch
    (rec, ne, chans, tags, nom), _ = case(2800, 12)
    max_epochs = rec.shape[1]
    ephs = to_records(geometry("north")["ephs"])
    lib, h = eng._lib, eng._h
    out, inf = np.full(8 * 12 * 32, 0xA5, np.uint8), np.full(8 * 12 * 24, 0xA5, np.uint8)
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs, d_info, d_fix = fill(8 * 12 * 32), fill(8 * 12 * 24), fill(8 * 80)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    good = gpsacq.smooth_params()
    ok = dict(rec=_p(rec), mx=max_epochs, ne=_p(ne), ch=_p(chans), tg=_p(tags), nw=_p(nom), nc=12, first=1000, step=2800, n_fix=8, pr=_p(good))
    too_many, negative = np.array(ne), np.array(ne)
    too_many[4], negative[2] = max_epochs + 1, -1
    prs = [gpsacq.smooth_params(**o) for o in (dict(window=0), dict(window=65537), dict(lock_epochs=-1), dict(lock_epochs=1025), dict(lock_num=0),
                                               dict(lock_num=3, lock_den=2), dict(lock_num=1, lock_den=1025), dict(jump=-1))]
    for pr in prs:
        assert not smooth_ref.params_valid(smooth_ref.par(pr))
    bad = [dict(rec=None), dict(ne=None), dict(ch=None), dict(tg=None), dict(nw=None), dict(nc=0), dict(nc=13), dict(nc=-1), dict(step=0),
           dict(n_fix=0), dict(ne=_p(too_many)), dict(ne=_p(negative)), dict(mx=max_epochs - 100), dict(first=(1 << 64) - 5, step=1)]
    bad += [dict(pr=_p(pr)) for pr in prs]
    for change in bad:
        a = dict(ok, **change)
        args = (a["mx"], a["ne"], a["ch"], a["tg"], a["nw"], a["nc"], a["first"], a["step"], a["n_fix"], a["pr"])
        assert lib.gpsacq_smooth_observables(h, a["rec"], *args, _p(out), _p(inf)) == 1, change
        d = None if a["rec"] is None else d_rec.data_ptr()
        assert lib.gpsacq_smooth_observables_device(h, d, *args, d_obs.data_ptr(), d_info.data_ptr(), 1) == 1, change
        assert lib.gpsacq_fix_smooth_track_device(h, _p(ephs), 12, d, *args, d_obs.data_ptr(), d_info.data_ptr(), d_fix.data_ptr(), 1) == 1, change
    args = (ok["mx"], ok["ne"], ok["ch"], ok["tg"], ok["nw"], ok["nc"], ok["first"], ok["step"], ok["n_fix"], ok["pr"])
    assert lib.gpsacq_smooth_observables(h, ok["rec"], *args, None, _p(inf)) == 1
    assert lib.gpsacq_smooth_observables_device(h, d_rec.data_ptr(), *args, None, d_info.data_ptr(), 1) == 1
    trk = lambda eph, n_eph, fx: lib.gpsacq_fix_smooth_track_device(h, eph, n_eph, d_rec.data_ptr(), *args, d_obs.data_ptr(), d_info.data_ptr(), fx, 1)
    assert trk(None, 12, d_fix.data_ptr()) == 1 and trk(_p(ephs), 0, d_fix.data_ptr()) == 1 and trk(_p(ephs), 12, None) == 1
    assert lib.gpsacq_smooth_default_params(None) == 1
    eng.synchronize()
    assert (out == 0xA5).all() and (inf == 0xA5).all()
    for d in (d_obs, d_info, d_fix):
        assert (d.cpu().numpy() == 0xA5).all()
    with pytest.raises(gpsacq.GpsAcqError) as ei:
        eng.smooth_observables(rec, ne, chans, tags, 1000, 2800, 8, params=prs[0], nom_words=nom)
    assert ei.value.code == 1 and "window" in str(ei.value)
    with pytest.raises(ValueError):
        eng.smooth_observables(rec, ne[:5], chans, tags, 1000, 1, 8)
    # and the same arguments, unbroken, work; params NULL is the defaults
    assert lib.gpsacq_smooth_observables(h, ok["rec"], *args, _p(out), _p(inf)) == 0 and not (out == 0xA5).all()
    out2 = np.full(8 * 12 * 32, 0xA5, np.uint8)
    assert lib.gpsacq_smooth_observables(h, ok["rec"], *args[:-1], None, _p(out2), None) == 0 and out2.tobytes() == out.tobytes()


# ---- 2. the whole chain --------------------------------------------------------------------------------------------------------
FS, FC, SPM = 5.456e6, 4.092e6, 5456
N_BYTES = int(20 * FS) // 8
R_STAR = int(19.5 * FS)
TOW0 = 64898
BIT0_MS = (TOW0 - 1) * 6000
REF_MS, REF_FRAC = BIT0_MS + 18_275, 0.3217e-3   # the receive time at R*


@pytest.fixture(scope="module")
def chain(eng):
    """tests/test_gpu_velocity.py's 20-s scenario by its recipe (stationary receiver, five satellites at amplitudes 0.15 .. 0.2,
    Dopplers consistent with the geometry at R*), built here once: capture, channels, decode; then the smoothed chain at instants
    1 ms apart from second 2 to the end of the records, and the raw one at the same instants."""
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
    tags, recs = [], []
    for c, prn in enumerate(prns):
        n = int(ne[c])
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=int(chans["epoch"][c]) - n + 1000)
        sf, _ = gpsacq.nav_subframes(bits)
        assert len(sf) >= 3, (prn, len(bits), len(sf))
        recs.append(gpsacq.ephemeris(sf, prn))
        tags.append(gpsacq.time_tag(sf[0], e0, c))
    tags, recs = np.concatenate(tags), np.concatenate(recs)
    first = 2 * int(FS)
    n_fix = (int(chans["next_sample"].min()) - 1 - first) // SPM + 1
    fill = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    d_fix, d_obs, d_info, d_raw, d_rawfix = fill(n_fix * 80), fill(n_fix * 5 * 32), fill(n_fix * 5 * 24), fill(n_fix * 5 * 32), fill(n_fix * 80)
    torch.cuda.synchronize()
    eng.fix_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_rawfix.data_ptr(), d_obs_ptr=d_raw.data_ptr())
    eng.fix_smooth_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_fix.data_ptr(), d_obs_ptr=d_obs.data_ptr(),
                                d_info_ptr=d_info.data_ptr())
    out = dict(geo=geo, ephs=recs, chans=chans, ne=ne, tags=tags, n_fix=n_fix, first=first,
               records=d_rec.cpu().numpy().view(gpsacq.TRACK_RECORD_DTYPE).reshape(5, max_epochs),
               obs=d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 5), info=d_info.cpu().numpy().view(gpsacq.SMOOTH_INFO_DTYPE).reshape(n_fix, 5),
               raw=d_raw.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 5), fix=d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE),
               rawfix=d_rawfix.cpu().numpy().view(gpsacq.FIX_DTYPE), capture=d_bits.cpu().numpy(),
               kernel_ms=eng.observables_last_ms()[:1] + eng.velocity_last_ms()[:1] + eng.smooth_last_ms())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_chain_equals_the_reference(eng, chain):
    """obs and info of the 20-s capture's records, 1 ms apart from second 2, against the reference; the fixes of the chain are
    Engine.fix on its observations"""
    import gpsacq
    assert (chain["chans"]["status"] == gpsacq.TRACK_OK).all() and chain["n_fix"] > 17000
    nom = rate_ref.nominal_words(chain["chans"])
    robs, rinfo = smooth_ref.smooth_observables(chain["records"], chain["ne"], chain["chans"], chain["tags"], nom, chain["first"], SPM, chain["n_fix"])
    _compare(chain["obs"], robs, "whole chain obs")
    _compare(chain["info"], rinfo, "whole chain info")
    assert chain["fix"].tobytes() == eng.fix(chain["ephs"], np.array(chain["obs"])).tobytes()
    assert chain["raw"].tobytes() == obs_ref.observables(chain["records"], chain["ne"], chain["chans"], chain["tags"], chain["first"], SPM, chain["n_fix"]).tobytes()
    flags = chain["info"]["flags"]
    assert not (flags & gpsacq.SMOOTH_UNLOCKED).any()  # from second 2 on every channel is in phase lock at the defaults
    assert (flags[0] == gpsacq.SMOOTH_RESET).all() and ((flags[999:] & gpsacq.SMOOTH_FULL) != 0).all()
    print("kernel ms (code_pos, carrier_acc, lock_acc, cmc, smooth_scan, smooth_out): %s" % (chain["kernel_ms"],))


def test_chain_position_scatter(chain):
    """A sign check like the CPU chain's, on positions: over the instants whose five windows are full, the fixes from smoothed
    observations scatter less about their mean than the raw ones.  With the carrier's sign or the factor 1540 wrong they scatter
    many times more.  Nothing here is a precision claim: the mean is not looked at.  Measured on an MI355X by this test: code_sigma_m
    1.763 / 1.907 / 1.758 / 1.847 / 1.833 m; over the 17 001 FULL instants scatter raw 5.403 m, smoothed 4.224 m (both carry the metres
    by which the generator's constant Dopplers leave the truth over 17 s), error of the mean 2.732 / 2.709 m."""
    import gpsacq
    full = ((chain["info"]["flags"] & gpsacq.SMOOTH_FULL) != 0).all(axis=1)
    ok = full & (chain["fix"]["status"] == gpsacq.FIX_OK) & (chain["rawfix"]["status"] == gpsacq.FIX_OK)
    assert ok.sum() > 16000

    def scatter(fix):
        xyz = np.stack([fix["x"][ok], fix["y"][ok], fix["z"][ok]], axis=1)
        return float(np.sqrt(((xyz - xyz.mean(axis=0)) ** 2).sum(axis=1).mean())), float(np.linalg.norm(xyz.mean(axis=0) - chain["geo"]["rx"]))

    (s_raw, e_raw), (s_sm, e_sm) = scatter(chain["rawfix"]), scatter(chain["fix"])
    sigma = gpsacq.code_sigma_m(np.array(chain["info"]))
    print("code_sigma_m per channel: %s m" % ["%.3f" % s for s in sigma])
    print("position over the %d FULL instants: scatter raw %.3f m, smoothed %.3f m; mean position error raw %.3f m, smoothed %.3f m"
          % (ok.sum(), s_raw, s_sm, e_raw, e_sm))
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    assert s_sm < s_raw


def test_gps_track_prints_smoothed_fixes(chain, tmp_path):
    """the front end on the same capture: without GPSACQ_SMOOTH_MS nothing changes; with it the same once-a-second fix lines in the
    same format, made from smoothed observations, and a sigma line per channel"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "cap.bin"
    chain["capture"].tofile(path)
    exe = os.path.join(root, "gnss-gps-sdr_amd", "bin", "gps_track")
    env = {k: v for k, v in os.environ.items() if k not in ("GPSACQ_SMOOTH_MS", "GPSACQ_VELOCITY")}
    plain = subprocess.run([exe, str(path), str(FC), str(FS)], capture_output=True, text=True, timeout=120, env=env)
    smooth = subprocess.run([exe, str(path), str(FC), str(FS)], capture_output=True, text=True, timeout=120, env=dict(env, GPSACQ_SMOOTH_MS="1000"))
    assert plain.returncode == 0 and smooth.returncode == 0, plain.stderr + smooth.stderr
    assert "sigma " not in plain.stdout
    keep = lambda text, drop: [l for l in text.splitlines() if not l.startswith(drop)]
    assert keep(smooth.stdout, ("fix ", "sigma ")) == keep(plain.stdout, ("fix ",))
    fixes_p = [l.split() for l in plain.stdout.splitlines() if l.startswith("fix ")]
    fixes_s = [l.split() for l in smooth.stdout.splitlines() if l.startswith("fix ")]
    sig = [l.split() for l in smooth.stdout.splitlines() if l.startswith("sigma ")]
    assert len(fixes_p) >= 18 and len(fixes_s) == len(fixes_p) and len(sig) == 5, smooth.stdout
    assert [f[1::2] for f in fixes_s] == [f[1::2] for f in fixes_p]  # the same fields
    assert fixes_s != fixes_p                                      # other numbers: the observations were smoothed
    for a, b in zip(fixes_p, fixes_s):                             # the same instants to within the code's noise
        assert abs(float(a[2]) - float(b[2])) < 1e-6, (a, b)
    for s in sig:
        d = dict(zip(s[1::2], s[2::2]))
        assert 0.1 < float(d["code_sigma_m"]) < 30.0 and int(d["full"]) > 10000, s
    print("gps_track sigma lines: %s" % [" ".join(s) for s in sig])
