"""Observables on the GPU (gpsacq_observables*, gpsacq_fix_track_device; csrc/obs_kernels.hip) against tests/obs_ref.py, the
model of include/gpsacq.h in Python integers.

1. fabricated records, byte for byte (tx_frac included: one IEEE division on both sides);
2. the device forms against the host form, fix_track_device against fix(observables()), argument errors;
3. the whole chain on a generated 20-s capture: search -> track -> NAV bits -> subframes -> ephemeris -> time tag ->
   fix_track_device, and the gps_track front end on the same capture.

The two physical assertions of 3 separate a locked, correctly counted chain from a broken one and are not precision claims: a
wrong millisecond is 300 km; half a chip (489 ns) on every satellite at the 5-satellite subset's PDOP of 2.19 is 321 m, hence
500 m.  The figures themselves are printed before the assertions (pytest -s).

The issue's 1001 instants end at R* + 500 spm = the capture's last sample + 1, where no channel has a record any more: the rows
past every channel's last whole epoch hold zero observations and come back GPSACQ_FIX_TOO_FEW; they are compared like the rest
and the physical figures are taken over the complete rows.

Figures of the same scenario run on the CPU (a numpy restatement of the generator's law, the C channel model started block by
block, obs_ref, nav_ref's solver): worst observation error at R* 5.3 ns, position error 2.5 m at R*, at most 5.2 m (mean 2.9 m)
over the 1000 complete instants; once a second as gps_track does, 16 m at second 1.  The device's own are printed with -s."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import nav_ref
import obs_ref
from nav_helpers import assert_fields_exact, geometry, to_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = 1575.42e6
POS_TOL, TIME_TOL = 1e-4, 1e-12  # tests/test_gpu_fix.py's derivation
MAX_EPOCHS = 1024
COUNTS = [1000, 0, 65, 129, 1, 63, 64, 1000, 129, 65, 64, 63]


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
    """12 fabricated channels at spm samples per millisecond, made once and never written to: records [12][1024] (the rows past
    each count filled with 0xFF bytes, which no kernel may read), n_epochs, chans, tags."""
    import gpsacq
    if spm in _pools:
        return _pools[spm]
    rec = np.full((12, MAX_EPOCHS), 0xFF, np.uint8).repeat(40, axis=1).view(gpsacq.TRACK_RECORD_DTYPE)
    assert rec.shape == (12, MAX_EPOCHS)
    chans = np.zeros(12, gpsacq.TRACK_CHAN_DTYPE)
    tags = np.zeros(12, gpsacq.TIME_TAG_DTYPE)
    rng = np.random.default_rng(spm)
    for c, n in enumerate(COUNTS):
        r, ch, _ = obs_ref.fabricate(100 * spm + c, n, spm, prn=c + 1)
        rec[c, :n] = r
        chans[c] = ch[0]
        tags[c] = (int(rng.integers(0, 6000)), int(rng.integers(0, obs_ref.WEEK_MS)), c, 1)
    first_epoch = chans["epoch"] - np.array(COUNTS)
    tags[0] = (int(first_epoch[0]) + 5, 604_799_990, 0, 1)          # tx_ms wraps the week inside the first 20 epochs
    tags[2] = (int(chans["epoch"][2]) + 1000, 123_456, 2, 1)        # tagged later than every observed epoch: negative difference
    tags[3]["valid"] = 0
    tags[7] = (int(first_epoch[7]) + 500, 3, 7, 1)                  # negative difference across the start of the week
    ne = np.array(COUNTS, np.int32)
    for a in (rec, chans, tags, ne):
        a.setflags(write=False)
    _pools[spm] = (rec, ne, chans, tags)
    return _pools[spm]


def _take(spm, cols):
    rec, ne, chans, tags = pool(spm)
    return rec[cols].copy(), ne[cols].copy(), chans[cols].copy(), tags[cols].copy()


def _compare(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if got.tobytes() == ref.tobytes():
        return
    bad = np.argwhere(got.view(np.uint8).reshape(got.shape + (32,)) != ref.view(np.uint8).reshape(ref.shape + (32,)))
    i, c = bad[0][:2]
    raise AssertionError("%s: %d observations differ, first at [%d][%d]: %r != %r" % (what, len({(a, b) for a, b, _ in bad}), i, c, got[i, c], ref[i, c]))


@pytest.mark.parametrize("step", ["1", "spm", "7spm+3"])
@pytest.mark.parametrize("n_fix", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_chans", [1, 4, 12])
@pytest.mark.parametrize("spm", [2800, 5456])
def test_fabricated_records_byte_for_byte(eng, spm, n_chans, n_fix, step):
    rx_step = {"1": 1, "spm": spm, "7spm+3": 7 * spm + 3}[step]
    cols = list(range(n_chans)) if n_chans > 1 else [(n_fix + rx_step) % 12]
    rec, ne, chans, tags = _take(spm, cols)
    starts = [int(rec["sample"][c, 0]) for c in range(len(cols)) if ne[c] > 0]
    first = max(0, (min(starts) if starts else 1000) - 3)  # the first instants lie before some channel's record 0
    got = eng.observables(rec, ne, chans, tags, first, rx_step, n_fix)
    ref = obs_ref.observables(rec, ne, chans, tags, first, rx_step, n_fix)
    _compare(got, ref, "spm %d n_chans %d n_fix %d step %s" % (spm, n_chans, n_fix, step))
    assert ((got["tx_frac"] >= 0) & (got["tx_frac"] < 1e-3)).all() and ((got["tx_ms"] >= 0) & (got["tx_ms"] < obs_ref.WEEK_MS)).all()
    if n_chans == 12 and n_fix == 257:
        assert not got["valid"][:, [1, 3]].any() and got[:, [1, 3]].tobytes() == bytes(32 * 2 * n_fix)  # no epochs; no valid tag
        if step == "7spm+3":  # 1800 epochs' worth of instants: past the end of every channel
            assert got["valid"][:100].any() and not got["valid"][150:].any()
        if step == "spm":  # the tag cases did what they are there for
            assert got["valid"][:, 0].sum() >= 240
            ms0 = got["tx_ms"][got["valid"][:, 0] == 1, 0]
            assert ms0.max() > 604_799_980 and ms0.min() < 20  # wrapped the week
            assert (got["tx_ms"][got["valid"][:, 7] == 1, 7] > 604_799_000).all()  # 3 ms - up to 500 epochs


@pytest.mark.parametrize("spm", [2800, 5456])
def test_edges_of_every_channel(eng, spm):
    """per channel: one sample before record 0, an epoch's first and last sample, next_sample - 1, next_sample (invalid)"""
    rec, ne, chans, tags = _take(spm, list(range(12)))
    for c in range(12):
        n = int(ne[c])
        if n == 0:
            continue
        s0, nxt = int(rec["sample"][c, 0]), int(chans["next_sample"][c])
        mid = int(rec["sample"][c, n // 2])
        for first, n_fix, want in ((s0 - 1, 3, [0, 1, 1]), (mid - 1, 2, [1 if n // 2 > 0 else 0, 1]), (nxt - 2, 4, [1, 1, 0, 0])):
            got = eng.observables(rec, ne, chans, tags, first, 1, n_fix)
            _compare(got, obs_ref.observables(rec, ne, chans, tags, first, 1, n_fix), "channel %d at %d" % (c, first))
            if tags["valid"][c]:
                assert list(got["valid"][:, c]) == want, (c, first)
        if tags["valid"][c] and n > 2:  # an epoch's last sample is the end of the code period, its first the start
            got = eng.observables(rec, ne, chans, tags, mid - 1, 1, 2)
            assert got["tx_frac"][0, c] > 0.999e-3 and got["tx_frac"][1, c] < 0.001e-3
            assert (int(got["tx_ms"][1, c]) - int(got["tx_ms"][0, c])) % obs_ref.WEEK_MS == 1


# ---- 2. device forms ---------------------------------------------------------------------------------------------------------
def test_device_forms_equal_host_form(eng):
    import gpsacq
    import torch
    rec, ne, chans, tags = _take(5456, list(range(12)))
    ephs = to_records(geometry("north")["ephs"])
    first, step, n_fix = int(rec["sample"][0, 0]) - 2, 3 * 5456 + 1, 130
    host = eng.observables(rec, ne, chans, tags, first, step, n_fix)
    host_fix = eng.fix(ephs, host)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_obs = torch.full((host.size * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs2 = torch.full((host.size * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_fix = torch.full((n_fix * gpsacq.FIX_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_fix2 = torch.full((n_fix * gpsacq.FIX_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.observables_device(d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, d_obs.data_ptr(), sync=False)
    eng.fix_track_device(ephs, d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, d_fix.data_ptr(), d_obs_ptr=d_obs2.data_ptr(),
                         sync=False)
    eng.fix_track_device(ephs, d_rec.data_ptr(), MAX_EPOCHS, ne, chans, tags, first, step, n_fix, d_fix2.data_ptr(), sync=True)  # scratch
    assert d_obs.cpu().numpy().tobytes() == host.tobytes()
    assert d_obs2.cpu().numpy().tobytes() == host.tobytes()
    assert d_fix.cpu().numpy().tobytes() == host_fix.tobytes()
    assert d_fix2.cpu().numpy().tobytes() == host_fix.tobytes()
    a, b = eng.observables_last_ms()
    assert a > 0 and b > 0
    assert (host_fix["n_used"] <= 10).all() and host_fix["n_used"].max() >= 4  # rows of fabricated times: they only have to be equal


def test_argument_errors_leave_the_output_untouched(eng):
    import gpsacq
    import torch
    rec, ne, chans, tags = _take(2800, list(range(12)))
    ephs = to_records(geometry("north")["ephs"])
    lib, h = eng._lib, eng._h
    out = np.full(8 * 12 * 32, 0xA5, np.uint8)
    d_out = torch.full((8 * 12 * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_fix = torch.full((8 * 80,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ok = dict(rec=_p(rec), mx=MAX_EPOCHS, ne=_p(ne), ch=_p(chans), tg=_p(tags), nc=12, first=1000, step=2800, n_fix=8)
    short = np.array(ne)
    short[4] = MAX_EPOCHS + 1
    negative = np.array(ne)
    negative[1] = -1
    bad = [dict(rec=None), dict(ne=None), dict(ch=None), dict(tg=None), dict(nc=0), dict(nc=13), dict(nc=-1), dict(step=0), dict(n_fix=0),
           dict(ne=_p(short)), dict(ne=_p(negative)), dict(mx=999), dict(first=(1 << 64) - 5, step=1)]
    for change in bad:
        a = dict(ok, **change)
        args = (a["mx"], a["ne"], a["ch"], a["tg"], a["nc"], a["first"], a["step"], a["n_fix"])
        assert lib.gpsacq_observables(h, a["rec"], *args, _p(out)) == 1, change
        d = None if a["rec"] is None else d_rec.data_ptr()
        assert lib.gpsacq_observables_device(h, d, *args, d_out.data_ptr(), 1) == 1, change
        assert lib.gpsacq_fix_track_device(h, _p(ephs), 12, d, *args, d_out.data_ptr(), d_fix.data_ptr(), 1) == 1, change
    args = (ok["mx"], ok["ne"], ok["ch"], ok["tg"], ok["nc"], ok["first"], ok["step"], ok["n_fix"])
    assert lib.gpsacq_observables(h, ok["rec"], *args, None) == 1
    assert lib.gpsacq_observables_device(h, d_rec.data_ptr(), *args, None, 1) == 1
    assert lib.gpsacq_fix_track_device(h, None, 12, d_rec.data_ptr(), *args, d_out.data_ptr(), d_fix.data_ptr(), 1) == 1
    assert lib.gpsacq_fix_track_device(h, _p(ephs), 0, d_rec.data_ptr(), *args, d_out.data_ptr(), d_fix.data_ptr(), 1) == 1
    assert lib.gpsacq_fix_track_device(h, _p(ephs), 12, d_rec.data_ptr(), *args, d_out.data_ptr(), None, 1) == 1
    eng.synchronize()
    assert (out == 0xA5).all() and (d_out.cpu().numpy() == 0xA5).all() and (d_fix.cpu().numpy() == 0xA5).all()
    with pytest.raises(gpsacq.GpsAcqError) as ei:
        eng.observables(rec, ne, chans, tags, 1000, 0, 8)
    assert ei.value.code == 1 and "rx_step" in str(ei.value)
    with pytest.raises(ValueError):
        eng.observables(rec, ne[:5], chans, tags, 1000, 1, 8)
    # and the same arguments, unbroken, work
    assert lib.gpsacq_observables(h, ok["rec"], *args, _p(out)) == 0 and not (out == 0xA5).all()


# ---- 3. the whole chain --------------------------------------------------------------------------------------------------------
FS, FC, SPM = 5.456e6, 4.092e6, 5456
N_BYTES = int(20 * FS) // 8
R_STAR = int(19.5 * FS)
TOW0 = 64898                       # bit 0 of every satellite's stream is satellite time (TOW0 - 1) * 6000 ms
BIT0_MS = (TOW0 - 1) * 6000
REF_MS, REF_FRAC = BIT0_MS + 18_275, 0.3217e-3   # the receive time at R*.  Bit 0 lies 1.3 s into the capture: a channel started
# from block b's hit begins b * 7.5 ms in (PRN 9: 60 ms) and bit sync skips its first 1000 epochs; a subframe 1 that starts inside them is lost


@pytest.fixture(scope="module")
def chain(eng):
    """the capture (device generator), the channels, the decode and the fixes, made once; nothing in it is written to later"""
    import gpsacq
    import torch
    geo = geometry("north")
    sel = geo["subsets"][5]
    ephs = [geo["ephs"][k] for k in sel]
    sats, nav, law = [], [], []
    amps = np.linspace(0.15, 0.2, len(sel))
    for j, eph in enumerate(ephs):
        t = nav_ref.truth_tx(eph, geo["rx"], REF_MS, np.array([REF_FRAC - 0.5, REF_FRAC, REF_FRAC + 0.5]))
        dop = L1 * ((t[2] - t[0]) - 1.0)
        tx_ms = (REF_MS - BIT0_MS) + t[1] * 1e3  # milliseconds after bit 0
        cp = tx_ms * FS / (1000.0 * (1.0 + dop / L1)) - R_STAR
        sats.append((int(eph["prn"]), float(amps[j]), float(dop), float(cp), 0.1 + 0.17 * j))
        nav.append(1 - 2 * nav_ref.encode_stream(eph, TOW0, ids=(1, 2, 3, 4, 5)).astype(np.int8))
        law.append((REF_MS, t[1]))
        assert abs(dop) < 6000 and -1.5 * FS < cp < -1.1 * FS
    nav = np.array(nav)
    assert nav.shape == (5, 1500)
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
        first_epoch = int(chans["epoch"][c]) - n
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=first_epoch + 1000)
        sf, _ = gpsacq.nav_subframes(bits)
        assert len(sf) >= 3, (prn, len(bits), len(sf))
        recs.append(gpsacq.ephemeris(sf, prn))
        tags.append(gpsacq.time_tag(sf[0], e0, c))
    tags, recs = np.concatenate(tags), np.concatenate(recs)
    n_fix, first = 1001, R_STAR - 500 * SPM
    d_fix = torch.zeros(n_fix * gpsacq.FIX_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_obs = torch.zeros(n_fix * 5 * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.fix_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_fix.data_ptr(), d_obs_ptr=d_obs.data_ptr())
    out = dict(geo=geo, ephs=ephs, sats=sats, law=law, chans=chans, ne=ne, tags=tags, recs=recs, n_fix=n_fix, first=first,
               records=d_rec.cpu().numpy().view(gpsacq.TRACK_RECORD_DTYPE).reshape(5, max_epochs),
               obs=d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE).reshape(n_fix, 5), fix=d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE),
               capture=d_bits.cpu().numpy(), kernel_ms=eng.observables_last_ms() + eng.fix_last_ms())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_chain_decodes_every_channel(chain):
    import gpsacq
    assert (chain["chans"]["status"] == gpsacq.TRACK_OK).all() and (chain["ne"] > 19900).all()
    for c, eph in enumerate(chain["ephs"]):
        assert gpsacq.ephemeris_valid(chain["recs"][c]), c
        assert_fields_exact(chain["recs"][c:c + 1], eph)
    tags = chain["tags"]
    assert (tags["valid"] == 1).all() and list(tags["eph"]) == [0, 1, 2, 3, 4]
    assert ((tags["ms"] - BIT0_MS) % 6000 == 0).all() and ((tags["ms"] - BIT0_MS) // 6000 <= 2).all() and (tags["ms"] >= BIT0_MS).all()


def test_chain_observations_equal_the_reference(chain):
    ref = obs_ref.observables(chain["records"], chain["ne"], chain["chans"], chain["tags"], chain["first"], SPM, chain["n_fix"])
    _compare(chain["obs"], ref, "whole chain")
    complete = chain["obs"]["valid"].all(axis=1)
    print("complete rows: %d of %d, kernel ms (code_pos, observe, sat_state, fix): %s" % (complete.sum(), complete.size, chain["kernel_ms"]))
    # only the instants past the last whole epoch of some channel are incomplete: at most the last three
    assert complete[:998].all()


def test_chain_fixes_equal_the_reference_solver(chain):
    import gpsacq
    obs, fix = chain["obs"], chain["fix"]
    complete = obs["valid"].all(axis=1)
    assert (fix["status"][complete] == gpsacq.FIX_OK).all() and (fix["n_used"][complete] == 5).all()
    assert (fix["status"][~complete] == gpsacq.FIX_TOO_FEW).all()
    worst = np.zeros(2)
    for k in np.linspace(0, 997, 20).astype(int):
        ref = nav_ref.fix(chain["ephs"], obs["eph"][k], obs["tx_ms"][k], obs["tx_frac"][k], obs["weight"][k])
        assert ref["ok"]
        dpos = np.abs(np.array([fix["x"][k], fix["y"][k], fix["z"][k]]) - ref["xyz"]).max()
        dt = abs(float(nav_ref.fold_ms(int(fix["rx_ms"][k]) - ref["rx_ms"])) * 1e-3 + (fix["rx_frac"][k] - ref["rx_frac"]))
        worst = np.maximum(worst, [dpos, dt])
    print("against the reference solver, 20 rows: position %.3g m, receive time %.3g s" % tuple(worst))
    assert worst[0] <= POS_TOL and worst[1] <= TIME_TOL


def test_chain_is_locked_and_counted_right(chain):
    """every observation at R* within half a chip of the generator's law, the fix at R* within 500 m of the receiver"""
    obs, fix, geo = chain["obs"], chain["fix"], chain["geo"]
    row = 500
    assert chain["first"] + row * SPM == R_STAR
    err = []
    for c, (ref_ms, t_sv) in enumerate(chain["law"]):  # the generator puts satellite time ref_ms + t_sv at sample R*
        err.append(float(nav_ref.fold_ms(int(obs["tx_ms"][row, c]) - ref_ms)) * 1e-3 + (obs["tx_frac"][row, c] - t_sv))
    complete = obs["valid"].all(axis=1)
    off = np.linalg.norm(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"], axis=1)
    rx_err = float(nav_ref.fold_ms(int(fix["rx_ms"][row]) - REF_MS)) * 1e-3 + (fix["rx_frac"][row] - REF_FRAC)
    print("observation error at R*: %s ns (worst %.1f ns)" % (["%.1f" % (e * 1e9) for e in err], max(abs(e) for e in err) * 1e9))
    print("position error at R*: %.2f m, receive time error %.1f ns, rms %.2f m; over the %d complete instants: max %.2f m, mean %.2f m"
          % (off[row], rx_err * 1e9, fix["rms"][row], complete.sum(), off[complete].max(), off[complete].mean()))
    assert max(abs(e) for e in err) < 489e-9
    assert off[row] < 500.0


def test_gps_track_prints_fixes(chain, tmp_path):
    """the front end on the same capture: one fix line per second, each within the same 500 m"""
    path = tmp_path / "cap.bin"
    chain["capture"].tofile(path)
    exe = os.path.join(ROOT, "gnss-gps-sdr_amd", "bin", "gps_track")
    out = subprocess.run([exe, str(path), str(FC), str(FS)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    fixes = [l.split() for l in out.stdout.splitlines() if l.startswith("fix ")]
    assert len(fixes) >= 18, out.stdout
    lat0, lon0, alt0 = chain["geo"]["lla"]
    worst = 0.0
    for f in fixes:
        d = dict(zip(f[1::2], f[2::2]))
        xyz = nav_ref.ecef_of(math.radians(float(d["lat"])), math.radians(float(d["lon"])), float(d["alt"]))
        off = float(np.linalg.norm(xyz - chain["geo"]["rx"]))
        worst = max(worst, off)
        secs = round((float(d["tow"]) - (REF_MS * 1e-3 + REF_FRAC - 19.5)))
        assert abs(float(d["tow"]) - (REF_MS * 1e-3 + REF_FRAC - 19.5 + secs)) < 1e-5 and int(d["n_used"]) >= 5, f
        assert off < 500.0, f
    print("gps_track: %d fix lines, worst %.1f m from the receiver" % (len(fixes), worst))
    assert abs(math.degrees(lat0) - float(dict(zip(fixes[-1][1::2], fixes[-1][2::2]))["lat"])) < 0.01
