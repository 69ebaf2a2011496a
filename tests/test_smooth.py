"""Carrier-smoothed observables on the host: the model of include/gpsacq.h ("Carrier-smoothed observables") as tests/smooth_ref.py
states it, checked against itself in independent ways -- coherent records against the raw observation, the prefix form of the window
sum against the direct one, resets, floor division, the epoch boundary, the scan kernel's indexing lane by lane -- then the chain
from a capture through the CPU channel model, plus struct sizes and exports.  Needs the library, no GPU."""
import os
import subprocess

import numpy as np
import pytest

import obs_ref
import smooth_ref
from smooth_ref import FULL, FULLW, INVALID, LOCKED, M64, RAW, RESET, UNLOCKED

pytestmark = pytest.mark.usefixtures("hip_artifacts")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gpsacq_smooth_default_params", "gpsacq_smooth_observables", "gpsacq_smooth_observables_device",
               "gpsacq_fix_smooth_track_device", "gpsacq_smooth_last_ms")


def test_struct_sizes_exports_and_defaults(tmp_path):
    import gpsacq
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_smooth_params) == 32 && sizeof(gpsacq_smooth_info) == 24, "sizes");\n'
                   '_Static_assert(offsetof(gpsacq_smooth_params, jump) == 16 && offsetof(gpsacq_smooth_params, invert) == 24, "no padding");\n'
                   '_Static_assert(offsetof(gpsacq_smooth_info, flags) == 4 && offsetof(gpsacq_smooth_info, cmc) == 8 && offsetof(gpsacq_smooth_info, corr) == 16, "no padding");\n'
                   '_Static_assert(GPSACQ_SMOOTH_RESET == 1 && GPSACQ_SMOOTH_UNLOCKED == 2 && GPSACQ_SMOOTH_FULL == 4, "flags");\n'
                   '_Static_assert(sizeof(gpsacq_obs) == 32 && sizeof(gpsacq_rate_obs) == 32 && sizeof(gpsacq_track_record) == 40, "the old structs keep their size");\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert (gpsacq.SMOOTH_PARAMS_DTYPE.itemsize, gpsacq.SMOOTH_INFO_DTYPE.itemsize) == (32, 24)
    for dt in (gpsacq.SMOOTH_PARAMS_DTYPE, gpsacq.SMOOTH_INFO_DTYPE):
        assert sum(dt[n].itemsize for n in dt.names) == dt.itemsize
    assert gpsacq.SMOOTH_INFO_DTYPE.names == ("window", "flags", "cmc", "corr")
    assert (gpsacq.SMOOTH_RESET, gpsacq.SMOOTH_UNLOCKED, gpsacq.SMOOTH_FULL) == (RESET, UNLOCKED, FULLW)
    lib = gpsacq.load_library()
    for name in NEW_SYMBOLS:
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", gpsacq.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert " T %s\n" % name in out, name
    for name in ("smooth_observables", "smooth_observables_device", "fix_smooth_track_device", "smooth_last_ms"):
        assert callable(getattr(gpsacq.Engine, name))
    p = gpsacq.smooth_params()
    assert {k: int(p[k][0]) for k in p.dtype.names} == smooth_ref.DEFAULTS and smooth_ref.DEFAULTS["jump"] == 385 << 32
    assert int(gpsacq.smooth_params(window=7, invert=1)["window"][0]) == 7
    with pytest.raises(TypeError):
        gpsacq.smooth_params(windw=3)


def test_code_sigma_m():
    import gpsacq
    info = np.zeros((6, 2), gpsacq.SMOOTH_INFO_DTYPE)
    info["flags"][:, 0] = [RESET, 0, FULLW, FULLW, FULLW | RESET, UNLOCKED]
    info["corr"][:, 0] = [1 << 40, 5, 1 << 32, -(1 << 32), 3 << 32, 9 << 32]
    sig = gpsacq.code_sigma_m(info)
    lam = 299792458.0 / 1575.42e6
    assert sig.shape == (2,) and np.isnan(sig[1])
    assert sig[0] == pytest.approx(np.std([1.0, -1.0, 3.0]) * lam, rel=1e-12)


def _tags(n_chans):
    import gpsacq
    tags = np.zeros(n_chans, gpsacq.TIME_TAG_DTYPE)
    tags["valid"], tags["eph"], tags["ms"], tags["epoch"] = 1, np.arange(n_chans), 1000, 7
    return tags


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("spm,window", [(2800, 1), (2800, 50), (5456, 300)])
def test_coherent_records_pass_the_raw_observation_through(spm, window, invert):
    """lo_rate = nom + 1540 k, ca_rate = cw + k: Z is constant, so q = c = 0, the smoothed obs are obs_ref's bytes, and the window
    counts 1 .. M and then stays.  With the spectrum declared inverted the carrier must run the other way for the same result."""
    n = 400
    rec, ch, nom = smooth_ref.fabricate_coherent(5 + spm, n, spm)
    if invert:
        rec["lo_rate"] = (2 * nom - rec["lo_rate"].astype(np.int64)) & 0xFFFFFFFF
    tags, ne = _tags(1), np.array([n], np.int32)
    first, step, n_fix = int(rec["sample"][0]), spm + 1, 380
    p = smooth_ref.par(window=window, lock_epochs=0, invert=invert)
    for direct in (False, True):
        obs, info = smooth_ref.smooth_observables(rec[None], ne, ch, tags, [nom], first, step, n_fix, p, direct=direct)
        raw = obs_ref.observables(rec[None], ne, ch, tags, first, step, n_fix)
        assert obs.tobytes() == raw.tobytes() and raw["valid"].all()
        assert not info["corr"].any() and not info["cmc"].any()
        assert list(info["window"][:, 0]) == [min(i + 1, window) for i in range(n_fix)]
        assert list(info["flags"][:, 0]) == [(RESET if i == 0 else 0) | (FULLW if i + 1 >= window else 0) for i in range(n_fix)]
    # the wrong sign is not constant: the test above would notice a flipped carrier
    wrong = smooth_ref.smooth_observables(rec[None], ne, ch, tags, [nom], first, step, n_fix, dict(p, invert=1 - invert, jump=0))[1]
    assert wrong["cmc"].any()


def test_prefix_form_equals_the_direct_form():
    """random Z with offsets near 2^63 and near the wrap, differences small against 2^63 / m: the prefix difference mod 2^64, read
    as int64, is the sum of the int64 differences; and mod 2^64 the two agree whatever Z does"""
    rng = np.random.default_rng(3)
    for base in (0, (1 << 63) - 5000, (1 << 63) + 17, M64 - 3000, 123456789 << 20):
        n = 300
        Z = [(base + int(v)) & M64 for v in rng.integers(-(1 << 40), 1 << 40, n)]
        S = smooth_ref.prefix(Z)
        for i, m in [(0, 1), (5, 6), (5, 3), (299, 300), (299, 64), (150, 1), (200, 77)]:
            d = smooth_ref.window_sum_direct(Z, i, m)
            assert abs(d) < 1 << 63 and smooth_ref.window_sum_prefix(S, Z, i, m) == d
    wild = [int(v) for v in rng.integers(0, 1 << 64, 200, dtype=np.uint64)]
    S = smooth_ref.prefix(wild)
    for i, m in [(199, 200), (100, 31), (7, 8)]:
        assert smooth_ref.window_sum_prefix(S, wild, i, m) == smooth_ref.s64(smooth_ref.window_sum_direct(wild, i, m))


def _series(Z, state=None, P=None):
    n = len(Z)
    state = [LOCKED] * n if state is None else state
    return state, list(range(n)), [FULL // 2] * n if P is None else P, [z & M64 if s == LOCKED else 0 for z, s in zip(Z, state)]


def test_resets_by_gap_jump_and_unlock():
    import gpsacq
    tag = _tags(1)[0]
    jump = 1000
    Z = [50, 60, 70, 80, 5000, 5010, 5020, 0, 0, 5030, 5040, 5050, 5060, 4061, 4059]
    state = [LOCKED] * 7 + [INVALID, RAW] + [LOCKED] * 6
    p = smooth_ref.par(window=3, jump=jump)
    out = smooth_ref.smooth_channel(*_series(Z, state), 100, tag, p)
    win = [None if o is None else o[1]["window"] for o in out]
    flg = [None if o is None else o[1]["flags"] for o in out]
    assert win == [1, 2, 3, 3, 1, 2, 3, None, 0, 1, 2, 3, 3, 3, 3]     # the window restarts at 1 after the jump, the gap and the unlock
    assert flg == [RESET, 0, FULLW, FULLW, RESET, 0, FULLW, None, UNLOCKED, RESET, 0, FULLW, FULLW, FULLW, FULLW]
    assert out[13][1]["cmc"] == 4061 - 5030                            # a step of 999 is no jump; cmc counts from the segment's start
    assert smooth_ref.segment_starts(state, _series(Z, state)[3], jump)[-1] == 9
    assert smooth_ref.segment_starts(state, _series(Z, state)[3], 998)[-1] == 13   # 999 > 998 is one
    assert smooth_ref.segment_starts(state, _series(Z, state)[3], 0)[4] == 0       # jump = 0: no jump test
    # a wrapped difference of 2^63 is INT64_MIN: a jump whatever the threshold
    assert smooth_ref.segment_starts([LOCKED, LOCKED], [5, (5 + (1 << 63)) & M64], (1 << 63) - 1) == [0, 1]
    # an UNLOCKED instant is the raw observation: P and the epoch untouched
    raw = out[8][0]
    assert raw["tx_frac"] == np.float64(FULL // 2) / np.float64(obs_ref.DIVISOR) and raw["tx_ms"] == (1000 + 100 + 8 - 7)
    assert out[8][1] == dict(window=0, flags=UNLOCKED, cmc=0, corr=0)
    assert gpsacq.SMOOTH_UNLOCKED == UNLOCKED


def test_negative_corrections_use_floor_division():
    tag = _tags(1)[0]
    p = smooth_ref.par(window=4, jump=0)
    # Z_i above the mean of its window: D < 0.  D = (0 - 10) + (3 - 10) + 0 = -17 over m = 3: q = floor(-5.67) = -6, c = floor(-6 / 1540) = -1
    out = smooth_ref.smooth_channel(*_series([0, 3, 10]), 0, tag, p)
    assert out[2][1]["corr"] == -6
    assert out[2][0]["tx_frac"] == np.float64(FULL // 2 - 1) / np.float64(obs_ref.DIVISOR)
    # exact quotients stay exact: D = -1540 * 4 over m = 2
    out = smooth_ref.smooth_channel(*_series([0, 2 * 1540 * 4]), 0, tag, p)
    assert out[1][1]["corr"] == -1540 * 4 and out[1][0]["tx_frac"] == np.float64(FULL // 2 - 4) / np.float64(obs_ref.DIVISOR)
    # positive: D = 17 over 3: q = 5, c = 0
    out = smooth_ref.smooth_channel(*_series([17, 0, 0]), 0, tag, p)
    assert out[2][1]["corr"] == 5 and out[2][0]["tx_frac"] == np.float64(FULL // 2) / np.float64(obs_ref.DIVISOR)


@pytest.mark.parametrize("tag_ms,epoch_off,want_down,want_up", [(1000, 0, 999, 1002), (0, 0, 604799999, 2), (604799999, 0, 604799998, 1),
                                                                (604799999, -1, 604799997, 0)])
def test_epoch_boundary_both_ways(tag_ms, epoch_off, want_down, want_up):
    """P~ leaves its code period: downward from P = 2 by a correction of -3 chips-units (k = -1, tx_ms one less, P~ = FULL - 1),
    upward from P = FULL - 2 by +3 (k = +1, tx_ms one more, P~ = 1); also across the end of the week"""
    import gpsacq
    tag = np.zeros(1, gpsacq.TIME_TAG_DTYPE)[0]
    tag["valid"], tag["ms"], tag["epoch"] = 1, tag_ms, 10
    p = smooth_ref.par(window=2, jump=0)
    # m = 2, D = Z_0 - Z_1, q = floor(D / 2), c = floor(q / 1540)
    down = smooth_ref.smooth_channel([LOCKED] * 2, [0, 0], [2, 2], [0, 2 * 1540 * 3], 10 + epoch_off, tag, p)[1]
    assert down[1]["corr"] == -1540 * 3 and down[0]["tx_ms"] == want_down
    assert down[0]["tx_frac"] == np.float64(FULL - 1) / np.float64(obs_ref.DIVISOR)
    up = smooth_ref.smooth_channel([LOCKED] * 2, [1, 1], [FULL - 2] * 2, [2 * 1540 * 3, 0], 10 + epoch_off, tag, p)[1]
    assert up[1]["corr"] == 1540 * 3 and up[0]["tx_ms"] == want_up
    assert up[0]["tx_frac"] == np.float64(1) / np.float64(obs_ref.DIVISOR)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_scan_indexing_equals_the_recursion(n):
    """k_smooth_scan's chunk / run / scan / carry indexing, restated lane by lane, against the plain prefix sum and the plain
    segment recursion: random states, Z near the wrap, jumps at random places"""
    rng = np.random.default_rng(100 + n)
    jump = 1 << 20
    state = [int(v) for v in rng.choice([LOCKED, LOCKED, LOCKED, LOCKED, LOCKED, LOCKED, RAW, INVALID], n)]
    walk = np.cumsum(rng.integers(-(1 << 19), 1 << 19, n) + (rng.random(n) < 0.05) * (1 << 22))
    Z = [(M64 - 1000 + int(w)) & M64 if s == LOCKED else 0 for w, s in zip(walk, state)]
    want_seg = smooth_ref.segment_starts(state, Z, jump)
    for lanes, run in ((64, 4), (8, 3)):
        S, seg = smooth_ref.scan_lanes(Z, state, jump, lanes=lanes, run=run)
        assert S == smooth_ref.prefix(Z) and None not in seg
        assert all(seg[i] == want_seg[i] for i in range(n) if state[i] == LOCKED)
    all_locked = smooth_ref.scan_lanes(Z, [LOCKED] * n, 0)[1]
    assert all_locked == [0] * n


def test_lock_test():
    p = smooth_ref.par(lock_epochs=4, lock_num=1, lock_den=2)
    ip, qp = [100, -100, 100, 100, 10, 10, 10, 10, 0, 0, 0, 0], [5, 5, -5, 5, 50, 100, 100, 100, 0, 0, 0, 0]
    ln, ld = smooth_ref.lock_sums(ip, qp)
    got = [smooth_ref.locked(ln, ld, t, p) for t in range(12)]
    # t < L - 1: never; full power in IP: locked; as QP takes over the ratio falls through 1 / 2; no power at all (D = 0): not locked
    assert got == [False, False, False, True, True, False, False, False, False, False, False, False]
    assert all(smooth_ref.locked(ln, ld, t, smooth_ref.par(lock_epochs=0)) for t in range(12))
    # exactly num / den counts as locked: N / D = (3 - 1) / (3 + 1) = 1 / 2
    ln, ld = smooth_ref.lock_sums([1, 1, 1, 0], [0, 0, 0, 1])
    assert smooth_ref.locked(ln, ld, 3, p)


# ---- the chain on the CPU: a capture by the generator's law, the C channel model, the reference ---------------------------------
def test_chain_smoothed_code_error_is_below_the_raw_one():
    """One satellite at amplitude 0.2, fs 5.456 MHz, 8 s, default loops, window 1000 over instants 1 ms apart.  The code error is the
    observation's code phase against the generator's law (code position (m + cp) * 1.023e6 (1 + fd / L1) / fs chips at sample m), in
    metres.  A sign check, not an accuracy claim: with the carrier's sign or the factor 1540 wrong the smoothed error is many times
    the raw one.  Printed for the record; measured with this test: 7998 instants, 6760 FULL, 5 RESET (all inside the pull-in),
    the last UNLOCKED instant at 0.239 s; code error 1 sigma over the FULL instants raw 1.370 m, smoothed 0.679 m; code_sigma_m 1.335 m;
    cmc drifts by 0.104 m/s (the truncated nominal words)."""
    import gpsacq
    import test_track_ref as ttr
    from track_helpers import run_model
    fs, fc, spm = 5.456e6, 4.092e6, 5456
    prn, amp, fd, cp, th = 9, 0.20, 1234.5, 1000.25, 0.3
    secs = 8
    nav = np.where(np.random.default_rng(2).integers(0, 2, 500) > 0, 1.0, -1.0)
    buf = np.concatenate([ttr.make_capture(fs, fc, [(prn, amp, fd, cp, th, nav)], spm * 1000, first_sample=k * spm * 1000, seed=40 + k)
                          for k in range(secs)])
    p = ttr.default_params(fs)
    chans = ttr.start_chan(fs, fc, prn, fd, cp, th, 100, p, dop_err=40.0)
    max_epochs = secs * 1000 + 8
    _, rec, ne = run_model(buf, 0, chans, p, max_epochs)
    assert int(chans["status"][0]) == 0 and ne[0] > (secs - 1) * 1000
    tags = _tags(1)
    nom = [(int(chans["lo_nom"][0]) & M64) >> 32]
    first = int(rec["sample"][0, 0])
    n_fix = (int(chans["next_sample"][0]) - first) // spm
    obs, info = smooth_ref.smooth_observables(rec, ne, chans, tags, nom, first, spm, n_fix)
    raw = obs_ref.observables(rec, ne, chans, tags, first, spm, n_fix)
    assert obs["valid"].all() and raw["valid"].all()
    R = first + spm * np.arange(n_fix, dtype=np.float64)
    truth = ((R + cp) * (1.023e6 * (1 + fd / 1575.42e6) / fs)) % 1023.0

    def err_m(o):
        d = o["tx_frac"][:, 0] * 1.023e6 - truth
        return (d - 1023.0 * np.round(d / 1023.0)) * (299792458.0 / 1.023e6)

    flags = info["flags"][:, 0]
    full = (flags & FULLW) != 0
    after2 = R >= 2 * fs
    unlocked = (flags & UNLOCKED) != 0
    e_raw, e_sm = err_m(raw), err_m(obs)
    s_raw, s_sm = float(np.std(e_raw[full])), float(np.std(e_sm[full]))
    sigma = gpsacq.code_sigma_m(info)
    print("chain on the CPU: %d instants, %d FULL, %d RESET, last UNLOCKED at %.3f s; code error 1 sigma raw %.3f m, smoothed %.3f m; "
          "code_sigma_m %.3f m; cmc drift %.3f m/s" % (n_fix, int(full.sum()), int(((flags & RESET) != 0).sum()),
                                                       (R[unlocked].max() / fs if unlocked.any() else 0.0), s_raw, s_sm, float(sigma[0]),
                                                       float(np.polyfit(R[full] / fs, info["cmc"][full, 0] * (0.1903 / 2 ** 32), 1)[0])))
    assert full.sum() > 5000
    assert not (unlocked & after2).any()
    assert s_sm < s_raw
    # the unsmoothed instants are the raw bytes
    assert obs[unlocked].tobytes() == raw[unlocked].tobytes()
