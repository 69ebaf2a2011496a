"""tests/aided_ref.py, the reference of "Aided acquisition" of include/gpsacq.h, checked on the CPU before the kernels are held
against it (tests/test_gpu_aided.py): its powers against tests/refine_ref.py's prompt sums where the two models coincide, its
prediction against the truth maker's geometry, a weak satellite found next to two absent ones, wrong laws told from the right
one, and the host-only defaults and argument checks of the library.  Each test prints what it measured before it asserts."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_ref
import gen_ref
import nav_ref
import rate_ref
import refine_ref
from coarse_helpers import phases

FS2, FC2, SPM2 = 2.046e6, 0.4e6, 2046  # the small window: two samples per chip
KMAX2 = int(5000.0 / (FS2 / 40000))


def random_bits(n_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)


# ---- the library's host-only side ----------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("hip_artifacts")
def test_defaults_and_argument_errors():
    import gpsacq
    lib = gpsacq.load_library()
    a, s = gpsacq.aid_params(), gpsacq.aided_params()
    assert a.dtype == gpsacq.AID_PARAMS_DTYPE and a.itemsize == 16 and s.itemsize == 32
    assert gpsacq.AID_DTYPE.itemsize == 40 and gpsacq.AIDED_DTYPE.itemsize == 64
    assert float(a["elev_min_deg"][0]) == 5.0 and float(a["reserved"][0]) == 0.0
    got = tuple(s[0].tolist())
    print("defaults:", got)
    assert got == (16, 1, 16, 1, gpsacq.THRESHOLD, aided_ref.RATIO_MIN)
    assert (gpsacq.AID_NO_FIX, gpsacq.AID_NO_EPH, gpsacq.AID_LOW, gpsacq.AID_OFF_GRID) == (aided_ref.AID_NO_FIX, aided_ref.AID_NO_EPH, aided_ref.AID_LOW,
                                                                                            aided_ref.AID_OFF_GRID)
    assert (gpsacq.AIDED_KEPT, gpsacq.AIDED_NO_AID, gpsacq.AIDED_SHORT, gpsacq.AIDED_FEW, gpsacq.AIDED_NO_POWER, gpsacq.AIDED_BELOW) == (
        aided_ref.KEPT, aided_ref.NO_AID, aided_ref.SHORT, aided_ref.FEW, aided_ref.NO_POWER, aided_ref.BELOW)
    q = gpsacq.aided_params(blocks=64, min_segments=9, code_half=127, dop_half=8, keep_snr=-1.0, ratio_min=0.0)
    assert tuple(q[0].tolist()) == (64, 9, 127, 8, -1.0, 0.0) and tuple(gpsacq.aided_params(code_half=0, dop_half=0)[0].tolist())[2:4] == (0, 0)
    for bad in (dict(blocks=0), dict(blocks=65), dict(blocks=1.5), dict(min_segments=0), dict(code_half=-1), dict(code_half=128), dict(dop_half=-1),
                dict(dop_half=9), dict(keep_snr=float("nan")), dict(ratio_min=float("inf"))):
        with pytest.raises(ValueError):
            gpsacq.aided_params(**bad)
    with pytest.raises(TypeError):
        gpsacq.aided_params(window=3)
    for bad in (91.0, -90.5, float("nan")):
        with pytest.raises(ValueError):
            gpsacq.aid_params(bad)
    assert float(gpsacq.aid_params(-90.0)["elev_min_deg"][0]) == -90.0
    # the C ABI without an engine: every entry point refuses, and says so
    assert lib.gpsacq_aid_default_params(None) == 1 and lib.gpsacq_aided_default_params(None) == 1
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf, aid, pk = np.zeros(64, np.uint8), np.zeros(2, gpsacq.AID_DTYPE), np.zeros(2, gpsacq.PEAK_DTYPE)
    out, fix = np.zeros(2, gpsacq.AIDED_DTYPE), np.zeros(2, gpsacq.FIX_DTYPE)
    eph = np.zeros(1, gpsacq.EPHEMERIS_DTYPE)
    assert lib.gpsacq_aided_search(None, p(buf), 64, 5120, None, p(aid), None, 2, None, p(out), p(pk), None) == 1
    assert lib.gpsacq_aided_search_device(None, p(buf), 64, 5120, None, p(aid), None, 2, None, p(out), p(pk), None, 1) == 1
    assert lib.gpsacq_aid_predict(None, p(eph), 1, p(fix), None, 2, 1, None, p(aid)) == 1
    assert lib.gpsacq_aid_predict_device(None, p(eph), 1, p(fix), None, 2, 1, None, p(aid), 1) == 1
    assert lib.gpsacq_aided_peaks_device(None, p(eph), 1, p(fix), None, p(buf), 64, 5120, None, None, 2, 1, None, None, None, p(out), p(pk), 1) == 1
    assert lib.gpsacq_aided_last_ms(None, None, None) == 1 and b"gpsacq_aided_last_ms" in lib.gpsacq_last_error()
    assert not out.view(np.uint8).any() and not pk.view(np.uint8).any() and not aid.view(np.uint8).any()


# ---- powers: where the two models coincide --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ca_center,lo_center", [(777, 23), (3, -KMAX2 + 1), (SPM2 - 2, KMAX2 - 1)])
def test_powers_are_refines_prompt_sums(ca_center, lo_center):
    """blocks 2, W 5, K 1: every (h, d) with base + h < spm must be refine_ref's `prompt` of the peak (ca_shift_h, lo_shift_d), bit
    for bit; across the wrap the two differ by design.  And the quick spelling of the sums equals the slow one everywhere"""
    W, K = 5, 1
    bits = random_bits(2 * 5120 + 640, 7)
    tasks = [(0, 11)]
    aid = [dict(flags=0, ca_center=ca_center, lo_center=lo_center)]
    kw = dict(blocks=2, code_half=W, dop_half=K, ratio_min=0.0)
    rec = aided_ref.aided_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, **kw)[0]
    quick = aided_ref.aided_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, stream=True, **kw)[0]
    assert np.array_equal(rec["powers"], quick["powers"]) and {k: v for k, v in rec.items() if k != "powers"} == {k: v for k, v in quick.items() if k != "powers"}
    base = (ca_center - W) % SPM2
    same, wrapped, differ = 0, 0, 0
    for d in range(2 * K + 1):
        for h in range(2 * W + 1):
            pk = [(30.0, lo_center - K + d, (base + h) % SPM2, 0.0)]
            want = refine_ref.refine(bits, 5120, tasks, pk, SPM2, FC2, FS2, blocks=2)[0]
            assert want["flags"] == 0 and want["segments"] == rec["segments"] == 2 * 40000 // SPM2
            if base + h < SPM2:
                assert int(rec["powers"][d][h]) == want["prompt"], (d, h)
                same += 1
            else:
                wrapped += 1
                differ += int(rec["powers"][d][h]) != want["prompt"]
    print("ca_center %d, lo_center %d: %d powers equal refine's prompt, %d across the wrap of which %d differ" % (ca_center, lo_center, same, wrapped, differ))
    assert same + wrapped == 33 and (wrapped > 0) == (base + 2 * W >= SPM2)
    assert rec["best"] == int(rec["powers"].max()) and rec["total"] == int(rec["powers"].astype(object).sum()) and rec["floor"] == 2 * SPM2 * rec["segments"]


def test_flags_and_the_key():
    bits = random_bits(5120 + 3 * SPM2 // 8 + 9, 3)
    ok = dict(flags=0, ca_center=5, lo_center=0)
    kw = dict(blocks=1, code_half=2, dop_half=1)
    run = lambda aid, tasks, **k: aided_ref.aided_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, **dict(kw, **k))
    blank = lambda r: {k: v for k, v in r.items() if k not in ("powers", "flags", "peak")} == dict(
        segments=0, n_code=0, n_dop=0, best_h=0, best_d=0, lo_shift=0, ca_shift=0, best=0, total=0, floor=0, ratio=0.0) and not r["powers"].any()
    # NO_AID: a flagged record, a centre off the code, a task out of range, no Doppler on the grid
    cases = [(dict(ok, flags=4), (0, 0)), (dict(ok, ca_center=SPM2), (0, 0)), (dict(ok, ca_center=-1), (0, 0)), (ok, (-1, 0)), (ok, (0, 32)), (ok, (9, 0)),
             (dict(ok, lo_center=KMAX2 + 2), (0, 0)), (dict(ok, lo_center=-KMAX2 - 2), (0, 0))]
    recs = run([c[0] for c in cases], [c[1] for c in cases])
    assert all(r["flags"] == aided_ref.NO_AID and blank(r) and r["peak"] == (0.0, 0, 0, 0.0) for r in recs)
    # one step beyond the grid: the rows of the invalid d are zero, the others are searched
    edge = run([dict(ok, lo_center=KMAX2 + 1), dict(ok, lo_center=-KMAX2 - 1)], [(0, 0), (0, 0)], ratio_min=0.0)
    assert edge[0]["powers"][0].any() and not edge[0]["powers"][1:].any() and edge[0]["lo_shift"] == KMAX2 and edge[0]["best_d"] == 0
    assert edge[1]["powers"][2].any() and not edge[1]["powers"][:2].any() and edge[1]["lo_shift"] == -KMAX2 and edge[1]["best_d"] == 2
    # KEPT comes first; a peak below keep_snr is searched
    pk = np.zeros(2, [("snr", "<f4"), ("lo_shift", "<i4"), ("ca_shift", "<i4"), ("max_pwr", "<f4")])
    pk[0], pk[1] = (25.0, 7, 99, 3.5), (24.9, 7, 99, 3.5)
    kept = run([dict(ok, flags=1), ok], [(0, 0), (0, 0)], peaks_in=pk, ratio_min=0.0)
    assert kept[0]["flags"] == aided_ref.KEPT and blank(kept[0]) and kept[0]["peak"] == (25.0, 7, 99, 3.5) and kept[1]["flags"] == 0
    # SHORT and FEW from the window; an all-zero capture: every power equal, the key picks the smallest d and h
    short = run([ok], [(1, 0)], min_segments=4, ratio_min=0.0)[0]
    assert short["segments"] == 3 and short["flags"] == aided_ref.SHORT | aided_ref.FEW and short["peak"] == (0.0, 0, 0, 0.0) and short["best"] > 0
    tie = aided_ref.aided_search(np.zeros(5120, np.uint8), 5120, [(0, 0)], [dict(ok, lo_center=KMAX2 + 1)], SPM2, FC2, FS2, KMAX2, blocks=1, code_half=0,
                                 dop_half=1)[0]
    assert tie["best_d"] == 0 and tie["best_h"] == 0
    zeros = np.zeros(5120, np.uint8)
    both = aided_ref.aided_search(zeros, 5120, [(0, 0)], [ok], SPM2, FC2, FS2, KMAX2, blocks=1, code_half=0, dop_half=0, ratio_min=0.0)[0]
    print("flags, key and edges hold; an all-zero capture reads ratio %.3f" % both["ratio"])
    below = run([ok], [(0, 0)], ratio_min=1e9)[0]
    assert below["flags"] == aided_ref.BELOW and below["peak"] == (0.0, 0, 0, 0.0) and below["best"] > 0


# ---- prediction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True])
def test_prediction_against_the_truth_maker(moving):
    geo, sel, present, absent, dops = ac.scene_sats()
    ephs = [geo["ephs"][k] for k in sel]
    ref_ms, frac = geo["ref_ms"] + 4321, ac.REF_FRAC
    fix = dict(status=0, x=geo["rx"][0], y=geo["rx"][1], z=geo["rx"][2], rx_ms=ref_ms % nav_ref.WEEK_MS, rx_frac=frac)
    vel = dict(status=0, vx=11.0, vy=-7.5, vz=3.25, drift=3e-7) if moving else None
    rows = aided_ref.predict(ephs, [fix], None if vel is None else [vel], len(sel), ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX)[0]
    truth, _ = phases(geo, sel, np.array([ref_ms]), np.array([frac]))
    worst_ca, worst_lo, worst_hz = 0.0, 0.0, 0.0
    for c, r in enumerate(rows):
        assert r["flags"] == 0 and 5.0 <= r["elev_deg"] <= 90.0, (c, r)
        want_ca = float(truth["tx_frac"][0][c]) * ac.FS
        d_ca = (r["ca_center"] - want_ca + ac.SPM / 2) % ac.SPM - ac.SPM / 2
        # rate_ref's rows run forwards on the predicted Doppler: y = rho' - e . (v_i - Omega x r_r) + c clock_drift = -e . v_r + c drift
        tx_ms = _tx_ms(ephs[c], fix, r["tx_frac"])
        H, y = rate_ref.vel_rows(ephs, [c], [tx_ms], [r["tx_frac"]], [r["doppler_hz"]], geo["rx"], fix["rx_ms"], frac)
        x = np.array([vel["vx"], vel["vy"], vel["vz"], nav_ref.C * vel["drift"]]) if moving else np.zeros(4)
        hz = abs(float(y[0] - H[0] @ x)) * ac.L1 / nav_ref.C
        want_lo = (dops[c] - (ac.L1 / nav_ref.C) * float(H[0] @ x)) / ac.STEP_HZ  # rho' moves by H . (v_r, c drift)
        worst_ca, worst_lo, worst_hz = max(worst_ca, abs(d_ca)), max(worst_lo, abs(r["lo_center"] - want_lo)), max(worst_hz, hz)
        assert r["lo_center"] == int(np.rint(r["doppler_hz"] / ac.STEP_HZ))
    print("moving %s: ca_center within %.3f samples of the truth maker's phase, lo_center within %.3f grid points of the generator's Doppler, "
          "doppler_hz within %.3g Hz of VELOCITY's row run forwards" % (moving, worst_ca, worst_lo, worst_hz))
    assert worst_ca <= 1.0 and worst_lo <= 1.0 and worst_hz <= 1e-6


def _tx_ms(eph, fix, tx_frac):
    """the millisecond the reference put the transmit time in: the one nearest 75 ms before the receive instant that carries tx_frac"""
    t = nav_ref.truth_tx(eph, np.array([fix["x"], fix["y"], fix["z"]]), fix["rx_ms"], np.array([fix["rx_frac"]]))[0]
    ms, f = nav_ref.split_time(fix["rx_ms"], t)
    assert abs(float(f) - tx_frac) < 1e-7
    return int(ms)


def test_prediction_flags():
    geo, sel, _, _, _ = ac.scene_sats()
    ephs = [geo["ephs"][k] for k in sel]
    fix = dict(status=0, x=geo["rx"][0], y=geo["rx"][1], z=geo["rx"][2], rx_ms=(geo["ref_ms"] + 4321) % nav_ref.WEEK_MS, rx_frac=ac.REF_FRAC)
    zero = dict(ca_center=0, lo_center=0, reserved=0, tx_frac=0.0, doppler_hz=0.0, elev_deg=0.0)
    assert aided_ref.predict_one(ephs[0], dict(fix, status=2), None, ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX) == dict(zero, flags=aided_ref.AID_NO_FIX)
    assert aided_ref.predict_one(None, fix, None, ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX) == dict(zero, flags=aided_ref.AID_NO_EPH)
    r = aided_ref.predict_one(ephs[0], fix, None, ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX, elev_min_deg=89.9)
    assert r["flags"] == aided_ref.AID_LOW and r["doppler_hz"] != 0.0
    r = aided_ref.predict_one(ephs[0], fix, dict(status=0, vx=0.0, vy=0.0, vz=0.0, drift=1e-5), ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX)
    assert r["flags"] == aided_ref.AID_OFF_GRID and abs(r["lo_center"]) > ac.KMAX  # 15.75 kHz of clock drift
    r2 = aided_ref.predict_one(ephs[0], fix, dict(status=3, vx=9.0, vy=9.0, vz=9.0, drift=1e-5), ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX)
    assert r2 == aided_ref.predict_one(ephs[0], fix, None, ac.FS, ac.SPM, ac.STEP_HZ, ac.KMAX)  # a velocity that is not OK is no velocity


# ---- detection --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weak_scene():
    """16 blocks by tests/gen_ref.py: five satellites at 0.2, one at WEAK_AMPLITUDE; the weak one and the two absent ones searched"""
    geo, sel, present, absent, dops = ac.scene_sats()
    y = gen_ref.LAW.bits(ac.FC, ac.FS, present, 1.0, 2024, 0, 16 * 40960)["y"]
    s01 = (y < 0.0).astype(np.uint8)
    chans = [present[5]] + absent
    aid = []
    for s in chans:
        ca, lo = ac.law_center(s, 0)
        aid.append(dict(flags=0, ca_center=int(round(ca)) % ac.SPM, lo_center=int(round(lo))))
    return dict(s01=s01, bits=np.packbits(s01, bitorder="little"), chans=chans, aid=aid, tasks=[(0, s[0] - 1) for s in chans], present=present)


def test_detection_of_a_weak_satellite(weak_scene):
    """Five satellites at amplitude 0.2 and one at WEAK_AMPLITUDE = 0.05, noise sigma 1, 16 blocks, the defaults (W 16, K 1,
    ratio_min 1.922).  Measured here on the CPU (printed by this test):
      the numpy FFT search of block 0 gives the weak PRN snr 15.80 (a noise peak, nowhere near its code phase) against the 25 a hit
      needs, and a strong one 147.9;
      the aided search puts it at ratio 2.453 >= 1.25 ratio_min = 2.4025, at its true code phase;
      the two absent PRNs read ratios 1.2619 and 1.2701 <= 0.8 ratio_min = 1.5376.
    Weaker amplitudes fall short of the first bound: 0.03 reads 1.625 (below ratio_min itself), 0.04 reads 1.977, 0.045 reads 2.201."""
    w = weak_scene
    snr = ac.numpy_search(w["s01"], w["chans"][0][0])
    strong = ac.numpy_search(w["s01"], w["present"][0][0])
    recs = aided_ref.aided_search(w["bits"], 5120, w["tasks"], w["aid"], ac.SPM, ac.FC, ac.FS, ac.KMAX, stream=True)
    ca_law, lo_law = ac.law_center(w["chans"][0], 0)
    print("amplitude %g: search snr of the weak PRN %.2f (a strong one: %.1f); aided ratio %.4f; absent PRNs %.4f and %.4f; ratio_min %.3f" %
          (ac.WEAK_AMPLITUDE, snr[0], strong[0], recs[0]["ratio"], recs[1]["ratio"], recs[2]["ratio"], aided_ref.RATIO_MIN))
    print("weak PRN: ca_shift %d (law %.2f), lo_shift %d (law %.2f)" % (recs[0]["ca_shift"], ca_law, recs[0]["lo_shift"], lo_law))
    assert 0.03 <= ac.WEAK_AMPLITUDE <= 0.05
    assert snr[0] < 25.0 and strong[0] >= 25.0
    assert recs[0]["ratio"] >= 1.25 * aided_ref.RATIO_MIN and recs[0]["flags"] == 0
    assert max(recs[1]["ratio"], recs[2]["ratio"]) <= 0.8 * aided_ref.RATIO_MIN
    assert recs[1]["flags"] == recs[2]["flags"] == aided_ref.BELOW and recs[1]["peak"] == (0.0, 0, 0, 0.0)
    assert abs((recs[0]["ca_shift"] - ca_law + ac.SPM / 2) % ac.SPM - ac.SPM / 2) <= 1.0 and abs(recs[0]["lo_shift"] - lo_law) <= 1.0 + 0.5
    assert recs[0]["peak"] == (float(np.float32(recs[0]["ratio"])), recs[0]["lo_shift"], recs[0]["ca_shift"], float(np.float32(recs[0]["best"])))


# ---- wrong laws -------------------------------------------------------------------------------------------------------------------
class HSign(aided_ref.Law):
    def code_index(self, base, h, spm):
        return base - h + 2 * spm  # the replica of h taken at sample j - h


class DSign(aided_ref.Law):
    def lo_shift_of(self, lo_center, K, d):
        return lo_center + K - d


class ReducedIndex(aided_ref.Law):
    def code_index(self, base, h, spm):
        return (base + h) % spm


class PhasePerSegment(aided_ref.Law):
    def carrier_sample(self, j, spm):
        return j % spm


class HalfFloor(aided_ref.Law):
    def floor_of(self, spm, segments):
        return spm * segments


def clean_signal(n_samples, prn, doppler_hz, code_phase_samples):
    """the generator's law without noise, one satellite, in float64 at fs = 2.046 MHz"""
    m = np.arange(n_samples, dtype=np.float64)
    idx = np.floor((m + code_phase_samples) * (ac.CPS * (1.0 + doppler_hz / ac.L1) / FS2)).astype(np.int64) % 1023
    chip = 1.0 - 2.0 * aided_ref.track_ref.chips(prn)[idx]
    return np.packbits((chip * np.cos(2.0 * np.pi * (((FC2 + doppler_hz) / FS2 * m + 0.123) % 1.0)) < 0.0).astype(np.uint8), bitorder="little")


@pytest.mark.parametrize("wrong", [HSign, DSign, ReducedIndex, PhasePerSegment, HalfFloor])
def test_wrong_laws_are_told_from_the_right_one(wrong):
    """a clean signal whose code phase lies 3 samples past the prediction and just below the wrap (base + h crosses spm inside the
    window), at a Doppler of -34 bins, predicted one bin too high: the right law finds it at best_h = W + 3.  The sample grid is
    commensurate with the chips, so reducing base + h moves exactly ONE sample of the window across a chip boundary, the one where
    the reduced count is zero, from chip 1022 to chip 0: the PRN is one whose two chips differ"""
    W, K, lo_true = 5, 1, -34
    prn = next(p for p in range(1, 33) if aided_ref.track_ref.chips(p)[0] != aided_ref.track_ref.chips(p)[1022])
    ca_true = SPM2 - 1
    dop = lo_true * FS2 / 40000
    cps = ac.CPS * (1.0 + dop / ac.L1) / FS2
    code_phase = ca_true * (ac.CPS / FS2) / cps  # samples at the Doppler-shifted rate that show ca_true samples' worth of chips
    bits = clean_signal(2 * 40000 + 64, prn, dop, code_phase)
    aid = [dict(flags=0, ca_center=ca_true - 3, lo_center=lo_true + 1)]
    kw = dict(blocks=2, code_half=W, dop_half=K, ratio_min=3.0)
    right = aided_ref.aided_search(bits, 5120, [(0, prn - 1)], aid, SPM2, FC2, FS2, KMAX2, **kw)[0]
    other = aided_ref.aided_search(bits, 5120, [(0, prn - 1)], aid, SPM2, FC2, FS2, KMAX2, law=wrong(), **kw)[0]
    print("%s: right law best (h %d, d %d) ca %d lo %d ratio %.1f; wrong law (h %d, d %d) ca %d lo %d ratio %.1f" % (
        wrong.__name__, right["best_h"], right["best_d"], right["ca_shift"], right["lo_shift"], right["ratio"], other["best_h"], other["best_d"],
        other["ca_shift"], other["lo_shift"], other["ratio"]))
    assert right["flags"] == 0 and (right["best_h"], right["ca_shift"]) == (W + 3, ca_true) and right["ratio"] > 100.0
    differs = [f for f in aided_ref.INT_FIELDS + ("ratio",) if right[f] != other[f]] + ([] if np.array_equal(right["powers"], other["powers"]) else ["powers"])
    assert differs, wrong.__name__
    print("   differs in", differs)
