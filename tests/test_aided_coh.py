"""tests/aided_coh_ref.py, the reference of "Coherent aided acquisition" of include/gpsacq.h, checked on the CPU before the kernel
is held against it (tests/test_gpu_aided_coh.py): the host-only side of the library, M = 1 and F = 0 against tests/aided_ref.py,
hand-made series whose powers are exact by hand, a noise-free signal that pins the sign of the fine Doppler and the bit edge, a
weak satellite that the non-coherent search misses, and five wrong laws told from the right one.  Each test prints what it
measured before it asserts."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_coh_ref as cr
import aided_ref
import gen_ref

FS2, FC2, SPM2 = 2.046e6, 0.4e6, 2046  # the small window: two samples per chip
STEP2 = FS2 / 40000
KMAX2 = int(5000.0 / STEP2)


# ---- 1. the library's host-only side --------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("hip_artifacts")
def test_sizes_defaults_exports_ranges_and_table():
    import gpsacq
    lib = gpsacq.load_library()
    s = gpsacq.aided_coh_params()
    assert s.dtype == gpsacq.AIDED_COH_PARAMS_DTYPE and s.itemsize == 48 and gpsacq.AIDED_COH_DTYPE.itemsize == 96
    got = tuple(s[0].tolist())
    print("defaults:", got)
    d = cr.DEFAULTS
    assert got == (d["blocks"], d["min_segments"], d["code_half"], d["dop_half"], d["coh_ms"], d["fine_half"], d["fine_step"], 0, gpsacq.THRESHOLD,
                   cr.RATIO_MIN)
    assert got[:7] == (16, 20, 16, 1, 20, 3, 25)
    for name in ("gpsacq_aided_coh_default_params", "gpsacq_aided_coh_table", "gpsacq_aided_coh_search", "gpsacq_aided_coh_search_device",
                 "gpsacq_aid_instant", "gpsacq_aid_instant_device", "gpsacq_aided_coh_peaks_device", "gpsacq_aided_coh_last_ms"):
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    q = gpsacq.aided_coh_params(blocks=64, min_segments=9, code_half=31, dop_half=8, coh_ms=1, fine_half=7, fine_step=512, keep_snr=-1.0, ratio_min=0.0)
    assert tuple(q[0].tolist()) == (64, 9, 31, 8, 1, 7, 512, 0, -1.0, 0.0)
    assert tuple(gpsacq.aided_coh_params(code_half=0, dop_half=0, fine_half=0, fine_step=1)[0].tolist())[2:7] == (0, 0, 20, 0, 1)
    for m in cr.COH_MS:
        assert int(gpsacq.aided_coh_params(coh_ms=m)["coh_ms"][0]) == m
    for bad in (dict(blocks=0), dict(blocks=65), dict(blocks=1.5), dict(min_segments=0), dict(code_half=-1), dict(code_half=32), dict(dop_half=-1),
                dict(dop_half=9), dict(coh_ms=0), dict(coh_ms=3), dict(coh_ms=8), dict(coh_ms=40), dict(fine_half=-1), dict(fine_half=8),
                dict(fine_step=0), dict(fine_step=513), dict(keep_snr=float("nan")), dict(ratio_min=float("inf"))):
        with pytest.raises(ValueError):
            gpsacq.aided_coh_params(**bad)
    with pytest.raises(TypeError):
        gpsacq.aided_coh_params(window=3)
    # the table against numpy's cos and sin, and the margin to a rounding tie that makes it the same everywhere
    tab = gpsacq.aided_coh_table()
    k = np.arange(1024)
    xc, xs = 16384.0 * np.cos(2.0 * np.pi * k / 1024.0), 16384.0 * np.sin(2.0 * np.pi * k / 1024.0)
    margin = min(np.abs(np.abs(x - np.floor(x)) - 0.5).min() for x in (xc, xs))
    tc, ts = cr.LAW.table()
    print("table: C[0] %d, S[256] %d, C[512] %d; nearest rounding tie %.2e away" % (tab[0][0], tab[1][256], tab[0][512], margin))
    assert tab.dtype == np.int16 and tab.shape == (2, 1024) and margin > 3.9e-4
    assert np.array_equal(tab[0], np.rint(xc).astype(np.int16)) and np.array_equal(tab[1], np.rint(xs).astype(np.int16))
    assert np.array_equal(tab[0], tc) and np.array_equal(tab[1], ts) and (tab[0][0], tab[1][0], tab[1][256], tab[0][512]) == (16384, 0, 16384, -16384)
    # the C ABI without an engine: every entry point refuses and writes nothing
    assert lib.gpsacq_aided_coh_default_params(None) == 1 and lib.gpsacq_aided_coh_table(None) == 1
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf, aid, pk = np.zeros(64, np.uint8), np.zeros(2, gpsacq.AID_DTYPE), np.zeros(2, gpsacq.PEAK_DTYPE)
    out, fix = np.zeros(2, gpsacq.AIDED_COH_DTYPE), np.zeros(2, gpsacq.FIX_DTYPE)
    info, prior, eph = np.zeros(2, gpsacq.COARSE_INFO_DTYPE), np.zeros(2, gpsacq.COARSE_PRIOR_DTYPE), np.zeros(1, gpsacq.EPHEMERIS_DTYPE)
    assert lib.gpsacq_aided_coh_search(None, p(buf), 64, 5120, None, p(aid), None, 2, None, p(out), p(pk), None) == 1
    assert lib.gpsacq_aided_coh_search_device(None, p(buf), 64, 5120, None, p(aid), None, 2, None, p(out), p(pk), None, 1) == 1
    assert lib.gpsacq_aid_instant(None, p(fix), p(info), p(prior), 2, p(fix)) == 1
    assert lib.gpsacq_aid_instant_device(None, p(fix), p(info), p(prior), 2, p(fix), 1) == 1
    assert lib.gpsacq_aided_coh_peaks_device(None, p(eph), 1, p(fix), None, None, None, p(buf), 64, 5120, None, None, 2, 1, None, None, None, None,
                                             p(out), p(pk), 1) == 1
    assert lib.gpsacq_aided_coh_last_ms(None, None, None, None) == 1 and b"gpsacq_aided_coh_last_ms" in lib.gpsacq_last_error()
    assert not out.view(np.uint8).any() and not pk.view(np.uint8).any() and not fix.view(np.uint8).any()


# ---- 2. M = 1, F = 0 is the non-coherent search ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ca_center,lo_center", [(777, 23), (SPM2 - 2, KMAX2)])
def test_one_segment_sums_are_the_aided_search(ca_center, lo_center):
    """fs = 2.046 MHz, blocks 2, W 5, K 1 on random bits: with M = 1 and F = 0 every period is one segment turned by C[0] = 2^14,
    S[0] = 0, so powers, best, its place, ca_shift, lo_shift, floor and ratio are aided_ref.aided_search's (its sample-by-sample
    spelling) bit for bit, and noncoh is best.  The second case crosses the code wrap and has an invalid d row"""
    bits = np.random.default_rng(7).integers(0, 256, 2 * 5120 + 640, dtype=np.uint8)
    tasks, aid = [(0, 11)], [dict(flags=0, ca_center=ca_center, lo_center=lo_center)]
    want = aided_ref.aided_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, blocks=2, code_half=5, dop_half=1, ratio_min=0.0)[0]
    got = cr.aided_coh_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, blocks=2, min_segments=1, code_half=5, dop_half=1, coh_ms=1, fine_half=0,
                              fine_step=25, ratio_min=0.0)[0]
    print("ca_center %d lo_center %d: best %d at (d %d, h %d), ratio %.4f; rows of invalid d: %d" % (
        ca_center, lo_center, got["best"], got["best_d"], got["best_h"], got["ratio"], sum(not want["powers"][d].any() for d in range(3))))
    assert got["powers"].shape == (3, 1, 1, 11) and np.array_equal(got["powers"][:, 0, 0, :], want["powers"])
    for f in ("flags", "segments", "n_code", "n_dop", "best_h", "best_d", "lo_shift", "ca_shift", "best", "floor", "ratio", "peak"):
        assert got[f] == want[f], f
    assert got["noncoh"] == got["best"] and (got["n_fine"], got["n_edge"], got["best_f"], got["best_e"]) == (1, 1, 0, 0)
    assert got["doppler_hz"] == got["lo_shift"] * FS2 / 40000.0
    assert (lo_center == KMAX2) == (not want["powers"][2].any())


# ---- 3. hand-made series, exact by hand -----------------------------------------------------------------------------------------
def hand_record(zi, zq, F, u, M, law=cr.LAW, min_segments=1):
    """steps 5 and 6 on one hand-made column: W = 0, K = 0"""
    z = [(np.array(zi, np.int64).reshape(-1, 1), np.array(zq, np.int64).reshape(-1, 1))]
    n = len(zi)
    return cr.record_of(z, [(True, 0, 0)], SPM2, FS2, 0.0, 0, 0, n, n, 0, 0, F, u, M, min_segments, 0.0, law)


def test_hand_made_series():
    a, b = 1200, -500
    quarter = [(a, b), (-b, a), (-a, -b), (b, -a)]  # (a + ib) i^s: a constant turn of 256 / 1024 cycle per segment
    # a constant turn of u / 1024 per segment, S <= M: one period, every product exact (C, S in {0, +-2^14})
    n = 16
    zi, zq = [quarter[s % 4][0] for s in range(n)], [quarter[s % 4][1] for s in range(n)]
    r = hand_record(zi, zq, 2, 256, 20)
    print("turn of 256/1024 per segment: best_f %d, best %d = %d^2 * %d; doppler_hz %.3f" % (r["best_f"], r["best"], n, a * a + b * b, r["doppler_hz"]))
    assert r["best_f"] == 2 + 1 and r["best"] == n * n * (a * a + b * b) and r["best_e"] == 0 and r["noncoh"] == n * (a * a + b * b)
    assert r["doppler_hz"] == 256.0 / 1024.0 * (FS2 / SPM2)  # +250 Hz: a positive f is a Doppler above the grid point's
    back = hand_record(zi, [-q for q in zq], 2, 256, 20)  # the mirrored series turns the other way
    assert back["best_f"] == 2 - 1 and back["best"] == r["best"]
    # f = 0 leaves i^s itself, whose sum over the one period of 16 segments (e = 0) is 0; e = 2 cuts it into 2 + 14: two sums of z0 (1 + i)
    assert int(r["powers"][0, 2, 0, 0]) == 0 and int(r["powers"][0, 2, 2, 0]) == 2 * 2 * (a * a + b * b)
    # a sign flip every 20 segments starting at segment 7: the edge is found, and the power there is the unflipped series'
    n = 50
    sign = [1 if ((s - 7) // 20) % 2 else -1 for s in range(n)]
    flat = hand_record([a] * n, [b] * n, 0, 25, 20)
    flip = hand_record([a * g for g in sign], [b * g for g in sign], 0, 25, 20)
    want = (7 * 7 + 20 * 20 + 20 * 20 + 3 * 3) * (a * a + b * b)  # the periods [0, 7), [7, 27), [27, 47), [47, 50): the partial ones count
    print("flips at 7, 27, 47 of %d segments: best_e %d, best %d (unflipped at e = 7: %d; whole periods alone would give %d)" % (
        n, flip["best_e"], flip["best"], int(flat["powers"][0, 0, 7, 0]), 800 * (a * a + b * b)))
    assert flip["best_e"] == 7 and flip["best"] == want == int(flat["powers"][0, 0, 7, 0])
    assert flat["best_e"] == 0 and flat["best"] == (20 * 20 + 20 * 20 + 10 * 10) * (a * a + b * b)  # unflipped: e = 0 and e = 10 tie, the smaller e wins
    # e at or beyond S: one period; S < M
    short = hand_record([a] * 5, [b] * 5, 0, 25, 20)
    assert [int(x) for x in short["powers"][0, 0, :, 0]] == [25 * (a * a + b * b)] + [(e * e + (5 - e) ** 2) * (a * a + b * b) for e in range(1, 5)] + \
        [25 * (a * a + b * b)] * 15
    assert short["best_e"] == 0  # among equals the smallest e
    # the shift is floor, after the sum: three segments of (5, -5) at k = 0 are +-15 * 2^14 exactly; one unit less rounds down
    assert hand_record([5] * 3, [-5] * 3, 0, 25, 20)["best"] == 2 * 15 * 15
    tc, ts = cr.LAW.table()
    assert (int(tc[1]), int(ts[1])) == (16384, 101)
    one = hand_record([3, 3], [-1, -1], 1, 1, 20)  # f = +1: segment 1 reads 3 * 16384 - 101 and -16384 - 3 * 101
    assert int(one["powers"][0, 2, 0, 0]) == ((6 * 16384 - 101) >> 14) ** 2 + ((-2 * 16384 - 303) >> 14) ** 2 == 5 * 5 + 3 * 3


# ---- 4. a noise-free signal: the sign of the fine Doppler and the bit edge ---------------------------------------------------------
EDGE, FINE_HZ = 7, 30.0


def clean_signal(n_samples, prn, doppler_hz, code_phase_samples, first_bit_period):
    """tests/test_aided.py's clean signal with a data bit that flips every 20 code periods, the first flip where code period
    `first_bit_period` starts"""
    m = np.arange(n_samples, dtype=np.float64)
    q = (m + code_phase_samples) * (ac.CPS * (1.0 + doppler_hz / ac.L1) / FS2)
    chip = 1.0 - 2.0 * aided_ref.track_ref.chips(prn)[np.floor(q).astype(np.int64) % 1023]
    bit = 1.0 - 2.0 * (np.floor((np.floor(q / 1023.0) - first_bit_period) / 20.0).astype(np.int64) % 2)
    return np.packbits((bit * chip * np.cos(2.0 * np.pi * (((FC2 + doppler_hz) / FS2 * m + 0.123) % 1.0)) < 0.0).astype(np.uint8), bitorder="little")


@pytest.fixture(scope="module")
def clean():
    """blocks 3 (58 segments), PRN 9 at grid point -34 plus 30 Hz, code phase 3 samples: code period k starts 3 samples before
    segment k, so the bits flip at segments 7, 27 and 47.  The segment sums are made once"""
    lo, W, K = -34, 5, 0
    dop = lo * STEP2 + FINE_HZ
    bits = clean_signal(3 * 40000 + 64, 9, dop, 3.0, EDGE)
    ok, lo_rate, ca_rate = aided_ref.nco_words(lo, FC2, FS2)
    segments = 3 * 40000 // SPM2
    z = cr.segment_sums(np.unpackbits(bits, bitorder="little"), 0, segments, SPM2, 9, (3 - W) % SPM2, 2 * W + 1, [(ok, lo_rate, ca_rate)])
    return dict(bits=bits, lo=lo, W=W, K=K, dop=dop, z=z, rates=[(ok, lo_rate, ca_rate)], segments=segments)


def clean_record(c, law=cr.LAW, F=3, u=10):
    return cr.record_of(c["z"], c["rates"], SPM2, FS2, 0.0, c["lo"], (3 - c["W"]) % SPM2, c["segments"], c["segments"], c["W"], c["K"], F, u, 20, 20, 3.0,
                        law)


def test_fine_doppler_sign_and_bit_edge(clean):
    """F = 3, u = 10: fine steps of 9.77 Hz.  The signal is 30 Hz ABOVE grid point -34: the right sign reads best_f = F + 3 (29.3 Hz)"""
    r = clean_record(clean)
    whole = cr.aided_coh_search(clean["bits"], 5120, [(0, 8)], [dict(flags=0, ca_center=3, lo_center=clean["lo"])], SPM2, FC2, FS2, KMAX2, blocks=3,
                                code_half=5, dop_half=0, fine_half=3, fine_step=10, ratio_min=3.0)[0]
    assert {k: v for k, v in whole.items() if k != "powers"} == {k: v for k, v in r.items() if k != "powers"} and np.array_equal(whole["powers"], r["powers"])
    step = 10 / 1024.0 * (FS2 / SPM2)
    print("clean signal at %.2f Hz: doppler_hz %.2f (best_f %d, fine step %.2f Hz), best_e %d, best_h %d, ratio %.1f against non-coherent %.1f" % (
        clean["dop"], r["doppler_hz"], r["best_f"], step, r["best_e"], r["best_h"], r["ratio"], r["noncoh"] / r["floor"]))
    assert r["flags"] == 0 and r["best_h"] == clean["W"] and r["ca_shift"] == 3
    assert abs(r["doppler_hz"] - clean["dop"]) <= step / 2 and r["best_f"] == 3 + 3
    assert r["best_e"] == EDGE
    assert r["ratio"] > 10.0 * r["noncoh"] / r["floor"]  # 7, 20, 20 and 11 segments add coherently


# ---- 5. detection -----------------------------------------------------------------------------------------------------------------
WEAK = 0.0337


def test_detection_below_the_noncoherent_threshold():
    """The scene of tests/aided_cases.py -- five satellites at amplitude 0.2, the sixth at WEAK, two absent PRNs, 16 blocks at 5.456
    MHz, noise seed 2024 -- with random navigation bits (16 per satellite, seed 5), the defaults of both searches (ratio_min 1.922
    and 10.73).  The measured ratio_min leaves amplitude 0.03 no room of a quarter (it reads 11.17: detected, but below 1.25 *
    10.73 = 13.41), so WEAK = 0.0337 was chosen on the CPU as tests/aided_cases.py's WEAK_AMPLITUDE was.  Measured here (printed by
    this test):
      the non-coherent search reads the weak PRN at ratio 1.911, BELOW its 1.922;
      the coherent search puts it at ratio 13.67 >= 13.41, at its true code phase, bit edge 7, 384.8 Hz against the generator's 389.8;
      the two absent PRNs read 3.23 and 3.49 <= 0.8 * 10.73 = 8.58.
    The window is narrow: 0.034 reads 13.84 but the non-coherent search then reads 1.9220, no longer BELOW; 0.035 reads 14.63 and
    1.959."""
    geo, sel, present, absent, dops = ac.scene_sats(weak=WEAK)
    nav = (1 - 2 * np.random.default_rng(5).integers(0, 2, (len(present), 16))).astype(np.int8)
    y = gen_ref.LAW.bits(ac.FC, ac.FS, present, 1.0, 2024, 0, 16 * 40960, nav=nav)["y"]
    bits = np.packbits((y < 0.0).astype(np.uint8), bitorder="little")
    chans = [present[5]] + absent
    aid = []
    for s in chans:
        ca, lo = ac.law_center(s, 0)
        aid.append(dict(flags=0, ca_center=int(round(ca)) % ac.SPM, lo_center=int(round(lo))))
    tasks = [(0, s[0] - 1) for s in chans]
    non = aided_ref.aided_search(bits, 5120, tasks[:1], aid[:1], ac.SPM, ac.FC, ac.FS, ac.KMAX, stream=True)[0]
    recs = cr.aided_coh_search(bits, 5120, tasks, aid, ac.SPM, ac.FC, ac.FS, ac.KMAX)
    ca_law, lo_law = ac.law_center(chans[0], 0)
    print("amplitude %g: non-coherent ratio %.4f (ratio_min %.3f, flags %d); coherent ratio %.4f, absent PRNs %.4f and %.4f; ratio_min %.3f" % (
        WEAK, non["ratio"], aided_ref.RATIO_MIN, non["flags"], recs[0]["ratio"], recs[1]["ratio"], recs[2]["ratio"], cr.RATIO_MIN))
    print("weak PRN: ca_shift %d (law %.2f), doppler_hz %.1f (generator %.1f), best_e %d, noncoh / floor %.4f" % (
        recs[0]["ca_shift"], ca_law, recs[0]["doppler_hz"], chans[0][2], recs[0]["best_e"], recs[0]["noncoh"] / recs[0]["floor"]))
    assert non["flags"] == aided_ref.BELOW
    assert recs[0]["flags"] == 0 and recs[0]["ratio"] >= 1.25 * cr.RATIO_MIN
    assert abs((recs[0]["ca_shift"] - ca_law + ac.SPM / 2) % ac.SPM - ac.SPM / 2) <= 1.0
    assert max(recs[1]["ratio"], recs[2]["ratio"]) <= 0.8 * cr.RATIO_MIN
    assert recs[1]["flags"] == recs[2]["flags"] == cr.BELOW and recs[1]["peak"] == (0.0, 0, 0, 0.0)
    assert abs(recs[0]["doppler_hz"] - chans[0][2]) <= 25 / 1024.0 * (ac.FS / ac.SPM)  # within a fine step of the generator's Doppler


# ---- 6. wrong laws ----------------------------------------------------------------------------------------------------------------
class RotationSign(cr.Law):
    def rotate(self, i, q, c, s):
        return i * c - q * s, q * c + i * s  # turned forward


class BoundariesLate(cr.Law):
    def boundaries(self, e, m, n_seg):
        return sorted({0, n_seg} | {s for s in range(1, n_seg) if s % m == (e + 1) % m})


class ShiftFirst(cr.Law):
    def terms(self, a):
        return a >> 14

    def period_value(self, total):
        return total


class IndexUnreduced(cr.Law):
    def table_index(self, f, u, s):
        return np.clip(f * u * s, 0, 1023)  # no modulo: an index beyond the table reads its nearest end


class NoPartialPeriods(cr.Law):
    def periods(self, bounds, m):
        return [(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi - lo == m]


@pytest.mark.parametrize("wrong", [RotationSign, BoundariesLate, ShiftFirst, IndexUnreduced, NoPartialPeriods])
def test_wrong_laws_are_told_from_the_right_one(clean, wrong):
    right, other = clean_record(clean), clean_record(clean, law=wrong())
    differs = [f for f in cr.INT_FIELDS + ("ratio", "doppler_hz") if right[f] != other[f]] + ([] if np.array_equal(right["powers"], other["powers"]) else ["powers"])
    print("%s: right law best_f %d best_e %d best %d; wrong law best_f %d best_e %d best %d; differs in %s" % (
        wrong.__name__, right["best_f"], right["best_e"], right["best"], other["best_f"], other["best_e"], other["best"], differs))
    assert (right["best_f"], right["best_e"]) == (6, EDGE)
    assert differs, wrong.__name__
    expected = {"RotationSign": "best_f", "BoundariesLate": "best_e", "ShiftFirst": "best", "IndexUnreduced": "best", "NoPartialPeriods": "best"}
    assert expected[wrong.__name__] in differs
