"""tests/aided_coh_iq_ref.py, the reference of "Coherent aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, checked on
the CPU before the kernel is held against it (tests/test_gpu_aided_coh_iq.py): the host-only side of the library, the quick
spellings against the slow ones on a 3-block window, M = 1 and F = 0 against tests/aided_iq_ref.py, four wrong laws told from the
right one on a noise-free signal with data bits, and the gain over the sign path on tests/test_aided_coh.py's scene written as an
8-bit IQ capture.  test_defaults_and_the_abi needs the library's new symbols; the other tests check the reference alone, on the CPU, and
every figure in their docstrings is a CPU figure.  Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_coh_iq_ref as qr
import aided_coh_ref
import aided_iq_cases as ic
import aided_iq_ref
import gen_ref
import iq_ref
import track_ref

FS2, FC2, SPM2 = 2.046e6, 0.4e6, 2046  # the small window: two samples per chip
STEP2 = FS2 / 40000
KMAX2 = int(5000.0 / STEP2)
REAL, COMPLEX = qr.REAL, qr.COMPLEX


def fields(r):
    return {k: v for k, v in r.items() if k != "powers"}


# ---- 1. the library's host-only side ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("hip_artifacts")
def test_defaults_and_the_abi():
    import gpsacq
    lib = gpsacq.load_library()
    s, one = gpsacq.aided_coh_params_iq8(), gpsacq.aided_coh_params()
    got = tuple(s[0].tolist())
    print("defaults:", got)
    assert got[:8] == (16, 20, 16, 1, 20, 3, 25, 0) == tuple(one[0].tolist())[:8] and got[8:] == (gpsacq.THRESHOLD, qr.RATIO_MIN)
    assert qr.RATIO_MIN > aided_coh_ref.RATIO_MIN and qr.DEFAULTS["ratio_min"] == qr.RATIO_MIN
    assert tuple(gpsacq.aided_coh_params_iq8(blocks=3, coh_ms=5, ratio_min=2.0)[0].tolist()) == (3, 20, 16, 1, 5, 3, 25, 0, gpsacq.THRESHOLD, 2.0)
    with pytest.raises(ValueError):
        gpsacq.aided_coh_params_iq8(code_half=32)
    for name in ("gpsacq_aided_coh_default_params_iq8", "gpsacq_aided_coh_search_iq8", "gpsacq_aided_coh_search_iq8_device",
                 "gpsacq_aided_coh_peaks_iq8_device", "gpsacq_aided_coh_iq8_last_ms"):
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    for name in ("aided_coh_search_iq8", "aided_coh_search_iq8_device", "aided_coh_peaks_iq8_device", "aided_coh_iq8_last_ms"):
        assert callable(getattr(gpsacq.Engine, name)), name
    # the C ABI without an engine: every entry point refuses and writes nothing
    assert lib.gpsacq_aided_coh_default_params_iq8(None) == 1
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf, aid, pk, out = np.zeros(64, np.uint8), np.zeros(2, gpsacq.AID_DTYPE), np.zeros(2, gpsacq.PEAK_DTYPE), np.zeros(2, gpsacq.AIDED_COH_DTYPE)
    inp = gpsacq.Iq8Input()
    fix, eph = np.zeros(2, gpsacq.FIX_DTYPE), np.zeros(1, gpsacq.EPHEMERIS_DTYPE)
    assert lib.gpsacq_aided_coh_search_iq8(None, ctypes.byref(inp), p(buf), 32, 81920, None, p(aid), None, 2, None, p(out), p(pk), None) == 1
    assert lib.gpsacq_aided_coh_search_iq8_device(None, ctypes.byref(inp), p(buf), 32, 81920, None, p(aid), None, 2, None, p(out), p(pk), None, 1) == 1
    assert lib.gpsacq_aided_coh_peaks_iq8_device(None, p(eph), 1, p(fix), None, None, None, ctypes.byref(inp), p(buf), 32, 81920, None, None, 2, 1, None, None,
                                                 None, None, p(out), p(pk), 1) == 1
    assert lib.gpsacq_aided_coh_iq8_last_ms(None, None, None, None, None) == 1 and b"gpsacq_aided_coh_iq8_last_ms" in lib.gpsacq_last_error()
    assert not out.view(np.uint8).any() and not pk.view(np.uint8).any()


# ---- 2. the quick spellings against the slow ones ---------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc,multibit,mix_hz,ca_center,M,F", [(False, True, REAL, FC2 - 0.3e6, 777, 20, 1), (True, False, COMPLEX, 0.35e6, SPM2 - 2, 5, 2),
                                                                     (True, True, REAL, FC2 + 0.35e6, 0, 4, 0)])
def test_slow_sums_against_the_quick_spellings(signed, dc, multibit, mix_hz, ca_center, M, F):
    """a 3-block window (58 segments) of random bytes at fs = 2.046 MHz: the sample-by-sample segment sums with one replica per
    hypothesis equal the one-stream spelling, and the Python-integer coherent sums equal the int64 spelling, records and all; the
    second prediction sits at -kmax (an invalid d row) and, in the last two cases, at a negative carrier"""
    iq = np.random.default_rng(7).integers(0, 256, 2 * (4 * 40960 + 333), dtype=np.uint8)
    tasks = [(0, 11), (1, 31)]
    aid = [dict(flags=0, ca_center=ca_center, lo_center=23), dict(flags=0, ca_center=ca_center, lo_center=-KMAX2)]
    kw = dict(signed=signed, mean=ic.MEAN if dc else None, mix_hz=mix_hz, multibit=multibit, blocks=3, min_segments=20, code_half=5, dop_half=1, coh_ms=M,
              fine_half=F, fine_step=40, ratio_min=0.0)
    slow = qr.aided_coh_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, **kw)
    quick = qr.aided_coh_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, stream=True, quick=True, **kw)
    for a, b in zip(slow, quick):
        assert np.array_equal(a["powers"], b["powers"]) and fields(a) == fields(b)
        assert a["flags"] == 0 and a["segments"] == 3 * 40000 // SPM2 == 58 and a["best"] == int(a["powers"].max()) and a["floor"] > 0
        assert a["powers"].shape == (3, 2 * F + 1, M, 11)
    rows = sum(int(not slow[1]["powers"][d].any()) for d in range(3))
    print("%s dc %d multibit %d M %d F %d: 2 x %d powers, records and peaks alike; ratios %.3f %.3f; %d row of invalid d" %
          ("S8" if signed else "U8", dc, multibit, M, F, slow[0]["powers"].size, slow[0]["ratio"], slow[1]["ratio"], rows))
    assert rows == 1


# ---- 3. M = 1, F = 0 is the non-coherent search on the IQ bytes --------------------------------------------------------------------
@pytest.mark.parametrize("ca_center,lo_center,multibit", [(777, 23, REAL), (SPM2 - 2, KMAX2, COMPLEX)])
def test_one_segment_sums_are_the_aided_search_iq8(ca_center, lo_center, multibit):
    """with M = 1 and F = 0 every period is one segment turned by C[0] = 2^14, S[0] = 0: powers, best, its place, floor and ratio are
    aided_iq_ref.aided_search's (its sample-by-sample spelling) bit for bit, and noncoh is best"""
    iq = np.random.default_rng(8).integers(0, 256, 2 * (2 * 40960 + 640), dtype=np.uint8)
    tasks, aid = [(0, 11)], [dict(flags=0, ca_center=ca_center, lo_center=lo_center)]
    mode = dict(signed=False, mean=ic.MEAN, mix_hz=ic.mix_of(multibit, 0.3e6, FC2), multibit=multibit)
    want = aided_iq_ref.aided_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, blocks=2, code_half=5, dop_half=1, ratio_min=0.0, **mode)[0]
    got = qr.aided_coh_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, blocks=2, min_segments=1, code_half=5, dop_half=1, coh_ms=1, fine_half=0,
                              fine_step=25, ratio_min=0.0, **mode)[0]
    print("ca_center %d lo_center %d multibit %d: best %d at (d %d, h %d), ratio %.4f; rows of invalid d: %d" % (
        ca_center, lo_center, multibit, got["best"], got["best_d"], got["best_h"], got["ratio"], sum(not want["powers"][d].any() for d in range(3))))
    assert got["powers"].shape == (3, 1, 1, 11) and np.array_equal(got["powers"][:, 0, 0, :], want["powers"])
    for f in ("flags", "segments", "n_code", "n_dop", "best_h", "best_d", "lo_shift", "ca_shift", "best", "floor", "ratio", "peak"):
        assert got[f] == want[f], f
    assert got["noncoh"] == got["best"] and (got["n_fine"], got["n_edge"], got["best_f"], got["best_e"]) == (1, 1, 0, 0)
    assert (lo_center == KMAX2) == (not want["powers"][2].any())


# ---- 4. wrong laws on a noise-free signal ------------------------------------------------------------------------------------------
EDGE, FINE_HZ, IF2 = 7, 30.0, 0.3e6


def clean_iq(n_samples, prn, doppler_hz, code_phase_samples, first_bit_period):
    """the generator's law without noise, one satellite, as int8 I, Q at fs = 2.046 MHz, amplitude 100, with a data bit that flips
    every 20 code periods, the first flip where code period `first_bit_period` starts"""
    m = np.arange(n_samples, dtype=np.float64)
    q = (m + code_phase_samples) * (ic.CPS * (1.0 + doppler_hz / ic.L1) / FS2)
    chip = 1.0 - 2.0 * track_ref.chips(prn)[np.floor(q).astype(np.int64) % 1023]
    bit = 1.0 - 2.0 * (np.floor((np.floor(q / 1023.0) - first_bit_period) / 20.0).astype(np.int64) % 2)
    ph = 2.0 * np.pi * (((IF2 + doppler_hz) / FS2 * m + 0.123) % 1.0)
    iq = np.zeros(2 * n_samples, np.int8)
    iq[0::2], iq[1::2] = np.rint(100 * bit * chip * np.cos(ph)), np.rint(100 * bit * chip * np.sin(ph))
    return iq


@pytest.fixture(scope="module")
def clean():
    """blocks 3 (58 segments), PRN 9 at grid point -34 plus 30 Hz, code phase 3 samples: code period k starts 3 samples before
    segment k, so the bits flip at segments 7, 27 and 47"""
    lo = -34
    return dict(iq=clean_iq(3 * 40000 + 64, 9, lo * STEP2 + FINE_HZ, 3.0, EDGE), lo=lo, dop=lo * STEP2 + FINE_HZ)


def clean_record(c, law=qr.LAW):
    return qr.aided_coh_search(c["iq"], 81920, [(0, 8)], [dict(flags=0, ca_center=3, lo_center=c["lo"])], SPM2, FC2, FS2, KMAX2, signed=True,
                               mix_hz=FC2 - IF2, multibit=REAL, blocks=3, code_half=5, dop_half=0, fine_half=3, fine_step=10, ratio_min=3.0, law=law,
                               stream=True)[0]


class ShiftFirst(qr.Law):
    def period_value(self, terms):
        return sum(t >> 14 for t in terms)  # the shift before the sum


class RotationSign(qr.Law):
    def rotate(self, i, q, c, s):
        return i * c - q * s, q * c + i * s  # turned forward


class UnitFloor(qr.Law):
    def floor_of(self, vi, vq, o, segments, spm):
        return 2 * spm * segments  # the 1-bit section's floor


class EdgeFromTheEnd(qr.Law):
    def boundaries(self, e, m, n_seg):
        return sorted({0, n_seg} | {s for s in range(1, n_seg) if s % m == (m - e) % m})  # e counted from the period's end


def test_fine_doppler_sign_and_bit_edge(clean):
    r = clean_record(clean)
    step = 10 / 1024.0 * (FS2 / SPM2)
    print("clean signal at %.2f Hz: doppler_hz %.2f (best_f %d, fine step %.2f Hz), best_e %d, best_h %d, ratio %.1f against non-coherent %.1f" % (
        clean["dop"], r["doppler_hz"], r["best_f"], step, r["best_e"], r["best_h"], r["ratio"], r["noncoh"] / r["floor"]))
    assert r["flags"] == 0 and r["best_h"] == 5 and r["ca_shift"] == 3 and r["best_e"] == EDGE
    assert abs(r["doppler_hz"] - clean["dop"]) <= step / 2 and r["best_f"] == 3 + 3
    assert r["ratio"] > 10.0 * r["noncoh"] / r["floor"]  # 7, 20, 20 and 11 segments add coherently


@pytest.mark.parametrize("wrong", [ShiftFirst, RotationSign, UnitFloor, EdgeFromTheEnd])
def test_wrong_laws_are_told_from_the_right_one(clean, wrong):
    right, other = clean_record(clean), clean_record(clean, law=wrong())
    differs = [f for f in qr.INT_FIELDS + ("ratio", "doppler_hz") if right[f] != other[f]] + ([] if np.array_equal(right["powers"], other["powers"]) else ["powers"])
    print("%s: right law best_f %d best_e %d best %d floor %d; wrong law best_f %d best_e %d best %d floor %d; differs in %s" % (
        wrong.__name__, right["best_f"], right["best_e"], right["best"], right["floor"], other["best_f"], other["best_e"], other["best"], other["floor"], differs))
    assert (right["best_f"], right["best_e"]) == (6, EDGE)
    expected = {"ShiftFirst": "best", "RotationSign": "best_f", "UnitFloor": "floor", "EdgeFromTheEnd": "best_e"}
    assert expected[wrong.__name__] in differs


# ---- 5. the gain over the sign path, references alone ------------------------------------------------------------------------------
WEAK = 0.0337  # tests/test_aided_coh.py's


def test_the_gain_over_the_sign_path():
    """tests/test_aided_coh.py's scene -- five satellites at amplitude 0.2 with navigation bits (16 per satellite, seed 5), the sixth
    at WEAK, two absent PRNs, 16 blocks at 5.456 MHz, noise seed 2024 -- written as an 8-bit IQ capture by tests/gen_ref.py (IF 0.4
    MHz, scale 16, sigma 1, int8) and searched with the defaults' window both ways on the same bytes: the multi-bit reference, and
    tests/iq_ref.py's conversion followed by tests/aided_coh_ref.py.  The measure is the weak satellite's ratio divided by the larger
    absent ratio of the same search: it must be larger multi-bit, and both searches must put their best at the true code phase.
    Measured here on the CPU (printed by this test): the weak satellite reads 28.19 multi-bit (absent PRNs 3.36 and 7.35:
    quotient 3.835) and 10.64 through the sign path (absent PRNs 3.11 and 3.89: quotient 2.738), ca_shift 4627 and 4626 against the
    law's 4626.77, doppler_hz 384.8 both ways against the generator's 389.8, best_e 7 both ways.  No threshold is named: the
    measured default of the multi-bit path, 28.56, lies just above this amplitude's ratio."""
    geo, sel, present, absent, dops = ac.scene_sats(weak=WEAK)
    nav = (1 - 2 * np.random.default_rng(5).integers(0, 2, (len(present), 16))).astype(np.int8)
    g = gen_ref.LAW.iq8(ac.FS, present, ic.IF_HZ, ic.SCALE, 1.0, 2024, 0, 16 * 40960, nav=nav)
    iq = gen_ref.LAW.quantise(g["v"], True).ravel()
    chans = [present[5]] + absent
    aid = []
    for s in chans:
        ca, lo = ac.law_center(s, 0)
        aid.append(dict(flags=0, ca_center=int(round(ca)) % ac.SPM, lo_center=int(round(lo))))
    tasks = [(0, s[0] - 1) for s in chans]
    mix = ac.FC - ic.IF_HZ
    multi = qr.aided_coh_search(iq, 81920, tasks, aid, ac.SPM, ac.FC, ac.FS, ac.KMAX, signed=True, mix_hz=mix, multibit=REAL, stream=True, ratio_min=0.0)
    bits = iq_ref.bits(iq.view(np.uint8), True, (0.0, 0.0), mix, ac.FS)
    sign = aided_coh_ref.aided_coh_search(bits, 5120, tasks, aid, ac.SPM, ac.FC, ac.FS, ac.KMAX, ratio_min=0.0)
    ca_law, lo_law = ac.law_center(chans[0], 0)
    q_multi = multi[0]["ratio"] / max(multi[1]["ratio"], multi[2]["ratio"])
    q_sign = sign[0]["ratio"] / max(sign[1]["ratio"], sign[2]["ratio"])
    print("amplitude %g: multi-bit weak %.4f absent %.4f %.4f quotient %.3f; sign path weak %.4f absent %.4f %.4f quotient %.3f" % (
        WEAK, multi[0]["ratio"], multi[1]["ratio"], multi[2]["ratio"], q_multi, sign[0]["ratio"], sign[1]["ratio"], sign[2]["ratio"], q_sign))
    print("weak PRN: ca_shift %d multi-bit, %d sign path (law %.2f); doppler_hz %.1f and %.1f (generator %.1f); best_e %d and %d" % (
        multi[0]["ca_shift"], sign[0]["ca_shift"], ca_law, multi[0]["doppler_hz"], sign[0]["doppler_hz"], chans[0][2], multi[0]["best_e"], sign[0]["best_e"]))
    for r in (multi[0], sign[0]):
        assert abs((r["ca_shift"] - ca_law + ac.SPM / 2) % ac.SPM - ac.SPM / 2) <= 1.0
    assert q_multi > q_sign
