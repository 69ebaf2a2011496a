"""tests/aided_iq_ref.py, the reference of "Aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, checked on the CPU before
the kernel is held against it (tests/test_gpu_aided_iq.py): its plain sums against its quick spelling, the measured floor on +-1
bytes and against random replicas, wrong readings of the text told from the right one, sign mode against tests/aided_ref.py, and the
gain over the sign path on captures made by tests/gen_ref.py.  Each test prints what it measured before it asserts (pytest -s)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

import aided_iq_cases as ic
import aided_iq_ref
import aided_ref
import gen_ref
import iq_ref
import refine_iq_ref
import track_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from iq8_oracle import iq8_to_bits  # noqa: E402

FS2, FC2, SPM2 = 2.046e6, 0.4e6, 2046  # the small window: two samples per chip
KMAX2 = int(5000.0 / (FS2 / 40000))
REAL, COMPLEX = ic.REAL, ic.COMPLEX


def random_iq(n_samples, seed):
    return np.random.default_rng(seed).integers(0, 256, 2 * n_samples, dtype=np.uint8)


# ---- the library's host-only side ----------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("hip_artifacts")
def test_defaults_and_the_abi():
    import gpsacq
    lib = gpsacq.load_library()
    s, one = gpsacq.aided_params_iq8(), gpsacq.aided_params()
    got = tuple(s[0].tolist())
    print("defaults:", got)
    assert got == (16, 1, 16, 1, gpsacq.THRESHOLD, aided_iq_ref.RATIO_MIN) and got[:5] == tuple(one[0].tolist())[:5]
    assert tuple(gpsacq.aided_params_iq8(blocks=3, ratio_min=2.0)[0].tolist()) == (3, 1, 16, 1, gpsacq.THRESHOLD, 2.0)
    with pytest.raises(ValueError):
        gpsacq.aided_params_iq8(code_half=128)
    assert lib.gpsacq_aided_default_params_iq8(None) == 1
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf, aid, pk, out = np.zeros(64, np.uint8), np.zeros(2, gpsacq.AID_DTYPE), np.zeros(2, gpsacq.PEAK_DTYPE), np.zeros(2, gpsacq.AIDED_DTYPE)
    inp = gpsacq.Iq8Input()
    fix, eph = np.zeros(2, gpsacq.FIX_DTYPE), np.zeros(1, gpsacq.EPHEMERIS_DTYPE)
    assert lib.gpsacq_aided_search_iq8(None, ctypes.byref(inp), p(buf), 32, 81920, None, p(aid), None, 2, None, p(out), p(pk), None) == 1
    assert lib.gpsacq_aided_search_iq8_device(None, ctypes.byref(inp), p(buf), 32, 81920, None, p(aid), None, 2, None, p(out), p(pk), None, 1) == 1
    assert lib.gpsacq_aided_peaks_iq8_device(None, p(eph), 1, p(fix), None, ctypes.byref(inp), p(buf), 32, 81920, None, None, 2, 1, None, None, None, p(out),
                                             p(pk), 1) == 1
    assert lib.gpsacq_aided_iq8_last_ms(None, None, None, None) == 1 and b"gpsacq_aided_iq8_last_ms" in lib.gpsacq_last_error()
    assert not out.view(np.uint8).any() and not pk.view(np.uint8).any()


# ---- plain against quick spelling ------------------------------------------------------------------------------------------------
# format, mean, REAL / COMPLEX and the carrier's sign: if_hz = fc - mix_hz (REAL) or -mix_hz (COMPLEX) is where the Doppler-free carrier
# sits, and the last two put it below zero
SPELLINGS = [(False, True, REAL, FC2 - 0.3e6, 777), (True, False, REAL, FC2 + 0.2e6, 3), (False, False, COMPLEX, -0.25e6, SPM2 - 2),
             (True, True, COMPLEX, 0.35e6, 1500), (True, True, REAL, FC2 + 0.35e6, 0)]


@pytest.mark.parametrize("signed,dc,multibit,mix_hz,ca_center", SPELLINGS)
def test_plain_sums_against_the_quick_spelling(signed, dc, multibit, mix_hz, ca_center):
    iq = random_iq(3 * 40960 + 333, 7)
    tasks = [(0, 11), (1, 31)]
    aid = [dict(flags=0, ca_center=ca_center, lo_center=23), dict(flags=0, ca_center=ca_center, lo_center=-KMAX2)]
    kw = dict(signed=signed, mean=ic.MEAN if dc else None, mix_hz=mix_hz, multibit=multibit, blocks=2, code_half=5, dop_half=1, ratio_min=0.0)
    plain = aided_iq_ref.aided_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, **kw)
    quick = aided_iq_ref.aided_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, stream=True, **kw)
    f = aided_iq_ref.LAW.carrier_hz(0.0, mix_hz, FC2, multibit)
    for a, b in zip(plain, quick):
        assert np.array_equal(a["powers"], b["powers"]) and {k: v for k, v in a.items() if k != "powers"} == {k: v for k, v in b.items() if k != "powers"}
        assert a["flags"] == 0 and a["segments"] == 2 * 40000 // SPM2 and a["best"] == int(a["powers"].max()) and a["floor"] > 0
        assert a["total"] == sum(int(x) for x in a["powers"].ravel())
    rows = sum(int(not plain[1]["powers"][d].any()) for d in range(3))
    print("%s dc %d multibit %d, carrier at %+.0f Hz: 2 x 33 powers, records and peaks alike; ratios %.3f %.3f; %d row of invalid d" %
          ("S8" if signed else "U8", dc, multibit, f, plain[0]["ratio"], plain[1]["ratio"], rows))
    assert rows == 1  # lo_center = -kmax: d = 0 is off the grid
    assert (f < 0) == (mix_hz > (0.0 if multibit == COMPLEX else FC2))


# ---- the floor -------------------------------------------------------------------------------------------------------------------
def test_the_floor_on_plus_minus_one_bytes():
    """v_i = +-1, v_q = 0: the measured floor is the 2 * spm * segments of gpsacq_aided_search, for S8 and for U8"""
    rng = np.random.default_rng(3)
    n = 40960 + 100
    iq = np.zeros(2 * n, np.int8)
    iq[0::2] = 1 - 2 * rng.integers(0, 2, n)
    aid = [dict(flags=0, ca_center=100, lo_center=0)]
    for raw, signed in ((iq, True), (ic.as_u8(iq), False)):
        r = aided_iq_ref.aided_search(raw, 81920, [(0, 4)], aid, SPM2, FC2, FS2, KMAX2, signed=signed, blocks=1, code_half=1, dop_half=0, stream=True)[0]
        assert r["segments"] == 19 and r["floor"] == 2 * SPM2 * r["segments"] == aided_ref.LAW.floor_of(SPM2, r["segments"])
    print("+-1 bytes: floor %d = 2 * %d * %d" % (r["floor"], SPM2, r["segments"]))


def test_the_floor_against_random_replicas():
    """E[I^2 + Q^2] over +-1 replicas drawn independently of the samples is 2 * sum (v_i^2 + v_q^2), exactly; the mean over N draws
    has the sampling error of N terms that are each a sum of two squared near-Gaussian sums, (I^2 + Q^2) with I, Q of variance
    sigma^2 = sum (v_i^2 + v_q^2) and uncorrelated: Var(I^2 + Q^2) = 2 sigma^4 + 2 sigma^4 = (2 sigma^2)^2 = floor^2 per segment.
    One segment, N = 4000 draws, seed fixed: the mean lies within 4 / sqrt(N) = 6.3 % of the floor (four standard errors)."""
    spm, N = 2046, 4000
    rng = np.random.default_rng(12)
    vi, vq = refine_iq_ref.samples(random_iq(spm, 5), False, ic.MEAN)
    C, S = aided_iq_ref.LAW.carrier((np.arange(spm, dtype=np.int64) * 123456789) % 2 ** 32)
    re_, im_ = aided_iq_ref.LAW.arms(vi, vq, C, S)
    floor = aided_iq_ref.LAW.floor_of(vi, vq, 0, 1, spm)
    h = 1 - 2 * rng.integers(0, 2, (N, spm))
    I, Q = h @ re_, h @ im_
    mean = float((I * I + Q * Q).mean())
    print("floor %d, mean of I^2 + Q^2 over %d random replicas %.0f: ratio %.4f (bound 1 +- %.4f)" % (floor, N, mean, mean / floor, 4 / math.sqrt(N)))
    assert int((re_ * re_).sum() + (im_ * im_).sum()) == floor  # exact: the cross terms cancel between I and Q
    assert abs(mean / floor - 1.0) <= 4 / math.sqrt(N)


# ---- wrong laws ------------------------------------------------------------------------------------------------------------------
class PhasePerSegment(aided_iq_ref.Law):
    def carrier_sample(self, j, spm):
        return j % spm  # the carrier counted from the segment


class ReducedIndex(aided_iq_ref.Law):
    def code_index(self, base, h, spm):
        return (base + h) % spm


class SSign(aided_iq_ref.Law):
    def carrier(self, ph):
        C, S = super().carrier(ph)
        return C, -S


class HalfFloor(aided_iq_ref.Law):
    def floor_of(self, vi, vq, o, segments, spm):
        return super().floor_of(vi, vq, o, segments, spm) // 2


class ByteStride(aided_iq_ref.Law):
    def window_start(self, block, stride):
        return block * stride  # stride instead of stride / 2


class FcInComplex(aided_iq_ref.Law):
    def carrier_hz(self, lo_dop, mix_hz, fc, multibit):
        return lo_dop - mix_hz + fc


class HSign(aided_iq_ref.Law):
    def code_index(self, base, h, spm):
        return base - h + 2 * spm  # the replica of h taken at sample j - h


def clean_iq(n_samples, first, prn, doppler_hz, code_phase_samples, if_hz):
    """the generator's law without noise, one satellite, as int8 I, Q at fs = 2.046 MHz: amplitude 100"""
    m = first + np.arange(n_samples, dtype=np.float64)
    idx = np.floor((m + code_phase_samples) * (ic.CPS * (1.0 + doppler_hz / ic.L1) / FS2)).astype(np.int64) % 1023
    chip = 1.0 - 2.0 * track_ref.chips(prn)[idx]
    ph = 2.0 * np.pi * (((if_hz + doppler_hz) / FS2 * m + 0.123) % 1.0)
    iq = np.zeros(2 * n_samples, np.int8)
    iq[0::2], iq[1::2] = np.rint(100 * chip * np.cos(ph)), np.rint(100 * chip * np.sin(ph))
    return iq


@pytest.mark.parametrize("wrong,multibit", [(PhasePerSegment, REAL), (ReducedIndex, REAL), (SSign, REAL), (HalfFloor, REAL), (ByteStride, REAL),
                                            (FcInComplex, COMPLEX), (HSign, REAL), (FcInComplex, REAL)])
def test_wrong_laws_are_told_from_the_right_one(wrong, multibit):
    """a clean complex signal in block 1 whose code phase lies 3 samples past the prediction and just below the wrap (base + h
    crosses spm inside the window), at a Doppler of -34 bins, predicted one bin too high: the right law finds it at best_h = W + 3
    with nearly all the floor's spm-fold in it.  (FcInComplex, REAL) is the control: in REAL mode that law IS the right one."""
    W, K, lo_true, if_hz = 5, 1, -34, 0.3e6
    prn = next(p for p in range(1, 33) if track_ref.chips(p)[0] != track_ref.chips(p)[1022])
    ca_true = SPM2 - 1
    dop = lo_true * FS2 / 40000
    cps = ic.CPS * (1.0 + dop / ic.L1) / FS2
    stride = 81920
    first = stride // 2  # block 1 starts here; the code phase is ca_true there
    code_phase = ca_true * (ic.CPS / FS2) / cps - first
    iq = clean_iq(first + 2 * 40000 + 64, 0, prn, dop, code_phase, if_hz)
    aid = [dict(flags=0, ca_center=ca_true - 3, lo_center=lo_true + 1)]
    kw = dict(signed=True, mix_hz=ic.mix_of(multibit, if_hz, FC2), multibit=multibit, blocks=2, code_half=W, dop_half=K, ratio_min=3.0)
    right = aided_iq_ref.aided_search(iq, stride, [(1, prn - 1)], aid, SPM2, FC2, FS2, KMAX2, **kw)[0]
    other = aided_iq_ref.aided_search(iq, stride, [(1, prn - 1)], aid, SPM2, FC2, FS2, KMAX2, law=wrong(), **kw)[0]
    print("%s: right law best (h %d, d %d) ca %d lo %d ratio %.1f; wrong law flags %d (h %d, d %d) ca %d lo %d ratio %.1f" % (
        wrong.__name__, right["best_h"], right["best_d"], right["ca_shift"], right["lo_shift"], right["ratio"], other["flags"], other["best_h"],
        other["best_d"], other["ca_shift"], other["lo_shift"], other["ratio"]))
    assert right["flags"] == 0 and (right["best_h"], right["ca_shift"]) == (W + 3, ca_true) and right["ratio"] > 0.5 * SPM2
    differs = [f for f in aided_ref.INT_FIELDS + ("ratio",) if right[f] != other[f]] + ([] if np.array_equal(right["powers"], other["powers"]) else ["powers"])
    print("   differs in", differs)
    assert bool(differs) == (not (wrong is FcInComplex and multibit == REAL)), wrong.__name__


# ---- sign mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc", [(False, True), (True, False)])
def test_sign_mode_is_the_one_bit_reference(signed, dc):
    """GPSACQ_SAMPLES_SIGN through the reference: tests/iq_ref.py's bits, packed, into tests/aided_ref.py with n_bytes = ceil(n_samples / 8)
    and stride / 16"""
    n_samples = 2 * 40960 + 77
    iq = random_iq(n_samples, 9)
    tasks = [(0, 11), (1, 0), (3, 5)]
    aid = [dict(flags=0, ca_center=777, lo_center=23), dict(flags=0, ca_center=1, lo_center=-KMAX2), dict(flags=0, ca_center=9, lo_center=0)]
    mean = ic.MEAN if dc else None
    mix = FC2 - 0.3e6
    got = aided_iq_ref.aided_search(iq, 81920, tasks, aid, SPM2, FC2, FS2, KMAX2, signed=signed, mean=mean, mix_hz=mix, multibit=0, blocks=2, code_half=5,
                                    ratio_min=1.0, stream=True)
    bits = iq_ref.bits(iq, signed, ic.MEAN if dc else (0.0, 0.0), mix, FS2)
    assert bits.size == (n_samples + 7) // 8
    want = aided_ref.aided_search(bits, 5120, tasks, aid, SPM2, FC2, FS2, KMAX2, blocks=2, code_half=5, ratio_min=1.0, stream=True)
    for a, b in zip(got, want):
        assert np.array_equal(a["powers"], b["powers"]) and {k: v for k, v in a.items() if k != "powers"} == {k: v for k, v in b.items() if k != "powers"}
    print("sign mode %s dc %d: flags %s, floors %s" % ("S8" if signed else "U8", dc, [r["flags"] for r in got], [r["floor"] for r in got]))
    assert [r["flags"] & 2 for r in got] == [0, 0, 2] and got[0]["floor"] == 2 * SPM2 * got[0]["segments"] and got[1]["flags"] & aided_ref.SHORT


# ---- the gain, references alone --------------------------------------------------------------------------------------------------
SEEDS = (2024, 2025, 2026)


@pytest.fixture(scope="module")
def gain_scene():
    """aided_iq_cases' scene by tests/gen_ref.py, three captures of 16 blocks (seeds 2024 to 2026): five satellites at 0.2, one at
    WEAK_AMPLITUDE, two absent PRNs; each searched with the defaults both ways on the same bytes: multi-bit (aided_iq_ref) and the
    sign path (iq8_oracle's conversion, then aided_ref).  Computed once."""
    sats = ic.weak_sats()
    chans = [sats[5]] + ic.ABSENT
    aid = []
    for s in chans:
        ca, lo = ic.law_center(s, 0)
        aid.append(dict(flags=0, ca_center=int(round(ca)) % ic.SPM, lo_center=int(round(lo))))
    tasks = [(0, s[0] - 1) for s in chans]
    rows = []
    for seed in SEEDS:
        g = gen_ref.LAW.iq8(ic.FS, sats, ic.IF_HZ, ic.SCALE, 1.0, seed, 0, 16 * 40960)
        iq = gen_ref.LAW.quantise(g["v"], True).ravel()
        mix = ic.FC - ic.IF_HZ
        multi = aided_iq_ref.aided_search(iq, 81920, tasks, aid, ic.SPM, ic.FC, ic.FS, ic.KMAX, signed=True, mix_hz=mix, multibit=REAL, stream=True)
        bits = iq8_to_bits(iq, signed=True, remove_dc=False, mix_hz=mix, fs=ic.FS)
        sign = aided_ref.aided_search(bits, 5120, tasks, aid, ic.SPM, ic.FC, ic.FS, ic.KMAX, stream=True)
        rows.append(dict(seed=seed, multi=multi, sign=sign))
    return dict(rows=rows, law=ic.law_center(chans[0], 0))


def test_the_gain_over_the_sign_path(gain_scene):
    """fs = 5.456 MHz, 16-block windows, the defaults of either path, WEAK_AMPLITUDE = 0.04.  Measured here on the CPU (printed by this
    test): the weak satellite reads 4.18, 3.83 and 4.40 multi-bit against 2.03, 1.96 and 1.99 through the sign path, both at the true
    code phase; the excess over 1 is 3.09, 2.95 and 3.42 times the sign path's, median 3.09 (4.9 dB).  The test asserts a median gain
    above 1 + half the measured excess, 2.045.  The absent PRNs read 1.39 to 2.01 multi-bit: none is detected at the recorded default
    ratio_min of 3.44.  (Amplitude 0.03 read 2.67 to 3.07 against 1.58 to 1.70 and 0.05 read 5.45 to 6.09 against 2.44 to 2.49.)"""
    gains = []
    ca_law, lo_law = gain_scene["law"]
    for r in gain_scene["rows"]:
        m, s = r["multi"], r["sign"]
        gain = (m[0]["ratio"] - 1.0) / (s[0]["ratio"] - 1.0)
        gains.append(gain)
        print("seed %d: weak PRN multi-bit ratio %.4f (ca_shift %d, law %.2f), sign path %.4f (ca_shift %d): gain %.3f; absent PRNs multi-bit %.4f %.4f, "
              "sign path %.4f %.4f" % (r["seed"], m[0]["ratio"], m[0]["ca_shift"], ca_law, s[0]["ratio"], s[0]["ca_shift"], gain, m[1]["ratio"], m[2]["ratio"],
                                       s[1]["ratio"], s[2]["ratio"]))
        assert abs((m[0]["ca_shift"] - ca_law + ic.SPM / 2) % ic.SPM - ic.SPM / 2) <= 1.0 and abs(m[0]["lo_shift"] - lo_law) <= 1.5
        assert m[0]["flags"] == 0 and m[0]["ratio"] >= aided_iq_ref.RATIO_MIN
        assert m[1]["flags"] == m[2]["flags"] == aided_iq_ref.BELOW and m[1]["peak"] == m[2]["peak"] == (0.0, 0, 0, 0.0)  # no absent PRN is detected
    med = float(np.median(gains))
    print("median gain %.3f (%.1f dB); ratio_min %.3f multi-bit, %.3f sign path" % (med, 10 * math.log10(med), aided_iq_ref.RATIO_MIN, aided_ref.RATIO_MIN))
    assert 0.03 <= ic.WEAK_AMPLITUDE <= 0.05
    assert med > 1.0 + 0.5 * (3.09 - 1.0)
