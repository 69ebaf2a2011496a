"""tests/refine_ref.py, the reference of gpsacq_refine ("Fine code phases: search peaks refined below a sample" of
include/gpsacq.h), checked on the CPU before the kernel is held against it (tests/test_gpu_refine.py): its sums against
tests/track_ref.py where the two models coincide and against a plain double loop where they do not, its estimate against a signal
whose code phase is known, and the argument checks of gpsacq.refine_params.  fs = 2.046 MHz, so that spm = 2046."""
import numpy as np
import pytest

import refine_ref
import track_ref

FS, FC, SPM = 2.046e6, 0.4e6, 2046
TWO32, FULL = 2 ** 32, 1023 * 2 ** 32

# What the estimator recovers of a noise-free code phase at fs = 2.046 MHz (two samples per chip), a window of 16 blocks,
# d = 0.25: measured by test_known_code_phases below as 0.0107 chips at the worst of the five phases (0.0, +-0.3, +-0.49
# samples: 0.0006, 0.0107, 0.0107, 0.0009, 0.0010); the constant leaves a quarter on top.  Whole-sample phases are off by up to
# 0.49 samples = 0.245 chips here.  The Doppler of that test, 48 bins = 2455 Hz, slides the code by 0.499 chips over the window:
# one period of the two-samples-per-chip staircase.  At 40 bins (0.415 chips, not a whole period) the same phases measured
# 0.046 chips at the worst: what the staircase leaves where the slide does not cover it evenly.
KNOWN_PHASE_TOL_CHIPS = 0.0135


def random_bits(n_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)


def test_one_segment_is_a_tracking_epoch():
    """ca_shift = 0, a negative lo_shift (the code NCO below 1/2 chip per sample: 2046 samples stay inside one period) and d = 0.5:
    the segment is an epoch of THE CHANNEL MODEL that starts at chip 0 with lo_phase 0"""
    bits = random_bits(5120, 1)
    ok, lo_rate, ca_rate = refine_ref.nco_words(-37, FC, FS)
    assert ok and ca_rate < TWO32 // 2 and (SPM - 1) * ca_rate < FULL
    s01 = np.unpackbits(bits, bitorder="little")
    for prn, o in ((1, 0), (32, 8 * 301)):
        got = refine_ref.segment_sums(s01, o, 1, SPM, prn, lo_rate, ca_rate, 0, TWO32 // 2)
        want = track_ref.epoch_sums(s01, 0, prn, [o], [SPM], [0], [lo_rate], [0], [ca_rate])
        assert got.tolist() == want.tolist()
        assert np.abs(got).max() > 0


def loop_sums(s01, o, segments, prn, lo_rate, ca_rate, P0, D):
    """step 4 as a double loop over segments and samples in Python integers, the carrier bits by THE CHANNEL MODEL's bit formulas"""
    c = track_ref.chips(prn).tolist()
    out = []
    for s in range(segments):
        acc = [0] * 6
        for i in range(SPM):
            j = s * SPM + i
            x = int(s01[o + j])
            ph = (j * lo_rate) % TWO32
            cos_bit, sin_bit = ((ph >> 31) ^ (ph >> 30)) & 1, 1 - (ph >> 31)
            P = (P0 + j * ca_rate) % FULL
            for k, X in enumerate(((P + D) % FULL, P, (P - D) % FULL)):
                chip = c[X >> 32]
                acc[2 * k] += 1 - 2 * (x ^ chip ^ cos_bit)
                acc[2 * k + 1] += 1 - 2 * (x ^ chip ^ sin_bit)
        out.append(acc)
    return out


def test_three_segments_against_a_double_loop():
    """ca_shift = spm - 1: the prompt wraps one sample into every segment, the early replica before it; 3 x 2046 < 40000, so
    blocks = 1 would give 19 segments -- the capture is cut so that three fit (SHORT)"""
    n_bytes = (8 * 7 + 3 * SPM + 100 + 7) // 8
    bits = random_bits(n_bytes, 2)
    ok, lo_rate, ca_rate = refine_ref.nco_words(23, FC, FS)
    P0 = ((SPM - 1) * ca_rate) % FULL
    assert ok and P0 + ca_rate >= FULL  # the wrap comes with the second sample
    s01 = np.unpackbits(bits, bitorder="little")
    D = TWO32 // 4
    got = refine_ref.segment_sums(s01, 56, 3, SPM, 7, lo_rate, ca_rate, P0, D)
    want = loop_sums(s01, 56, 3, 7, lo_rate, ca_rate, P0, D)
    assert got.tolist() == want
    # and the record made of them
    rec = refine_ref.refine(bits, 7, [(1, 6)], [(30.0, 23, SPM - 1, 0.0)], SPM, FC, FS, blocks=1, min_segments=4, snr_min=25.0)[0]
    assert rec["segments"] == 3 and rec["flags"] == refine_ref.SHORT | refine_ref.FEW and not refine_ref.usable(rec)
    assert (rec["lo_rate"], rec["ca_rate"]) == (lo_rate, ca_rate)
    for k, name in enumerate(("early", "prompt", "late")):
        assert rec[name] == sum(r[2 * k] ** 2 + r[2 * k + 1] ** 2 for r in want)
    off, tx = refine_ref.estimate(rec["early"], rec["late"], P0, D)
    assert (rec["offset_chips"], rec["tx_frac"]) == (off, tx) and 0.0 <= tx < 1e-3 and abs(off) <= 0.75


def clean_signal(n_samples, prn, doppler_hz, code_phase_samples, carrier_phase):
    """gpsacq_generate's law without noise, one satellite, in float64: bit = chip * cos(2 pi ((fc + doppler) / fs m + phase)) < 0,
    chip index floor((m + code_phase) * 1.023e6 (1 + doppler / L1) / fs) mod 1023"""
    m = np.arange(n_samples, dtype=np.float64)
    idx = np.floor((m + code_phase_samples) * (refine_ref.CPS * (1.0 + doppler_hz / refine_ref.L1) / FS)).astype(np.int64) % 1023
    chip = 1.0 - 2.0 * track_ref.chips(prn)[idx]
    y = chip * np.cos(2.0 * np.pi * (((FC + doppler_hz) / FS * m + carrier_phase) % 1.0))
    return np.packbits((y < 0.0).astype(np.uint8), bitorder="little")


def test_known_code_phases():
    lo_shift, prn, ca_shift = 48, 12, 777
    dop = lo_shift * FS / 40000  # on the grid: 2455 Hz, 1.59 chips/s of code Doppler
    window_s = 16 * 40000 / FS
    assert dop / 1540.0 * window_s > 1.0 / 16  # the code slides by more than 1/16 chip over the window
    cps = refine_ref.CPS * (1.0 + dop / refine_ref.L1) / FS
    worst = 0.0
    for frac in (0.0, 0.3, -0.3, 0.49, -0.49):
        cp = ca_shift + frac
        bits = clean_signal(16 * 40000 + 64, prn, dop, cp, 0.123)
        rec = refine_ref.refine(bits, 5120, [(0, prn - 1)], [(100.0, lo_shift, ca_shift, 0.0)], SPM, FC, FS)[0]
        assert rec["flags"] == 0 and rec["segments"] == 16 * 40000 // SPM
        assert rec["prompt"] > min(rec["early"], rec["late"])
        want = (cp * cps) % 1023.0
        err = (rec["tx_frac"] * 1.023e6 - want + 511.5) % 1023.0 - 511.5
        whole = ((ca_shift * cps) % 1023.0 - want + 511.5) % 1023.0 - 511.5
        print("code phase %+.2f samples: fine %+.4f chips (offset %+.4f), whole-sample %+.4f chips" % (frac, err, rec["offset_chips"], whole))
        worst = max(worst, abs(err))
    print("worst %.4f chips, KNOWN_PHASE_TOL_CHIPS %.4f" % (worst, KNOWN_PHASE_TOL_CHIPS))
    assert worst <= KNOWN_PHASE_TOL_CHIPS


def test_no_hit_and_no_power():
    bits = random_bits(2 * 5120, 3)
    pk = lambda snr=30.0, lo=0, ca=5: (snr, lo, ca, 0.0)
    cases = [(pk(snr=24.9), (0, 0)), (pk(snr=float("nan")), (0, 0)), (pk(ca=-1), (0, 0)), (pk(ca=SPM), (0, 0)), (pk(), (2, 0)), (pk(), (-1, 0)),
             (pk(), (0, 32)), (pk(), (0, -1)), (pk(lo=40000), (0, 0)), (pk(lo=-40000), (0, 0))]
    recs = refine_ref.refine(bits, 5120, [c[1] for c in cases], [c[0] for c in cases], SPM, FC, FS, blocks=1)
    zero = dict(flags=refine_ref.NO_HIT, segments=0, lo_rate=0, ca_rate=0, early=0, prompt=0, late=0, offset_chips=0.0, tx_frac=0.0)
    assert all(r == zero for r in recs)
    # a capture that ends inside the first segment: no segment, no power
    rec = refine_ref.refine(bits, 5120, [(1, 3)], [pk()], SPM, FC, FS, blocks=1, n_bytes=5120 + 200)[0]
    assert rec["flags"] == refine_ref.SHORT | refine_ref.FEW | refine_ref.NO_POWER and rec["segments"] == 0 and rec["ca_rate"] > 0
    assert rec["tx_frac"] == 0.0 and not refine_ref.usable(rec)


@pytest.mark.usefixtures("hip_artifacts")
def test_refine_params_checks():
    import gpsacq
    p = gpsacq.refine_params()
    assert p.dtype == gpsacq.REFINE_PARAMS_DTYPE and p.itemsize == 24 and gpsacq.FINE_DTYPE.itemsize == 56
    assert (int(p["blocks"][0]), int(p["min_segments"][0]), float(p["half_spacing_chips"][0]), float(p["snr_min"][0])) == (16, 1, 0.25, gpsacq.THRESHOLD)
    q = gpsacq.refine_params(blocks=64, min_segments=100, half_spacing_chips=0.5, snr_min=-3.0)
    assert (int(q["blocks"][0]), int(q["min_segments"][0]), float(q["half_spacing_chips"][0]), float(q["snr_min"][0])) == (64, 100, 0.5, -3.0)
    assert float(gpsacq.refine_params(half_spacing_chips=1.0 / 64)["half_spacing_chips"][0]) == 1.0 / 64
    for bad in (dict(blocks=0), dict(blocks=65), dict(blocks=1.5), dict(min_segments=0), dict(half_spacing_chips=0.015), dict(half_spacing_chips=0.51),
                dict(half_spacing_chips=float("nan")), dict(snr_min=float("inf")), dict(snr_min=float("nan"))):
        with pytest.raises(ValueError):
            gpsacq.refine_params(**bad)
    with pytest.raises(TypeError):
        gpsacq.refine_params(spacing=0.25)
    assert (gpsacq.FINE_NO_HIT, gpsacq.FINE_SHORT, gpsacq.FINE_NO_POWER, gpsacq.FINE_FEW) == (refine_ref.NO_HIT, refine_ref.SHORT, refine_ref.NO_POWER,
                                                                                               refine_ref.FEW)
