"""Tracking channels on an 8-bit IQ capture, CPU side: the model of the multi-bit complex channel (tests/c/track_model_iq.c,
written from include/gpsacq.h) against a numpy restatement of its sums and against the 1-bit model on degenerate captures; the
host-only entry points; the ABI; and the model under the independent reference of tests/track_ref.py (complex integer samples)
over the scenarios of test_track_ref.sweep at 2.046 .. 40 MHz, with bytes on the rails (-128 included), means up to (-128, 127)
and carriers on both sides of zero; the supported-RMS boundary of gpsacq_track_default_params_iq8; lock from 60 Hz off at 10, 20
and 40 MHz.  The kernel itself is checked against this model in tests/test_gpu_track_iq.py and tests/test_gpu_track_iq_sweep.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import track_iq_helpers as iqh
from test_track_ref import FS_FC
from track_helpers import ROOT, run_model
from track_iq_helpers import host_capture, host_chan, numpy_epoch_sums, run_model_iq


def _params(fs, shift_down=0, fll_epochs=40):
    """gpsacq_track_default_params restated for fs <= 10 MHz, every loop shift lowered by shift_down (the CPU tests have no engine)"""
    import gpsacq
    nl = int(math.ceil(fs / 1000))
    r = nl / 10000
    adj = round(2.0 * math.log2(10000 / nl)) - shift_down
    return gpsacq.TrackParams(20 + adj, 27 + adj, 11 + adj, 23 + adj, 25 + adj, fll_epochs, -1, 250, int(1200 * 1200 * r * r * 2.0 ** shift_down),
                              int(1400 * 1400 * r * r * 2.0 ** shift_down), int(10000 / fs * 2 ** 64), int(4 * 10000 / 1540 / fs * 2 ** 64), nl // 2,
                              min(2 * nl, 65535))


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("dc", [(0, 0), (7, -5)])
def test_model_sums_match_numpy(signed, dc):
    """~120 epochs each of three channels (positive, negative and near-zero carrier) over a small noisy capture: every epoch's six
    sums, run one epoch at a time, equal the numpy restatement of the header's formulas; and one call equals the single steps."""
    fs, if_hz = 2.8e6, 41e3
    sats = [(5, 0.3, 1500.0, 700.0, 0.1), (12, 0.25, -2200.0, 1999.0, 0.6), (30, 0.2, 300.0, 2500.0, 0.3)]
    iq = host_capture(int(0.125 * fs), fs, sats, if_hz, 20.0, signed, seed=3 + signed, dc=(float(dc[0]), float(dc[1])))
    p = _params(fs, shift_down=10)
    start = np.concatenate([host_chan(5, fs, if_hz + 1500.0, 1500.0, 700.0, p.fll_epochs), host_chan(12, fs, -640e3, -2200.0, 1999.0, p.fll_epochs),
                            host_chan(30, fs, 150.0, 300.0, 2500.0, p.fll_epochs)])
    one = start.copy()
    _, rec1, ne1 = run_model_iq(iq, 0, signed, dc, one, p, 200)
    assert (ne1 > 110).all()
    step = start.copy()
    epochs = 0
    for c in range(3):
        for t in range(int(ne1[c])):
            ch = step[c:c + 1]
            n, want = numpy_epoch_sums(iq, 0, signed, dc, ch[0], int(ch["prn"][0]))
            first = int(ch["next_sample"][0])
            _, rec, ne = run_model_iq(iq, 0, signed, dc, ch, p, 1)
            assert ne[0] == 1 and int(ch["next_sample"][0]) == first + n
            r = rec[0, 0]
            assert [int(r[k]) for k in ("ie", "qe", "ip", "qp", "il", "ql")] == want, (c, t)
            assert r == rec1[c, t]
            epochs += 1
    assert epochs > 330
    assert step.tobytes() == one.tobytes()


def test_degenerate_capture_is_the_one_bit_model():
    """I = 1 - 2 bit, Q = 0 (int8, no mean removed) through the IQ model = tests/c/track_model.c on the bits: the same records and
    the same final state, same params -- the identity the header states."""
    fs, fc = 2.8e6, 0.7e6
    rng = np.random.default_rng(8)
    n = int(0.3 * fs) // 8 * 8
    m = np.arange(n)
    # a real-IF signal under noise, hard-limited: the 1-bit stream of gpsacq_generate's law (made here with numpy)
    from track_iq_helpers import CPS, L1, chips_pm1
    dop, cp = 2100.0, 1234.0
    q = np.floor((m + cp) * CPS * (1 + dop / L1) / fs).astype(np.int64)
    y = rng.standard_normal(n) + 0.3 * chips_pm1(9)[q % 1023] * np.cos(2 * np.pi * ((fc + dop) / fs * m + 0.2))
    bit = (y < 0).astype(np.uint8)
    bits = np.packbits(bit, bitorder="little")
    iq = np.zeros(2 * n, np.int8)
    iq[0::2] = 1 - 2 * bit.astype(np.int8)
    p = _params(fs)
    a = host_chan(9, fs, fc + 2100.0, dop, cp, p.fll_epochs)
    b = a.copy()
    pa, ra, na = run_model(bits, 0, a, p, 400)
    pb, rb, nb = run_model_iq(iq, 0, True, (0, 0), b, p, 400)
    assert na[0] == nb[0] and na[0] > 290
    assert ra[0, :na[0]].tobytes() == rb[0, :nb[0]].tobytes() and np.array_equal(pa, pb)
    assert a.tobytes() == b.tobytes()
    assert np.abs(pa[0, 150:na[0], 0]).mean() > 3 * np.abs(pa[0, 150:na[0], 1]).mean()  # and it is a locked channel, not noise


def test_model_windows_and_resume():
    """pieces whose starts are not multiples of 8 samples = one call; a max_epochs cut resumes"""
    fs = 2.8e6
    sats = [(5, 0.3, 1500.0, 700.0, 0.1)]
    iq = host_capture(int(0.1 * fs), fs, sats, -90e3, 12.0, False, seed=9, dc=(3.0, 2.0))
    p = _params(fs, shift_down=9)
    start = host_chan(5, fs, -90e3 + 1500.0, 1500.0, 700.0, p.fll_epochs)
    one = start.copy()
    _, rec1, ne1 = run_model_iq(iq, 0, False, (3, 2), one, p, 200)
    pieces, recs = start.copy(), []
    for end in (70001, 150003, iq.size // 2):
        first = int(pieces["next_sample"][0]) - 3
        _, r, ne = run_model_iq(iq[2 * first:2 * end], first, False, (3, 2), pieces, p, 200)
        recs.append(r[0, :ne[0]])
    assert pieces.tobytes() == one.tobytes() and np.array_equal(np.concatenate(recs), rec1[0, :ne1[0]])
    cut = start.copy()
    _, ra, na = run_model_iq(iq, 0, False, (3, 2), cut, p, 33)
    _, rb, nb = run_model_iq(iq, 0, False, (3, 2), cut, p, 200)
    assert na[0] == 33 and cut.tobytes() == one.tobytes()
    assert np.array_equal(np.concatenate([ra[0, :33], rb[0, :nb[0]]]), rec1[0, :ne1[0]])


@pytest.mark.usefixtures("hip_artifacts")
def test_accumulate_power_is_exact():
    import gpsacq
    lib = gpsacq.load_library()
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 256, 2 * 100003, dtype=np.uint8)
    for fmt, a in ((0, raw.astype(np.int64) - 128), (1, raw.view(np.int8).astype(np.int64))):
        pw = (ctypes.c_uint64 * 2)(5, 7)  # it adds to what is there
        assert lib.gpsacq_iq8_accumulate_power(None, raw.ctypes.data_as(ctypes.c_void_p), raw.size // 2, fmt, pw) == 0
        assert pw[0] == 5 + int((a[0::2] ** 2).sum()) and pw[1] == 7 + int((a[1::2] ** 2).sum())
    assert lib.gpsacq_iq8_accumulate_power(None, raw.ctypes.data_as(ctypes.c_void_p), 10, 5, pw) == 1  # unknown format
    assert lib.gpsacq_iq8_accumulate_power(None, None, 10, 0, pw) == 1


@pytest.mark.usefixtures("hip_artifacts")
def test_iq8_tracking_abi():
    """the new entry points are exported and declared, and no struct of the ABI changed size"""
    import gpsacq
    lib = gpsacq.load_library()
    header = open(os.path.join(ROOT, "include", "gpsacq.h")).read()
    for name in ("gpsacq_track_iq8", "gpsacq_track_iq8_device", "gpsacq_track_iq8_last_ms", "gpsacq_track_start_iq8", "gpsacq_track_default_params_iq8",
                 "gpsacq_iq8_accumulate_power", "gpsacq_generate_iq8_range", "gpsacq_generate_iq8_range_device"):
        assert hasattr(lib, name) and name in gpsacq.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert gpsacq.TRACK_CHAN_DTYPE.itemsize == 160 and gpsacq.TRACK_RECORD_DTYPE.itemsize == 40 and gpsacq.SUBFRAME_DTYPE.itemsize == 56
    assert ctypes.sizeof(gpsacq.TrackParams) == 72 and ctypes.sizeof(gpsacq.Iq8Input) == 64 and ctypes.sizeof(gpsacq.Handoff) == 32
    # the host-only entry points refuse a null engine before any device call
    p = gpsacq.TrackParams()
    assert lib.gpsacq_track_default_params_iq8(None, 16.0, ctypes.byref(p)) == 1
    ch = np.zeros(1, gpsacq.TRACK_CHAN_DTYPE)
    assert lib.gpsacq_track_start_iq8(None, None, 1, None, 0, None, ch.ctypes.data_as(ctypes.c_void_p)) == 1


# ---- the model under the independent reference ---------------------------------------------------------------------------------
_IDS = [f"{fs / 1e6:g}MHz" for fs, _ in FS_FC]


@pytest.mark.parametrize("fs", [fs for fs, _ in FS_FC], ids=_IDS)
def test_model_equals_reference_iq(fs):
    """tests/c/track_model_iq.c against track_ref.audit (every epoch's geometry and loop arithmetic, the final state; the six sums
    of every epoch below 10 MHz, of 30 seeded ones per channel from there on) over every scenario of the sweep.  First, on the
    inputs alone: at 2.046 .. 5.456 MHz at least 0.5 % of the bytes lie on a rail and both rails occur (measured 4.4 % at scale
    60 with no mean, half the bytes under the mean (-128, 127)), the window starts off the 8-sample grid and its byte count is
    2 .. 14 mod 16; then, on the model's reports, what each scenario aims at."""
    reps, sats, first, buf, case = iqh.sweep_iq(fs)
    lo, hi = iqh.rail_share(buf, case["signed"])
    print("fs %g scale %d dc %s signed %d if %.1f rms %.2f rails %.4f %.4f" % (fs, case["scale"], case["dc"], case["signed"], case["if_hz"], case["rms"], lo, hi))
    if fs <= 5.456e6:
        assert lo + hi >= 0.005 and lo > 0 and hi > 0, (lo, hi)
    assert first % 8 != 0 and np.asarray(buf).size % 16 == 2 * (1 + case["i"] % 7)
    assert case["rms"] < iqh.iq8_rms_bound(fs)
    iqh.check_sweep_reports(reps)
    r = {k: v[0] for k, v in reps.items()}
    assert sum(x["short_first"] for x in r["wrap"]) >= 2  # (a start past 1022.97 chips may land on the next period)


def test_branch_coverage_iq():
    """the census of test_track_ref.test_branch_coverage over the IQ sweep: every branch it aims at was taken somewhere, by
    channels of all 32 PRNs; and the rotation put every mean, both byte formats and carriers of both signs to work"""
    tot = dict(agc_down=0, agc_up=0, ring_wraps=0, fll_epochs=0, costas_epochs=0, costas_adj_epochs=0, aid=0, late_wrap=0, early_wrap=0,
               short_first=0)
    lost, stops, prns, dcs, fmts, signs = set(), set(), set(), set(), set(), set()
    for fs, _ in FS_FC:
        reps, sats, _, _, case = iqh.sweep_iq(fs)
        prns |= {s[0] for s in sats}
        dcs.add(case["dc"])
        fmts.add(case["signed"])
        signs |= {np.sign(case["if_hz"] + s[2]) for s in sats}
        for v in reps.values():
            for x in v[0]:
                for k in tot:
                    tot[k] += len(x[k]) if k == "aid" else int(x[k])
                lost |= x["lost"]
                stops.add(x["stop"])
    assert all(v > 0 for v in tot.values()), tot
    assert lost == {"lo_int", "lo_rate", "ca_int", "ca_rate", "min_epoch", "max_epoch"}
    assert stops == {"window", "max_epochs", "lost", "entered_lost"}
    assert prns == set(range(1, 33))
    assert dcs == set(iqh.IQ_DC) and fmts == {True, False} and signs == {-1.0, 1.0}


_ALL_FS = sorted(iqh.IQ_SCALE)


def test_default_params_iq8_boundary():
    """gpsacq_track_default_params_iq8, restated from the header, answers up to the sample RMS at which log2(4 rms^2) = ca_ki + 1/2
    (ca_ki of the 1-bit defaults, the smallest shift) and not beyond:

        fs, MHz    2.046  2.8  4   5.456  6.5  8.184  10    16.368  20   40
        RMS up to  152    107  76  53     38   38     26.9  13.4    9.5  3.36

    (at 40 MHz an 8-bit capture may use less than two bits).  Just below the boundary every shift is in range, ca_ki is 0 and
    the AGC levels are the 1-bit ones times 2^g; just above there is no answer.  The scales of the sweep keep inside it."""
    from test_track_ref import default_params
    table = dict(zip(_ALL_FS, (152, 107, 76, 53, 38, 38, 26.9, 13.4, 9.5, 3.36)))
    for fs in _ALL_FS:
        b = iqh.iq8_rms_bound(fs)
        digits = 0 if table[fs] >= 30 else (1 if table[fs] >= 9 else 2)
        assert math.floor(b * 10 ** digits) == round(table[fs] * 10 ** digits), (fs, b)
        base = default_params(fs)
        ok, bad = iqh.default_params_iq8(fs, b * (1 - 1e-9)), iqh.default_params_iq8(fs, b * (1 + 1e-9))
        assert bad is None and ok is not None, fs
        g = base.ca_ki
        assert ok.ca_ki == 0 and [base.lo_ki - ok.lo_ki, base.lo_kp - ok.lo_kp, base.ca_kp - ok.ca_kp, base.fll_k - ok.fll_k] == [g] * 4
        assert min(ok.lo_ki, ok.lo_kp) >= 1 and (ok.agc_lo, ok.agc_hi) == (base.agc_lo * 2 ** g, base.agc_hi * 2 ** g)
        # one step of g further down the RMS scale, and the clamp at the top of the shifts
        low = iqh.default_params_iq8(fs, b / math.sqrt(2) * (1 - 1e-9))
        assert low.ca_ki == 1
        tiny = iqh.default_params_iq8(fs, 1e-9)
        assert max(tiny.lo_ki, tiny.lo_kp, tiny.ca_ki, tiny.ca_kp, tiny.fll_k) == 62
        for x in (0.0, -1.0, float("nan"), float("inf")):
            assert iqh.default_params_iq8(fs, x) is None
    for fs, _ in FS_FC:
        assert iqh.IQ_SCALE[fs] * 1.05 < iqh.iq8_rms_bound(fs)  # room for the satellites' sum a^2 / 2 <= 0.1; the sweep asserts its RMS


@pytest.mark.parametrize("fs", sorted(iqh.LOCK_CASES), ids=lambda v: f"{v / 1e6:g}MHz")
def test_iq8_defaults_lock_at_high_fs(fs):
    """1.1 s at 10 (the HackRF flow: IF 2.6 MHz, int8), 20 and 40 MHz, amplitudes inside the supported RMS (scale 25 / 9 / 3), two
    satellites of amplitude 0.25 started 60 Hz off: through the 500-epoch FLL and on under the Costas loop.  Both end TRACK_OK,
    after epoch 700 the carrier deviates less than the 60 Hz it started with (measured here: at most 56.1 / 50.7 / 30.0 Hz; the
    word of an epoch carries the Costas loop's proportional term, 19 / 15 / 9 Hz rms), the prompt power on I is at least 10 times
    that on Q (measured: 136 and up).  Satellites, window and seeds are those of test_track_ref.test_defaults_lock_at_high_fs.  The
    run is audited by the reference."""
    sats, n, case = iqh.lock_setup(fs)
    buf = iqh.host_lock_capture(fs, sats, n, case)
    p, ch, rms = iqh.lock_params_and_chans(fs, buf, sats, case)
    assert rms < iqh.iq8_rms_bound(fs)
    reps, prompt, rec, ne = iqh.run_and_audit_iq(buf, 0, ch, p, sum_epochs=30, fmt=(case["signed"],) + case["dc"])
    print("fs %g rms %.2f (dev Hz, I/Q power)" % (fs, rms), iqh.assert_locked(fs, case, sats, reps, prompt, rec, ne))
