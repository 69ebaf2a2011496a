"""Tracking channels on an 8-bit IQ capture, CPU side: the model of the multi-bit complex channel (tests/c/track_model_iq.c,
written from include/gpsacq.h) against a numpy restatement of its sums and against the 1-bit model on degenerate captures; the
host-only entry points; the ABI.  The kernel itself is checked against this model in tests/test_gpu_track_iq.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

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
