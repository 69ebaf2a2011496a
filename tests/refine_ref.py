"""An independent reference of gpsacq_refine, written in numpy and Python integers from the text "Fine code phases: search peaks
refined below a sample" of include/gpsacq.h (THE MODEL, PER TASK, steps 1-6).  It shares no code with csrc/refine_kernels.hip:

* the NCO words are Python float arithmetic, one IEEE operation per line of the text;
* the carrier signs are tests/track_ref.py's (the float64 signs of cos and -sin with the tie rule at the quarter points);
* the chips are read from the oracle's C/A generator (track_ref.chips) at the positions X >> 32 reduced mod 1023;
* the window is laid out sample by sample (no words, no masks, no popcounts), the six sums of a segment are int64 sums over its
  samples, the squares are Python integers, the estimate is Python floats with math.sqrt.

refine() returns one dict per task with the fields of gpsacq_fine; same() compares a FINE_DTYPE array against them."""
import math

import numpy as np

import track_ref

TWO32 = 2 ** 32
FULL = 1023 * TWO32
L1, CPS = 1575.42e6, 1.023e6
NO_HIT, SHORT, NO_POWER, FEW = 1, 2, 4, 8
INT_FIELDS = ("flags", "segments", "lo_rate", "ca_rate", "early", "prompt", "late")
OFFSET_TOL, TX_FRAC_TOL = 1e-12, 1e-15  # fp64 rounding of a handful of operations on values <= 1023, times 10^3


def nco_words(lo_shift, fc, fs, step_hz=0.0):
    """step 1: (in range, lo_rate, ca_rate); step_hz <= 0 is the reference grid, lo_shift in FFT bins of fs / 40000"""
    lo_dop = lo_shift * step_hz if step_hz > 0 else lo_shift * fs / 40000
    ca_dop = lo_dop / L1 * CPS
    lo_f, ca_f = fc + lo_dop, CPS + ca_dop
    if not (0 <= lo_f < fs and 0 <= ca_f < fs):
        return False, 0, 0
    return True, int(lo_f / fs * 4294967296.0), int(ca_f / fs * 4294967296.0)


def segment_sums(samples01, o, segments, spm, prn, lo_rate, ca_rate, P0, D):
    """step 4: the six sums IE QE IP QP IL QL of every segment, int64 [segments][6]; samples01: the capture, 0/1 per sample"""
    j = np.arange(segments * spm, dtype=np.int64)
    cb, sb = track_ref.carrier_signs((j * lo_rate) % TWO32)
    v = 1 - 2 * samples01[o:o + segments * spm].astype(np.int64)
    re_, im_ = v * (1 - 2 * cb), v * (1 - 2 * sb)
    P = (P0 + j * ca_rate) % FULL  # j ca_rate < 2^22 2^32
    c = track_ref.chips(prn)
    out = np.zeros((segments, 6), np.int64)
    for k, X in enumerate(((P + D) % FULL, P, (P - D) % FULL)):
        h = 1 - 2 * c[(X // TWO32) % 1023].astype(np.int64)
        out[:, 2 * k] = (h * re_).reshape(segments, spm).sum(axis=1)
        out[:, 2 * k + 1] = (h * im_).reshape(segments, spm).sum(axis=1)
    return out


def estimate(early, late, P0, D):
    """step 5: (offset_chips, tx_frac) of early + late > 0"""
    d = D / 4294967296.0
    a_e, a_l = math.sqrt(float(early)), math.sqrt(float(late))
    offset = ((1.0 - d) * (a_e - a_l)) / (a_e + a_l)
    pos = P0 / 4294967296.0 + offset
    if pos < 0.0:
        pos += 1023.0
    elif pos >= 1023.0:
        pos -= 1023.0
    tx = pos / 1.023e6
    return offset, tx if tx < 1e-3 else 0.0


def refine(bits, stride, tasks, peaks, spm, fc, fs, step_hz=0.0, blocks=16, min_segments=1, half_spacing_chips=0.25, snr_min=25.0, n_bytes=None):
    """gpsacq_refine of the capture bits[:n_bytes] (uint8): tasks a list of (block, prn index) or None for (t, t % 32); peaks a
    PEAK_DTYPE array or a list of (snr, lo_shift, ca_shift, ...) rows.  Returns a list of dicts."""
    bits = np.asarray(bits, np.uint8).ravel()
    n_bytes = bits.size if n_bytes is None else int(n_bytes)
    samples01 = np.unpackbits(bits[:n_bytes], bitorder="little")
    total = 8 * n_bytes
    D = int(half_spacing_chips * 4294967296.0)
    out = []
    rows = peaks.ravel().tolist() if isinstance(peaks, np.ndarray) else list(peaks)
    for t, pk in enumerate(rows):
        snr, lo_shift, ca_shift = float(pk[0]), int(pk[1]), int(pk[2])
        block, prn = (t, t % 32) if tasks is None else (int(tasks[t][0]), int(tasks[t][1]))
        rec = dict(flags=NO_HIT, segments=0, lo_rate=0, ca_rate=0, early=0, prompt=0, late=0, offset_chips=0.0, tx_frac=0.0)
        out.append(rec)
        ok, lo_rate, ca_rate = nco_words(lo_shift, fc, fs, step_hz)
        o = 8 * block * stride
        if not (snr >= snr_min) or not 0 <= ca_shift < spm or block < 0 or not 0 <= prn < 32 or o >= total or not ok or ca_rate == 0:
            continue
        fit = blocks * 40000 // spm
        segments = min(fit, (total - o) // spm)
        P0 = (ca_shift * ca_rate) % FULL
        s = segment_sums(samples01, o, segments, spm, prn + 1, lo_rate, ca_rate, P0, D).tolist()
        early, prompt, late = (sum(r[2 * k] * r[2 * k] + r[2 * k + 1] * r[2 * k + 1] for r in s) for k in range(3))
        flags = (SHORT if segments < fit else 0) | (FEW if segments < min_segments else 0)
        rec.update(segments=segments, lo_rate=lo_rate, ca_rate=ca_rate, early=early, prompt=prompt, late=late)
        if early + late == 0:
            flags |= NO_POWER
        else:
            rec["offset_chips"], rec["tx_frac"] = estimate(early, late, P0, D)
        rec["flags"] = flags
    return out


def usable(rec):
    """step 6"""
    return not int(rec["flags"]) & (NO_HIT | NO_POWER | FEW)


def same(got, ref, label=""):
    """a FINE_DTYPE array against refine()'s dicts: every integer field equal, offset_chips within OFFSET_TOL, tx_frac within
    TX_FRAC_TOL and in [0, 1e-3).  Returns the two largest differences."""
    got = np.asarray(got).ravel()
    assert got.size == len(ref), (label, got.size, len(ref))
    worst = [0.0, 0.0]
    for i, r in enumerate(ref):
        for f in INT_FIELDS:
            assert int(got[f][i]) == r[f], (label, i, f, int(got[f][i]), r[f])
        d_off, d_tx = abs(float(got["offset_chips"][i]) - r["offset_chips"]), abs(float(got["tx_frac"][i]) - r["tx_frac"])
        assert d_off <= OFFSET_TOL and d_tx <= TX_FRAC_TOL, (label, i, d_off, d_tx)
        assert 0.0 <= got["tx_frac"][i] < 1e-3, (label, i, got["tx_frac"][i])
        worst = [max(worst[0], d_off), max(worst[1], d_tx)]
    return worst
