"""An independent reference of gpsacq_refine_iq8 in multi-bit mode, written in numpy and Python integers from the text "Snapshot
chain on an 8-bit IQ capture" of include/gpsacq.h (THE MULTI-BIT PATH) and the steps of "Fine code phases" it points to.  It shares
no code with csrc/snapshot_iq_kernels.hip:

* the NCO words are Python float arithmetic, one IEEE operation per line of the text; llround is spelled out (half away from zero);
* the sample is tests/track_ref.py's iq_samples (v = byte - off - dc), the carrier signs its carrier_signs (the float64 signs of cos
  and -sin with the tie rule at the quarter points), the chips its C/A generator at the positions X >> 32 reduced mod 1023;
* the window is laid out sample by sample (no groups, no weight bytes, no dot products), the six sums of a segment are int64 sums
  over its samples, the squares are Python integers, the estimate is tests/refine_ref.py's (steps 5 and 6 are unchanged).

Every sentence a wrong reading could change is a method of Law, so that tests/test_snapshot_iq.py can tell wrong laws from the
right one.  refine() returns one dict per task with the fields of gpsacq_fine; refine_ref.same() compares an array against them."""
import math

import numpy as np

import refine_ref
import track_ref

TWO32 = 2 ** 32
FULL = 1023 * TWO32
L1, CPS = 1575.42e6, 1.023e6
NO_HIT, SHORT, NO_POWER, FEW = 1, 2, 4, 8
REAL, COMPLEX = 1, 2


def llround(x):
    """C's llround of a finite double: to nearest, halves away from zero; exact (floor and the remainder are)"""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return -r if x < 0 else r


class Law:
    """The multi-bit path.  A mutant overrides one method."""

    def carrier_hz(self, lo_dop, mix_hz, fc, multibit):
        """f: where the satellite sits in the raw capture, left to right"""
        return lo_dop - mix_hz + (0.0 if multibit == COMPLEX else fc)

    def dc(self, mean):
        """nearbyint of the mean that is removed, ties to even (Python's round)"""
        return 0 if mean is None else int(round(float(mean)))

    def carrier(self, ph):
        """(C, S) = (1 - 2 cos bit, 1 - 2 sin bit) of uint32 phases"""
        cb, sb = track_ref.carrier_signs(ph)
        return 1 - 2 * cb.astype(np.int64), 1 - 2 * sb.astype(np.int64)

    def arms(self, vi, vq, C, S):
        """the complex sample times the two-level exp(-i 2 pi ph): (v_i C - v_q S, v_i S + v_q C)"""
        return vi * C - vq * S, vi * S + vq * C


LAW = Law()


def nco_words(lo_shift, fc, fs, mix_hz, multibit, step_hz=0.0, law=LAW):
    """NCO WORDS and their part of NOT A HIT: (in range, lo_rate, ca_rate, f, lo_dop)"""
    lo_dop = lo_shift * step_hz if step_hz > 0 else lo_shift * fs / 40000
    ca_dop = lo_dop / L1 * CPS
    ca_f = CPS + ca_dop
    f = law.carrier_hz(lo_dop, mix_hz, fc, multibit)
    if not (abs(f) < fs / 2 and 0 <= ca_f < fs):
        return False, 0, 0, f, lo_dop
    return True, llround(f / fs * 4294967296.0) % TWO32, int(ca_f / fs * 4294967296.0), f, lo_dop


def samples(iq, signed, mean=None, law=LAW):
    """(v_i, v_q) of the capture as int64 arrays; mean: (mean_i, mean_q) where it is removed, else None"""
    mi, mq = (None, None) if mean is None else mean
    vi, vq = track_ref.iq_samples(np.asarray(iq).view(np.uint8).ravel(), signed, law.dc(mi), law.dc(mq))
    return vi.astype(np.int64), vq.astype(np.int64)


def segment_sums(vi, vq, o, segments, spm, prn, lo_rate, ca_rate, P0, D, law=LAW):
    """SUMS: IE QE IP QP IL QL of every segment, int64 [segments][6]; prn 1 .. 32"""
    j = np.arange(segments * spm, dtype=np.int64)
    C, S = law.carrier((j * lo_rate) % TWO32)
    re_, im_ = law.arms(vi[o:o + segments * spm], vq[o:o + segments * spm], C, S)
    P = (P0 + j * ca_rate) % FULL  # j ca_rate < 2^22 2^32
    c = track_ref.chips(prn)
    out = np.zeros((segments, 6), np.int64)
    for k, X in enumerate(((P + D) % FULL, P, (P - D) % FULL)):
        h = 1 - 2 * c[(X // TWO32) % 1023].astype(np.int64)
        out[:, 2 * k] = (h * re_).reshape(segments, spm).sum(axis=1)
        out[:, 2 * k + 1] = (h * im_).reshape(segments, spm).sum(axis=1)
    return out


def window(t, pk, tasks, n_samples, stride, spm, fc, fs, mix_hz, multibit, step_hz, blocks, snr_min, law=LAW):
    """steps 1 to 3 of task t: None where it is no hit, else dict(prn, o, fit, segments, lo_rate, ca_rate, P0, f, lo_dop)"""
    snr, lo_shift, ca_shift = float(pk[0]), int(pk[1]), int(pk[2])
    block, prn = (t, t % 32) if tasks is None else (int(tasks[t][0]), int(tasks[t][1]))
    ok, lo_rate, ca_rate, f, lo_dop = nco_words(lo_shift, fc, fs, mix_hz, multibit, step_hz, law)
    o = block * (stride // 2)
    if not (snr >= snr_min) or not 0 <= ca_shift < spm or block < 0 or not 0 <= prn < 32 or o >= n_samples or not ok or ca_rate == 0:
        return None
    fit = blocks * 40000 // spm
    return dict(prn=prn, o=o, fit=fit, segments=min(fit, (n_samples - o) // spm), lo_rate=lo_rate, ca_rate=ca_rate, P0=(ca_shift * ca_rate) % FULL, f=f,
                lo_dop=lo_dop)


def rows_of(peaks):
    return peaks.ravel().tolist() if isinstance(peaks, np.ndarray) else list(peaks)


def refine(iq, stride, tasks, peaks, spm, fc, fs, signed=False, mean=None, mix_hz=0.0, multibit=REAL, step_hz=0.0, blocks=16, min_segments=1,
           half_spacing_chips=0.25, snr_min=25.0, n_samples=None, law=LAW):
    """gpsacq_refine_iq8 of the capture iq[:2 * n_samples] (bytes) in multi-bit mode: tasks a list of (block, prn index) or None for
    (t, t % 32); peaks a PEAK_DTYPE array or a list of (snr, lo_shift, ca_shift, ...) rows; stride in bytes; mean: (mean_i, mean_q)
    with remove_dc, else None.  Returns a list of dicts."""
    vi, vq = samples(iq, signed, mean, law)
    n_samples = vi.size if n_samples is None else int(n_samples)
    vi, vq = vi[:n_samples], vq[:n_samples]  # nothing at or beyond byte 2 n_samples is read
    D = int(half_spacing_chips * 4294967296.0)
    out = []
    for t, pk in enumerate(rows_of(peaks)):
        rec = dict(flags=NO_HIT, segments=0, lo_rate=0, ca_rate=0, early=0, prompt=0, late=0, offset_chips=0.0, tx_frac=0.0)
        out.append(rec)
        w = window(t, pk, tasks, n_samples, stride, spm, fc, fs, mix_hz, multibit, step_hz, blocks, snr_min, law)
        if w is None:
            continue
        s = segment_sums(vi, vq, w["o"], w["segments"], spm, w["prn"] + 1, w["lo_rate"], w["ca_rate"], w["P0"], D, law).tolist()
        early, prompt, late = (sum(r[2 * k] * r[2 * k] + r[2 * k + 1] * r[2 * k + 1] for r in s) for k in range(3))
        assert all(abs(x) <= 512 * spm for r in s for x in r) and max(early, prompt, late) < 2 ** 64, "the bound of the text is wrong"
        flags = (SHORT if w["segments"] < w["fit"] else 0) | (FEW if w["segments"] < min_segments else 0)
        rec.update(segments=w["segments"], lo_rate=w["lo_rate"], ca_rate=w["ca_rate"], early=early, prompt=prompt, late=late)
        if early + late == 0:
            flags |= NO_POWER
        else:
            rec["offset_chips"], rec["tx_frac"] = refine_ref.estimate(early, late, w["P0"], D)
        rec["flags"] = flags
    return out
