"""An independent reference of gpsacq_fine_doppler_iq8 in multi-bit mode, written in numpy and Python integers from FINE DOPPLER of
"Snapshot chain on an 8-bit IQ capture" of include/gpsacq.h.  It shares no code with csrc/snapshot_iq_kernels.hip:

* window, NCO words and the per-sample prompt sums are tests/refine_iq_ref.py's (sample by sample, no groups, no dot products);
* the normalisation is Python integers: bit_length, a floor division for the arithmetic shift;
* the lag-1 sums are tests/dop_ref.py's lag_sums on Python integers of any size, so a sum that left 63 bits would show instead of
  wrapping, and bounds() checks every TERM against the text as well;
* the estimate is Python floats with math.atan2 and math.hypot.

Norm is the normalisation as the text has it; a mutant overrides its shift.  fine_doppler() returns one dict per task with the
fields of gpsacq_dopfine (and k, the shift, beside them); dop_ref.same() compares an array against them."""
import math

import dop_ref
import refine_iq_ref
from refine_iq_ref import FULL, TWO32

NO_HIT, SHORT, NO_POWER, FEW, WEAK = 1, 2, 4, 8, 16


class Norm:
    def k_of(self, iq):
        """k = max(0, bitlength(M) - 12), M the largest |I_s| or |Q_s|"""
        m = max((max(abs(i), abs(q)) for i, q in iq), default=0)
        return max(0, m.bit_length() - 12)

    def shift(self, v, k):
        """(v + 2^(k-1)) >> k, arithmetic; v itself when k = 0"""
        return v if k == 0 else (v + 2 ** (k - 1)) // 2 ** k   # Python's // floors, as an arithmetic shift does

    def shifted(self, iq):
        k = self.k_of(iq)
        return k, [(self.shift(i, k), self.shift(q, k)) for i, q in iq]


NORM = Norm()


def bounds(shifted):
    """the text's bounds on the shifted values, their squares and every term of the lag-1 sums, in Python integers"""
    assert all(abs(i) <= 2 ** 12 and abs(q) <= 2 ** 12 for i, q in shifted)
    sq = [(i * i - q * q, 2 * i * q, i * i + q * q) for i, q in shifted]
    assert all(abs(a) <= 2 ** 25 and abs(b) <= 2 ** 25 for a, b, _ in sq)
    for s in range(1, len(sq)):
        terms = (sq[s][0] * sq[s - 1][0] + sq[s][1] * sq[s - 1][1], sq[s][1] * sq[s - 1][0] - sq[s][0] * sq[s - 1][1], sq[s][2] * sq[s - 1][2])
        assert all(abs(x) <= 2 ** 50 for x in terms), "a term left the bound of the text"
    assert len(shifted) < 2 ** 12


def estimate(re, im, mag, spm, fs, lo_rate, base_hz):
    """ESTIMATE of "Cold snapshot fixes" with this section's doppler_hz: (no power, coherence, df_hz, doppler_hz)"""
    if mag == 0 or (re == 0 and im == 0):
        return True, 0.0, 0.0, 0.0
    T = float(spm) / fs
    df = math.atan2(float(im), float(re)) / ((4.0 * 3.141592653589793) * T)
    word = lo_rate - TWO32 if lo_rate >= 2 ** 31 else lo_rate  # (int32)lo_rate
    return False, math.hypot(float(re), float(im)) / float(mag), df, ((float(word) * fs) / 4294967296.0 - base_hz) + df


def record(iq, fit, spm, fs, lo_rate, ca_rate, base_hz, min_segments=2, coherence_min=0.0, norm=NORM):
    """the record of a hit from its per-segment (I, Q): everything from the normalisation on"""
    iq = [(int(i), int(q)) for i, q in iq]
    k, sh = norm.shifted(iq)
    bounds(sh)
    re, im, mag, _ = dop_ref.lag_sums(sh)
    power = sum(i * i + q * q for i, q in iq)
    assert -2 ** 62 < re < 2 ** 62 and -2 ** 62 < im < 2 ** 62 and mag < 2 ** 62 and power < 2 ** 64, "OVERFLOW: the bound of the text is wrong"
    none, coh, df, dop = estimate(re, im, mag, spm, fs, lo_rate, base_hz)
    flags = (SHORT if len(iq) < fit else 0) | (FEW if len(iq) < min_segments else 0) | (NO_POWER if none else 0) | (WEAK if coh < coherence_min else 0)
    return dict(flags=flags, segments=len(iq), lo_rate=lo_rate, ca_rate=ca_rate, re=re, im=im, mag=mag, power=power, coherence=coh, df_hz=df,
                doppler_hz=dop, k=k)


def fine_doppler(iq, stride, tasks, peaks, spm, fc, fs, signed=False, mean=None, mix_hz=0.0, multibit=refine_iq_ref.REAL, step_hz=0.0, blocks=16,
                 min_segments=2, snr_min=25.0, coherence_min=0.0, n_samples=None, law=refine_iq_ref.LAW, norm=NORM):
    """gpsacq_fine_doppler_iq8 of the capture iq[:2 * n_samples] in multi-bit mode; arguments as refine_iq_ref.refine"""
    vi, vq = refine_iq_ref.samples(iq, signed, mean, law)
    n_samples = vi.size if n_samples is None else int(n_samples)
    vi, vq = vi[:n_samples], vq[:n_samples]
    out = []
    for t, pk in enumerate(refine_iq_ref.rows_of(peaks)):
        w = refine_iq_ref.window(t, pk, tasks, n_samples, stride, spm, fc, fs, mix_hz, multibit, step_hz, blocks, snr_min, law)
        if w is None:
            out.append(dict(flags=NO_HIT, segments=0, lo_rate=0, ca_rate=0, re=0, im=0, mag=0, power=0, coherence=0.0, df_hz=0.0, doppler_hz=0.0, k=0))
            continue
        sums = refine_iq_ref.segment_sums(vi, vq, w["o"], w["segments"], spm, w["prn"] + 1, w["lo_rate"], w["ca_rate"], w["P0"], TWO32 // 4, law)
        out.append(record([(r[2], r[3]) for r in sums.tolist()], w["fit"], spm, fs, w["lo_rate"], w["ca_rate"], w["f"] - w["lo_dop"], min_segments,
                          coherence_min, norm))
    return out
