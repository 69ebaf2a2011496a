"""An independent reference of "Aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, written in numpy and Python numbers
from that text and the steps of "Aided acquisition" B it points to.  It shares no code with csrc/aided_iq_kernels.hip:

* the NCO words are Python float arithmetic, one IEEE operation per line of the text; llround is tests/refine_iq_ref.py's;
* the sample is tests/refine_iq_ref.py's (v = byte - off - dc), the carrier signs tests/track_ref.py's, the chips its C/A generator;
* the window is laid out sample by sample: hypothesis (h, d) has its own replica, chip[((base + h + j) ca_rate mod FULL) >> 32] at
  window sample j, and the two sums of a segment are plain sums over its samples -- no prefix sums, no transition lists; the squares,
  their sums and the floor are Python integers, the ratio is one Python division.

Law is a class so that tests/test_aided_iq.py can derive wrong laws from it, one method each, and tell them from the right one.
Law.powers_stream is a second, quicker spelling (one chip stream per d, np.correlate) that the CPU test holds against powers().
Sign mode (multibit = 0) is tests/iq_ref.py's conversion followed by tests/aided_ref.py."""
import numpy as np

import aided_ref
import iq_ref
import refine_iq_ref
import track_ref

TWO32 = 2 ** 32
FULL = 1023 * TWO32
L1, CPS = 1575.42e6, 1.023e6
SIGN, REAL, COMPLEX = 0, 1, 2
KEPT, NO_AID, SHORT, FEW, NO_POWER, BELOW = 1, 2, 4, 8, 16, 32
NOT_DETECTED = NO_AID | FEW | NO_POWER | BELOW
# gpsacq_aided_default_params_iq8's ratio_min: the largest ratio of 2304 draws on absent PRNs, 2.9517, plus a quarter of its excess over 1
# (include/gpsacq.h, "Aided acquisition on an 8-bit IQ capture", DEFAULT RATIO_MIN)
RATIO_MIN = 3.44


class Law:
    """THE MULTI-BIT PATH.  Every method restates one sentence of the header; a mutant overrides one of them."""

    def lo_shift_of(self, lo_center, K, d):
        return lo_center - K + d

    def base_of(self, ca_center, W, spm):
        return (ca_center - W) % spm

    def code_index(self, base, h, spm):
        """what multiplies ca_rate in P0(h, d): base + h, NOT reduced"""
        return base + h

    def carrier_sample(self, j, spm):
        """the sample count the carrier phase is taken at: from the window's first sample"""
        return j

    def carrier_hz(self, lo_dop, mix_hz, fc, multibit):
        """f_d, left to right"""
        return lo_dop - mix_hz + (0.0 if multibit == COMPLEX else fc)

    def window_start(self, block, stride):
        """o: the block's first SAMPLE; stride counts bytes, two to a sample"""
        return block * (stride // 2)

    def carrier(self, ph):
        """(C, S) = (1 - 2 cos bit, 1 - 2 sin bit) of uint32 phases"""
        cb, sb = track_ref.carrier_signs(ph)
        return 1 - 2 * cb.astype(np.int64), 1 - 2 * sb.astype(np.int64)

    def arms(self, vi, vq, C, S):
        """(v_i C - v_q S, v_i S + v_q C)"""
        return vi * C - vq * S, vi * S + vq * C

    def floor_of(self, vi, vq, o, segments, spm):
        """2 * sum of v_i^2 + v_q^2 over the samples of the window's segments, a Python integer"""
        a, b = vi[o:o + segments * spm], vq[o:o + segments * spm]
        return 2 * (int((a * a).sum()) + int((b * b).sum()))

    def wiped(self, vi, vq, o, n, lo_rate, spm):
        j = np.arange(n, dtype=np.int64)
        C, S = self.carrier((self.carrier_sample(j, spm) * lo_rate) % TWO32)
        return self.arms(vi[o:o + n], vq[o:o + n], C, S)

    def powers(self, vi, vq, o, segments, spm, prn, base, n_code, rates):
        """step 4: power(h, d), Python integers [n_dop][n_code]; rates: per d (valid, lo_rate, ca_rate); prn 1 .. 32"""
        n = segments * spm
        j = np.arange(n, dtype=np.int64)
        c = track_ref.chips(prn)
        out = []
        for valid, lo_rate, ca_rate in rates:
            if not valid or segments == 0:
                out.append([0] * n_code)
                continue
            re_, im_ = self.wiped(vi, vq, o, n, lo_rate, spm)
            row = []
            for h in range(n_code):
                P = (self.code_index(base, h, spm) * ca_rate + j * ca_rate) % FULL
                chip = 1 - 2 * c[P // TWO32].astype(np.int64)
                I = (chip * re_).reshape(segments, spm).sum(axis=1)
                Q = (chip * im_).reshape(segments, spm).sum(axis=1)
                row.append(sum(a * a + b * b for a, b in zip(I.tolist(), Q.tolist())))
            out.append(row)
        return out

    def powers_stream(self, vi, vq, o, segments, spm, prn, base, n_code, rates):
        """powers() once more through "the replica of h at sample j is the replica of h = 0 at sample j + h": ONE chip stream per d,
        every hypothesis a slice of it (np.correlate in float64: |sums| <= 512 spm < 2^25, exact).  Only for the law's own
        code_index and carrier_sample."""
        n = segments * spm
        c = track_ref.chips(prn)
        q = np.arange(n + n_code - 1, dtype=np.int64)
        out = []
        for valid, lo_rate, ca_rate in rates:
            if not valid or segments == 0:
                out.append([0] * n_code)
                continue
            re_, im_ = (x.astype(np.float64) for x in self.wiped(vi, vq, o, n, lo_rate, spm))
            stream = (1 - 2 * c[((base + q) * ca_rate % FULL) // TWO32].astype(np.int64)).astype(np.float64)
            acc = [0] * n_code
            for s in range(segments):
                seg = stream[s * spm:(s + 1) * spm + n_code - 1]
                I = np.correlate(seg, re_[s * spm:(s + 1) * spm], "valid")
                Q = np.correlate(seg, im_[s * spm:(s + 1) * spm], "valid")
                for h in range(n_code):
                    acc[h] += int(I[h]) * int(I[h]) + int(Q[h]) * int(Q[h])
            out.append(acc)
        return out


LAW = Law()


def nco_words(lo_shift, fc, fs, mix_hz, multibit, kmax, step_hz=0.0, law=LAW):
    """step 3 of one Doppler index: (valid, lo_rate, ca_rate)"""
    if step_hz > 0:
        lo_dop = lo_shift * step_hz
    else:
        lo_dop = lo_shift * fs
        lo_dop = lo_dop / 40000.0
    ca_dop = lo_dop / L1
    ca_dop = ca_dop * CPS
    ca_f = CPS + ca_dop
    f = law.carrier_hz(lo_dop, mix_hz, fc, multibit)
    if not (abs(lo_shift) <= kmax and abs(f) < fs / 2 and 0 <= ca_f < fs):
        return False, 0, 0
    lo_rate = f / fs
    lo_rate = refine_iq_ref.llround(lo_rate * 4294967296.0) % TWO32
    ca_rate = ca_f / fs
    ca_rate = int(ca_rate * 4294967296.0)
    return ca_rate != 0, lo_rate, ca_rate


def aided_search(iq, stride, tasks, aid, spm, fc, fs, kmax, signed=False, mean=None, mix_hz=0.0, multibit=REAL, step_hz=0.0, peaks_in=None, blocks=16,
                 min_segments=1, code_half=16, dop_half=1, keep_snr=25.0, ratio_min=RATIO_MIN, n_samples=None, law=LAW, stream=False):
    """gpsacq_aided_search_iq8 of the capture iq[:2 * n_samples] (bytes): tasks a list of (block, prn index) or None for (t, t % 32);
    aid a list of dicts or an AID_DTYPE array; peaks_in None or PEAK_DTYPE rows; stride in bytes; mean: (mean_i, mean_q) with
    remove_dc, else None.  Returns one dict per task: the fields of gpsacq_aided, `peak` and `powers` (uint64 [2K + 1][2W + 1]).
    stream: the sums by Law.powers_stream."""
    raw = np.ascontiguousarray(np.asarray(iq)).view(np.uint8).ravel()
    n_samples = raw.size // 2 if n_samples is None else int(n_samples)
    if multibit == SIGN:
        packed = iq_ref.bits(raw[:2 * n_samples], signed, (0.0, 0.0) if mean is None else mean, mix_hz, fs)  # the last byte filled up with zeros
        n_bytes = (n_samples + 7) // 8
        assert packed.size == n_bytes
        return aided_ref.aided_search(packed, stride // 16, tasks, aid, spm, fc, fs, kmax, step_hz=step_hz, peaks_in=peaks_in, blocks=blocks,
                                      min_segments=min_segments, code_half=code_half, dop_half=dop_half, keep_snr=keep_snr, ratio_min=ratio_min,
                                      n_bytes=n_bytes, stream=stream)
    vi, vq = refine_iq_ref.samples(raw[:2 * n_samples], signed, mean)
    W, K = int(code_half), int(dop_half)
    n_code, n_dop = 2 * W + 1, 2 * K + 1
    rows_in = None if peaks_in is None else (peaks_in.ravel().tolist() if isinstance(peaks_in, np.ndarray) else list(peaks_in))
    out = []
    for t in range(len(aid)):
        a = aid[t]
        block, prn = (t, t % 32) if tasks is None else (int(tasks[t][0]), int(tasks[t][1]))
        rec = dict(flags=NO_AID, segments=0, n_code=0, n_dop=0, best_h=0, best_d=0, lo_shift=0, ca_shift=0, best=0, total=0, floor=0, ratio=0.0,
                   peak=(0.0, 0, 0, 0.0), powers=np.zeros((n_dop, n_code), np.uint64))
        out.append(rec)
        if rows_in is not None and float(rows_in[t][0]) >= keep_snr:  # 1. KEPT
            rec.update(flags=KEPT, peak=tuple(rows_in[t]))
            continue
        ca_center, lo_center = int(a["ca_center"]), int(a["lo_center"])
        o = law.window_start(block, stride)
        if int(a["flags"]) != 0 or not 0 <= ca_center < spm or block < 0 or not 0 <= prn < 32 or o >= n_samples:  # 2. NO_AID
            continue
        rates = [nco_words(law.lo_shift_of(lo_center, K, d), fc, fs, mix_hz, multibit, kmax, step_hz, law) for d in range(n_dop)]  # 3. hypotheses
        if not any(r[0] for r in rates):
            continue
        fit = blocks * 40000 // spm
        segments = min(fit, (n_samples - o) // spm)
        base = law.base_of(ca_center, W, spm)
        pw = (law.powers_stream if stream else law.powers)(vi, vq, o, segments, spm, prn + 1, base, n_code, rates)  # 4. sums
        best, best_d, best_h, tot = -1, 0, 0, 0
        for d in range(n_dop):  # 5. the key: larger power, then smaller d, then smaller h
            if not rates[d][0]:
                continue
            for h in range(n_code):
                tot += pw[d][h]
                if pw[d][h] > best:
                    best, best_d, best_h = pw[d][h], d, h
        floor = law.floor_of(vi, vq, o, segments, spm)
        true_floor = Law.floor_of(law, vi, vq, o, segments, spm)
        assert best <= spm * true_floor and true_floor < 2 ** 46 and best < 2 ** 62, "the bound of the text is wrong"
        ratio = float(best) / float(floor) if floor else 0.0
        flags = (SHORT if segments < fit else 0) | (FEW if segments < min_segments else 0) | (NO_POWER if best == 0 else 0)
        flags |= BELOW if ratio < ratio_min else 0
        rec.update(flags=flags, segments=segments, n_code=n_code, n_dop=n_dop, best_h=best_h, best_d=best_d, lo_shift=lo_center - K + best_d,
                   ca_shift=(base + best_h) % spm, best=best, total=tot % 2 ** 64, floor=floor, ratio=ratio,
                   powers=np.array(pw, dtype=object).astype(np.uint64))
        if not flags & NOT_DETECTED:  # 6. the output peak
            rec["peak"] = (float(np.float32(ratio)), rec["lo_shift"], rec["ca_shift"], float(np.float32(best)))
    return out


same = aided_ref.same  # records, peaks and powers against aided_search()'s dicts: integers equal, ratio within 1e-12 relative
