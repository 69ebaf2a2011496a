"""An independent reference of "Coherent aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, written in numpy and Python
integers from that text and the two sections it composes.  It shares no code with csrc/aided_coh_iq_kernels.hip:

* the NCO words are tests/aided_iq_ref.py's (Python float arithmetic, one IEEE operation per line), the sample is
  tests/refine_iq_ref.py's (v = byte - off - dc), the carrier signs tests/track_ref.py's, the chips its C/A generator;
* the segment sums are laid out sample by sample: hypothesis (h, d) has its own replica, chip[((base + h + j) ca_rate mod FULL) >> 32]
  at window sample j, and (I_s, Q_s) are plain sums over the samples of segment s -- no prefix sums, no transition lists;
* the coherent sums are Python integers: the table of tests/aided_coh_ref.py's law (math.cos), the index by Python's true modulo,
  A_s and B_s one product each, the boundaries as a sorted set, every period summed by itself and shifted once; the powers, the
  key, noncoh and the floor are Python integers, the ratio is one Python division.

Law is a class of one method per sentence so that tests/test_aided_coh_iq.py can derive wrong laws from it and tell them from
the right one.  Law.segment_sums_stream (one chip stream per d, np.correlate) and Law.powers_quick (int64 numpy: the BOUNDS of the
text keep every value below 2^63) are second, quicker spellings that the CPU test holds against the slow ones; tools/aided_floor.py
measures the default with them.  Sign mode (multibit = 0) is tests/iq_ref.py's conversion followed by tests/aided_coh_ref.py."""
import numpy as np

import aided_coh_ref
import aided_iq_ref
import iq_ref
import refine_iq_ref
import track_ref

TWO32, FULL = aided_iq_ref.TWO32, aided_iq_ref.FULL
SIGN, REAL, COMPLEX = 0, 1, 2
KEPT, NO_AID, SHORT, FEW, NO_POWER, BELOW = 1, 2, 4, 8, 16, 32
NOT_DETECTED = NO_AID | FEW | NO_POWER | BELOW
COH_MS = aided_coh_ref.COH_MS
MAX_Z = 5120
INT_FIELDS = aided_coh_ref.INT_FIELDS
# gpsacq_aided_coh_default_params_iq8's ratio_min (include/gpsacq.h, "Coherent aided acquisition on an 8-bit IQ capture", DEFAULT
# RATIO_MIN): tools/aided_floor.py --iq8 --coherent
RATIO_MIN = 28.56
DEFAULTS = dict(aided_coh_ref.DEFAULTS, ratio_min=RATIO_MIN)


class Law(aided_iq_ref.Law):
    """The sample, the carrier and the replica are aided_iq_ref.Law's sentences; what follows restates steps 4 and 5 of the text."""

    # ---- step 4: the segment sums, kept with their signs -------------------------------------------------------------------
    def segment_sums(self, vi, vq, o, segments, spm, prn, base, n_code, rates):
        """per d None (not valid) or (I, Q), int64 [segments][n_code]: sample by sample, one replica per hypothesis; prn 1 .. 32"""
        n = segments * spm
        j = np.arange(n, dtype=np.int64)
        c = track_ref.chips(prn)
        out = []
        for valid, lo_rate, ca_rate in rates:
            if not valid:
                out.append(None)
                continue
            re_, im_ = self.wiped(vi, vq, o, n, lo_rate, spm)
            zi, zq = np.zeros((segments, n_code), np.int64), np.zeros((segments, n_code), np.int64)
            for h in range(n_code):
                P = (self.code_index(base, h, spm) * ca_rate + j * ca_rate) % FULL
                chip = 1 - 2 * c[P // TWO32].astype(np.int64)
                zi[:, h] = (chip * re_).reshape(segments, spm).sum(axis=1)
                zq[:, h] = (chip * im_).reshape(segments, spm).sum(axis=1)
            out.append((zi, zq))
        return out

    def segment_sums_stream(self, vi, vq, o, segments, spm, prn, base, n_code, rates):
        """segment_sums() once more through "the replica of h at sample j is the replica of h = 0 at sample j + h": ONE chip stream
        per d, every hypothesis a slice of it (np.correlate in float64: |sums| <= 512 spm < 2^25, exact)"""
        n = segments * spm
        c = track_ref.chips(prn)
        q = np.arange(n + n_code - 1, dtype=np.int64)
        out = []
        for valid, lo_rate, ca_rate in rates:
            if not valid:
                out.append(None)
                continue
            re_, im_ = (x.astype(np.float64) for x in self.wiped(vi, vq, o, n, lo_rate, spm))
            stream = (1 - 2 * c[((base + q) * ca_rate % FULL) // TWO32].astype(np.int64)).astype(np.float64)
            zi, zq = np.zeros((segments, n_code), np.int64), np.zeros((segments, n_code), np.int64)
            for s in range(segments):
                seg = stream[s * spm:(s + 1) * spm + n_code - 1]
                zi[s] = np.rint(np.correlate(seg, re_[s * spm:(s + 1) * spm], "valid")).astype(np.int64)
                zq[s] = np.rint(np.correlate(seg, im_[s * spm:(s + 1) * spm], "valid")).astype(np.int64)
            out.append((zi, zq))
        return out

    # ---- step 5: the coherent sums ------------------------------------------------------------------------------------------
    def table(self):
        """the ROTATION TABLE is data of the model: "Coherent aided acquisition", step 5"""
        tc, ts = aided_coh_ref.LAW.table()
        return tc.tolist(), ts.tolist()

    def table_index(self, f, u, s):
        """k_s = (f u s) mod 1024, a true modulo"""
        return (f * u * s) % 1024

    def rotate(self, i, q, c, s):
        """z_s turned BACK: A = I C + Q S, B = Q C - I S"""
        return i * c + q * s, q * c - i * s

    def boundaries(self, e, m, n_seg):
        """{0, S} and every 0 < s < S with s = e mod M"""
        return sorted({0, n_seg} | {s for s in range(1, n_seg) if s % m == e})

    def period_value(self, terms):
        """A' = floor((sum of A_s over the period) / 2^14): an arithmetic shift AFTER the sum"""
        return sum(terms) >> 14

    def powers(self, zi, zq, fine_half, u, m):
        """power(h, g, e) as Python integers [n_fine][M][n_code] from the segment sums zi, zq (int64 [S][n_code])"""
        n_seg, n_code = zi.shape
        tc, ts = self.table()
        cols = [(zi[:, h].tolist(), zq[:, h].tolist()) for h in range(n_code)]
        bounds = [self.boundaries(e, m, n_seg) for e in range(m)]
        out = []
        for g in range(2 * fine_half + 1):
            k = [self.table_index(g - fine_half, u, s) for s in range(n_seg)]
            rows = [[0] * n_code for _ in range(m)]
            for h, (ci, cq) in enumerate(cols):
                ab = [self.rotate(ci[s], cq[s], tc[k[s]], ts[k[s]]) for s in range(n_seg)]
                a, b = [x[0] for x in ab], [x[1] for x in ab]
                for e in range(m):
                    acc = 0
                    for lo, hi in zip(bounds[e][:-1], bounds[e][1:]):
                        va, vb = self.period_value(a[lo:hi]), self.period_value(b[lo:hi])
                        acc += va * va + vb * vb
                    rows[e][h] = acc
            out.append(rows)
        return out

    def powers_quick(self, zi, zq, fine_half, u, m):
        """powers() once more in int64 numpy, every h at once: |A_s| < 2^40, a period of at most 20 segments < 2^45, A' < 2^30,
        a power < 2^60 (BOUNDS).  Only for the law's own rotate, boundaries and period_value."""
        n_seg, n_code = zi.shape
        tc, ts = (np.array(x, np.int64) for x in self.table())
        s = np.arange(n_seg, dtype=np.int64)
        out = np.zeros((2 * fine_half + 1, m, n_code), np.int64)
        for g in range(2 * fine_half + 1):
            k = np.mod((g - fine_half) * u * s, 1024)
            a = zi * tc[k][:, None] + zq * ts[k][:, None]
            b = zq * tc[k][:, None] - zi * ts[k][:, None]
            for e in range(m):
                bd = self.boundaries(e, m, n_seg)
                for lo, hi in zip(bd[:-1], bd[1:]):
                    va, vb = a[lo:hi].sum(axis=0) >> 14, b[lo:hi].sum(axis=0) >> 14
                    out[g, e] += va * va + vb * vb
        return out.tolist()

    # ---- step 6: floor is THE MEASURED FLOOR of the IQ section: aided_iq_ref.Law.floor_of, whatever the partition ------------


LAW = Law()


def record_of(z, rates, floor, spm, fs, step_hz, lo_center, base, segments, fit, W, K, F, u, M, min_segments, ratio_min, law=LAW, quick=False):
    """steps 5 to 7 from the segment sums z (per d None or (I, Q)) and the floor: the record's fields, `peak` and `powers`"""
    n_code, n_dop, n_fine = 2 * W + 1, 2 * K + 1, 2 * F + 1
    powers = np.zeros((n_dop, n_fine, M, n_code), np.uint64)
    best, place = -1, (0, 0, 0, 0)
    for d in range(n_dop):
        if z[d] is None:
            continue
        pw = (law.powers_quick if quick else law.powers)(z[d][0], z[d][1], F, u, M)
        powers[d] = np.array(pw, dtype=object).astype(np.uint64).reshape(n_fine, M, n_code)
        for g in range(n_fine):  # the key: larger power, then smaller d, g, e, h
            for e in range(M):
                for h in range(n_code):
                    if pw[g][e][h] > best:
                        best, place = pw[g][e][h], (d, g, e, h)
    d, g, e, h = place
    zi, zq = z[d]
    noncoh = sum(a * a + b * b for a, b in zip(zi[:, h].tolist(), zq[:, h].tolist()))
    assert best <= M * max(segments, 1) * 2 ** 18 * spm * spm * (1 + 2.0 ** -13) and best < 2 ** 60, "the bound of the text is wrong"
    ratio = float(best) / float(floor) if floor else 0.0
    lo_shift = lo_center - K + d
    if step_hz > 0:
        lo_dop = lo_shift * step_hz
    else:
        lo_dop = lo_shift * fs
        lo_dop = lo_dop / 40000.0
    fine = float((g - F) * u) / 1024.0
    fine = fine * (fs / float(spm))
    flags = (SHORT if segments < fit else 0) | (FEW if segments < min_segments else 0) | (NO_POWER if best == 0 else 0) | (BELOW if ratio < ratio_min else 0)
    rec = dict(flags=flags, segments=segments, n_code=n_code, n_dop=n_dop, n_fine=n_fine, n_edge=M, best_h=h, best_d=d, best_f=g, best_e=e,
               lo_shift=lo_shift, ca_shift=(base + h) % spm, best=best, noncoh=noncoh, floor=floor, ratio=ratio, doppler_hz=lo_dop + fine, reserved=0.0,
               peak=(0.0, 0, 0, 0.0), powers=powers)
    if not flags & NOT_DETECTED:
        rec["peak"] = (float(np.float32(ratio)), lo_shift, rec["ca_shift"], float(np.float32(best)))
    return rec


def aided_coh_search(iq, stride, tasks, aid, spm, fc, fs, kmax, signed=False, mean=None, mix_hz=0.0, multibit=REAL, step_hz=0.0, peaks_in=None,
                     n_samples=None, law=LAW, stream=False, quick=False, **params):
    """gpsacq_aided_coh_search_iq8 of the capture iq[:2 * n_samples] (bytes): tasks a list of (block, prn index) or None for
    (t, t % 32); aid a list of dicts or an AID_DTYPE array; peaks_in None or PEAK_DTYPE rows; stride in bytes; mean: (mean_i, mean_q)
    with remove_dc, else None; params: the fields of gpsacq_aided_coh_params (DEFAULTS where left out; sign mode:
    aided_coh_ref.DEFAULTS).  Returns one dict per task: the fields of gpsacq_aided_coh, `peak` and `powers`
    (uint64 [2K + 1][2F + 1][M][2W + 1]).  stream, quick: the sums by the law's quicker spellings."""
    raw = np.ascontiguousarray(np.asarray(iq)).view(np.uint8).ravel()
    n_samples = raw.size // 2 if n_samples is None else int(n_samples)
    if multibit == SIGN:
        packed = iq_ref.bits(raw[:2 * n_samples], signed, (0.0, 0.0) if mean is None else mean, mix_hz, fs)  # the last byte filled up with zeros
        n_bytes = (n_samples + 7) // 8
        assert packed.size == n_bytes
        return aided_coh_ref.aided_coh_search(packed, stride // 16, tasks, aid, spm, fc, fs, kmax, step_hz=step_hz, peaks_in=peaks_in, n_bytes=n_bytes, **params)
    p = dict(DEFAULTS, **params)
    W, K, F, u, M = int(p["code_half"]), int(p["dop_half"]), int(p["fine_half"]), int(p["fine_step"]), int(p["coh_ms"])
    assert M in COH_MS and 0 <= W <= 31 and 0 <= K <= 8 and 0 <= F <= 7 and 1 <= u <= 512
    vi, vq = refine_iq_ref.samples(raw[:2 * n_samples], signed, mean)
    n_code, n_dop, n_fine = 2 * W + 1, 2 * K + 1, 2 * F + 1
    rows_in = None if peaks_in is None else (peaks_in.ravel().tolist() if isinstance(peaks_in, np.ndarray) else list(peaks_in))
    out = []
    for t in range(len(aid)):
        a = aid[t]
        block, prn = (t, t % 32) if tasks is None else (int(tasks[t][0]), int(tasks[t][1]))
        rec = dict({f: 0 for f in INT_FIELDS}, flags=NO_AID, ratio=0.0, doppler_hz=0.0, reserved=0.0, peak=(0.0, 0, 0, 0.0),
                   powers=np.zeros((n_dop, n_fine, M, n_code), np.uint64))
        out.append(rec)
        if rows_in is not None and float(rows_in[t][0]) >= p["keep_snr"]:  # 1. KEPT
            rec.update(flags=KEPT, peak=tuple(rows_in[t]))
            continue
        ca_center, lo_center = int(a["ca_center"]), int(a["lo_center"])
        o = law.window_start(block, stride)
        if int(a["flags"]) != 0 or not 0 <= ca_center < spm or block < 0 or not 0 <= prn < 32 or o >= n_samples:  # 2. NO_AID
            continue
        rates = [aided_iq_ref.nco_words(law.lo_shift_of(lo_center, K, d), fc, fs, mix_hz, multibit, kmax, step_hz, law) for d in range(n_dop)]  # 3. hypotheses
        if not any(r[0] for r in rates):
            continue
        fit = p["blocks"] * 40000 // spm
        assert fit * n_code <= MAX_Z
        segments = min(fit, (n_samples - o) // spm)
        base = law.base_of(ca_center, W, spm)
        z = (law.segment_sums_stream if stream else law.segment_sums)(vi, vq, o, segments, spm, prn + 1, base, n_code, rates)  # 4. segment sums
        floor = law.floor_of(vi, vq, o, segments, spm)
        rec.update(record_of(z, rates, floor, spm, fs, step_hz, lo_center, base, segments, fit, W, K, F, u, M, p["min_segments"], p["ratio_min"], law, quick))
    return out


same = aided_coh_ref.same  # records, peaks and powers against aided_coh_search()'s dicts: integers equal, ratio within 1e-12 relative
