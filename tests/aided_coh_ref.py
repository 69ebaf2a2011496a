"""An independent reference of "Coherent aided acquisition: 20 ms sums, bit edge and fine Doppler" of include/gpsacq.h (THE
MODEL, A. SEARCH and B. THE RECEIVE INSTANT), written in numpy and Python integers from that text.  It shares no code with
csrc/aided_kernels.hip:

* steps 1 to 3 are spelled as tests/aided_ref.py spells them (its NCO words, its carrier signs), the reference of the section the
  text points to;
* the segment sums are sums over samples: ONE chip stream per (segment, d), every hypothesis a slice of it (np.correlate), kept
  with their signs -- no words, no masks, no popcounts; tests/test_aided_coh.py holds their squares against aided_ref's
  sample-by-sample powers;
* the coherent sums follow the text sentence by sentence: the table from math.cos, the index by Python's true modulo, the prefix
  of the turned series in int64 (a period stays below 2^36), the boundaries as a sorted set, one shift per period; the powers and
  the key are Python integers.

Law is a class of one method per sentence so that tests/test_aided_coh.py can derive wrong laws from it and tell them from the
right one."""
import math

import numpy as np

import aided_ref
import track_ref

TWO32, FULL = aided_ref.TWO32, aided_ref.FULL
KEPT, NO_AID, SHORT, FEW, NO_POWER, BELOW = 1, 2, 4, 8, 16, 32
NOT_DETECTED = NO_AID | FEW | NO_POWER | BELOW
COH_MS = (1, 2, 4, 5, 10, 20)
MAX_Z = 5120
INT_FIELDS = ("flags", "segments", "n_code", "n_dop", "n_fine", "n_edge", "best_h", "best_d", "best_f", "best_e", "lo_shift", "ca_shift", "best",
              "noncoh", "floor")
RATIO_TOL = 1e-12    # relative: one fp64 division of two integers below 2^53
DOPPLER_TOL = 1e-9   # Hz: a few fp64 operations on values below 1e5
# gpsacq_aided_coh_default_params' ratio_min (include/gpsacq.h, DEFAULT RATIO_MIN): tools/aided_floor.py --coherent
RATIO_MIN = 10.73
DEFAULTS = dict(blocks=16, min_segments=20, code_half=16, dop_half=1, coh_ms=20, fine_half=3, fine_step=25, keep_snr=25.0, ratio_min=RATIO_MIN)
C_MPS, WEEK_MS = 2.99792458e8, 604800000


class Law:
    """step 5, COHERENT SUMS.  Every method restates one sentence of the header; a mutant overrides one of them."""

    def table(self):
        """C[k] = nearbyint(2^14 cos(2 pi k / 1024)), S likewise, int64 arrays of 1024"""
        c = [int(np.rint(16384.0 * math.cos(2.0 * math.pi * k / 1024.0))) for k in range(1024)]
        s = [int(np.rint(16384.0 * math.sin(2.0 * math.pi * k / 1024.0))) for k in range(1024)]
        return np.array(c, np.int64), np.array(s, np.int64)

    def table_index(self, f, u, s):
        """k_s = (f u s) mod 1024, a true modulo; s an int64 array"""
        return np.mod(f * u * s, 1024)

    def rotate(self, i, q, c, s):
        """z_s turned BACK: A = I C + Q S, B = Q C - I S"""
        return i * c + q * s, q * c - i * s

    def boundaries(self, e, m, n_seg):
        """{0, S} and every 0 < s < S with s = e mod M"""
        return sorted({0, n_seg} | {s for s in range(1, n_seg) if s % m == e})

    def periods(self, bounds, m):
        """consecutive boundaries; the partial periods at both ends count"""
        return list(zip(bounds[:-1], bounds[1:]))

    def terms(self, a):
        """what is summed over a period: A_s itself"""
        return a

    def period_value(self, total):
        """A' = floor(sum / 2^14): an arithmetic shift AFTER the sum"""
        return total >> 14

    def powers(self, zi, zq, fine_half, u, m):
        """power(h, g, e) as Python integers [n_fine][M][n_code] from the segment sums zi, zq (int64 [S][n_code])"""
        n_seg, n_code = zi.shape
        tc, ts = self.table()
        s = np.arange(n_seg, dtype=np.int64)
        out = []
        for g in range(2 * fine_half + 1):
            k = self.table_index(g - fine_half, u, s)
            a, b = self.rotate(zi, zq, tc[k][:, None], ts[k][:, None])
            pa = np.concatenate([np.zeros((1, n_code), np.int64), np.cumsum(self.terms(a), axis=0)])
            pb = np.concatenate([np.zeros((1, n_code), np.int64), np.cumsum(self.terms(b), axis=0)])
            rows = []
            for e in range(m):
                acc = [0] * n_code
                for lo, hi in self.periods(self.boundaries(e, m, n_seg), m):
                    va, vb = self.period_value(pa[hi] - pa[lo]), self.period_value(pb[hi] - pb[lo])
                    for h in range(n_code):
                        acc[h] += int(va[h]) * int(va[h]) + int(vb[h]) * int(vb[h])
                rows.append(acc)
            out.append(rows)
        return out


LAW = Law()


def segment_sums(samples01, o, segments, spm, prn, base, n_code, rates, carriers=None):
    """step 4: per d None (not valid) or (I, Q), int64 [segments][n_code], the prompt sums of hypothesis (h, d) over segment s.
    rates: per d (valid, lo_rate, ca_rate); carriers: per d (+-1 of cos, +-1 of -sin) of this window where the caller has them"""
    n = segments * spm
    v = (1 - 2 * samples01[o:o + n].astype(np.int64)).astype(np.float64)
    c = track_ref.chips(prn)
    q = np.arange(n + n_code - 1, dtype=np.int64)
    out = []
    for d, (valid, lo_rate, ca_rate) in enumerate(rates):
        if not valid:
            out.append(None)
            continue
        cre, cim = carriers[d] if carriers is not None else aided_ref.carrier_pm((np.arange(n, dtype=np.int64) * lo_rate) % TWO32)
        stream = (1 - 2 * c[((base + q) * ca_rate % FULL) // TWO32].astype(np.int64)).astype(np.float64)  # base + h + j, NOT reduced
        re_, im_ = v * cre, v * cim
        zi, zq = np.zeros((segments, n_code), np.int64), np.zeros((segments, n_code), np.int64)
        for s in range(segments):
            seg = stream[s * spm:(s + 1) * spm + n_code - 1]
            zi[s] = np.rint(np.correlate(seg, re_[s * spm:(s + 1) * spm], "valid")).astype(np.int64)  # |sums| <= spm: exact in float64
            zq[s] = np.rint(np.correlate(seg, im_[s * spm:(s + 1) * spm], "valid")).astype(np.int64)
        out.append((zi, zq))
    return out


def record_of(z, rates, spm, fs, step_hz, lo_center, base, segments, fit, W, K, F, u, M, min_segments, ratio_min, law=LAW):
    """steps 5 and 6 from the segment sums z (segment_sums' list): the record's fields, `peak` and `powers`"""
    n_code, n_dop, n_fine = 2 * W + 1, 2 * K + 1, 2 * F + 1
    powers = np.zeros((n_dop, n_fine, M, n_code), np.uint64)
    best, place, noncoh = -1, (0, 0, 0, 0), 0
    for d in range(n_dop):
        if z[d] is None:
            continue
        zi, zq = z[d]
        pw = law.powers(zi, zq, F, u, M)
        powers[d] = np.array(pw, dtype=np.uint64)
        for g in range(n_fine):  # the key: larger power, then smaller d, g, e, h
            for e in range(M):
                for h in range(n_code):
                    if pw[g][e][h] > best:
                        best, place = pw[g][e][h], (d, g, e, h)
    d, g, e, h = place
    zi, zq = z[d]
    noncoh = sum(int(a) * int(a) + int(b) * int(b) for a, b in zip(zi[:, h].tolist(), zq[:, h].tolist()))
    floor = 2 * spm * segments
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


def aided_coh_search(bits, stride, tasks, aid, spm, fc, fs, kmax, step_hz=0.0, peaks_in=None, n_bytes=None, law=LAW, **params):
    """gpsacq_aided_coh_search of the capture bits[:n_bytes] (uint8): tasks a list of (block, prn index) or None for (t, t % 32);
    aid a list of dicts or an AID_DTYPE array; peaks_in None or PEAK_DTYPE rows; params: the fields of gpsacq_aided_coh_params
    (DEFAULTS where left out).  Returns one dict per task: the fields of gpsacq_aided_coh, `peak` and `powers`
    (uint64 [2K + 1][2F + 1][M][2W + 1])."""
    p = dict(DEFAULTS, **params)
    W, K, F, u, M = int(p["code_half"]), int(p["dop_half"]), int(p["fine_half"]), int(p["fine_step"]), int(p["coh_ms"])
    assert M in COH_MS and 0 <= W <= 31 and 0 <= K <= 8 and 0 <= F <= 7 and 1 <= u <= 512
    bits = np.asarray(bits, np.uint8).ravel()
    n_bytes = bits.size if n_bytes is None else int(n_bytes)
    samples01 = np.unpackbits(bits[:n_bytes], bitorder="little")
    total = 8 * n_bytes
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
        o = 8 * block * stride
        if int(a["flags"]) != 0 or not 0 <= ca_center < spm or block < 0 or not 0 <= prn < 32 or o >= total:  # 2. NO_AID
            continue
        rates = []
        for d in range(n_dop):  # 3. hypotheses
            lo = lo_center - K + d
            ok, lo_rate, ca_rate = aided_ref.nco_words(lo, fc, fs, step_hz)
            rates.append((ok and abs(lo) <= kmax, lo_rate, ca_rate))
        if not any(r[0] for r in rates):
            continue
        fit = p["blocks"] * 40000 // spm
        assert fit * n_code <= MAX_Z
        segments = min(fit, (total - o) // spm)
        base = (ca_center - W) % spm
        z = segment_sums(samples01, o, segments, spm, prn + 1, base, n_code, rates)  # 4. segment sums
        rec.update(record_of(z, rates, spm, fs, step_hz, lo_center, base, segments, fit, W, K, F, u, M, p["min_segments"], p["ratio_min"], law))
    return out


def same(got, ref, peaks=None, powers=None, label=""):
    """AIDED_COH_DTYPE records (and PEAK_DTYPE peaks, uint64 powers) against aided_coh_search()'s dicts: every integer equal, ratio
    within RATIO_TOL relative, doppler_hz within DOPPLER_TOL, reserved 0, peaks byte for byte.  Returns the largest relative
    difference of ratio."""
    got = np.asarray(got).ravel()
    assert got.size == len(ref), (label, got.size, len(ref))
    worst = 0.0
    for i, r in enumerate(ref):
        for f in INT_FIELDS:
            assert int(got[f][i]) == r[f], (label, i, f, int(got[f][i]), r[f])
        rel = abs(float(got["ratio"][i]) - r["ratio"]) / max(r["ratio"], 1e-300)
        assert rel <= RATIO_TOL, (label, i, float(got["ratio"][i]), r["ratio"])
        assert abs(float(got["doppler_hz"][i]) - r["doppler_hz"]) <= DOPPLER_TOL and float(got["reserved"][i]) == 0.0, (label, i)
        worst = max(worst, rel)
        if peaks is not None:
            pk = peaks.ravel()[i]
            want = np.zeros(1, pk.dtype)
            want[0] = tuple(r["peak"])
            assert pk.tobytes() == want.tobytes(), (label, i, pk, r["peak"])
        if powers is not None:
            assert np.array_equal(np.asarray(powers).reshape(len(ref), *r["powers"].shape)[i], r["powers"]), (label, i)
    return worst


# ---- B. THE RECEIVE INSTANT ---------------------------------------------------------------------------------------------------
def instant(fix, info, prior):
    """gpsacq_aid_instant: FIX_DTYPE, COARSE_INFO_DTYPE and COARSE_PRIOR_DTYPE arrays of one length; returns the fixes.  Python
    floats, one IEEE operation per line; round() is to nearest, ties to even"""
    out = np.array(fix, copy=True).ravel()
    for i in range(out.size):
        if int(out["status"][i]) != 0:
            continue
        coarse_s, bias_m = float(info["coarse_s"].ravel()[i]), float(info["bias_m"].ravel()[i])
        if not (math.isfinite(coarse_s) and math.isfinite(bias_m)):
            out["status"][i] = 2
            continue
        t = 1e3 * coarse_s
        t = float(np.rint(t))
        t = t * 1e-3
        t = t - bias_m / C_MPS
        k = float(np.floor(1e3 * t))  # a float, as in the text: floor(-0.0) is -0.0, and t - 1e-3 k is then +0.0
        if not -2 ** 31 <= k <= 2 ** 31 - 1:
            out["status"][i] = 2
            continue
        out["rx_ms"][i] = (int(prior["rx_ms"].ravel()[i]) + int(k)) % WEEK_MS
        out["rx_frac"][i] = t - 1e-3 * k
    return out
