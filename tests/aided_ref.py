"""An independent reference of "Aided acquisition: predicted code phase and Doppler, windowed search" of include/gpsacq.h (THE
MODEL, A. PREDICTION and B. WINDOWED SEARCH), written in numpy and Python numbers from that text.  It shares no code with
csrc/aided_kernels.hip and is not built on tests/refine_ref.py:

* the NCO words are Python float arithmetic, one IEEE operation per line of the text;
* the window is laid out sample by sample (no words, no masks, no popcounts, no shared chip stream): hypothesis (h, d) has its
  own replica, chip[((base + h + j) ca_rate mod FULL) >> 32] at window sample j, and its own carrier signs (tests/track_ref.py's:
  the float64 signs of cos and -sin with the tie rule at the quarter points); the two sums of a segment are sums over its
  samples, the squares and their sums are Python integers, the ratio is one Python division;
* the prediction takes the orbit from tests/nav_ref.py and tests/rate_ref.py and the local frame from tests/atm_ref.py, the
  references of the sections the text points to.

Law is a class so that tests/test_aided.py can derive wrong laws from it, one method each, and tell them from the right one."""
import math

import numpy as np

import atm_ref
import nav_ref
import rate_ref
import track_ref

TWO32 = 2 ** 32
FULL = 1023 * TWO32
L1, CPS = 1575.42e6, 1.023e6
AID_NO_FIX, AID_NO_EPH, AID_LOW, AID_OFF_GRID = 1, 2, 4, 8
KEPT, NO_AID, SHORT, FEW, NO_POWER, BELOW = 1, 2, 4, 8, 16, 32
NOT_DETECTED = NO_AID | FEW | NO_POWER | BELOW
INT_FIELDS = ("flags", "segments", "n_code", "n_dop", "best_h", "best_d", "lo_shift", "ca_shift", "best", "total", "floor")
RATIO_TOL = 1e-12  # relative: one fp64 division of two integers below 2^53
# gpsacq_aided_default_params' ratio_min: the largest ratio of 2304 draws on absent PRNs, 1.7376, plus a quarter of its excess over 1
# (include/gpsacq.h, DEFAULT RATIO_MIN)
RATIO_MIN = 1.922


def nco_words(lo_shift, fc, fs, step_hz=0.0):
    """refine step 1: (in range, lo_rate, ca_rate); step_hz <= 0 is the reference grid, lo_shift in FFT bins of fs / 40000"""
    if step_hz > 0:
        lo_dop = lo_shift * step_hz
    else:
        lo_dop = lo_shift * fs
        lo_dop = lo_dop / 40000.0
    ca_dop = lo_dop / L1
    ca_dop = ca_dop * CPS
    lo_f = fc + lo_dop
    ca_f = CPS + ca_dop
    if not (0 <= lo_f < fs and 0 <= ca_f < fs):
        return False, 0, 0
    lo_rate = lo_f / fs
    lo_rate = int(lo_rate * 4294967296.0)
    ca_rate = ca_f / fs
    ca_rate = int(ca_rate * 4294967296.0)
    return ca_rate != 0, lo_rate, ca_rate


class Law:
    """B. WINDOWED SEARCH.  Every method restates one sentence of the header; a mutant overrides one of them."""

    def lo_shift_of(self, lo_center, K, d):
        return lo_center - K + d

    def code_index(self, base, h, spm):
        """what multiplies ca_rate in P0(h, d): base + h, NOT reduced"""
        return base + h

    def base_of(self, ca_center, W, spm):
        return (ca_center - W) % spm

    def carrier_sample(self, j, spm):
        """the sample count the carrier phase is taken at: from the window's first sample"""
        return j

    def floor_of(self, spm, segments):
        return 2 * spm * segments

    def powers(self, samples01, o, segments, spm, prn, base, n_code, rates):
        """step 4: power(h, d), Python integers [n_dop][n_code]; rates: per d (valid, lo_rate, ca_rate).  samples01: 0/1 per sample"""
        j = np.arange(segments * spm, dtype=np.int64)
        v = 1 - 2 * samples01[o:o + segments * spm].astype(np.int64)
        c = track_ref.chips(prn)
        out = []
        for valid, lo_rate, ca_rate in rates:
            if not valid or segments == 0:
                out.append([0] * n_code)
                continue
            cb, sb = track_ref.carrier_signs((self.carrier_sample(j, spm) * lo_rate) % TWO32)
            re_, im_ = (v * (1 - 2 * cb)).astype(np.float64), (v * (1 - 2 * sb)).astype(np.float64)  # |sums| <= spm: exact in float64
            row = []
            for h in range(n_code):
                P = (self.code_index(base, h, spm) * ca_rate + j * ca_rate) % FULL
                chip = (1 - 2 * c[P // TWO32].astype(np.int64)).astype(np.float64)
                I = (chip * re_).reshape(segments, spm).sum(axis=1)
                Q = (chip * im_).reshape(segments, spm).sum(axis=1)
                row.append(sum(int(a) * int(a) + int(b) * int(b) for a, b in zip(I.tolist(), Q.tolist())))
            out.append(row)
        return out

    def powers_stream(self, samples01, o, segments, spm, prn, base, n_code, rates, carriers=None):
        """powers() once more through the sentence "the replica of h at sample j is the replica of h = 0 at sample j + h": ONE chip
        stream per d, every hypothesis a slice of it.  Still one product per sample and hypothesis (np.correlate), thirty times
        quicker; tests/test_aided.py holds it against powers(), tools/aided_floor.py measures the noise floor with it.
        carriers: per d (re_, im_) of this window where the caller has them already"""
        n = segments * spm
        v = (1 - 2 * samples01[o:o + n].astype(np.int64)).astype(np.float64)
        c = track_ref.chips(prn)
        q = np.arange(n + n_code - 1, dtype=np.int64)
        out = []
        for d, (valid, lo_rate, ca_rate) in enumerate(rates):
            if not valid or segments == 0:
                out.append([0] * n_code)
                continue
            if carriers is not None:
                cre, cim = carriers[d]
            else:
                cre, cim = carrier_pm((np.arange(n, dtype=np.int64) * lo_rate) % TWO32)
            stream = (1 - 2 * c[((base + q) * ca_rate % FULL) // TWO32].astype(np.int64)).astype(np.float64)
            re_, im_ = v * cre, v * cim
            acc = [0] * n_code
            for s in range(segments):
                seg = stream[s * spm:(s + 1) * spm + n_code - 1]
                I = np.correlate(seg, re_[s * spm:(s + 1) * spm], "valid")
                Q = np.correlate(seg, im_[s * spm:(s + 1) * spm], "valid")
                for h in range(n_code):
                    acc[h] += int(I[h]) * int(I[h]) + int(Q[h]) * int(Q[h])
            out.append(acc)
        return out


def carrier_pm(ph):
    """(+-1 of cos, +-1 of -sin) as float64 of uint32 phases (int64 array)"""
    cb, sb = track_ref.carrier_signs(ph)
    return (1 - 2 * cb).astype(np.float64), (1 - 2 * sb).astype(np.float64)


LAW = Law()


def aid_usable(a):
    return int(a["flags"]) == 0


def aided_search(bits, stride, tasks, aid, spm, fc, fs, kmax, step_hz=0.0, peaks_in=None, blocks=16, min_segments=1, code_half=16, dop_half=1,
                 keep_snr=25.0, ratio_min=RATIO_MIN, n_bytes=None, law=LAW, stream=False):
    """gpsacq_aided_search of the capture bits[:n_bytes] (uint8): tasks a list of (block, prn index) or None for (t, t % 32); aid a
    list of dicts or an AID_DTYPE array (flags, ca_center, lo_center are read); peaks_in None or PEAK_DTYPE rows.  Returns one
    dict per task: the fields of gpsacq_aided, `peak` (snr, lo_shift, ca_shift, max_pwr) and `powers` (uint64 [2K + 1][2W + 1]).
    stream: the sums by Law.powers_stream, the quicker spelling."""
    bits = np.asarray(bits, np.uint8).ravel()
    n_bytes = bits.size if n_bytes is None else int(n_bytes)
    samples01 = np.unpackbits(bits[:n_bytes], bitorder="little")
    total = 8 * n_bytes
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
        o = 8 * block * stride
        if not aid_usable(a) or not 0 <= ca_center < spm or block < 0 or not 0 <= prn < 32 or o >= total:  # 2. NO_AID
            continue
        rates = []
        for d in range(n_dop):  # 3. hypotheses
            lo = law.lo_shift_of(lo_center, K, d)
            ok, lo_rate, ca_rate = nco_words(lo, fc, fs, step_hz)
            rates.append((ok and abs(lo) <= kmax, lo_rate, ca_rate))
        if not any(r[0] for r in rates):
            continue
        fit = blocks * 40000 // spm
        segments = min(fit, (total - o) // spm)
        base = law.base_of(ca_center, W, spm)
        pw = (law.powers_stream if stream else law.powers)(samples01, o, segments, spm, prn + 1, base, n_code, rates)  # 4. sums
        best, best_d, best_h, tot = -1, 0, 0, 0
        for d in range(n_dop):  # 5. the key: larger power, then smaller d, then smaller h
            if not rates[d][0]:
                continue
            for h in range(n_code):
                tot += pw[d][h]
                if pw[d][h] > best:
                    best, best_d, best_h = pw[d][h], d, h
        floor = law.floor_of(spm, segments)
        ratio = float(best) / float(floor) if floor else 0.0
        flags = (SHORT if segments < fit else 0) | (FEW if segments < min_segments else 0) | (NO_POWER if best == 0 else 0)
        flags |= BELOW if ratio < ratio_min else 0
        rec.update(flags=flags, segments=segments, n_code=n_code, n_dop=n_dop, best_h=best_h, best_d=best_d, lo_shift=lo_center - K + best_d,
                   ca_shift=(base + best_h) % spm, best=best, total=tot, floor=floor, ratio=ratio, powers=np.array(pw, dtype=np.uint64))
        if not flags & NOT_DETECTED:  # 6. the output peak
            rec["peak"] = (float(np.float32(ratio)), rec["lo_shift"], rec["ca_shift"], float(np.float32(best)))
    return out


def same(got, ref, peaks=None, powers=None, label=""):
    """AIDED_DTYPE records (and PEAK_DTYPE peaks, uint64 powers [n][n_dop][n_code]) against aided_search()'s dicts: every integer
    equal, ratio within RATIO_TOL relative, peaks byte for byte.  Returns the largest relative difference of ratio."""
    got = np.asarray(got).ravel()
    assert got.size == len(ref), (label, got.size, len(ref))
    worst = 0.0
    for i, r in enumerate(ref):
        for f in INT_FIELDS:
            assert int(got[f][i]) == r[f], (label, i, f, int(got[f][i]), r[f])
        rel = abs(float(got["ratio"][i]) - r["ratio"]) / max(r["ratio"], 1e-300)
        assert rel <= RATIO_TOL, (label, i, float(got["ratio"][i]), r["ratio"])
        worst = max(worst, rel)
        if peaks is not None:
            pk = peaks.ravel()[i]
            want = np.zeros(1, pk.dtype)
            want[0] = tuple(r["peak"])
            assert pk.tobytes() == want.tobytes(), (label, i, pk, r["peak"])
        if powers is not None:
            assert np.array_equal(np.asarray(powers).reshape(len(ref), *r["powers"].shape)[i], r["powers"]), (label, i)
    return worst


# ---- A. PREDICTION ------------------------------------------------------------------------------------------------------------
def _turn(p, a):
    c, s = math.cos(a), math.sin(a)
    return np.array([p[0] * c - p[1] * s, p[0] * s + p[1] * c, p[2]])


def predict_one(eph, fix, vel, fs, spm, step_hz, kmax, elev_min_deg=5.0):
    """one (fix, channel): eph a nav_ref dict or None (not valid); fix and vel dicts / records (vel None: at rest).  Returns the
    fields of gpsacq_aid"""
    zero = dict(flags=0, ca_center=0, lo_center=0, reserved=0, tx_frac=0.0, doppler_hz=0.0, elev_deg=0.0)
    if int(fix["status"]) != 0:
        return dict(zero, flags=AID_NO_FIX)
    if eph is None:
        return dict(zero, flags=AID_NO_EPH)
    rr = np.array([float(fix["x"]), float(fix["y"]), float(fix["z"])])
    rx_ms, rx_frac = int(fix["rx_ms"]), float(fix["rx_frac"])
    # light time: COARSE A's two passes, times counted from the receive instant
    tau, cc = 75e-3, 0.0
    for _ in range(2):
        ms, frac = nav_ref.split_time(rx_ms, rx_frac + -tau)
        p, dt = nav_ref.sat_state(eph, int(ms), float(frac))
        tau = float(np.linalg.norm(rr - _turn(p[0], -nav_ref.OMEGA_E * tau))) / nav_ref.C
        cc = float(dt[0])
    ms, tx_frac = nav_ref.split_time(rx_ms, rx_frac + (cc - tau))
    ms, tx_frac = int(ms), float(tx_frac)
    ca_center = int(np.rint(tx_frac * fs)) % spm
    # Doppler: VELOCITY's row read backwards, the satellite at the uncorrected time T
    p, dt = nav_ref.sat_state(eph, ms, tx_frac)
    v, cd = rate_ref.sat_rate(eph, ms, tx_frac)
    om = nav_ref.OMEGA_E
    th = om * (float(nav_ref.fold_ms(ms - rx_ms)) * 1e-3 + ((tx_frac - float(dt[0])) - rx_frac))
    ri = _turn(p[0], th)
    vi = _turn(v[0] + np.array([-om * p[0][1], om * p[0][0], 0.0]), th)
    e = (ri - rr) / np.linalg.norm(ri - rr)
    vr, drift = np.zeros(3), 0.0
    if vel is not None and int(vel["status"]) == 0:
        vr, drift = np.array([float(vel["vx"]), float(vel["vy"]), float(vel["vz"])]), float(vel["drift"])
    rho = float(e @ (vi - (vr + np.array([-om * rr[1], om * rr[0], 0.0])))) + nav_ref.C * drift - nav_ref.C * float(cd[0])
    doppler = -(L1 / nav_ref.C) * rho
    lat, lon, _ = atm_ref.geodetic(rr)
    _, el = atm_ref.view(lat, lon, ri - rr)
    elev = float(el) * 180.0 / math.pi
    if not (np.all(np.isfinite(ri)) and math.isfinite(doppler) and math.isfinite(tx_frac) and math.isfinite(elev)):
        return dict(zero, flags=AID_NO_EPH)
    lo_center = int(np.rint(doppler / step_hz))
    flags = (AID_LOW if elev < elev_min_deg else 0) | (AID_OFF_GRID if abs(lo_center) > kmax else 0)
    return dict(flags=flags, ca_center=ca_center, lo_center=lo_center, reserved=0, tx_frac=tx_frac, doppler_hz=doppler, elev_deg=elev)


def predict(ephs, fixes, vels, n_chans, fs, spm, step_hz, kmax, elev_min_deg=5.0):
    """gpsacq_aid_predict: ephs a list of nav_ref dicts (None: not valid), fixes FIX_DTYPE records, vels VEL_DTYPE records or None.
    Returns [n_fix][n_chans] dicts"""
    return [[predict_one(ephs[c] if c < len(ephs) else None, fixes[f], None if vels is None else vels[f], fs, spm, step_hz, kmax, elev_min_deg)
             for c in range(n_chans)] for f in range(len(fixes))]
