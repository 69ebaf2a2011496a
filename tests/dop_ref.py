"""An independent reference of "Cold snapshot fixes: fine Doppler and a Doppler-only position solver" of include/gpsacq.h, written
in numpy and Python integers from that text.  It shares no code with csrc/doppler_kernels.hip:

* fine_doppler(): the NCO words and the per-sample prompt sums are tests/refine_ref.py's (nco_words, segment_sums: sample by
  sample, no words, no masks, no popcounts); the squares and the lag-1 sums are Python integers of any size, so a sum that left 63
  bits would show instead of wrapping; the estimate is Python floats with math.atan2 and math.hypot.
* lag_sums() / estimate(): the same arithmetic on hand-made (I, Q) sequences.
* rate_obs_fine(): the rule of RATE OBSERVATIONS.
* doppler_fix(): the solver on the orbit functions of tests/nav_ref.py and tests/rate_ref.py (through coarse_ref._states), numpy's
  linear solve, atm_ref.geodetic.

same() and same_fix() compare DOPFINE_DTYPE and DOPPLER_FIX_DTYPE arrays against the dicts."""
import math

import numpy as np

import atm_ref
import coarse_ref
import nav_ref
import refine_ref

TWO32 = 2 ** 32
FULL = 1023 * TWO32
L1 = 1575.42e6
C = nav_ref.C
OMEGA_E = nav_ref.OMEGA_E
WEEK_MS = nav_ref.WEEK_MS
NO_HIT, SHORT, NO_POWER, FEW, WEAK = 1, 2, 4, 8, 16
FIX_OK, FIX_TOO_FEW, FIX_NO_CONVERGE = 0, 1, 2
INCONSISTENT = 1
RMS_MAX_MPS = 3.0
INT_FIELDS = ("flags", "segments", "lo_rate", "ca_rate", "re", "im", "mag", "power")
# two correctly rounded atan2s differ by a few ulp of pi, under 1e-12 Hz after the division by 4 pi T; 1e-9 Hz leaves three
# decades over that and sits nine decades below the physics.  coherence is a quotient of two numbers near 1e18 .. 1e30 in (0, 1]
DF_TOL, COHERENCE_TOL = 1e-9, 1e-12
PLACE_TOL, DRIFT_TOL = 1e-3, 1e-13  # two Newton runs that stop at 1e-3 m from identical starts, in fp64


# ---- 1. fine Doppler -----------------------------------------------------------------------------------------------------------
def lag_sums(iq):
    """LAG-1 SUMS of a sequence of (I, Q) pairs: (re, im, mag, power) as Python integers"""
    iq = [(int(i), int(q)) for i, q in iq]
    sq = [(i * i - q * q, 2 * i * q, i * i + q * q) for i, q in iq]
    re = sum(sq[s][0] * sq[s - 1][0] + sq[s][1] * sq[s - 1][1] for s in range(1, len(sq)))
    im = sum(sq[s][1] * sq[s - 1][0] - sq[s][0] * sq[s - 1][1] for s in range(1, len(sq)))
    mag = sum(sq[s][2] * sq[s - 1][2] for s in range(1, len(sq)))
    return re, im, mag, sum(p for _, _, p in sq)


def estimate(re, im, mag, spm, fs, fc, lo_rate):
    """ESTIMATE: (no power, coherence, df_hz, doppler_hz)"""
    if mag == 0 or (re == 0 and im == 0):
        return True, 0.0, 0.0, 0.0
    T = float(spm) / fs
    df = math.atan2(float(im), float(re)) / ((4.0 * 3.141592653589793) * T)
    return False, math.hypot(float(re), float(im)) / float(mag), df, ((float(lo_rate) * fs) / 4294967296.0 - fc) + df


def record(iq, fit, spm, fs, fc, lo_rate, ca_rate, min_segments=2, coherence_min=0.0):
    """the record of a hit from its per-segment (I, Q): everything from SQUARES on"""
    re, im, mag, power = lag_sums(iq)
    assert -2 ** 63 <= re < 2 ** 63 and -2 ** 63 <= im < 2 ** 63 and mag < 2 ** 64 and power < 2 ** 64, "OVERFLOW: the bound of the text is wrong"
    none, coh, df, dop = estimate(re, im, mag, spm, fs, fc, lo_rate)
    flags = (SHORT if len(iq) < fit else 0) | (FEW if len(iq) < min_segments else 0) | (NO_POWER if none else 0) | (WEAK if coh < coherence_min else 0)
    return dict(flags=flags, segments=len(iq), lo_rate=lo_rate, ca_rate=ca_rate, re=re, im=im, mag=mag, power=power, coherence=coh, df_hz=df,
                doppler_hz=dop)


def fine_doppler(bits, stride, tasks, peaks, spm, fc, fs, step_hz=0.0, blocks=16, min_segments=2, snr_min=25.0, coherence_min=0.0, n_bytes=None):
    """gpsacq_fine_doppler of the capture bits[:n_bytes] (uint8): tasks a list of (block, prn index) or None for (t, t % 32); peaks a
    PEAK_DTYPE array or a list of (snr, lo_shift, ca_shift, ...) rows.  Returns a list of dicts."""
    bits = np.asarray(bits, np.uint8).ravel()
    n_bytes = bits.size if n_bytes is None else int(n_bytes)
    samples01 = np.unpackbits(bits[:n_bytes], bitorder="little")
    total = 8 * n_bytes
    out = []
    rows = peaks.ravel().tolist() if isinstance(peaks, np.ndarray) else list(peaks)
    for t, pk in enumerate(rows):
        snr, lo_shift, ca_shift = float(pk[0]), int(pk[1]), int(pk[2])
        block, prn = (t, t % 32) if tasks is None else (int(tasks[t][0]), int(tasks[t][1]))
        ok, lo_rate, ca_rate = refine_ref.nco_words(lo_shift, fc, fs, step_hz)
        o = 8 * block * stride
        if not (snr >= snr_min) or not 0 <= ca_shift < spm or block < 0 or not 0 <= prn < 32 or o >= total or not ok or ca_rate == 0:
            out.append(dict(flags=NO_HIT, segments=0, lo_rate=0, ca_rate=0, re=0, im=0, mag=0, power=0, coherence=0.0, df_hz=0.0, doppler_hz=0.0))
            continue
        fit = blocks * 40000 // spm
        segments = min(fit, (total - o) // spm)
        P0 = (ca_shift * ca_rate) % FULL
        sums = refine_ref.segment_sums(samples01, o, segments, spm, prn + 1, lo_rate, ca_rate, P0, TWO32 // 4)  # columns 2, 3: I_P, Q_P
        out.append(record([(r[2], r[3]) for r in sums.tolist()], fit, spm, fs, fc, lo_rate, ca_rate, min_segments, coherence_min))
    return out


def usable(rec):
    return not int(rec["flags"]) & (NO_HIT | NO_POWER | FEW | WEAK)


def same(got, ref, label=""):
    """a DOPFINE_DTYPE array against fine_doppler()'s dicts: every integer field equal, df_hz and doppler_hz within DF_TOL,
    coherence within COHERENCE_TOL.  Returns the three largest differences (coherence, df_hz, doppler_hz)."""
    got = np.asarray(got).ravel()
    assert got.size == len(ref), (label, got.size, len(ref))
    worst = [0.0, 0.0, 0.0]
    for i, r in enumerate(ref):
        for f in INT_FIELDS:
            assert int(got[f][i]) == r[f], (label, i, f, int(got[f][i]), r[f])
        d = [abs(float(got[f][i]) - r[f]) for f in ("coherence", "df_hz", "doppler_hz")]
        assert d[0] <= COHERENCE_TOL and d[1] <= DF_TOL and d[2] <= DF_TOL, (label, i, d)
        worst = [max(a, b) for a, b in zip(worst, d)]
    return worst


def rate_obs_fine(peaks, dopfine, snr_min):
    """RATE OBSERVATIONS: (valid, doppler_hz, weight) arrays of peaks' shape; dopfine: a DOPFINE_DTYPE array of that shape"""
    valid = (peaks["snr"].astype(np.float64) >= snr_min) & ((dopfine["flags"] & (NO_HIT | NO_POWER | FEW | WEAK)) == 0) & np.isfinite(dopfine["doppler_hz"])
    return valid, np.where(valid, dopfine["doppler_hz"], 0.0), np.where(valid, 1.0, 0.0)


# ---- 2. Doppler fix ------------------------------------------------------------------------------------------------------------
def usable_columns(ephs, obs, rate_obs, rx_ms, eph_valid=None):
    """USABLE of the text: bool [n][m]"""
    e = obs["eph"].astype(np.int64)
    ok = (obs["valid"] != 0) & (rate_obs["valid"] != 0) & (e >= 0) & (e < len(ephs)) & np.isfinite(rate_obs["doppler_hz"])
    with np.errstate(invalid="ignore"):
        ok &= np.isfinite(rate_obs["weight"]) & (rate_obs["weight"] >= 0.0)
    good = np.ones(len(ephs), bool) if eph_valid is None else np.asarray(eph_valid, bool)
    ok &= good[np.clip(e, 0, len(ephs) - 1)]
    return ok & ((rx_ms >= 0) & (rx_ms < WEEK_MS))[:, None]


def satellites(ephs, eph_index, use, rx_ms, tau):
    """SATELLITE: r and vi (n, m, 3) and the clock drift d (n, m) of the usable columns at their light times tau (n, m)"""
    k, frac = coarse_ref.split(-tau)
    p, _, v, d = coarse_ref._states(ephs, eph_index, use, (rx_ms[:, None] + k) % WEEK_MS, frac, rates=True)
    a = -OMEGA_E * tau
    q = v + np.stack([-OMEGA_E * p[..., 1], OMEGA_E * p[..., 0], np.zeros(use.shape)], -1)
    return coarse_ref.turn(p, a), coarse_ref.turn(q, a), d


def rows(r, vi, d, doppler_hz, pos, g):
    """PASS: the rows h (n, m, 4), the residuals, the predictions and the ranges (n, m) at the state pos (n, 3), g (n,)"""
    D = r - pos[:, None, :]
    rng = np.sqrt((D * D).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):  # columns and rows that are not in use have no range
        inv = 1.0 / rng
        e = D * inv[..., None]
    w = vi - np.stack([-OMEGA_E * pos[:, 1], OMEGA_E * pos[:, 0], np.zeros(len(pos))], -1)[:, None, :]
    ew = (e * w).sum(-1)
    pred = (ew + g[:, None]) - C * d
    res = -(C / L1) * doppler_hz - pred
    h = -(w - ew[..., None] * e) * inv[..., None] + np.stack([-OMEGA_E * e[..., 1], OMEGA_E * e[..., 0], np.zeros(e.shape[:2])], -1)
    return np.concatenate([h, np.ones(e.shape[:2] + (1,))], -1), res, pred, rng


def pdop_of(H):
    """sqrt of the trace of the position block of (H^T H)^-1, inverted at a unit diagonal; 0 where the pivot rule fails"""
    A = H.T @ H
    if not coarse_ref.positive_definite(A):
        return 0.0
    s = 1.0 / np.sqrt(np.diag(A))
    try:
        Q = np.linalg.inv(A * np.outer(s, s)) * np.outer(s, s)
    except np.linalg.LinAlgError:
        return 0.0
    pd = math.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]) if Q[0, 0] + Q[1, 1] + Q[2, 2] > 0 else float("nan")
    return pd if math.isfinite(pd) else 0.0


def doppler_fix(ephs, obs, rate_obs, rx_ms, rms_max_mps=RMS_MAX_MPS, eph_valid=None):
    """obs: OBS_DTYPE [n_fix][sats] (eph and valid are read), rate_obs: RATE_OBS_DTYPE of that shape, rx_ms: int (n_fix,).  Returns
    one dict per row: status, n_used, iterations, flags, and for FIX_OK xyz, lat, lon, alt, drift, rms, pdop, H (the rows of the
    usable columns the last step was made from); prior: (x, y, z), NaN where the row gives none."""
    n, m = obs.shape
    rx_ms = np.broadcast_to(np.asarray(rx_ms, np.int64).ravel(), (n,)).copy()
    eph_index = obs["eph"].astype(np.int64)
    dop = np.where(np.isfinite(rate_obs["doppler_hz"]), rate_obs["doppler_hz"], 0.0)
    weight = rate_obs["weight"].astype(np.float64)
    use = usable_columns(ephs, obs, rate_obs, rx_ms, eph_valid)
    nan3 = (float("nan"),) * 3
    out = [dict(status=FIX_TOO_FEW, n_used=int(use[i].sum()), iterations=0, flags=0, prior=nan3) for i in range(n)]
    tau = np.full((n, m), 75e-3)
    pos, g, rms = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    active = use.sum(1) >= 4
    for i in np.nonzero(active)[0]:
        out[i]["status"] = FIX_NO_CONVERGE
    if active.any():  # START
        r, _, _ = satellites(ephs, eph_index, use & active[:, None], rx_ms, tau)
        for i in np.nonzero(active)[0]:
            c = use[i]
            u = (r[i, c] * (1.0 / np.sqrt((r[i, c] ** 2).sum(-1)))[:, None]).sum(0)
            un = math.sqrt(float((u * u).sum()))
            if un >= 1e-6:
                pos[i] = 6371000.0 * u / un
            else:
                active[i] = False
    done = np.zeros(n, bool)
    for _ in range(20):
        if not active.any():
            break
        cols = use & active[:, None]
        r, vi, d = satellites(ephs, eph_index, cols, rx_ms, tau)
        H, res, _, rng = rows(r, vi, d, dop, pos, g)
        tau = np.where(cols, rng / C, tau)
        for i in np.nonzero(active)[0]:
            c = use[i]
            h, rr, w = H[i, c], res[i, c], weight[i, c]
            active[i] = False  # until the step is made
            if not w.sum() > 0:
                continue
            rms[i] = math.sqrt(float((w * rr * rr).sum() / w.sum()))
            A = h.T @ (w[:, None] * h)
            if not coarse_ref.positive_definite(A):
                continue
            s = 1.0 / np.sqrt(np.diag(A))  # the solve at a unit diagonal: metres and metres per second differ by 1e4
            step = np.linalg.solve(A * np.outer(s, s), (h.T @ (w * rr)) * s) * s
            if not np.all(np.isfinite(step)):
                continue
            pos[i], g[i] = pos[i] + step[:3], g[i] + step[3]
            out[i]["iterations"] += 1
            if not math.sqrt(float((pos[i] ** 2).sum())) <= 1e8:
                continue
            if math.sqrt(float((step[:3] ** 2).sum())) < 1e-3:
                done[i] = True
                cw = c & (weight[i] > 0)
                lat, lon, alt = atm_ref.geodetic(pos[i])
                out[i].update(status=FIX_OK, xyz=pos[i].copy(), lat=lat, lon=lon, alt=alt, drift=float(g[i] / C), rms=float(rms[i]),
                              pdop=pdop_of(H[i, cw]) if cw.any() else 0.0, H=h.copy())
                if out[i]["n_used"] >= 5 and rms[i] > rms_max_mps:
                    out[i]["flags"] |= INCONSISTENT
                else:
                    out[i]["prior"] = tuple(float(v) for v in pos[i])
            else:
                active[i] = True
    return out


def same_fix(got, prior, ref, rx_ms, label=""):
    """DOPPLER_FIX_DTYPE and COARSE_PRIOR_DTYPE arrays against doppler_fix()'s dicts: status, n_used, iterations and flags equal; a
    FIX_OK row's place within PLACE_TOL, drift within DRIFT_TOL, lat / lon within 1e-9 rad and alt within 2 mm (PLACE_TOL through
    the geodetic formulas, doubled), rms within 1e-6 m/s (PLACE_TOL times the largest entry of a row, 2e-4 per second, rounded up)
    and pdop within 1e-4 of itself (fp64's 1e-16 times the condition of the unscaled H^T H, metres against metres per second:
    below 1e12); any other row all zeros; the priors' places equal the fixes' or NaN.  Returns the largest differences (place,
    drift)."""
    got, prior = np.asarray(got).ravel(), np.asarray(prior).ravel()
    rx_ms = np.broadcast_to(np.asarray(rx_ms, np.int64).ravel(), (len(ref),))
    assert got.size == len(ref) == prior.size, (label, got.size, len(ref), prior.size)
    worst = [0.0, 0.0]
    for i, r in enumerate(ref):
        for f in ("status", "n_used", "iterations", "flags"):
            assert int(got[f][i]) == r[f], (label, i, f, int(got[f][i]), r[f])
        assert int(prior["rx_ms"][i]) == int(rx_ms[i]) and int(prior["reserved"][i]) == 0, (label, i)
        pxyz = np.array([prior["x"][i], prior["y"][i], prior["z"][i]])
        if r["status"] != FIX_OK:
            assert got[i].tobytes()[16:] == bytes(72) and np.isnan(pxyz).all(), (label, i)
            continue
        xyz = np.array([got["x"][i], got["y"][i], got["z"][i]])
        d_place, d_drift = float(np.linalg.norm(xyz - r["xyz"])), abs(float(got["drift"][i]) - r["drift"])
        assert d_place <= PLACE_TOL and d_drift <= DRIFT_TOL, (label, i, d_place, d_drift)
        assert abs(got["lat"][i] - r["lat"]) <= 1e-9 and abs(got["lon"][i] - r["lon"]) <= 1e-9 and abs(got["alt"][i] - r["alt"]) <= 2e-3, (label, i)
        assert abs(got["rms"][i] - r["rms"]) <= 1e-6 and abs(got["pdop"][i] - r["pdop"]) <= 1e-4 * r["pdop"], (label, i, got["rms"][i], r["rms"],
                                                                                                             got["pdop"][i], r["pdop"])
        if r["flags"] & INCONSISTENT:
            assert np.isnan(pxyz).all(), (label, i)
        else:
            assert (pxyz == xyz).all(), (label, i)
        worst = [max(worst[0], d_place), max(worst[1], d_drift)]
    return worst
