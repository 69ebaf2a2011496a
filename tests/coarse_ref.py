"""Reference of the coarse-time fix tests: a float64 numpy restatement of "Coarse-time fixes: positions from code phases alone"
of include/gpsacq.h, written from that text and not from the kernel.  The orbit is tests/nav_ref.py's, velocity and clock drift are
tests/rate_ref.py's analytic ones (themselves checked against central differences in tests/test_rate_ref.py).

A batch of rows at a time, because nav_ref evaluates one ephemeris at many times in one call: the satellite states of all rows
are made per ephemeris, everything after that is per row -- steps A (whole milliseconds, with the smallest rounding margin of the
row), B (five unknowns, numpy.linalg.solve on the weighted normal equations) and C (records).  The dilution figures invert the
normal matrix after scaling it to a unit diagonal, so that the reference's own error is that of the scaled matrix (a Cholesky
factorisation, which the kernel uses, has that property by itself).
"""
import math

import numpy as np

import atm_ref
import nav_ref
import rate_ref

C = nav_ref.C
OMEGA_E = nav_ref.OMEGA_E
WEEK_MS = nav_ref.WEEK_MS
FIX_OK, FIX_TOO_FEW, FIX_NO_CONVERGE = 0, 1, 2
INCONSISTENT = 1
RMS_MAX_M = C / 1.023e6


def split(t):
    """t seconds (array) into (whole milliseconds, fraction in [0, 1e-3)): FIX's rule"""
    t = np.asarray(t, np.float64)
    k = np.floor(t * 1e3)
    frac = t - k * 1e-3
    lo = frac < 0.0
    k, frac = np.where(lo, k - 1, k), np.where(lo, frac + 1e-3, frac)
    hi = frac >= 1e-3
    k, frac = np.where(hi, k + 1, k), np.where(hi, frac - 1e-3, frac)
    return k.astype(np.int64), frac


def turn(p, a):
    """R(a) p: p (..., 3) about z by the angles a (...)"""
    ca, sa = np.cos(a), np.sin(a)
    return np.stack([p[..., 0] * ca - p[..., 1] * sa, p[..., 0] * sa + p[..., 1] * ca, p[..., 2]], axis=-1)


def usable(eph_index, valid, tx_frac, weight, n_eph):
    ok = (valid != 0) & (eph_index >= 0) & (eph_index < n_eph) & np.isfinite(weight) & (weight >= 0.0)
    with np.errstate(invalid="ignore"):
        ok &= np.isfinite(tx_frac) & (tx_frac >= 0.0) & (tx_frac < 1e-3)
    return ok


def _states(ephs, eph_index, use, ms, frac, rates=False):
    """satellite states of the entries `use` of [n][m] arrays: p (n, m, 3), cc (n, m) and, with rates, v (n, m, 3), d (n, m)"""
    p, cc = np.zeros(use.shape + (3,)), np.zeros(use.shape)
    v, d = np.zeros(use.shape + (3,)), np.zeros(use.shape)
    for e in np.unique(eph_index[use]):
        sel = use & (eph_index == e)
        p[sel], cc[sel] = nav_ref.sat_state(ephs[e], ms[sel], frac[sel])
        if rates:
            v[sel], d[sel] = rate_ref.sat_rate(ephs[e], ms[sel], frac[sel])
    return (p, cc, v, d) if rates else (p, cc)


def whole_ms(ephs, eph_index, use, tx_frac, prior_xyz, rx_ms):
    """Step A: (ref (n,), N (n, m), smallest rounding margin per row in milliseconds; 0.5 where no column was rounded)"""
    n, m = use.shape
    tau = np.full((n, m), 75e-3)
    for _ in range(2):
        k, frac = split(-tau)
        p, cc = _states(ephs, eph_index, use, (rx_ms[:, None] + k) % WEEK_MS, frac)
        d = prior_xyz[:, None, :] - turn(p, -OMEGA_E * tau)
        tau = np.where(use, np.sqrt((d * d).sum(-1)) / C, 75e-3)
    P = cc - tau
    ref = np.where(use.any(1), use.argmax(1), -1)
    r = np.maximum(ref, 0)
    rows = np.arange(n)
    Nr = np.rint((P[rows, r] - tx_frac[rows, r]) * 1e3)
    delta = Nr * 1e-3 + tx_frac[rows, r] - P[rows, r]
    x = (delta[:, None] + P - tx_frac) * 1e3
    N = np.rint(x)
    N[rows, r] = Nr
    others = use.copy()
    others[rows, r] = False  # the reference's own rounding picks the common integer, which is free: only the others can go wrong
    margin = np.where(others, 0.5 - np.abs(x - N), 0.5).min(1)
    return ref, np.where(use, N, 0).astype(np.int64), margin


def _rows(ephs, eph_index, use, tx_frac, N, rx_ms, pos, b, s):
    """at the states given (pos (n, 3), b (n,), s (n,)): rows h (n, m, 5), residuals (n, m), and the split of the uncorrected
    times T_k + s as millisecond of week and fraction"""
    k, frac = split(tx_frac + s[:, None])
    ms = (rx_ms[:, None] + N + k) % WEEK_MS
    p, cc, v, d = _states(ephs, eph_index, use, ms, frac, rates=True)
    rho = C * (cc - (N * 1e-3 + tx_frac)) - b[:, None]
    th = -OMEGA_E * rho / C
    los = pos[:, None, :] - turn(p, th)
    rng = np.sqrt((los * los).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = los / rng[..., None]
    hs = -(C * d + (u * turn(v, th)).sum(-1))
    H = np.concatenate([u, np.ones(use.shape + (1,)), hs[..., None]], axis=-1)
    return H, rho - rng, ms, frac


def positive_definite(A):
    """the pivot rule of the text: Cholesky's pivots, each above 1e-13 of its diagonal entry (the first: above 0)"""
    n = len(A)
    L = np.zeros((n, n))
    for j in range(n):
        p = A[j, j] - (L[j, :j] ** 2).sum()
        if not p > (0.0 if j == 0 else 1e-13 * A[j, j]):
            return False
        L[j, j] = math.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return True


def dilution(H):
    """(pdop, cdop) of the five-column H: from (H^T H)^-1, inverted at a unit diagonal; (0, 0) where that fails"""
    A = H.T @ H
    dg = np.diag(A)
    if not positive_definite(A):
        return 0.0, 0.0
    D = 1.0 / np.sqrt(dg)
    try:
        Q = np.linalg.inv(A * np.outer(D, D)) * np.outer(D, D)
    except np.linalg.LinAlgError:
        return 0.0, 0.0
    if not (np.all(np.isfinite(Q)) and np.all(np.diag(Q) > 0)):
        return 0.0, 0.0
    return math.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]), math.sqrt(Q[4, 4])


def coarse_fix(ephs, obs, prior, rms_max_m=RMS_MAX_M, hold_s=False):
    """obs: an OBS_DTYPE array [n_fix][sats] (eph, valid, tx_frac and weight are read), prior: a COARSE_PRIOR_DTYPE array [n_fix].
    Returns one dict per row: status, n_used, iterations, ref, flags, margin (ms), N ((sats,) whole milliseconds), and for a fix
    that is FIX_OK xyz, rx_ms, rx_frac, lat, lon, alt, rms, coarse_s, bias_m, pdop, cdop, H (the rows h of the usable columns at the
    final state) and obs_out ({column: (tx_ms, tx_frac)}).
    hold_s: the model WITHOUT its fifth unknown (s stays 0), to show what it is for."""
    n, m = obs.shape
    eph_index = obs["eph"].astype(np.int64)
    tx_frac = obs["tx_frac"].astype(np.float64)
    weight = obs["weight"].astype(np.float64)
    prior_xyz = np.stack([prior["x"], prior["y"], prior["z"]], 1).astype(np.float64)
    rx_ms = prior["rx_ms"].astype(np.int64)
    use = usable(eph_index, obs["valid"], tx_frac, weight, len(ephs))
    tx_frac = np.where(use, tx_frac, 0.0)
    ref, N, margin = whole_ms(ephs, eph_index, use, tx_frac, prior_xyz, rx_ms)
    out = [dict(status=FIX_TOO_FEW, n_used=int(use[i].sum()), iterations=0, ref=int(ref[i]), flags=0, margin=float(margin[i]), N=N[i], obs_out={})
           for i in range(n)]
    pos, b, s, rms = prior_xyz.copy(), np.zeros(n), np.zeros(n), np.zeros(n)
    active = use.sum(1) >= 5
    done = np.zeros(n, bool)
    for i in np.nonzero(active)[0]:
        out[i]["status"] = FIX_NO_CONVERGE
    for _ in range(20):
        if not active.any():
            break
        H, res, _, _ = _rows(ephs, eph_index, use & active[:, None], tx_frac, N, rx_ms, pos, b, s)
        for i in np.nonzero(active)[0]:
            c = use[i]
            h, r, w = (H[i, c, :4] if hold_s else H[i, c]), res[i, c], weight[i, c]
            active[i] = False  # until the step is made
            if not w.sum() > 0:
                continue
            rms[i] = math.sqrt(float((w * r * r).sum() / w.sum()))
            A = h.T @ (w[:, None] * h)
            if not positive_definite(A):
                continue
            step = np.linalg.solve(A, h.T @ (w * r))
            if not np.all(np.isfinite(step)):
                continue
            if hold_s:
                step = np.append(step, 0.0)
            pos[i], b[i], s[i] = pos[i] + step[:3], b[i] + step[3], s[i] + step[4]
            out[i]["iterations"] += 1
            if not abs(s[i]) < 302400.0:
                continue
            if math.sqrt(float((step[:3] ** 2).sum())) < 1e-4 and abs(step[4]) < 1e-7:
                done[i] = True
            else:
                active[i] = True
    if done.any():
        H, _, ms, frac = _rows(ephs, eph_index, use & done[:, None], tx_frac, N, rx_ms, pos, b, s)
        k, f = split(s - b / C)
        for i in np.nonzero(done)[0]:
            c = use[i] & (weight[i] > 0)
            pd, cd = dilution(H[i, c]) if c.any() else (0.0, 0.0)
            lat, lon, alt = atm_ref.geodetic(pos[i])
            out[i].update(status=FIX_OK, xyz=pos[i].copy(), rx_ms=int((rx_ms[i] + k[i]) % WEEK_MS), rx_frac=float(f[i]), lat=lat, lon=lon, alt=alt,
                          rms=float(rms[i]), coarse_s=float(s[i]), bias_m=float(b[i]), pdop=pd, cdop=cd, H=H[i, use[i]],
                          obs_out={int(j): (int(ms[i, j]), float(frac[i, j])) for j in np.nonzero(use[i])[0]})
            if out[i]["n_used"] >= 6 and rms[i] > rms_max_m:
                out[i]["flags"] |= INCONSISTENT
    return out


def coarse_obs(peaks, fs, snr_min):
    """k_coarse_obs's arithmetic: (valid, eph, tx_frac, weight) arrays of peaks' shape [n_fix][n_chans]"""
    valid = (peaks["snr"].astype(np.float64) >= snr_min) & (peaks["ca_shift"] >= 0) & (peaks["ca_shift"].astype(np.float64) < fs / 1000.0)
    eph = np.broadcast_to(np.arange(peaks.shape[1]), peaks.shape)
    return valid, np.where(valid, eph, 0), np.where(valid, peaks["ca_shift"].astype(np.float64) / fs, 0.0), np.where(valid, 1.0, 0.0)
