"""Reference of the velocity tests: the models of include/gpsacq.h ("Carrier observables", "Velocity and clock drift") in Python
integers and numpy.float64, written from that text and not from the kernels.

  * accumulated Doppler per epoch (the forward prefix sum), the rate observation, and a lane-by-lane restatement of the chunk /
    run / scan indexing the header prescribes for k_carrier_acc;
  * a forward simulator of the carrier NCO over fabricated records (lo_phase bookkeeping only);
  * analytic satellite velocity and clock drift;
  * the first-order velocity solve (numpy.linalg.solve on the weighted normal equations) and its gain matrix.

Nothing here loads the library except for the record dtypes."""
import math

import numpy as np

import nav_ref

M64 = (1 << 64) - 1
L1 = 1575.42e6
TWO32 = 4294967296.0
VEL_OK, VEL_TOO_FEW, VEL_NO_FIX, VEL_SINGULAR = 0, 1, 2, 3


def s64(v):
    """two's-complement reading of v mod 2^64"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def d_word(lo_rate, nom_word):
    """d_t: the difference wraps in 32 bits and is then sign-extended"""
    v = (int(lo_rate) - int(nom_word)) & 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def carrier_acc(samples, lo_rates, next_sample, nom_word):
    """[A_0 .. A_n] of the model, signed 64-bit values as Python integers"""
    n = len(samples)
    acc = [0] * (n + 1)
    for t in range(n):
        end = int(samples[t + 1]) if t + 1 < n else int(next_sample)
        acc[t + 1] = s64(acc[t] + (end - int(samples[t])) * d_word(lo_rates[t], nom_word))
    return acc


def carrier_acc_lanes(samples, lo_rates, next_sample, nom_word, lanes=64, run=4):
    """The same numbers by the kernel's prescribed indexing: chunks of lanes * run epochs, each lane summing `run` consecutive
    epochs, one inclusive scan over the lanes by doubling offsets (a lane takes from the lane `off` below it when there is one),
    a 64-bit carry between chunks.  Writes A_0 = 0 and A_{t+1} for every epoch t < n; returns the list, None where nothing was
    written."""
    n = len(samples)
    out = [None] * (n + 1)
    out[0] = 0
    carry = 0
    chunk = lanes * run
    for base in range(0, n, chunk):
        pre = [[0] * run for _ in range(lanes)]
        tot = [0] * lanes
        for lane in range(lanes):
            t0 = base + lane * run
            acc = 0
            for j in range(run):
                t = t0 + j
                if t < n:
                    end = int(samples[t + 1]) if t + 1 < n else int(next_sample)
                    acc = (acc + ((end - int(samples[t])) & M64) * (d_word(lo_rates[t], nom_word) & M64)) & M64
                pre[lane][j] = acc
            tot[lane] = acc
        incl = list(tot)
        off = 1
        while off < lanes:
            incl = [(incl[l] + incl[l - off]) & M64 if l >= off else incl[l] for l in range(lanes)]
            off <<= 1
        for lane in range(lanes):
            left = (carry + incl[lane] - tot[lane]) & M64
            for j in range(run):
                t = base + lane * run + j
                if t < n:
                    out[t + 1] = s64(left + pre[lane][j])
        carry = (carry + incl[lanes - 1]) & M64
    return out


def acc_at(samples, lo_rates, acc, nom_word, X):
    """A(X) for samples[0] <= X < next_sample"""
    t = int(np.searchsorted(np.asarray(samples, np.uint64), np.uint64(X), side="right")) - 1
    return s64(acc[t] + (X - int(samples[t])) * d_word(lo_rates[t], nom_word))


def rate_observation(samples, lo_rates, next_sample, acc, nom_word, R, W, fs):
    """(adr, doppler_hz) of receive sample R, or None when the observation cannot be made"""
    n = len(samples)
    Ra = R - W // 2
    Rb = Ra + W
    if n == 0 or Ra < int(samples[0]) or R >= int(next_sample) or Rb >= int(next_sample):
        return None
    D = s64(acc_at(samples, lo_rates, acc, nom_word, Rb) - acc_at(samples, lo_rates, acc, nom_word, Ra))
    num = np.float64(D) * np.float64(fs)          # one rounding
    den = np.float64(W) * np.float64(TWO32)       # exact
    return acc_at(samples, lo_rates, acc, nom_word, R), num / den


def nominal_words(chans):
    """the 1-bit rule: (uint32)((uint64)lo_nom >> 32)"""
    return [(int(v) & M64) >> 32 for v in chans["lo_nom"]]


def rate_observables(records, n_epochs, chans, nom_words, first_rx_sample, rx_step, n_fix, avg_samples, fs):
    """RATE_OBS_DTYPE [n_fix][n_chans] of the model"""
    import gpsacq
    n_chans = len(n_epochs)
    out = np.zeros((n_fix, n_chans), gpsacq.RATE_OBS_DTYPE)
    for c in range(n_chans):
        n = int(n_epochs[c])
        if n == 0:
            continue
        smp, rate = records["sample"][c, :n], records["lo_rate"][c, :n]
        nxt = int(chans["next_sample"][c])
        acc = carrier_acc(smp, rate, nxt, int(nom_words[c]))
        for i in range(n_fix):
            hit = rate_observation(smp, rate, nxt, acc, int(nom_words[c]), first_rx_sample + i * rx_step, int(avg_samples), fs)
            if hit is None:
                continue
            o = out[i, c]
            o["valid"], o["adr"], o["doppler_hz"], o["weight"] = 1, hit[0], hit[1], 1.0
    return out


def nco_phase_walk(samples, lo_rates, next_sample, lo_phase0=0):
    """THE CHANNEL MODEL's carrier bookkeeping run forward: lo_phase at the start of every epoch and at next_sample (mod 2^32)"""
    ph = [lo_phase0 & 0xFFFFFFFF]
    for t in range(len(samples)):
        end = int(samples[t + 1]) if t + 1 < len(samples) else int(next_sample)
        ph.append((ph[-1] + (end - int(samples[t])) * int(lo_rates[t])) & 0xFFFFFFFF)
    return ph


def walk_lo_rate(rec, seed, nom_word, span, sign=0):
    """records with lo_rate replaced by a random walk around nom_word (mod 2^32): steps of up to span / 16, kept within +-span;
    sign -1 / +1 keeps every d_t strictly negative / positive"""
    rng = np.random.default_rng(seed)
    rec = rec.copy()
    d = -span // 2 if sign < 0 else span // 2 if sign > 0 else 0
    lo, hi = (-span, -1) if sign < 0 else (1, span) if sign > 0 else (-span, span)
    for t in range(len(rec)):
        d = min(max(d + int(rng.integers(-(span // 16) - 1, span // 16 + 2)), lo), hi)
        rec["lo_rate"][t] = (nom_word + d) & 0xFFFFFFFF
    return rec


# ---- satellite velocity and clock drift ---------------------------------------------------------------------------------------
def velocity_at(eph, tk):
    """d / dt of IS-GPS-200 Table 20-IV at tk seconds of GPS time from t_oe: ECEF (n, 3), m/s"""
    tk = np.atleast_1d(np.asarray(tk, np.float64))
    A = eph["sqrt_a"] ** 2
    e = eph["e"]
    n = math.sqrt(nav_ref.MU / A ** 3) + eph["dn"]
    E = nav_ref._kepler(eph, tk)
    sE, cE = np.sin(E), np.cos(E)
    nu = np.arctan2(math.sqrt(1 - e * e) * sE, cE - e)
    phi = nu + eph["omega"]
    s2, c2 = np.sin(2 * phi), np.cos(2 * phi)
    u = phi + eph["c_us"] * s2 + eph["c_uc"] * c2
    r = A * (1 - e * cE) + eph["c_rs"] * s2 + eph["c_rc"] * c2
    inc = eph["i_0"] + eph["c_is"] * s2 + eph["c_ic"] * c2 + eph["idot"] * tk
    om = eph["omega_0"] + (eph["omega_dot"] - nav_ref.OMEGA_E) * tk - nav_ref.OMEGA_E * float(eph["t_oe"])
    Ed = n / (1 - e * cE)
    nud = Ed * math.sqrt(1 - e * e) / (1 - e * cE)
    ud = nud * (1 + 2 * (eph["c_us"] * c2 - eph["c_uc"] * s2))
    rd = A * e * sE * Ed + 2 * nud * (eph["c_rs"] * c2 - eph["c_rc"] * s2)
    idd = eph["idot"] + 2 * nud * (eph["c_is"] * c2 - eph["c_ic"] * s2)
    omd = eph["omega_dot"] - nav_ref.OMEGA_E
    xp, yp = r * np.cos(u), r * np.sin(u)
    xpd, ypd = rd * np.cos(u) - yp * ud, rd * np.sin(u) + xp * ud
    so, co, si, ci = np.sin(om), np.cos(om), np.sin(inc), np.cos(inc)
    x = xp * co - yp * ci * so
    y = xp * so + yp * ci * co
    return np.stack([xpd * co - ypd * ci * so + yp * si * so * idd - omd * y,
                     xpd * so + ypd * ci * co - yp * si * co * idd + omd * x,
                     ypd * si + yp * ci * idd], axis=-1)


def clock_drift(eph, tk, tc):
    """a_f1 + 2 a_f2 t + F e sqrt_a cos E E' at (uncorrected) satellite time tk from t_oe, tc from t_oc"""
    tc = np.asarray(tc, np.float64)
    A = eph["sqrt_a"] ** 2
    n = math.sqrt(nav_ref.MU / A ** 3) + eph["dn"]
    cE = np.cos(nav_ref._kepler(eph, np.atleast_1d(np.asarray(tk, np.float64))))
    return eph["a_f1"] + 2 * eph["a_f2"] * tc + nav_ref.F_REL * eph["e"] * eph["sqrt_a"] * cE * (n / (1 - eph["e"] * cE))


def sat_rate(eph, tx_ms, tx_frac):
    """(velocities (n, 3), clock drifts (n,)) at the uncorrected satellite times (tx_ms, tx_frac)"""
    tx_ms = np.atleast_1d(np.asarray(tx_ms, np.int64))
    tx_frac = np.atleast_1d(np.asarray(tx_frac, np.float64))
    tk0 = nav_ref.fold_ms(tx_ms - 1000 * int(eph["t_oe"])) * 1e-3 + tx_frac
    tc = nav_ref.fold_ms(tx_ms - 1000 * int(eph["t_oc"])) * 1e-3 + tx_frac
    dt = nav_ref.clock_correction(eph, tk0, tc)
    return velocity_at(eph, tk0 - dt), clock_drift(eph, tk0, tc)


# ---- the velocity solve --------------------------------------------------------------------------------------------------------
def vel_rows(ephs, eph_index, tx_ms, tx_frac, doppler_hz, rx_xyz, rx_ms, rx_frac):
    """(H (n, 4), y (n,)) of the model: rows (-e_i, 1), right-hand sides rho'_i - e_i . (v_i - Omega_e x r_r) + c clock_drift_i"""
    H, y = [], []
    om = nav_ref.OMEGA_E
    rr = np.asarray(rx_xyz, np.float64)
    for j, k in enumerate(eph_index):
        eph = ephs[k]
        p, dtc = nav_ref.sat_state(eph, tx_ms[j], tx_frac[j])
        v, cd = sat_rate(eph, tx_ms[j], tx_frac[j])
        rs, vs = p[0], v[0]
        dt = float(nav_ref.fold_ms(int(tx_ms[j]) - int(rx_ms))) * 1e-3 + ((float(tx_frac[j]) - float(dtc[0])) - float(rx_frac))
        th = om * dt
        c, s = math.cos(th), math.sin(th)
        ri = np.array([rs[0] * c - rs[1] * s, rs[0] * s + rs[1] * c, rs[2]])
        w = vs + np.array([-om * rs[1], om * rs[0], 0.0])
        vi = np.array([w[0] * c - w[1] * s, w[0] * s + w[1] * c, w[2]])
        e = (ri - rr) / np.linalg.norm(ri - rr)
        rho_dot = -(nav_ref.C / L1) * float(doppler_hz[j])
        H.append([-e[0], -e[1], -e[2], 1.0])
        y.append(rho_dot - e @ (vi - np.array([-om * rr[1], om * rr[0], 0.0])) + nav_ref.C * float(cd[0]))
    return np.array(H), np.array(y)


def gain(H, w):
    """(H^T W H)^-1 H^T W: what one unit of error in a right-hand side does to the solution"""
    w = np.asarray(w, np.float64)
    return np.linalg.solve(H.T @ (w[:, None] * H), H.T * w)


def enu_of(lat, lon, v):
    sl, cl, sp, cp = math.sin(lon), math.cos(lon), math.sin(lat), math.cos(lat)
    return np.array([-sl * v[0] + cl * v[1], -sp * cl * v[0] - sp * sl * v[1] + cp * v[2], cp * cl * v[0] + cp * sl * v[1] + sp * v[2]])


def velocity(ephs, obs_row, rate_row, fix):
    """One velocity from a fix's rows (OBS_DTYPE, RATE_OBS_DTYPE records) and its FIX_DTYPE record, by the model: dict(status,
    n_used, v (ECEF), enu, drift, rms)."""
    if int(fix["status"]) != 0:
        return dict(status=VEL_NO_FIX, n_used=0)
    use = [j for j in range(len(obs_row))
           if obs_row["valid"][j] and 0 <= obs_row["eph"][j] < len(ephs) and rate_row["valid"][j]
           and np.isfinite(rate_row["weight"][j]) and rate_row["weight"][j] >= 0 and np.isfinite(rate_row["doppler_hz"][j])
           and np.isfinite(obs_row["weight"][j]) and obs_row["weight"][j] >= 0]
    if len(use) < 4:
        return dict(status=VEL_TOO_FEW, n_used=len(use))
    H, y = vel_rows(ephs, obs_row["eph"][use], obs_row["tx_ms"][use], obs_row["tx_frac"][use], rate_row["doppler_hz"][use],
                    (fix["x"], fix["y"], fix["z"]), int(fix["rx_ms"]), float(fix["rx_frac"]))
    w = np.asarray(rate_row["weight"][use], np.float64)
    N = H.T @ (w[:, None] * H)
    if np.linalg.cond(N) > 1e12:
        return dict(status=VEL_SINGULAR, n_used=len(use))
    x = np.linalg.solve(N, H.T @ (w * y))
    res = y - H @ x
    return dict(status=VEL_OK, n_used=len(use), v=x[:3], enu=enu_of(float(fix["lat"]), float(fix["lon"]), x[:3]), drift=x[3] / nav_ref.C,
                rms=math.sqrt((w * res * res).sum() / w.sum()))
