"""Reference of the signal-quality tests: the model of include/gpsacq.h ("Signal quality per observation") in Python integers
masked to 64 bits, numpy.float64 for the named double operations and math.log10, written from that text and not from the kernels.

  * the three prefix sums over the epochs and the window sums as their differences -- and, apart from them, as a loop over the window;
  * the values, the lock test, the flags and the weight of one window;
  * the info record of every (instant, channel) and the weights written into a row of observations;
  * the capture, channels and constants of the physical check, shared by the CPU test (the C model's records) and the GPU test.

Nothing here loads the library except for the record dtypes."""
import math

import numpy as np

M64 = (1 << 64) - 1
NO_POWER, SATURATED, UNLOCKED, FULL, SHORT = 1, 2, 4, 8, 16
DEFAULTS = dict(epochs=200, min_epochs=20, lock_num=1, lock_den=2, require_lock=1, reserved=0,
                cn0_min_lin=10.0 ** (30 / 10), cn0_ref_lin=10.0 ** (45 / 10), cn0_cap_dbhz=99.0)
INT_KEYS = ("epochs", "min_epochs", "lock_num", "lock_den", "require_lock", "reserved")
FLOOR_SNR = (2 / math.pi) / (2 - 2 / math.pi)   # noise alone: E|x|^2 / (E x^2 + E y^2 - E|x|^2) for unit Gaussians
FLOOR_DBHZ = 10 * math.log10(1000 * FLOOR_SNR)  # 26.69


def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def par(params=None, **over):
    """a dict from None (the defaults), a dict or a QUALITY_PARAMS_DTYPE record: Python integers and numpy.float64"""
    out = dict(DEFAULTS)
    if params is not None:
        if isinstance(params, dict):
            out.update(params)
        else:
            rec = np.asarray(params).ravel()[0]
            out.update({k: rec[k] for k in rec.dtype.names})
    out.update(over)
    return {k: int(v) if k in INT_KEYS else np.float64(v) for k, v in out.items()}


def params_valid(p):
    return (1 <= p["min_epochs"] <= p["epochs"] <= 1024 and 1 <= p["lock_num"] <= p["lock_den"] <= 1024
            and math.isfinite(p["cn0_min_lin"]) and p["cn0_min_lin"] >= 0 and math.isfinite(p["cn0_ref_lin"]) and p["cn0_ref_lin"] > 0
            and math.isfinite(p["cn0_cap_dbhz"]))


def prefix_sums(ip, qp):
    """([PA_0 .. PA_n], [PD_0 .. PD_n], [PN_0 .. PN_n]): the sums over u < t of |ip|, ip^2 + qp^2, ip^2 - qp^2, mod 2^64"""
    pa, pd, pn = [0], [0], [0]
    for a, b in zip(ip, qp):
        a, b = int(a), int(b)
        pa.append((pa[-1] + abs(a)) & M64)
        pd.append((pd[-1] + a * a + b * b) & M64)
        pn.append((pn[-1] + a * a - b * b) & M64)
    return pa, pd, pn


def window_sums_prefix(sums, t, m):
    """(A, D, N) of the window u = t-m+1 .. t as differences of the prefix sums"""
    return tuple((s[t + 1] - s[t + 1 - m]) & M64 for s in sums)


def window_sums_direct(ip, qp, t, m):
    """(A, D, N) of the same window by a loop over its epochs"""
    A = D = N = 0
    for u in range(t - m + 1, t + 1):
        a, b = int(ip[u]), int(qp[u])
        A = (A + abs(a)) & M64
        D = (D + a * a + b * b) & M64
        N = (N + a * a - b * b) & M64
    return A, D, N


def evaluate(A, D, N, m, p):
    """the info record of one window as a dict"""
    sig = (A * A) & M64
    tot = (m * D) & M64
    noise = (tot - sig) & M64
    flags = (FULL if m == p["epochs"] else 0) | (SHORT if m < p["min_epochs"] else 0)
    locked = D != 0 and s64(N * p["lock_den"]) >= s64(D * p["lock_num"])
    if not locked:
        flags |= UNLOCKED
    lin, db = np.float64(0.0), np.float64(0.0)
    if D == 0 or sig == 0:
        flags |= NO_POWER
    elif noise == 0:
        flags |= SATURATED
        lin, db = np.float64(np.inf), p["cn0_cap_dbhz"]
    else:
        snr = np.float64(float(sig)) / np.float64(float(noise))   # int -> float rounds to nearest even
        lin = snr * np.float64(1000.0)
        db = np.float64(10.0) * np.float64(math.log10(lin))
    weight = np.float64(0.0)
    gated = (flags & (NO_POWER | SHORT)) != 0 or ((flags & UNLOCKED) != 0 and p["require_lock"] != 0) or lin < p["cn0_min_lin"]
    if not gated:
        w = lin / p["cn0_ref_lin"]
        weight = w if w < 1.0 else np.float64(1.0)
    return dict(epochs=m, flags=flags, sig=sig, noise=noise, lin=lin, cn0_dbhz=db, weight=weight)


def window_of(t, p):
    return min(t + 1, p["epochs"])


def channel_series(ip, qp, p, direct=False):
    """the info dict of every epoch t of one channel taken as the window's last"""
    sums = None if direct else prefix_sums(ip, qp)
    out = []
    for t in range(len(ip)):
        m = window_of(t, p)
        out.append(evaluate(*(window_sums_direct(ip, qp, t, m) if direct else window_sums_prefix(sums, t, m)), m, p))
    return out


def quality(records, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, params=None, direct=False):
    """QUALITY_INFO_DTYPE [n_fix][n_chans] of the model"""
    import gpsacq
    p = par(params)
    assert params_valid(p)
    n_chans = len(n_epochs)
    info = np.zeros((n_fix, n_chans), gpsacq.QUALITY_INFO_DTYPE)
    for c in range(n_chans):
        n = int(n_epochs[c])
        if n == 0 or not int(tags[c]["valid"]):
            continue
        rec = records[c]
        smp, nxt = np.asarray(rec["sample"][:n], np.uint64), int(chans[c]["next_sample"])
        ip, qp = rec["ip"][:n], rec["qp"][:n]
        sums = None if direct else prefix_sums(ip, qp)
        done = {}
        for i in range(n_fix):
            R = first_rx_sample + i * rx_step
            if R < int(smp[0]) or R >= nxt:
                continue
            t = int(np.searchsorted(smp, np.uint64(R), side="right")) - 1
            if t not in done:
                m = window_of(t, p)
                done[t] = evaluate(*(window_sums_direct(ip, qp, t, m) if direct else window_sums_prefix(sums, t, m)), m, p)
            for k, v in done[t].items():
                info[k][i, c] = v
    return info


def apply_weights(obs, info):
    """a copy of obs with the weight of every observation whose valid != 0 replaced by info's"""
    out = np.array(obs)
    sel = out["valid"] != 0
    out["weight"][sel] = info["weight"][sel]
    return out


# ---- the physical check: two satellites 10 dB apart and a channel on noise ----------------------------------------------------------
PHYS_FS, PHYS_SCALE, PHYS_SEED, PHYS_WINDOW = 2.046e6, 30.0, 1, 100
PHYS_CN0 = (50.0, 40.0)
# Measured by tests/test_quality.py::test_physical_capture_on_the_cpu_model with this file on the records of the CPU model of the
# channels (tests/c/track_model_iq.c) over this capture, eight disjoint windows of 100 epochs from 0.7 s on (the GPU's records are
# byte for byte the model's, so these are properties of the model and not of the kernels under test): the estimates read 48.299 and
# 38.820 dB-Hz in the mean, 1.701 and 1.180 dB below the truth -- the loss of the two-level carrier replica, of the rounding to
# 8 bits and of the estimator's bias, 1.44 dB in the mean; standard deviation over the windows 0.879 and 0.387 dB, of their
# difference 1.090 dB.  The margins of the assertions are three times those.
PHYS_LOSS_DB = 1.44
PHYS_SPREAD_DB = (0.879, 0.387)
PHYS_DIFF_SPREAD_DB = 1.090
_phys = []


def physical_case():
    """(capture, loop settings, the three channels at sample 0): 1.5 s of 8-bit complex samples at 2.046 MHz made with numpy by the
    generator's law (track_iq_helpers.host_capture: noise of sigma 1 per arm, times 30, rounded), the carrier at 0.26 fs, PRN 6 at
    50 dB-Hz and PRN 29 at 40 by C/N0 = a^2 / (2 sigma^2) fs; channels started from the known code phase and Doppler, the third
    on PRN 17, which is not in the capture.  Made once; the channels are handed out as a copy."""
    import track_iq_helpers as iqh
    if not _phys:
        fs, if_hz = PHYS_FS, 0.26 * PHYS_FS
        amps = [float(np.sqrt(2 * 10 ** (c / 10) / fs)) for c in PHYS_CN0]
        assert abs(amps[0] / amps[1] - math.sqrt(10.0)) < 1e-12
        rng = np.random.default_rng(3)
        sats = [(6, amps[0], 1830.0, 411.3, 0.21, 1 - 2 * rng.integers(0, 2, 9)), (29, amps[1], -2610.0, 1502.7, 0.64, 1 - 2 * rng.integers(0, 2, 9))]
        buf = iqh.host_capture(int(1.5 * fs), fs, [s[:5] for s in sats], if_hz, PHYS_SCALE, True, PHYS_SEED, nav=[s[5] for s in sats])
        buf.setflags(write=False)
        p = iqh.default_params_iq8(fs, iqh.capture_rms(buf, True, (0, 0)))
        chans = np.concatenate([iqh.start_chan_iq(fs, if_hz, s[0], s[2], s[3], s[4], 0, p) for s in sats] +
                               [iqh.start_chan_iq(fs, if_hz, 17, 900.0, 700.0, 0.0, 0, p)])
        _phys.append((buf, p, chans))
    buf, p, chans = _phys[0]
    return buf, p, chans.copy()


def physical_instants(chans):
    """(first_rx_sample, rx_step, n_fix): 102 ms apart from 0.7 s -- disjoint windows of PHYS_WINDOW epochs, after the pull-in -- to
    the end of the two satellites' records"""
    step, first = int(PHYS_FS * (PHYS_WINDOW + 2) / 1000), int(0.7 * PHYS_FS)
    return first, step, (int(chans["next_sample"][:2].min()) - 1 - first) // step + 1


def physical_check(info, every, status, n_noise, lost_code, say=print):
    """the assertions of the physical check on info (QUALITY_INFO_DTYPE [n_fix][3] at physical_instants) and `every` (the info of the
    noise-only channel with every one of its epochs as a window's last)"""
    cn0 = info["cn0_dbhz"]
    mean, spread = cn0.mean(axis=0), cn0.std(axis=0, ddof=1)
    diff = cn0[:, 0] - cn0[:, 1]
    say("C/N0 over %d windows of %d epochs: mean %s, std %s dB-Hz, loss %s dB; difference %.3f dB, std %.3f dB" %
        (len(cn0), PHYS_WINDOW, np.round(mean, 3), np.round(spread, 3), np.round(np.array(PHYS_CN0) - mean[:2], 3), diff.mean(), diff.std(ddof=1)))
    assert len(cn0) == 8
    # (a) locked, full windows, a weight everywhere
    assert (info["flags"][:, :2] == FULL).all() and (info["weight"][:, :2] > 0).all()
    # (b) 10 dB apart
    assert abs((mean[0] - mean[1]) - 10.0) < 3 * PHYS_DIFF_SPREAD_DB
    # (c) each at its true C/N0 less the implementation loss
    for c in range(2):
        assert abs(mean[c] - (PHYS_CN0[c] - PHYS_LOSS_DB)) < 3 * PHYS_SPREAD_DB[c], (c, mean[c])
    # the absent PRN: LOST, or below the gate with weight 0 in at least 95 % of its full windows
    full = every[(every["flags"] & FULL) != 0]
    share = float(((full["weight"] == 0) & (full["lin"] < DEFAULTS["cn0_min_lin"])).mean()) if full.size else 1.0
    say("absent PRN: status %d, %d epochs, %d full windows, %.1f %% of them below the gate, mean %.2f, largest reading %.2f dB-Hz" %
        (status, n_noise, full.size, 100 * share, full["cn0_dbhz"].mean() if full.size else 0.0, full["cn0_dbhz"].max() if full.size else 0.0))
    assert status == lost_code or (full.size > 1000 and share >= 0.95)
