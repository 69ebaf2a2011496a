"""Reference of the atmosphere tests: the section "Atmosphere, elevation mask and DOP" of include/gpsacq.h restated in numpy,
written from that text and not from the kernels.

  * geodetic (the header's LatLonAlt iteration), the view (azimuth, elevation), Klobuchar, Saastamoinen;
  * fix_atm: stage 0, mask, three rounds, on nav_ref.sat_state and a delay-aware copy of nav_ref.solve that starts where it is told;
  * DOP through numpy.linalg.inv;
  * truth_tx_atm: nav_ref.truth_tx with the light-time equation |s - r| + D(view at the TRUE position) = c (t_rx - t_tx);
  * a page-18 encoder: subframe-4 words with the eight fields set and every free bit random.

Parameters are a dict(alpha=[4], beta=[4], elev_mask=radians, flags=bits).
"""
import math

import numpy as np

import nav_ref
from nav_ref import C, OMEGA_E, WEEK_MS, WGS84_A, WGS84_E2
from track_helpers import PREAMBLE, encode_subframe

PI = math.pi
ATM_IONO, ATM_TROPO, ROUNDS = 1, 2, 3
FIX_OK, FIX_TOO_FEW, FIX_NO_CONVERGE = 0, 1, 2
ALPHA_EXP = (-30, -27, -24, -24)
BETA_EXP = (11, 14, 16, 16)
# coefficients that make the ionosphere matter, in field units (codes)
ALPHA_CODES = (20, 2, -1, -2)
BETA_CODES = (55, 4, -2, -6)


def coefficients(alpha_codes=ALPHA_CODES, beta_codes=BETA_CODES):
    return ([math.ldexp(float(c), e) for c, e in zip(alpha_codes, ALPHA_EXP)], [math.ldexp(float(c), e) for c, e in zip(beta_codes, BETA_EXP)])


def params(alpha=None, beta=None, elev_mask=math.radians(5.0), flags=ATM_IONO | ATM_TROPO):
    a, b = coefficients()
    return dict(alpha=list(a if alpha is None else alpha), beta=list(b if beta is None else beta), elev_mask=float(elev_mask), flags=int(flags))


# ---- page 18 ------------------------------------------------------------------------------------------------------------
# first ICD bit (1..300, parity bits counted) of the eight 8-bit fields: word 3 starts at bit 61, word 4 at 91, word 5 at 121
PAGE18_BITS = {"alpha": (69, 77, 91, 99), "beta": (107, 121, 129, 137)}


def page18_words(alpha_codes, beta_codes, tow, rng=None, page_byte=0x78, sf_id=4):
    """ten 24-bit data words of subframe 4 page 18 (data ID 01, SV/page ID 56 = the byte 0x78) with the eight signed codes;
    bits no field owns are random (rng) or zero"""
    src = np.zeros(300, np.uint8) if rng is None else rng.integers(0, 2, 300).astype(np.uint8)

    def put(first, n, v):
        for k in range(n):
            src[first - 1 + k] = (v >> (n - 1 - k)) & 1

    put(1, 8, PREAMBLE)
    put(31, 17, tow & 0x1FFFF)
    put(50, 3, sf_id)
    put(61, 8, page_byte)
    for first, code in zip(PAGE18_BITS["alpha"] + PAGE18_BITS["beta"], tuple(alpha_codes) + tuple(beta_codes)):
        put(first, 8, int(code) & 0xFF)
    return [nav_ref._slice(src, 30 * w + 1, 24) for w in range(10)]


def frame_bits(eph, tow0, sf4_words, seed=None):
    """one frame, subframes 1 2 3 4 5, as a 0/1 stream; subframe 4 carries sf4_words (its TOW must be tow0 + 3)"""
    rng = None if seed is None else np.random.default_rng(seed)
    out, d29, d30 = [], 0, 0
    for k, sf_id in enumerate((1, 2, 3, 4, 5)):
        words = sf4_words if sf_id == 4 else nav_ref.subframe_words(eph, sf_id, tow0 + k, rng)
        b, d29, d30 = encode_subframe(words, d29, d30)
        out += b
    return np.array(out, np.uint8)


# ---- geodesy and view -----------------------------------------------------------------------------------------------------
def geodetic(xyz):
    x, y, z = (float(v) for v in xyz)
    p = math.sqrt(x * x + y * y)
    if not p > 1e-6:
        return (-PI / 2 if z < 0 else PI / 2), 0.0, abs(z) - WGS84_A * math.sqrt(1 - WGS84_E2)
    # tan(lon / 2) = y / (x + p) = (p - x) / y, each where its sum does not cancel; y == 0 with x < 0 is the antimeridian, pi
    lon = 2 * math.atan2(y, x + p) if x >= 0 else math.copysign(2 * math.atan2(p - x, abs(y)), 1.0 if y >= 0 else -1.0)
    lat = math.atan(z / (p * (1 - WGS84_E2)))
    alt = 0.0
    for _ in range(10):
        prev = alt
        N = WGS84_A / math.sqrt(1 - WGS84_E2 * math.sin(lat) ** 2)
        alt = p / math.cos(lat) - N
        lat = math.atan(z / (p * (1 - WGS84_E2 * N / (N + alt))))
        if abs(alt - prev) < 1e-9:
            break
    return lat, lon, alt


def view(lat, lon, d):
    """(az, el) of d = satellite - receiver (ECEF, (..., 3)) in the local frame at (lat, lon)"""
    d = np.asarray(d, np.float64)
    sp, cp, sl, cl = math.sin(lat), math.cos(lat), math.sin(lon), math.cos(lon)
    e = -sl * d[..., 0] + cl * d[..., 1]
    n = -sp * cl * d[..., 0] - sp * sl * d[..., 1] + cp * d[..., 2]
    u = cp * cl * d[..., 0] + cp * sl * d[..., 1] + sp * d[..., 2]
    return np.arctan2(e, n), np.arctan2(u, np.hypot(e, n))


def klobuchar_x(az, el, lat, lon, tow, p):
    """(x, F, AMP): the phase of the cosine, the obliquity factor and the amplitude, IS-GPS-200 Figure 20-4"""
    az, el, tow = np.asarray(az, np.float64), np.asarray(el, np.float64), np.asarray(tow, np.float64)
    E = el / PI
    psi = 0.0137 / (E + 0.11) - 0.022
    phi_i = np.clip(lat / PI + psi * np.cos(az), -0.416, 0.416)
    lam_i = lon / PI + psi * np.sin(az) / np.cos(phi_i * PI)
    phi_m = phi_i + 0.064 * np.cos((lam_i - 1.617) * PI)
    t = 4.32e4 * lam_i + tow
    t = t - 86400.0 * np.floor(t / 86400.0)
    F = 1 + 16 * (0.53 - E) ** 3
    a, b = p["alpha"], p["beta"]
    amp = np.maximum(((a[3] * phi_m + a[2]) * phi_m + a[1]) * phi_m + a[0], 0.0)
    per = np.maximum(((b[3] * phi_m + b[2]) * phi_m + b[1]) * phi_m + b[0], 72000.0)
    return 2 * PI * (t - 50400.0) / per, F, amp


def klobuchar(az, el, lat, lon, tow, p):
    el = np.asarray(el, np.float64)
    if not p["flags"] & ATM_IONO:
        return np.zeros(el.shape)
    with np.errstate(all="ignore"):  # satellites below the horizon are computed and thrown away
        x, F, amp = klobuchar_x(az, el, lat, lon, tow, p)
        day = C * F * (5e-9 + amp * (1 - x * x / 2 + x ** 4 / 24))
        out = np.where(np.abs(x) < 1.57, day, C * F * 5e-9)
    return np.where(el > 0, out, 0.0)


def saastamoinen(el, lat, alt, p):
    el = np.asarray(el, np.float64)
    if not p["flags"] & ATM_TROPO or alt < -100 or alt > 1e4:
        return np.zeros(el.shape)
    h = max(alt, 0.0)
    P = 1013.25 * (1 - 2.2557e-5 * h) ** 5.2568
    T = 288.16 - 6.5e-3 * h
    e = 6.108 * 0.7 * math.exp((17.15 * T - 4684) / (T - 38.45))
    zen = 0.0022768 * P / (1 - 0.00266 * math.cos(2 * lat) - 0.00028 * h / 1000) + 0.002277 * (1255 / T + 0.05) * e
    with np.errstate(all="ignore"):
        return np.where(el > 0, zen / np.sin(el), 0.0)


def turned(sat_xyz, t_tx, t_rx):
    """satellite states (..., 3) turned by Omega_e (t_tx - t_rx) about z"""
    sat_xyz = np.asarray(sat_xyz, np.float64)
    th = OMEGA_E * (np.asarray(t_tx, np.float64) - t_rx)
    c, s = np.cos(th), np.sin(th)
    return np.stack([sat_xyz[..., 0] * c - sat_xyz[..., 1] * s, sat_xyz[..., 0] * s + sat_xyz[..., 1] * c, sat_xyz[..., 2]], -1)


def views(rx_xyz, sat_turned, tow, p):
    """dict(az, el, iono, tropo) of satellites already turned into the receive frame, seen from rx_xyz at time of week tow"""
    lat, lon, alt = geodetic(rx_xyz)
    az, el = view(lat, lon, np.asarray(sat_turned) - np.asarray(rx_xyz, np.float64))
    return dict(az=az, el=el, iono=klobuchar(az, el, lat, lon, tow, p), tropo=saastamoinen(el, lat, alt, p), lla=(lat, lon, alt))


# ---- truth maker ---------------------------------------------------------------------------------------------------------
def truth_tx_atm(eph, rx_xyz, ref_ms, t_rx, p):
    """nav_ref.truth_tx with the delays of the model on the path: |R(theta) sat(t_tx) - rx| + D = c (t_rx - t_tx), D seen from
    the true position at the true receive time.  Returns the uncorrected satellite times as offsets from ref_ms."""
    t_rx = np.atleast_1d(np.asarray(t_rx, np.float64))
    ref_ms = np.asarray(ref_ms, np.int64)
    bk = nav_ref.fold_ms(ref_ms - 1000 * int(eph["t_oe"])) * 1e-3
    bc = nav_ref.fold_ms(ref_ms - 1000 * int(eph["t_oc"])) * 1e-3
    tow = np.mod(ref_ms, WEEK_MS) * 1e-3 + t_rx
    t_tx = t_rx - 75e-3
    for _ in range(10):
        s = turned(nav_ref.position(eph, bk + t_tx), t_tx, t_rx)
        rng = np.sqrt(((s - rx_xyz) ** 2).sum(-1))
        v = views(rx_xyz, s, tow, p)
        new = t_rx - (rng + v["iono"] + v["tropo"]) / C
        done = np.max(np.abs(new - t_tx)) < 1e-16
        t_tx = new
        if done:
            break
    t_sv = t_tx.copy()
    for _ in range(8):
        new = t_tx + nav_ref.clock_correction(eph, bk + t_sv, bc + t_sv)
        done = np.max(np.abs(new - t_sv)) < 1e-16
        t_sv = new
        if done:
            break
    assert done
    return t_sv


# ---- solver --------------------------------------------------------------------------------------------------------------
def solve_from(sat_xyz, t_tx, weight, delay, t0, pos, bias):
    """nav_ref.solve's iteration from (pos, bias) with every residual reduced by its delay.  Returns dict(ok, pos, bias, rms,
    iterations)."""
    w = np.asarray(weight, np.float64)
    pos = np.array(pos, np.float64)
    for it in range(20):
        t_rx = t0 - bias / C
        d = pos - turned(sat_xyz, t_tx, t_rx)
        rng = np.sqrt((d * d).sum(1))
        res = C * (t_rx - t_tx) - delay - rng
        H = np.concatenate([d / rng[:, None], np.ones((len(rng), 1))], 1)
        with np.errstate(all="ignore"):
            rms = math.sqrt((w * res * res).sum() / w.sum())
        try:
            step = np.linalg.solve(H.T @ (w[:, None] * H), H.T @ (w * res))
        except np.linalg.LinAlgError:
            return dict(ok=False, iterations=it)
        if not np.all(np.isfinite(step)):
            return dict(ok=False, iterations=it)
        pos = pos + step[:3]
        bias += step[3]
        if math.sqrt((step[:3] ** 2).sum()) < 1e-4:
            return dict(ok=True, pos=pos, bias=bias, rms=rms, iterations=it + 1)
    return dict(ok=False, iterations=20)


def dops(rx_xyz, sat_turned):
    """(gdop, pdop, hdop, vdop, tdop) of the rows (unit vector satellite -> receiver, 1); zeros with fewer than four rows"""
    if len(sat_turned) < 4:
        return (0.0,) * 5
    d = np.asarray(rx_xyz) - np.asarray(sat_turned)
    H = np.concatenate([d / np.sqrt((d * d).sum(1))[:, None], np.ones((len(d), 1))], 1)
    Q = np.linalg.inv(H.T @ H)
    lat, lon, _ = geodetic(rx_xyz)
    sp, cp, sl, cl = math.sin(lat), math.cos(lat), math.sin(lon), math.cos(lon)
    R = np.array([[-sl, cl, 0.0], [-sp * cl, -sp * sl, cp], [cp * cl, cp * sl, sp]])
    Qp = R @ Q[:3, :3] @ R.T
    return (math.sqrt(Qp[0, 0] + Qp[1, 1] + Qp[2, 2] + Q[3, 3]), math.sqrt(Qp[0, 0] + Qp[1, 1] + Qp[2, 2]), math.sqrt(Qp[0, 0] + Qp[1, 1]),
            math.sqrt(Qp[2, 2]), math.sqrt(Q[3, 3]))


def fix_atm(ephs, eph_index, tx_ms, tx_frac, weight, p):
    """One corrected fix from the USABLE observations of a row.  Returns dict(status, n_used, kept (bool per observation given),
    n_masked, iterations (total), stages (steps per stage), and for status 0: xyz, rx_ms, rx_frac, rms, lla, dop (five), sat (the
    satellites turned into the final receive frame), delay)."""
    tx_ms = np.asarray(tx_ms, np.int64)
    w = np.asarray(weight, np.float64)
    n = len(tx_ms)
    out = dict(status=FIX_TOO_FEW, n_used=n, kept=np.ones(n, bool), n_masked=0, iterations=0, stages=[])
    if n < 4:
        return out
    first = int(tx_ms[0])
    d = nav_ref.fold_ms(tx_ms - first)
    ms0 = first + int(d.min())
    xyz, t = [], []
    for j, k in enumerate(eph_index):
        pos, dt = nav_ref.sat_state(ephs[k], tx_ms[j], tx_frac[j])
        xyz.append(pos[0])
        t.append(float(d[j] - d.min()) * 1e-3 + tx_frac[j] - dt[0])
    xyz, t = np.array(xyz), np.array(t)
    t0 = t.mean() + 75e-3
    pos, bias = np.zeros(3), 0.0
    kept = np.ones(n, bool)
    delay = np.zeros(n)
    for stage in range(ROUNDS + 1):
        st = solve_from(xyz[kept], t[kept], w[kept], delay[kept], t0, pos, bias)
        out["iterations"] += st["iterations"]
        out["stages"].append(st["iterations"])
        if not st["ok"]:
            out["status"] = FIX_NO_CONVERGE
            return out
        pos, bias = st["pos"], st["bias"]
        t_rx = t0 - bias / C
        if stage == ROUNDS:
            break
        v = views(pos, turned(xyz, t, t_rx), (ms0 % WEEK_MS) * 1e-3 + t_rx, p)
        if stage == 0:
            kept = ~(v["el"] < p["elev_mask"])
            out["kept"], out["n_masked"], out["n_used"] = kept, int(n - kept.sum()), int(kept.sum())
            if kept.sum() < 4:
                return out
            if kept.all() and p["flags"] == 0:
                break
        delay = v["iono"] + v["tropo"]
    ms, frac = nav_ref.split_time(ms0, t_rx)
    sat = turned(xyz, t, t_rx)
    out.update(status=FIX_OK, xyz=pos, rx_ms=int(ms), rx_frac=float(frac), t_rx=t_rx, rms=st["rms"], lla=geodetic(pos), sat=sat, delay=delay,
               dop=dops(pos, sat[kept & (w > 0)]))
    return out


def truth_times(ephs, rx_xyz, ref_ms, t_rx, p):
    """(tx_ms, tx_frac), each [n_fix][len(ephs)]: what a receiver at rx_xyz reads off its replicas at receive times ref_ms[k] +
    t_rx[k] through the model's atmosphere"""
    ms = np.zeros((len(t_rx), len(ephs)), np.int32)
    frac = np.zeros((len(t_rx), len(ephs)))
    for j, eph in enumerate(ephs):
        ms[:, j], frac[:, j] = nav_ref.split_time(ref_ms, truth_tx_atm(eph, rx_xyz, ref_ms, t_rx, p))
    return ms, frac
