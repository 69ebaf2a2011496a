"""Reference of the navigation-solver tests: an independent float64 numpy restatement of IS-GPS-200 (Tables 20-I, 20-III, 20-IV,
20.3.3.3.3.1) and of the fix model in include/gpsacq.h, written from those texts and not from the library.

  * ephemeris encoder / decoder on bit strings: fields <-> integer codes <-> the 300 bits of a subframe, by the ICD's own bit
    numbers 1..300 (the decoder never goes through 24-bit words);
  * satellite state and clock correction;
  * a truth maker: receiver position + receive time -> the uncorrected satellite times a receiver would read off its replicas;
  * a solver of the same model (numpy.linalg.solve on the weighted normal equations), working in time offsets;
  * the synthetic 12-satellite constellation of the tests, and PDOP.

Times of week are (ms, frac) pairs as in the library; inside, a time is a float offset in seconds from a reference millisecond.
"""
import itertools
import math

import numpy as np

from track_helpers import PREAMBLE, encode_subframe

GPS_PI = 3.1415926535898
MU = 3.986005e14
OMEGA_E = 7.2921151467e-5
C = 2.99792458e8
F_REL = -4.442807633e-10
WEEK_MS = 604800000
WGS84_A = 6378137.0
WGS84_E2 = 0.00669437999014132

# name: (subframe, [(first ICD bit 1..300, bits), ...] most significant piece first, signed, power of two, semicircles)
FIELDS = {
    "week": (1, [(61, 10)], False, 0, False),
    "iodc": (1, [(83, 2), (211, 8)], False, 0, False),
    "t_gd": (1, [(197, 8)], True, -31, False),
    "t_oc": (1, [(219, 16)], False, 4, False),
    "a_f2": (1, [(241, 8)], True, -55, False),
    "a_f1": (1, [(249, 16)], True, -43, False),
    "a_f0": (1, [(271, 22)], True, -31, False),
    "iode2": (2, [(61, 8)], False, 0, False),
    "c_rs": (2, [(69, 16)], True, -5, False),
    "dn": (2, [(91, 16)], True, -43, True),
    "m_0": (2, [(107, 8), (121, 24)], True, -31, True),
    "c_uc": (2, [(151, 16)], True, -29, False),
    "e": (2, [(167, 8), (181, 24)], False, -33, False),
    "c_us": (2, [(211, 16)], True, -29, False),
    "sqrt_a": (2, [(227, 8), (241, 24)], False, -19, False),
    "t_oe": (2, [(271, 16)], False, 4, False),
    "c_ic": (3, [(61, 16)], True, -29, False),
    "omega_0": (3, [(77, 8), (91, 24)], True, -31, True),
    "c_is": (3, [(121, 16)], True, -29, False),
    "i_0": (3, [(137, 8), (151, 24)], True, -31, True),
    "c_rc": (3, [(181, 16)], True, -5, False),
    "omega": (3, [(197, 8), (211, 24)], True, -31, True),
    "omega_dot": (3, [(241, 24)], True, -43, True),
    "iode3": (3, [(271, 8)], False, 0, False),
    "idot": (3, [(279, 14)], True, -43, True),
}
INT_FIELDS = ("week", "iodc", "iode2", "iode3", "t_oc", "t_oe")
SIGNED_FIELDS = tuple(k for k, v in FIELDS.items() if v[2])


def _width(name):
    return sum(n for _, n in FIELDS[name][1])


def value_of(name, code):
    """the field's value from its integer code: code * 2^k, exact, then once times the GPS pi for semicircle fields"""
    _, _, _, exp2, semi = FIELDS[name]
    if name in INT_FIELDS:
        return int(code) << exp2
    v = math.ldexp(float(code), exp2)
    return v * GPS_PI if semi else v


def code_of(name, value):
    """nearest integer code of a value, clipped to the field's range"""
    _, _, signed, exp2, semi = FIELDS[name]
    w = _width(name)
    code = int(round(math.ldexp(float(value) / (GPS_PI if semi else 1.0), -exp2)))
    lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
    return min(max(code, lo), hi)


def quantise(eph):
    """every field through the encoder and back: what a decode of the encoded subframes returns, exactly"""
    out = dict(eph)
    for name in FIELDS:
        out[name] = value_of(name, code_of(name, eph[name]))
    return out


# ---- subframes as bit strings ---------------------------------------------------------------------------------------------
def source_bits(bits300, d30_prev=0):
    """the 300 transmitted bits of a subframe with D30* taken off the 24 data bits of every word (parity bits left as sent)"""
    b = np.array(bits300, np.uint8).copy()
    assert b.size == 300
    for w in range(10):
        star = d30_prev if w == 0 else int(bits300[30 * w - 1])
        b[30 * w:30 * w + 24] ^= star
    return b


def _slice(src, first, n):
    v = 0
    for k in range(first - 1, first - 1 + n):
        v = (v << 1) | int(src[k])
    return v


def decode_subframes(subframes300):
    """ephemeris dict from transmitted 300-bit subframes (upright, each starting at its preamble), folded in order;
    returns (eph, have mask).  Slices the ICD's bit numbers directly."""
    eph = {name: 0 for name in FIELDS}
    eph["tow"] = 0
    have = 0
    for bits in subframes300:
        src = source_bits(bits)
        sf_id = _slice(src, 50, 3)
        if sf_id not in (1, 2, 3):
            continue
        have |= 1 << (sf_id - 1)
        eph["tow"] = _slice(src, 31, 17)
        for name, (sf, pieces, signed, _, _) in FIELDS.items():
            if sf != sf_id:
                continue
            code = 0
            for first, n in pieces:
                code = (code << n) | _slice(src, first, n)
            w = _width(name)
            if signed and code >> (w - 1):
                code -= 1 << w
            eph[name] = value_of(name, code)
    return eph, have


def ephemeris_valid(eph, have):
    return have == 7 and eph["iode2"] != 0 and (eph["iodc"] & 0xFF) == eph["iode2"] == eph["iode3"]


def subframe_words(eph, sf_id, tow, rng=None):
    """ten 24-bit data words of subframe sf_id (1..5) carrying eph's fields; bits no field owns are random (rng) or zero"""
    src = np.zeros(300, np.uint8) if rng is None else rng.integers(0, 2, 300).astype(np.uint8)

    def put(first, n, v):
        for k in range(n):
            src[first - 1 + k] = (v >> (n - 1 - k)) & 1

    put(1, 8, PREAMBLE)
    put(31, 17, tow & 0x1FFFF)
    put(50, 3, sf_id)
    for name, (sf, pieces, _, _, _) in FIELDS.items():
        if sf != sf_id:
            continue
        code = code_of(name, eph[name]) if name not in INT_FIELDS else int(eph[name]) >> FIELDS[name][3]
        code &= (1 << _width(name)) - 1
        left = _width(name)
        for first, n in pieces:
            left -= n
            put(first, n, (code >> left) & ((1 << n) - 1))
    return [_slice(src, 30 * w + 1, 24) for w in range(10)]


def encode_stream(eph, tow0, ids=(1, 2, 3, 4, 5), seed=None, d29=0, d30=0):
    """consecutive subframes with the given IDs, TOW counting up from tow0, as a 0/1 bit stream (track_helpers' parity encoder)"""
    rng = None if seed is None else np.random.default_rng(seed)
    out = []
    for k, sf_id in enumerate(ids):
        b, d29, d30 = encode_subframe(subframe_words(eph, sf_id, tow0 + k, rng), d29, d30)
        out += b
    return np.array(out, np.uint8)


# ---- satellite state ----------------------------------------------------------------------------------------------------
def fold_ms(d):
    d = np.asarray(d, np.int64)
    return np.where(d > WEEK_MS // 2, d - WEEK_MS, np.where(d < -WEEK_MS // 2, d + WEEK_MS, d))


def _kepler(eph, tk):
    A = eph["sqrt_a"] ** 2
    n = math.sqrt(MU / A ** 3) + eph["dn"]
    M = eph["m_0"] + n * np.asarray(tk, np.float64)
    E = M.copy()
    for _ in range(30):
        prev = E
        E = M + eph["e"] * np.sin(E)
        if np.max(np.abs(E - prev)) < 1e-12:
            break
    return E


def clock_correction(eph, tk, tc):
    """a_f0 + a_f1 t + a_f2 t^2 + F e sqrt(A) sin E - t_gd at satellite time tk from t_oe, tc from t_oc"""
    tc = np.asarray(tc, np.float64)
    return eph["a_f0"] + eph["a_f1"] * tc + eph["a_f2"] * tc * tc + F_REL * eph["e"] * eph["sqrt_a"] * np.sin(_kepler(eph, tk)) - eph["t_gd"]


def position(eph, tk):
    """IS-GPS-200 Table 20-IV: ECEF (n, 3) at tk seconds of GPS time from t_oe"""
    tk = np.atleast_1d(np.asarray(tk, np.float64))
    A = eph["sqrt_a"] ** 2
    e = eph["e"]
    E = _kepler(eph, tk)
    nu = np.arctan2(math.sqrt(1 - e * e) * np.sin(E), np.cos(E) - e)
    phi = nu + eph["omega"]
    s2, c2 = np.sin(2 * phi), np.cos(2 * phi)
    u = phi + eph["c_us"] * s2 + eph["c_uc"] * c2
    r = A * (1 - e * np.cos(E)) + eph["c_rs"] * s2 + eph["c_rc"] * c2
    inc = eph["i_0"] + eph["c_is"] * s2 + eph["c_ic"] * c2 + eph["idot"] * tk
    om = eph["omega_0"] + (eph["omega_dot"] - OMEGA_E) * tk - OMEGA_E * float(eph["t_oe"])
    xp, yp = r * np.cos(u), r * np.sin(u)
    return np.stack([xp * np.cos(om) - yp * np.cos(inc) * np.sin(om), xp * np.sin(om) + yp * np.cos(inc) * np.cos(om), yp * np.sin(inc)], axis=-1)


def sat_state(eph, tx_ms, tx_frac):
    """(positions (n, 3), clock corrections (n,)) at the uncorrected satellite times (tx_ms, tx_frac)"""
    tx_ms = np.atleast_1d(np.asarray(tx_ms, np.int64))
    tx_frac = np.atleast_1d(np.asarray(tx_frac, np.float64))
    tk0 = fold_ms(tx_ms - 1000 * int(eph["t_oe"])) * 1e-3 + tx_frac
    tc = fold_ms(tx_ms - 1000 * int(eph["t_oc"])) * 1e-3 + tx_frac
    dt = clock_correction(eph, tk0, tc)
    return position(eph, tk0 - dt), dt


def split_time(ref_ms, off):
    """(ms of week, frac in [0, 1e-3)) of ref_ms + off seconds"""
    off = np.asarray(off, np.float64)
    k = np.floor(off * 1e3)
    frac = off - k * 1e-3
    k = np.where(frac < 0, k - 1, np.where(frac >= 1e-3, k + 1, k))
    frac = off - k * 1e-3
    return np.mod(np.asarray(ref_ms, np.int64) + k.astype(np.int64), WEEK_MS).astype(np.int32), frac


# ---- truth maker ---------------------------------------------------------------------------------------------------------
def truth_tx(eph, rx_xyz, ref_ms, t_rx):
    """Uncorrected satellite times seen at receive times ref_ms + t_rx (t_rx: seconds, array; ref_ms: one millisecond of week or
    one per receive time, so that t_rx can stay below a millisecond) by a receiver at rx_xyz, as offsets from ref_ms: the
    light-time equation |R(theta) sat(t_tx) - rx| = c (t_rx - t_tx), theta = Omega_e (t_tx - t_rx), then the clock
    correction inverted by fixed point (t_sv - dt(t_sv) = t_tx)."""
    t_rx = np.atleast_1d(np.asarray(t_rx, np.float64))
    bk = fold_ms(np.asarray(ref_ms, np.int64) - 1000 * int(eph["t_oe"])) * 1e-3
    bc = fold_ms(np.asarray(ref_ms, np.int64) - 1000 * int(eph["t_oc"])) * 1e-3
    t_tx = t_rx - 75e-3
    for _ in range(8):  # contracts by v / c ~ 1e-5 per pass
        p = position(eph, bk + t_tx)
        th = OMEGA_E * (t_tx - t_rx)
        xe = p[:, 0] * np.cos(th) - p[:, 1] * np.sin(th)
        ye = p[:, 0] * np.sin(th) + p[:, 1] * np.cos(th)
        rng = np.sqrt((rx_xyz[0] - xe) ** 2 + (rx_xyz[1] - ye) ** 2 + (rx_xyz[2] - p[:, 2]) ** 2)
        new = t_rx - rng / C
        done = np.max(np.abs(new - t_tx)) < 1e-16
        t_tx = new
        if done:
            break
    t_sv = t_tx.copy()
    for _ in range(8):  # contracts by ~1e-10 per pass
        new = t_tx + clock_correction(eph, bk + t_sv, bc + t_sv)
        done = np.max(np.abs(new - t_sv)) < 1e-16
        t_sv = new
        if done:
            break
    assert done  # below 1e-15 s
    return t_sv


# ---- solver --------------------------------------------------------------------------------------------------------------
def solve(sat_xyz, t_tx, weight):
    """The fix model of include/gpsacq.h on corrected transmit times given as offsets (seconds): returns dict(ok, xyz, t_rx (same
    offset base), rms, iterations).  Normal equations with the time unknown in metres, numpy.linalg.solve."""
    sat_xyz = np.asarray(sat_xyz, np.float64)
    t_tx = np.asarray(t_tx, np.float64)
    w = np.asarray(weight, np.float64)
    t0 = t_tx.mean() + 75e-3
    pos, bias = np.zeros(3), 0.0
    for it in range(20):
        t_rx = t0 - bias / C
        th = OMEGA_E * (t_tx - t_rx)
        sat = np.stack([sat_xyz[:, 0] * np.cos(th) - sat_xyz[:, 1] * np.sin(th), sat_xyz[:, 0] * np.sin(th) + sat_xyz[:, 1] * np.cos(th), sat_xyz[:, 2]], 1)
        d = pos - sat
        rng = np.sqrt((d * d).sum(1))
        res = C * (t_rx - t_tx) - rng
        H = np.concatenate([d / rng[:, None], np.ones((len(rng), 1))], 1)
        rms = math.sqrt((w * res * res).sum() / w.sum())
        try:
            step = np.linalg.solve(H.T @ (w[:, None] * H), H.T @ (w * res))
        except np.linalg.LinAlgError:
            return dict(ok=False, iterations=it)
        if not np.all(np.isfinite(step)):
            return dict(ok=False, iterations=it)
        pos = pos + step[:3]
        bias += step[3]
        if math.sqrt((step[:3] ** 2).sum()) < 1e-4:  # every step is applied; one below 1e-4 m is the last
            return dict(ok=True, xyz=pos, t_rx=t0 - bias / C, rms=rms, iterations=it + 1)
    return dict(ok=False, iterations=20)


def fix(ephs, eph_index, tx_ms, tx_frac, weight):
    """One fix from uncorrected satellite times: satellite states, offsets from the earliest millisecond, solve, receive time
    back as (ms, frac).  Returns solve()'s dict plus rx_ms, rx_frac."""
    tx_ms = np.asarray(tx_ms, np.int64)
    first = int(tx_ms[0])
    d = fold_ms(tx_ms - first)
    ms0 = first + int(d.min())
    xyz, t = [], []
    for j, k in enumerate(eph_index):
        p, dt = sat_state(ephs[k], tx_ms[j], tx_frac[j])
        xyz.append(p[0])
        t.append(float(d[j] - d.min()) * 1e-3 + tx_frac[j] - dt[0])
    out = solve(np.array(xyz), np.array(t), weight)
    if out["ok"]:
        ms, frac = split_time(ms0, out["t_rx"])
        out["rx_ms"], out["rx_frac"] = int(ms), float(frac)
    return out


# ---- geodesy -------------------------------------------------------------------------------------------------------------
def ecef_of(lat, lon, alt):
    N = WGS84_A / math.sqrt(1 - WGS84_E2 * math.sin(lat) ** 2)
    return np.array([(N + alt) * math.cos(lat) * math.cos(lon), (N + alt) * math.cos(lat) * math.sin(lon), (N * (1 - WGS84_E2) + alt) * math.sin(lat)])


def pdop(rx_xyz, sat_xyz):
    """sqrt(trace of the position block of (H^T H)^-1), H rows (unit vector, 1)"""
    d = np.asarray(rx_xyz) - np.asarray(sat_xyz)
    H = np.concatenate([d / np.sqrt((d * d).sum(1))[:, None], np.ones((len(d), 1))], 1)
    return math.sqrt(np.trace(np.linalg.inv(H.T @ H)[:3, :3]))


def elevation(rx_xyz, sat_xyz):
    up = np.asarray(rx_xyz) / np.linalg.norm(rx_xyz)  # geocentric vertical: good to 0.2 degrees, only used to pick satellites
    d = np.asarray(sat_xyz) - np.asarray(rx_xyz)
    return np.arcsin((d @ up) / np.sqrt((d * d).sum(-1)))


# ---- the synthetic constellation -------------------------------------------------------------------------------------------
T_OE = 388800            # seconds of week (a multiple of 16)
REF_MS = 389_400_000     # the tests' receive times start here: t_oe + 600 s
RX_LLA = (math.radians(47.3), math.radians(8.5), 100.0)   # a mid-latitude point, 100 m up
RX_LLA_SOUTH = (math.radians(-60.0), math.radians(170.0), 100.0)


def make_constellation(rx_xyz, seed=20111, n=12, n_visible=9, t_oe=T_OE, ref_ms=REF_MS):
    """n quantised ephemerides (PRN 1..n): elements as in a real almanac, Omega_0 and M_0 drawn over the sphere until the first
    n_visible satellites stand at least 10 degrees above rx_xyz's horizon at ref_ms (the rest fall where they fall)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = len(out)
        eph = dict(
            week=597, iodc=0x100 | (k + 1), iode2=k + 1, iode3=k + 1, t_oc=t_oe, t_oe=t_oe,
            t_gd=rng.uniform(-2e-8, 2e-8), a_f0=rng.uniform(-5e-4, 5e-4), a_f1=rng.uniform(-2e-11, 2e-11), a_f2=0.0,
            sqrt_a=5153.6 + rng.uniform(-0.3, 0.3), e=rng.uniform(0.001, 0.02), i_0=rng.uniform(0.94, 0.99),
            omega_0=rng.uniform(-math.pi, math.pi), m_0=rng.uniform(-math.pi, math.pi), omega=rng.uniform(-math.pi, math.pi),
            dn=rng.uniform(3e-9, 6e-9), omega_dot=rng.uniform(-9e-9, -7e-9), idot=rng.uniform(-5e-10, 5e-10),
            c_rs=rng.uniform(-80, 80), c_rc=rng.uniform(150, 350), c_us=rng.uniform(-9e-6, 9e-6), c_uc=rng.uniform(-5e-6, 5e-6),
            c_is=rng.uniform(-2e-7, 2e-7), c_ic=rng.uniform(-2e-7, 2e-7))
        eph = quantise(eph)
        eph["prn"] = k + 1
        p = position(eph, float(fold_ms(ref_ms - 1000 * t_oe)) * 1e-3)[0]
        if k < n_visible and elevation(rx_xyz, p) < math.radians(10):
            continue
        out.append(eph)
    return out


def best_subset(rx_xyz, sat_xyz, candidates, k):
    """the k of `candidates` (indices) with the lowest PDOP"""
    best = min(itertools.combinations(candidates, k), key=lambda c: pdop(rx_xyz, sat_xyz[list(c)]))
    return list(best), pdop(rx_xyz, sat_xyz[list(best)])
