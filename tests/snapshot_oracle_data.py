"""Reader of tests/golden/snapshot_oracle.npz (made by tests/golden/make_snapshot_oracle.py from tests/snapshot_oracle.py) on top of
tests/golden/nav_oracle.npz, shared by tests/test_snapshot_oracle.py and tests/test_gpu_snapshot_oracle.py.  numpy only: the record
layouts below are the library's (gnss-gps-sdr_amd/python/gpsacq), restated so that the CPU test needs no library; the GPU test
asserts that they are equal.

The tolerances are the project's own, unchanged, each with the file it is taken from."""
import os

import numpy as np

import nav_oracle_data as nod
from nav_oracle_data import ALT_TOL, LATLON_TOL, POS_TOL, TIME_TOL, angle_diff, constellation  # noqa: F401  (tests/nav_oracle_data.py)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_oracle.npz")
C, L1, WEEK_MS = 2.99792458e8, 1575.42e6, 604800000
MASK = np.radians(5.0)
RX_TIME_WORST, COARSE_S_WORST, MARGIN_MIN_MS = 7e-11, 7e-11, 0.05   # tests/test_coarse.py
RX_TOL, S_TOL, CDOP_MEASURED = 10 * RX_TIME_WORST, 10 * COARSE_S_WORST, 1.9e-3   # tests/test_gpu_coarse.py: TIME_TOL, S_TOL, CDOP_MEASURED
DOP_REL_TOL, FRAC_TOL, EDGE = 1e-9, 1e-12, 1e-8                     # tests/test_gpu_coarse.py: pdop / cdop, obs_out's tx_frac, the edge rule
PLACE_TOL, DRIFT_TOL = 1e-3, 1e-13                                  # tests/dop_ref.py (tests/test_gpu_doppler.py's figures)
DOP_PDOP_REL, DOP_RMS_TOL, DOP_ALT_TOL = 1e-4, 1e-6, 2e-3           # tests/dop_ref.py, same_fix
AID_FRAC_TOL, AID_DOPPLER_TOL, AID_ELEV_TOL = 1e-12, 1e-6, 1e-9     # tests/test_gpu_aided.py
H_FD = 0.05
PER_SAT = 900.0 ** 2 / C + C * 2e-15 / (2 * H_FD) + 1e-6            # tests/test_gpu_nav_oracle.py's derived bound per satellite, m/s
TIE_RULE, TIE_CAP = 1e-6, 0.02                                      # tests/test_nav_oracle.py's cap on excluded cases
SIGMA_EXACT = 10.0                                                  # tests/coarse_raim_cases.py's SIGMA_M
RAIM_SHIFT = 0.3e-3
FIX_OK, INCONSISTENT = 0, 1
VEL_OK = 0
AID_LOW, AID_OFF_GRID = 4, 8
RAIM_UNCHECKED, RAIM_PASS, RAIM_EXCLUDED = 1, 2, 3

OBS_DTYPE = np.dtype([("eph", "<i4"), ("valid", "<i4"), ("tx_ms", "<i4"), ("reserved", "<i4"), ("tx_frac", "<f8"), ("weight", "<f8")])
RATE_OBS_DTYPE = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("adr", "<i8"), ("doppler_hz", "<f8"), ("weight", "<f8")])
COARSE_PRIOR_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("rx_ms", "<i4"), ("reserved", "<i4")])
FIX_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("iterations", "<i4"), ("rx_ms", "<i4"), ("rx_frac", "<f8"),
                      ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("lat", "<f8"), ("lon", "<f8"), ("alt", "<f8"), ("rms", "<f8")])
VEL_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("vx", "<f8"), ("vy", "<f8"), ("vz", "<f8"), ("ve", "<f8"), ("vn", "<f8"),
                      ("vu", "<f8"), ("drift", "<f8"), ("rms", "<f8")])
DTYPES = dict(OBS_DTYPE=OBS_DTYPE, RATE_OBS_DTYPE=RATE_OBS_DTYPE, COARSE_PRIOR_DTYPE=COARSE_PRIOR_DTYPE, FIX_DTYPE=FIX_DTYPE, VEL_DTYPE=VEL_DTYPE)

_cache = {}


def load():
    """both fixtures' arrays in one dict, read once, read-only"""
    if "data" not in _cache:
        with np.load(PATH) as z:
            data = {k: z[k] for k in z.files}
        for v in data.values():
            v.setflags(write=False)
        data.update(nod.load())
        _cache["data"] = data
    return _cache["data"]


def all_ephs():
    """the 11 constellations one after the other: satellite s of fix site f is ephemeris 12 f + s"""
    if "ephs" not in _cache:
        _cache["ephs"] = [e for f in range(len(load()["fix_site"])) for e in constellation(f)]
    return _cache["ephs"]


def fold_ms(d):
    d = np.asarray(d, np.int64)
    return np.where(d > WEEK_MS // 2, d - WEEK_MS, np.where(d < -WEEK_MS // 2, d + WEEK_MS, d))


def rows():
    """the 88 fix rows, site outer and instant inner: dict(site [88][3], lla [88][3], ref_ms [88], t_rx [88], up [88][12] (fix_el >=
    5 degrees), vac_ms / vac_frac [88][12], f [88] (fix site of the row), j [88] (instant))"""
    if "rows" not in _cache:
        d = load()
        F, J, S = d["fix_vac_ms"].shape
        r = dict(site=np.repeat(d["site_xyz"][d["fix_site"]], J, axis=0), lla=np.repeat(d["site_lla"][d["fix_site"]], J, axis=0),
                 ref_ms=d["fix_ref_ms"].ravel().astype(np.int64), t_rx=d["fix_t_rx"].ravel().copy(), up=(d["fix_el"] >= MASK).reshape(F * J, S),
                 vac_ms=d["fix_vac_ms"].reshape(F * J, S).astype(np.int64), vac_frac=d["fix_vac_frac"].reshape(F * J, S).copy(),
                 f=np.repeat(np.arange(F), J), j=np.tile(np.arange(J), F))
        for v in r.values():
            v.setflags(write=False)
        _cache["rows"] = r
    return _cache["rows"]


def phase_obs(masked=True, sel=None):
    """OBS [n][12] of code phases alone: tx_frac = fix_vac_frac, tx_ms = 0, weight 1, valid on the columns at fix_el >= 5 degrees
    (masked) or on all twelve.  sel: row indices, default all 88"""
    r = rows()
    sel = np.arange(len(r["f"])) if sel is None else np.asarray(sel)
    obs = np.zeros((len(sel), 12), OBS_DTYPE)
    obs["eph"] = 12 * r["f"][sel][:, None] + np.arange(12)[None, :]
    obs["tx_frac"], obs["weight"] = r["vac_frac"][sel], 1.0
    obs["valid"] = r["up"][sel] if masked else 1
    return obs


def rate_obs(which="model", masked=True):
    """RATE_OBS [88][12] of the fixture's Dopplers (which: "model" or "phys"), weight 1"""
    d, r = load(), rows()
    ro = np.zeros((88, 12), RATE_OBS_DTYPE)
    ro["doppler_hz"], ro["weight"] = d["dop_" + which].reshape(88, 12), 1.0
    ro["valid"] = r["up"] if masked else 1
    return ro


def drifts():
    """the receiver clock drift of each of the 88 rows"""
    return load()["dop_drift"][rows()["j"]]


def coarse_prior(xyz, rx_ms):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    p = np.zeros(len(xyz), COARSE_PRIOR_DTYPE)
    p["x"], p["y"], p["z"], p["rx_ms"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], np.asarray(rx_ms, np.int64) % WEEK_MS
    return p


def priors(seed=1, km=30.0, secs=30.0):
    """COARSE_PRIOR [88]: km kilometres from the site in a seeded random direction, secs seconds from fix_ref_ms, early and late in
    turn (tests/coarse_helpers.py's priors)"""
    r = rows()
    rng = np.random.default_rng(seed)
    n = len(r["f"])
    way = rng.normal(size=(n, 3))
    way *= km * 1e3 / np.linalg.norm(way, axis=1)[:, None]
    sign = np.where((np.arange(n) + seed) % 2 == 0, 1, -1)
    return coarse_prior(r["site"] + way, r["ref_ms"] + sign * int(secs * 1000))


def rx_error(rx_ms, rx_frac, sel=None):
    """receive times against fix_ref_ms + fix_t_rx, seconds"""
    r = rows()
    sel = np.arange(len(r["f"])) if sel is None else np.asarray(sel)
    return fold_ms(np.asarray(rx_ms, np.int64) - r["ref_ms"][sel]) * 1e-3 + (np.asarray(rx_frac) - r["t_rx"][sel])


def pred_fix():
    """FIX [R] of the prediction rows"""
    d = load()
    fx = np.zeros(len(d["pred_site"]), FIX_DTYPE)
    fx["x"], fx["y"], fx["z"] = d["pred_xyz"].T
    fx["rx_ms"], fx["rx_frac"], fx["n_used"] = d["pred_rx_ms"], d["pred_rx_frac"], 8
    return fx


def pred_vel():
    """VEL [R] of the prediction rows"""
    d = load()
    v = np.zeros(len(d["pred_site"]), VEL_DTYPE)
    v["status"], v["vx"], v["vy"], v["vz"], v["drift"] = d["pred_vel"].T
    return v


def engine_grid():
    """(fs, spm, doppler_step_hz, kmax) the stored grid positions belong to"""
    d = load()
    return float(d["pred_fs"].ravel()[0]), int(d["pred_spm"].ravel()[0]), float(d["pred_step_hz"].ravel()[0]), int(d["pred_kmax"].ravel()[0])


def code_phase_bound():
    """[88][12] seconds: how far the PREDICTED code phase may stand from the true one, fix_vac_frac.  LIGHT TIME, pass 2, takes
    "position and clock correction cc at the uncorrected time -tau": the satellite clock reads -tau there, so the orbit is evaluated
    at the GPS time -tau - cc, cc too early, and cc itself at a satellite time cc off.  T = cc - tau' is therefore off by cc (range
    rate / c + clock drift).  The range rate of each case is the fixture's physical Doppler, -(c / L1) dop_phys - c drift_r + c d, and
    c |d| is at most 2 m/s over the whole fields of a_f1 and a_f2 (c 2^15 2^-43 = 1.1 m/s, c 2 a_f2 t below 0.02 m/s, the relativistic term
    below 0.01 m/s).  With a_f0 over its whole field (+-0.98 ms) and 930 m/s this reaches 3e-9 s, a sixtieth of a sample at 5.456 MHz."""
    d = load()
    rate = np.abs((C / L1) * d["dop_phys"] + C * d["dop_drift"][None, :, None]) + 2.0
    return (np.abs(d["fix_clock"]) * (rate + 2.0) / C).reshape(88, 12)


def pred_integer_cases():
    """(code [R][S], doppler [R][S]): the predictions whose grid position stands TIE_RULE or more from a rounding tie, the only ones
    compared as integers"""
    d = load()
    away = lambda x: np.abs(np.abs(x - np.floor(x)) - 0.5) >= TIE_RULE
    return away(d["pred_ca_pos"]), away(d["pred_lo_pos"])


def tie_case():
    """(OBS [T][12] over the masked columns, COARSE_PRIOR [T], row index of each into rows())"""
    d, r = load(), rows()
    row = 8 * d["tie_site"] + d["tie_instant"]
    return phase_obs(True, row), coarse_prior(d["tie_xyz"], d["tie_rx_ms"]), row


def raim_case():
    """test 3's rows: (OBS [88][12] over the masked columns with one code phase moved by RAIM_SHIFT, the moved column per row): column
    0, the reference (at fix_el >= 5 degrees in every row: tests/test_snapshot_oracle.py asserts it), on even rows and the last
    masked-in column on odd rows"""
    r = rows()
    obs = phase_obs(True)
    col = np.array([0 if i % 2 == 0 else np.flatnonzero(u)[-1] for i, u in enumerate(r["up"])])
    i = np.arange(len(col))
    obs["tx_frac"][i, col] = (obs["tx_frac"][i, col] + RAIM_SHIFT) % 1e-3
    return obs, col
