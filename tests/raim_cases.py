"""Observation batches of the integrity tests (tests/test_raim.py, tests/test_gpu_raim.py) and the glue between OBS_DTYPE rows and
tests/raim_ref.py: noise of a known sigma on exact observations of the "north" geometry, one satellite's transmit time pulled,
the reference of a row with its indices mapped back to the row's columns, and the preconditions a row must meet before a GPU
result is compared with it (asserted on the reference alone)."""
import math

import numpy as np

import atm_ref
import nav_ref
import raim_ref
from nav_helpers import geometry

SIGMA_M = 3.0
MARGIN = 0.05       # distance of a statistic from the threshold it is compared with, relative
RUNNER_UP = 1.05    # the second smallest T_k over the smallest
_truth = {}


def truth(flags, n=130):
    """(geo, ref_ms[n], t_rx[n], obs[n][12]) of the "north" geometry: exact observations through the model's atmosphere with the
    delays of `flags` on the path (0: vacuum); made once per flags and never written to"""
    import gpsacq
    if flags not in _truth:
        geo = geometry("north")
        k = np.arange(n)
        ref_ms = (geo["ref_ms"] + k.astype(np.int64)) % nav_ref.WEEK_MS  # 1 ms apart: the elevations stand still
        t_rx = (0.137e-3 + k * 0.0131e-3) % 1e-3
        tx_ms, tx_frac = atm_ref.truth_times(geo["ephs"], geo["rx"], ref_ms, t_rx, atm_ref.params(flags=flags))
        obs = np.zeros(tx_ms.shape, gpsacq.OBS_DTYPE)
        obs["tx_ms"], obs["tx_frac"], obs["eph"], obs["valid"], obs["weight"] = tx_ms, tx_frac, np.arange(12), 1, 1.0
        obs.setflags(write=False)
        _truth[flags] = (geo, ref_ms, t_rx, obs)
    return _truth[flags]


def shift(ob, metres):
    """ob (a writable OBS_DTYPE array) with every transmit time moved by metres / c (same shape, or broadcast)"""
    ms, frac = nav_ref.split_time(ob["tx_ms"], ob["tx_frac"] + np.asarray(metres, np.float64) / nav_ref.C)
    ob["tx_ms"], ob["tx_frac"] = ms, frac
    return ob


def noisy(obs, seed, sigma_m=SIGMA_M):
    """a copy of obs with seeded Gaussian noise of sigma_m / sqrt(weight) metres on every transmit time"""
    ob = obs.copy()
    rng = np.random.default_rng(seed)
    w = np.where(ob["weight"] > 0, ob["weight"], 1.0)
    return shift(ob, rng.normal(0.0, sigma_m, ob.shape) / np.sqrt(w))


def usable(geo, row):
    return [s for s in range(len(row)) if row["valid"][s] and 0 <= row["eph"][s] < len(geo["ephs"]) and row["weight"][s] >= 0
            and math.isfinite(row["weight"][s])]


def reference(geo, row, p, rp):
    """raim_ref.fix_raim of one OBS_DTYPE row (its usable observations); used_mask and excluded are in the row's columns"""
    u = usable(geo, row)
    ref = raim_ref.fix_raim(geo["ephs"], row["eph"][u], row["tx_ms"][u], row["tx_frac"][u], row["weight"][u], p, rp)
    ref["usable"] = u
    ref["used_mask"] = sum(1 << u[j] for j in range(len(u)) if ref["kept"][j])
    ref["excluded"] = u[ref["raim"]["excluded"]] if ref["raim"]["excluded"] >= 0 else -1
    return ref


def precondition(ref, p, rp):
    """None, or why the row is too close to a decision for a comparison of two fp64 implementations to be meaningful"""
    full, raim = ref["full"], ref["raim"]
    if full["status"] != 0:
        return None
    el = atm_ref.view(full["lla"][0], full["lla"][1], full["sat"] - full["xyz"])[1]
    if np.abs(el - p["elev_mask"]).min() < math.radians(1.0):
        return "elevation %.3f degrees from the mask" % np.degrees(np.abs(el - p["elev_mask"]).min())
    d = raim["dof"] + (1 if raim["status"] == raim_ref.EXCLUDED else 0)
    if d < 1:
        return None
    thr = rp["threshold"]
    if abs(raim["stat_full"] / thr[d - 1] - 1) < MARGIN:
        return "stat_full %.4g next to %.4g" % (raim["stat_full"], thr[d - 1])
    t = sorted(ref["candidates"].values())
    if t:
        if abs(t[0] / thr[d - 2] - 1) < MARGIN:
            return "winner %.4g next to %.4g" % (t[0], thr[d - 2])
        if len(t) > 1 and t[0] <= thr[d - 2] and t[1] < RUNNER_UP * t[0]:
            return "runner-up %.4g next to the winner %.4g" % (t[1], t[0])
    return None


# ---- the batches ---------------------------------------------------------------------------------------------------------------
FAULT_M = 150.0
_batches = {}


def _batch(cols, flags, elev_mask, seed, rows, faults, weights=None, exclude=1):
    """(geo, ob, p, rp): rows `rows` of the truth with the delays of `flags`, columns `cols`, optional weights [n][len(cols)], noise
    of SIGMA_M from `seed`, then faults {row: (col, metres)} on top"""
    geo, _, _, obs = truth(flags)
    ob = obs[rows][:, cols].copy()
    if weights is not None:
        ob["weight"] = weights
    ob = noisy(ob, seed)
    for r, (c, m) in faults.items():
        ob[r:r + 1, c:c + 1] = shift(ob[r:r + 1, c:c + 1].copy(), m)
    return geo, ob, atm_ref.params(flags=flags, elev_mask=elev_mask), raim_ref.params(SIGMA_M, exclude=exclude)


def batch(name):
    """The named batch of the GPU tests, made once: (geo, ob [n][sats] OBS_DTYPE, atmosphere params, raim params).  Twelve
    columns: satellites 9 and 10 stand below the horizon, so the 5-degree mask leaves ten (dof 6) and a fault on 9 or 10 is
    masked away."""
    if name in _batches:
        return _batches[name]
    geo = geometry("north")
    all12, mask5, none = list(range(12)), math.radians(5.0), -math.pi / 2
    up = [k for k in range(12) if geo["elevation"][k] > 0]
    six = nav_ref.best_subset(geo["rx"], geo["sat_xyz"], up, 6)[0]
    if name == "one":        # a lone group
        b = _batch(all12, 3, mask5, 11, slice(0, 1), {0: (4, FAULT_M)})
    elif name == "three":    # a partial wave: clean, the fault in the first and in the last lane of the group
        b = _batch(all12, 3, mask5, 12, slice(0, 3), {1: (0, FAULT_M), 2: (11, -FAULT_M)})
    elif name == "sixtyseven":  # neither a multiple of 4 nor of the block, with every special row
        faults = {r: ((5 * r) % 12, FAULT_M if r % 2 else -FAULT_M) for r in range(67) if (r * r + r // 3) % 4 == 0}
        faults.update({5: (2, FAULT_M), 9: (3, 3000.0), 64: (0, 60.0), 66: (11, FAULT_M)})
        faults.pop(13, None)
        geo_, ob, p, rp = _batch(all12, 3, mask5, 13, slice(0, 67), faults)
        ob["valid"][5, 6] = 0         # a hole mid-row, next to a fault
        ob["weight"][9, 3] = 0.0      # the fault sits on a weight-0 observation: never a candidate, adds nothing to T
        ob["valid"][13, 3:] = 0       # three usable: FULL fails
        ob["valid"][14, :] = 0        # nothing at all
        b = (geo_, ob, p, rp)
    elif name == "mixed":    # 130 rows, faulted and clean alternating irregularly: passing and excluding groups share a wave
        faults = {r: ((7 * r + 3) % 12, (60.0, 150.0, -300.0, 3000.0)[r % 4]) for r in range(130) if (r * r + 3 * r) % 7 in (0, 1, 3)}
        b = _batch(all12, 3, mask5, 14, slice(0, 130), faults)
    elif name == "plain":    # the plain fix: nothing masked, no delays, FINAL without rounds; all twelve used (dof 8)
        b = _batch(all12, 0, none, 15, slice(0, 9), {r: ((4 * r + 1) % 12, FAULT_M) for r in (0, 2, 3, 6, 8)})
    elif name == "plain_masked":  # no delays but the mask drops two: FINAL runs its rounds with zero delays
        b = _batch(all12, 0, mask5, 16, slice(0, 5), {1: (7, FAULT_M), 4: (0, -FAULT_M)})
    elif name == "weights":  # weights spread over 0.25 .. 4
        w = 2.0 ** np.random.default_rng(17).uniform(-2.0, 2.0, (8, 12))
        b = _batch(all12, 3, mask5, 17, slice(0, 8), {r: ((3 * r + 2) % 9, FAULT_M) for r in (0, 1, 4, 5, 7)}, weights=w)
    elif name == "six":      # dof 2: an exclusion leaves dof 1, where the winner need not be the faulted one.  No fault on column 5:
        # without column 4 or without column 5 this geometry gives statistics 1e-3 apart, whatever the noise (ten seeds tried)
        b = _batch(six, 3, mask5, 18, slice(0, 8), {0: (0, FAULT_M), 2: (2, FAULT_M), 3: (3, -FAULT_M), 5: (1, FAULT_M), 7: (1, -FAULT_M)})
    elif name == "five":     # dof 1: a faulted row is FAILED, never EXCLUDED
        b = _batch(geo["subsets"][5], 3, mask5, 19, slice(0, 6), {r: (r % 5, FAULT_M) for r in (1, 2, 4)})
    elif name == "four":     # dof 0: UNCHECKED
        b = _batch(geo["subsets"][4], 3, mask5, 20, slice(0, 4), {2: (1, FAULT_M)})
    elif name == "all_faulted":
        b = _batch(all12, 3, mask5, 21, slice(0, 8), {r: ((r * 5) % 9, FAULT_M) for r in range(8)})
    elif name == "none_faulted":
        b = _batch(all12, 3, mask5, 22, slice(0, 8), {})
    elif name == "no_exclusion":  # exclude = 0 on the rows of "three"
        geo_, ob, p, rp = batch("three")
        b = (geo_, ob, p, dict(rp, exclude=0))
    else:
        raise KeyError(name)
    b[1].setflags(write=False)
    _batches[name] = b
    return b


BATCHES = ("one", "three", "sixtyseven", "mixed", "plain", "plain_masked", "weights", "six", "five", "four", "all_faulted", "none_faulted",
           "no_exclusion")
_refs = {}


def references(name):
    """[reference(row) for the rows of batch(name)], computed once and shared"""
    if name not in _refs:
        geo, ob, p, rp = batch(name)
        _refs[name] = [reference(geo, ob[k], p, rp) for k in range(len(ob))]
    return _refs[name]
