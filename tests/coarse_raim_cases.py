"""Batches of the coarse-time integrity tests (tests/test_coarse_raim.py on the CPU, tests/test_gpu_coarse_raim.py on the GPU) and
the preconditions a row must meet before a GPU result is compared with tests/coarse_raim_ref.py, asserted on the reference alone.

A batch is tests/test_coarse.py's make_case (exact code phases of a geometry, priors 30 km / 30 s off), seeded Gaussian noise of
SIGMA_M / sqrt(weight) metres on every code phase, and FAULTS on top: a code phase moved by so many metres, modulo the millisecond,
as a false peak moves it.  The faults are 0.9 .. 60 km anywhere and 105 km (0.35 ms) on the reference column: a false column is
rounded to its whole millisecond like any other, the prior's 30 km / 30 s have used 0.1 - 0.25 ms of the half millisecond already,
and a larger fault sits on the rounding edge in FULL and in every candidate that keeps it (the one exception is below).  Faults,
seeds and sigma were chosen on the CPU so that the reference alone meets the precondition.

PRECONDITION.  Two fp64 evaluations of one model agree in what they decide only where the decision is not a matter of rounding:
    MARGIN         every statistic stands 5 % off the threshold it meets (the figure of tests/raim_cases.py)
    RUNNER_UP      the second smallest T_k is 1.05 times the smallest
    MARGIN_MIN_MS  the whole milliseconds of FULL and of every candidate were rounded 0.05 ms from the edge (tests/test_coarse.py)
NARROW ROWS.  A fault of 0.48 ms on the reference column leaves FULL, and every candidate that keeps the column, 0.02 ms of
rounding margin and less: which way they round is not the model's business, and FULL's rms -- stat_full -- with it.  What IS
decided: such a solve keeps a column 144 km off or takes a millisecond wrong, 300 km, so its statistic is 1e6 and more against a
threshold of 20, FULL fails the test and none of those candidates wins; the candidate that drops the column has its margin like any
other row.  narrow(row) says so, and such a row is compared on status, excluded and the output solution only -- not on stat_full
and not on n_candidates (a solve 300 km off may or may not converge).  At most one row in eight of a batch may be narrow."""
import numpy as np

import coarse_raim_ref
import coarse_ref
import nav_ref
import raim_ref
from nav_helpers import geometry
from test_coarse import MARGIN_MIN_MS, make_case

SIGMA_M = 10.0
MARGIN = 0.05
RUNNER_UP = 1.05
NARROW_T = 1e4   # what a narrow row's FULL and losing candidates must exceed: no rounding of theirs brings 1e4 below 30


def move(ob, row, col, metres):
    ob["tx_frac"][row, col] = (ob["tx_frac"][row, col] + metres / nav_ref.C) % 1e-3


def noisy(obs, seed, sigma_m=SIGMA_M):
    ob = obs.copy()
    w = np.where(ob["weight"] > 0, ob["weight"], 1.0)
    ob["tx_frac"] = (ob["tx_frac"] + np.random.default_rng(seed).normal(0.0, sigma_m, ob.shape) / np.sqrt(w) / nav_ref.C) % 1e-3
    return ob


def narrow(row):
    return row["full"]["status"] == coarse_ref.FIX_OK and row["full"]["margin"] < MARGIN_MIN_MS


def precondition(row, rp):
    """None, or why the row is too close to a decision for a comparison of two fp64 implementations to be meaningful"""
    full, raim = row["full"], row["raim"]
    if full["status"] != coarse_ref.FIX_OK:
        return None if full["n_used"] < 5 else "FULL did not converge"
    d, thr = row["n_w"] - 5, rp["threshold"]
    T = sorted(row["candidates"].items(), key=lambda kt: kt[1])
    if narrow(row):
        if raim["status"] != coarse_raim_ref.EXCLUDED:
            return "a narrow row that is not mended"
        k = raim["excluded"]
        if row["cand"][k]["margin"] < MARGIN_MIN_MS:
            return "the winner's margin %.3f ms" % row["cand"][k]["margin"]
        if abs(T[0][1] / thr[d - 2] - 1) < MARGIN:
            return "winner %.4g next to %.4g" % (T[0][1], thr[d - 2])
        if raim["stat_full"] < NARROW_T or any(t < NARROW_T for _, t in T[1:]):
            return "a narrow row whose other solves are not far off"
        if any(c["margin"] < MARGIN_MIN_MS and j in row["candidates"] and row["candidates"][j] < NARROW_T for j, c in row["cand"].items()):
            return "a candidate on the rounding edge with a small statistic"
        return None
    if full["margin"] < MARGIN_MIN_MS:
        return "FULL's margin %.3f ms" % full["margin"]
    if d < 1:
        return None
    if abs(raim["stat_full"] / thr[d - 1] - 1) < MARGIN:
        return "stat_full %.4g next to %.4g" % (raim["stat_full"], thr[d - 1])
    for k, c in row["cand"].items():
        if c["margin"] < MARGIN_MIN_MS:
            return "candidate %d's margin %.3f ms" % (k, c["margin"])
        if c["status"] == coarse_ref.FIX_NO_CONVERGE:
            return "candidate %d did not converge" % k
    if T:
        if abs(T[0][1] / thr[d - 2] - 1) < MARGIN:
            return "winner %.4g next to %.4g" % (T[0][1], thr[d - 2])
        if len(T) > 1 and T[0][1] <= thr[d - 2] and T[1][1] < RUNNER_UP * T[0][1]:
            return "runner-up %.4g next to the winner %.4g" % (T[1][1], T[0][1])
    return None


# ---- the batches ---------------------------------------------------------------------------------------------------------------
KM = 1e3
_batches, _refs = {}, {}


def _sel(which, sats):
    geo = geometry(which)
    up = [k for k in range(12) if geo["elevation"][k] > 0]
    if sats == "up":
        return up
    if sats in geo["subsets"]:
        return geo["subsets"][sats]
    return nav_ref.best_subset(geo["rx"], geo["sat_xyz"], up, sats)[0]


def _batch(which, sats, n, seed, faults, weights=None, exclude=1, sigma_m=SIGMA_M, p_fa=1e-3):
    """(geo, ob, prior, rp): n rows of the geometry's `sats` satellites, optional weights [n][sats], noise of sigma_m from `seed`,
    then faults {row: (col, metres) or a list of them} on top"""
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, _sel(which, sats), n, seed=seed)
    if weights is not None:
        obs["weight"] = weights
    ob = noisy(obs, seed, sigma_m)
    for r, f in faults.items():
        for c, metres in (f if isinstance(f, list) else [f]):
            move(ob, r, c, metres)
    return geo, ob, prior, raim_ref.params(sigma_m, p_fa=p_fa, exclude=exclude)


def batch(name):
    """The named batch, made once: (geo, ob [n][sats] OBS_DTYPE, prior [n], raim params)"""
    if name in _batches:
        return _batches[name]
    if name == "one":          # a lone group
        b = _batch("north", 8, 1, 11, {0: (4, 30 * KM)})
    elif name == "three":      # a partial wave: clean, a small fault on the reference column, a fault on the last column
        b = _batch("north", 8, 3, 12, {1: (0, 3 * KM), 2: (7, -30 * KM)})
    elif name == "sixtyseven":  # neither a multiple of 4 nor of the block, twelve columns, with every special row
        sizes = (0.9 * KM, -3 * KM, 30 * KM, -60 * KM, 45 * KM)
        faults = {r: ((5 * r) % 12, sizes[r % 5]) for r in range(67) if (r * r + r // 3) % 4 == 0}
        faults.update({5: (2, 30 * KM), 9: (3, 60 * KM), 20: (1, 30 * KM), 64: (0, 105 * KM), 66: (11, 30 * KM)})
        for r in (13, 14):
            faults.pop(r, None)
        geo, ob, prior, rp = _batch("north", 12, 67, 13, faults)
        ob["valid"][5, 6] = 0         # a hole mid-row, next to a fault
        ob["weight"][9, 3] = 0.0      # the fault sits on a weight-0 observation: never a candidate, adds nothing to T
        ob["valid"][13, 4:] = 0       # four usable: TOO_FEW
        ob["valid"][14, :] = 0        # nothing at all
        ob["valid"][20, 0] = 0        # an invalid first column: ref = 1, and the fault is on it
        b = (geo, ob, prior, rp)
    elif name == "mixed":      # 130 rows of eight, faulted and clean alternating irregularly: passing and excluding groups share a wave
        sizes = (0.9 * KM, 30 * KM, -60 * KM, 3 * KM)
        faults = {r: ((7 * r + 3) % 8, sizes[r % 4]) for r in range(130) if (r * r + 3 * r) % 7 in (0, 1, 3)}
        faults.update({64: (0, 105 * KM), 65: (0, -105 * KM), 129: (7, 30 * KM)})  # 0.35 ms on the reference column, either way
        faults[58] = (1, 30 * KM)  # with -60 km here the candidate without column 0 rounds 0.034 ms from the edge
        b = _batch("north", 8, 130, 14, faults)
    elif name == "south":      # the nine satellites above the southern receiver's horizon
        b = _batch("south", "up", 8, 15, {0: (0, 105 * KM), 2: (8, 0.9 * KM), 3: (4, -30 * KM), 5: (1, 60 * KM), 6: (0, 0.9 * KM)})
    elif name == "rollover":   # t0 on either side of the end of the week
        b = _batch("rollover", 8, 30, 16, {r: ((3 * r + 1) % 8, (30 * KM, -3 * KM, 60 * KM)[r % 3]) for r in range(0, 30, 2)})
    elif name == "weights":    # weights spread over 0.25 .. 4
        w = 2.0 ** np.random.default_rng(17).uniform(-2.0, 2.0, (8, 9))
        b = _batch("south", "up", 8, 17, {r: ((3 * r + 2) % 9, 30 * KM) for r in (0, 1, 4, 5, 7)}, weights=w)
    elif name == "narrow":     # 0.48 ms on the reference column: only a candidate that does step A again mends it
        b = _batch("north", 8, 8, 18, {1: (0, 0.48e-3 * nav_ref.C), 6: (5, 30 * KM)})
    elif name == "seven":      # d = 2: an exclusion leaves one degree of freedom, where the winner need not be the faulted column
        b = _batch("north", 7, 8, 19, {0: (0, 0.9 * KM), 2: (2, 30 * KM), 3: (6, -3 * KM), 5: (1, 105 * KM), 7: (4, -30 * KM)})
    elif name == "six":        # d = 1: a faulted row is FAILED and no candidate is tried
        b = _batch("north", 6, 6, 20, {r: (r % 6, 30 * KM) for r in (1, 2, 4)})
    elif name == "five":       # d = 0: UNCHECKED
        b = _batch("north", 5, 4, 21, {2: (1, 0.9 * KM)})
    elif name == "four":       # TOO_FEW: NONE
        b = _batch("north", 4, 3, 22, {})
    elif name == "all_faulted":
        b = _batch("north", 8, 8, 23, {r: ((r * 5) % 8, (30 * KM, -60 * KM, 0.9 * KM)[r % 3]) for r in range(8)})
    elif name == "none_faulted":
        b = _batch("north", 8, 8, 24, {})
    elif name == "two_faults":  # no single exclusion mends two false peaks
        b = _batch("north", 8, 4, 25, {0: [(1, 30 * KM), (6, -60 * KM)], 2: [(0, 3 * KM), (3, 45 * KM)]})
    elif name == "between":    # a false peak and 28 m on another column: the best candidate lies between threshold[d - 2] and [d - 1]
        b = _batch("north", 8, 4, 31, {1: [(2, 30 * KM), (5, 28.0)]})
    elif name == "tie":        # CPU only (an exact tie is no row of RUNNER_UP): eleven satellites, column 5 twice, 50 m on both copies,
        # 1 m of noise.  Without either copy the row is the same list of numbers, so T_5 == T_6 to the bit, and both are the smallest
        geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", list(range(11)), 2, seed=32)
        ob = noisy(obs, 32, 1.0)
        ob = np.concatenate([ob[:, :6], ob[:, 5:]], axis=1)
        for c in (5, 6):
            move(ob, 0, c, 50.0)
            move(ob, 1, c, 50.0)
        b = (geo, ob, prior, raim_ref.params(SIGMA_M))
    elif name == "no_exclusion":  # exclude = 0 on the rows of "three"
        geo, ob, prior, rp = batch("three")
        b = (geo, ob, prior, dict(rp, exclude=0))
    elif name == "own_table":  # a caller's thresholds, ten times the table's: 0.9 km still fails them, noise never does
        geo, ob, prior, rp = batch("south")
        b = (geo, ob, prior, dict(rp, threshold=[10.0 * t + j for j, t in enumerate(rp["threshold"])]))
    else:
        raise KeyError(name)
    b[1].setflags(write=False)
    _batches[name] = b
    return b


BATCHES = ("one", "three", "sixtyseven", "mixed", "south", "rollover", "weights", "narrow", "seven", "six", "five", "four", "all_faulted",
           "none_faulted", "two_faults", "between", "no_exclusion", "own_table")
CPU_ONLY = ("tie",)


def references(name):
    """coarse_raim_ref.coarse_fix_raim of batch(name), computed once and shared"""
    if name not in _refs:
        geo, ob, prior, rp = batch(name)
        _refs[name] = coarse_raim_ref.coarse_fix_raim(geo["ephs"], ob, prior, rp)
    return _refs[name]
