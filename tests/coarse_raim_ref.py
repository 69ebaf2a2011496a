"""Reference of the coarse-time integrity tests: "Coarse-time fix integrity: residual test and one-satellite exclusion" of
include/gpsacq.h, written from that text on top of tests/coarse_ref.py.  FULL is coarse_ref.coarse_fix of the batch; a candidate
is literally the row with `valid` of one column cleared, given to coarse_ref.coarse_fix again -- from the prior, step A included.
All candidates of a batch go through ONE call (coarse_ref evaluates an ephemeris at many times at once).

`law` swaps one rule of the text for a plausible wrong one, so that tests/test_coarse_raim.py can show that its rows tell the
two apart:
    "keep_ms"    the candidates keep FULL's whole milliseconds (and only move the reference column on)
    "count_w"    T from the rms taken as unweighted: rms^2 n_w / sigma^2 in place of rms^2 W / sigma^2, and n_w - 1 for W - w_k
    "dof4"       d = n_w - 4, the four-state count
    "same_thr"   the candidates are held to threshold[d - 1]
    "tie_high"   on a tie the highest k wins
"""
import numpy as np

import coarse_ref

NONE, UNCHECKED, PASS, EXCLUDED, FAILED = 0, 1, 2, 3, 4
LAWS = ("keep_ms", "count_w", "dof4", "same_thr", "tie_high")


def _prior_ok(prior):
    ok = (prior["rx_ms"] >= 0) & (prior["rx_ms"] < coarse_ref.WEEK_MS)
    return ok & np.isfinite(prior["x"]) & np.isfinite(prior["y"]) & np.isfinite(prior["z"])


def _fix(ephs, obs, prior, rms_max_m, keep_N=None):
    """coarse_ref.coarse_fix; keep_N (n, m): the wrong law "keep_ms", step A's integers replaced by these"""
    if keep_N is None:
        return coarse_ref.coarse_fix(ephs, obs, prior, rms_max_m)
    step_a = coarse_ref.whole_ms

    def kept(ephs_, eph_index, use, tx_frac, prior_xyz, rx_ms):
        ref, _, margin = step_a(ephs_, eph_index, use, tx_frac, prior_xyz, rx_ms)
        return ref, np.where(use, keep_N, 0).astype(np.int64), margin
    coarse_ref.whole_ms = kept
    try:
        return coarse_ref.coarse_fix(ephs, obs, prior, rms_max_m)
    finally:
        coarse_ref.whole_ms = step_a


def coarse_fix_raim(ephs, obs, prior, rp, rms_max_m=coarse_ref.RMS_MAX_M, law=None):
    """obs [n_fix][sats] OBS_DTYPE, prior [n_fix] COARSE_PRIOR_DTYPE, rp = raim_ref.params(...) (sigma_m, threshold, exclude).
    One dict per row: out (coarse_ref's dict of the solution that is output: FULL's, or the winner's with FULL's iterations
    added), full (FULL's dict), raim (status, dof, excluded, n_candidates, stat_full, stat, threshold), W, n_w, candidates ({k: T_k}
    of the candidates that were FIX_OK) and cand ({k: coarse_ref's dict} of every candidate tried).
    A row whose prior names no place or instant (the _device form's NaN prior) has nothing usable."""
    assert law is None or law in LAWS
    n, m = obs.shape
    ok = _prior_ok(prior)
    obs, prior = obs.copy(), prior.copy()
    obs["valid"][~ok] = 0
    for name in "xyz":
        prior[name][~ok] = 0.0
    prior["rx_ms"][~ok] = 0
    full = _fix(ephs, obs, prior, rms_max_m)
    weight = obs["weight"].astype(np.float64)
    use = coarse_ref.usable(obs["eph"].astype(np.int64), obs["valid"], obs["tx_frac"].astype(np.float64), weight, len(ephs))
    sigma2, thr = float(rp["sigma_m"]) ** 2, [float(t) for t in rp["threshold"]]
    rows, todo = [], []
    for i in range(n):
        raim = dict(status=NONE, dof=0, excluded=-1, n_candidates=0, stat_full=0.0, stat=0.0, threshold=0.0)
        row = dict(out=full[i], full=full[i], raim=raim, W=0.0, n_w=0, candidates={}, cand={})
        rows.append(row)
        if full[i]["status"] != coarse_ref.FIX_OK:
            continue
        W = 0.0
        for k in np.nonzero(use[i])[0]:  # in column order, as the text's sum reads
            W += weight[i, k]
        n_w = int((use[i] & (weight[i] > 0)).sum())
        d = n_w - (4 if law == "dof4" else 5)
        T = full[i]["rms"] ** 2 * (n_w if law == "count_w" else W) / sigma2
        row.update(W=W, n_w=n_w)
        raim.update(dof=d, stat_full=T, stat=T)
        if d < 1:
            raim["status"] = UNCHECKED
            continue
        raim["threshold"] = thr[d - 1]
        if T <= thr[d - 1]:
            raim["status"] = PASS
            continue
        raim["status"] = FAILED
        if rp["exclude"] and d >= 2:
            todo += [(i, int(k)) for k in np.nonzero(use[i] & (weight[i] > 0))[0]]
    if todo:
        ii = np.array([i for i, _ in todo])
        c_obs = obs[ii].copy()
        c_obs["valid"][np.arange(len(todo)), [k for _, k in todo]] = 0
        keep = np.stack([full[i]["N"] for i in ii]) if law == "keep_ms" else None
        cand = _fix(ephs, c_obs, prior[ii], rms_max_m, keep)
        for (i, k), c in zip(todo, cand):
            rows[i]["cand"][k] = c
            if c["status"] == coarse_ref.FIX_OK:
                rest = rows[i]["n_w"] - 1 if law == "count_w" else rows[i]["W"] - weight[i, k]
                rows[i]["candidates"][k] = c["rms"] ** 2 * rest / sigma2
    for i in sorted({i for i, _ in todo}):
        row, raim = rows[i], rows[i]["raim"]
        d, T_k = raim["dof"], row["candidates"]
        raim["n_candidates"] = len(T_k)
        if not T_k:
            continue
        best = min(T_k.values())
        k = (max if law == "tie_high" else min)(k for k in T_k if T_k[k] == best)
        limit = thr[d - 1] if law == "same_thr" else thr[d - 2]
        if not best <= limit:
            continue
        win = dict(row["cand"][k])
        win["iterations"] += row["full"]["iterations"]
        row["out"] = win
        raim.update(status=EXCLUDED, dof=d - 1, excluded=k, stat=best, threshold=thr[d - 2])
    return rows
