"""Coarse-time fix integrity on the CPU: the C ABI's host side, the reference of the GPU tests (tests/coarse_raim_ref.py, written
from "Coarse-time fix integrity: residual test and one-satellite exclusion" of include/gpsacq.h) on the rows where the text says
what must come out, five plausible wrong laws each told from the right one, and the precondition of every GPU batch.  No device
is needed.  Each test prints what it found before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_raim_cases as cases
import coarse_raim_ref
import coarse_ref
import raim_ref
from coarse_raim_ref import EXCLUDED, FAILED, NONE, PASS, UNCHECKED
from test_coarse import make_case

pytestmark = pytest.mark.usefixtures("hip_artifacts")  # the records' layouts and the host-side checks come from the library


def err(geo, sol):
    return float(np.linalg.norm(sol["xyz"] - geo["rx"]))


# ---- 1. the host side of the C ABI ---------------------------------------------------------------------------------------------
def test_exports_records_and_argument_errors():
    import gpsacq
    from nav_helpers import to_records
    lib = gpsacq.load_library()
    for name in ("gpsacq_coarse_raim_batch", "gpsacq_coarse_raim_batch_device", "gpsacq_coarse_raim_last_ms"):
        assert name in gpsacq.EXPORTS and getattr(lib, name) is not None
    for name in ("coarse_fix_raim", "coarse_fix_raim_device", "coarse_raim_last_ms"):
        assert callable(getattr(gpsacq.Engine, name))
    assert gpsacq.RAIM_PARAMS_DTYPE.itemsize == 88 and gpsacq.FIX_RAIM_DTYPE.itemsize == 40 and gpsacq.COARSE_INFO_DTYPE.itemsize == 40
    rp = gpsacq.raim_params(cases.SIGMA_M)
    assert rp["threshold"][0].tolist() == raim_ref.params(cases.SIGMA_M)["threshold"] and rp["exclude"][0] == 1 and rp["sigma_m"][0] == cases.SIGMA_M
    # without an engine every call is an argument error and writes nothing
    geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case("north", "8", 2, seed=1)
    rec = to_records(geo["ephs"])
    fix, info, raim = np.zeros(2, gpsacq.FIX_DTYPE), np.zeros(2, gpsacq.COARSE_INFO_DTYPE), np.zeros(2, gpsacq.FIX_RAIM_DTYPE)
    out = np.zeros_like(obs)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpsacq_coarse_raim_batch(None, p(rec), 12, p(obs), p(prior), 2, 8, None, p(rp), p(fix), p(info), p(out), p(raim)) == 1
    assert lib.gpsacq_coarse_raim_batch_device(None, p(rec), 12, p(obs), p(prior), 2, 8, None, p(rp), p(fix), p(info), None, p(raim), 1) == 1
    assert lib.gpsacq_coarse_raim_last_ms(None, None, None) == 1
    assert not any(a.view(np.uint8).any() for a in (fix, info, raim, out))


# ---- 2. what the text says must come out -----------------------------------------------------------------------------------------
def test_exact_code_phases_pass():
    for which, name in (("north", "8"), ("south", "up"), ("rollover", "8")):
        geo, sel, ref_ms, t_rx, obs, tx_ms, prior = make_case(which, name, 4, seed=5)
        rp = raim_ref.params(cases.SIGMA_M)
        rows = coarse_raim_ref.coarse_fix_raim(geo["ephs"], obs, prior, rp)
        print(which, "T of exact code phases:", ["%.3g" % r["raim"]["stat_full"] for r in rows])
        for r in rows:
            assert r["raim"] == dict(status=PASS, dof=len(sel) - 5, excluded=-1, n_candidates=0, stat_full=r["raim"]["stat_full"],
                                     stat=r["raim"]["stat_full"], threshold=rp["threshold"][len(sel) - 6])
            assert r["raim"]["stat_full"] < 1e-6 and r["out"] is r["full"]


@pytest.mark.parametrize("which,sats", [("north", 8), ("south", "up")])
def test_the_false_column_is_the_one_excluded(which, sats):
    """eight and nine satellites, one column moved by 0.9 .. 105 km, every column in turn"""
    n_cols = len(cases._sel(which, sats))
    sizes = (0.9e3, 30e3, -3e3, 60e3, -30e3)
    faults = {r: (r % n_cols, 105e3 if r % n_cols == 0 and r >= n_cols else sizes[r % 5]) for r in range(2 * n_cols)}
    geo, ob, prior, rp = cases._batch(which, sats, 2 * n_cols, 61, faults)
    rows = coarse_raim_ref.coarse_fix_raim(geo["ephs"], ob, prior, rp)
    for i, r in enumerate(rows):
        k, ra = faults[i][0], r["raim"]
        runner = sorted(r["candidates"].values())[1]
        print("%s row %d: %.1f km on column %d: FULL %.0f m off (T %.3g), without it %.1f m (T %.3g, runner-up %.3g)" %
              (which, i, faults[i][1] / 1e3, k, err(geo, r["full"]), ra["stat_full"], err(geo, r["out"]), ra["stat"], runner))
        assert ra["status"] == EXCLUDED and ra["excluded"] == k and ra["dof"] == n_cols - 6 and ra["n_candidates"] == n_cols
        assert ra["stat"] <= ra["threshold"] == rp["threshold"][n_cols - 7] and ra["stat_full"] > rp["threshold"][n_cols - 6] and runner > 1.05 * ra["threshold"]
        assert err(geo, r["full"]) > 250.0 and err(geo, r["out"]) < 150.0  # 10 m of noise at pdop ~2; the fault moved FULL by hundreds of metres
        # the output IS the coarse-time fix of the row without the column: `valid` cleared, everything from the prior again
        cut = ob[i:i + 1].copy()
        cut["valid"][0, k] = 0
        want = coarse_ref.coarse_fix(geo["ephs"], cut, prior[i:i + 1])[0]
        got = r["out"]
        assert got["iterations"] == want["iterations"] + r["full"]["iterations"] and got["n_used"] == n_cols - 1
        assert got["ref"] == want["ref"] == (1 if k == 0 else 0) and k not in got["obs_out"] and got["flags"] == 0
        # (to rounding: nav_ref iterates Kepler's equation for a whole batch at once, so a row's bits depend on its neighbours)
        for key, tol in (("rms", 1e-6), ("coarse_s", 1e-9), ("bias_m", 1e-2), ("pdop", 1e-9), ("cdop", 1e-9), ("rx_frac", 1e-9)):
            assert abs(got[key] - want[key]) <= tol, key
        assert np.abs(got["xyz"] - want["xyz"]).max() <= 1e-6 and (got["N"] == want["N"]).all() and got["rx_ms"] == want["rx_ms"]
        assert sorted(got["obs_out"]) == sorted(want["obs_out"])


def test_seven_six_and_five_satellites():
    rp = cases.batch("seven")[3]
    seven, six, five, four = (cases.references(n) for n in ("seven", "six", "five", "four"))
    # seven: d = 2, the exclusion runs, and a candidate has one degree of freedom
    assert all(r["n_w"] == 7 for r in seven)
    assert [r["raim"]["status"] for r in seven] == [EXCLUDED, PASS, EXCLUDED, EXCLUDED, PASS, EXCLUDED, PASS, EXCLUDED]
    assert all(r["raim"]["dof"] == (1 if r["raim"]["status"] == EXCLUDED else 2) for r in seven)
    assert all(r["raim"]["threshold"] == rp["threshold"][0] and r["raim"]["n_candidates"] == 7 for r in seven if r["raim"]["status"] == EXCLUDED)
    geo = cases.batch("seven")[0]
    print("seven satellites, excluded / planted:", [(r["raim"]["excluded"], round(err(geo, r["out"]))) for r in seven])
    assert [r["raim"]["excluded"] for r in seven][2:] == [2, 6, -1, 1, -1, 4]  # the large faults are found; row 0's 900 m: inherent to one degree of freedom
    # six: d = 1, FAILED with no candidate tried
    assert [r["raim"]["status"] for r in six] == [PASS, FAILED, FAILED, PASS, FAILED, PASS]
    assert all(r["raim"]["dof"] == 1 and r["raim"]["n_candidates"] == 0 and not r["cand"] and r["out"] is r["full"] for r in six)
    assert all(r["raim"]["threshold"] == rp["threshold"][0] for r in six)
    # five: UNCHECKED, whatever the code phases
    assert all(r["raim"]["status"] == UNCHECKED and r["raim"]["dof"] == 0 and r["raim"]["threshold"] == 0.0 and not r["cand"] for r in five)
    assert err(cases.batch("five")[0], five[2]["out"]) > 1000.0
    # four: no fix to judge
    assert all(r["raim"] == dict(status=NONE, dof=0, excluded=-1, n_candidates=0, stat_full=0.0, stat=0.0, threshold=0.0) for r in four)


def test_weight_zero_two_faults_and_no_exclusion():
    geo, ob, prior, rp = cases.batch("sixtyseven")
    rows = cases.references("sixtyseven")
    # row 9: 60 km on a weight-0 observation -- it adds nothing, does not count and is no candidate
    assert ob["weight"][9, 3] == 0.0 and rows[9]["raim"]["status"] == PASS and rows[9]["n_w"] == 11 and rows[9]["raim"]["dof"] == 6
    assert err(geo, rows[9]["out"]) < 100.0
    w1 = ob[9:10].copy()
    w1["weight"][0, 3] = 1.0
    assert coarse_raim_ref.coarse_fix_raim(geo["ephs"], w1, prior[9:10], rp)[0]["raim"]["excluded"] == 3
    # row 5: a hole next to the fault; row 20: an invalid first column, and the fault on the reference; rows 13, 14: too few
    assert rows[5]["raim"]["excluded"] == 2 and rows[5]["raim"]["n_candidates"] == 11 and rows[5]["raim"]["dof"] == 5
    assert rows[20]["full"]["ref"] == 1 and rows[20]["raim"]["excluded"] == 1 and rows[20]["out"]["ref"] == 2
    assert rows[13]["raim"]["status"] == NONE and rows[14]["raim"]["status"] == NONE and rows[14]["full"]["ref"] == -1
    # two false peaks: no single exclusion mends the row
    two = cases.references("two_faults")
    assert [r["raim"]["status"] for r in two] == [FAILED, PASS, FAILED, PASS]
    assert all(r["raim"]["n_candidates"] == 8 and r["raim"]["dof"] == 3 and r["out"] is r["full"] for r in (two[0], two[2]))
    assert min(min(r["candidates"].values()) for r in (two[0], two[2])) > 30.0
    # exclude = 0: the same rows as "three", FAILED where that batch excludes
    off, on = cases.references("no_exclusion"), cases.references("three")
    assert [r["raim"]["status"] for r in on] == [PASS, EXCLUDED, EXCLUDED] and [r["raim"]["status"] for r in off] == [PASS, FAILED, FAILED]
    assert all(not r["cand"] and r["raim"]["n_candidates"] == 0 and r["raim"]["stat"] == r["raim"]["stat_full"] for r in off)
    assert [r["raim"]["stat_full"] for r in off] == [r["raim"]["stat_full"] for r in on]


# ---- 3. five wrong laws ----------------------------------------------------------------------------------------------------------
def told_apart(a, b):
    """the raim records of two evaluations differ by more than two fp64 implementations of ONE law can: in status, dof, excluded or
    n_candidates, or by 1 % in a statistic"""
    ra, rb = a["raim"], b["raim"]
    if any(ra[k] != rb[k] for k in ("status", "dof", "excluded", "n_candidates")):
        return True
    return any(abs(ra[k] - rb[k]) > 0.01 * abs(ra[k]) for k in ("stat_full", "stat", "threshold"))


@pytest.mark.parametrize("law,name,row", [("keep_ms", "narrow", 1), ("count_w", "weights", 0), ("dof4", "six", 1), ("same_thr", "between", 1),
                                          ("tie_high", "tie", 0)])
def test_wrong_laws_are_told_apart(law, name, row):
    geo, ob, prior, rp = cases.batch(name)
    right = cases.references(name)
    wrong = coarse_raim_ref.coarse_fix_raim(geo["ephs"], ob, prior, rp, law=law)
    a, b = right[row]["raim"], wrong[row]["raim"]
    print("%s on row %d of %r:\n  right %s\n  wrong %s" % (law, row, name, a, b))
    assert told_apart(right[row], wrong[row])
    if law == "keep_ms":    # 0.48 ms on the reference column: FULL's whole milliseconds are mixed, and only step A done again mends the row
        assert right[row]["full"]["margin"] < 0.02 and a["status"] == EXCLUDED and a["excluded"] == 0 and b["status"] == FAILED
        assert right[row]["cand"][0]["margin"] >= 0.2 and err(geo, right[row]["out"]) < 150.0 < 5e4 < err(geo, right[row]["full"])
        assert (right[row]["cand"][0]["N"][1:] - right[row]["full"]["N"][1:]).std() > 0  # not one common integer
    elif law == "count_w":  # weights 0.25 .. 4: W is not n_w
        assert a["status"] == b["status"] == EXCLUDED and abs(b["stat"] / a["stat"] - 1) > 0.05
    elif law == "dof4":     # six satellites: one degree of freedom and no candidate -- not two, and six candidates of zero residual
        assert (a["status"], a["dof"], a["n_candidates"]) == (FAILED, 1, 0)
        assert (b["status"], b["n_candidates"]) == (EXCLUDED, 6) and b["stat"] < 1e-6
    elif law == "same_thr":  # the best candidate lies between threshold[d - 2] and threshold[d - 1]
        best = min(right[row]["candidates"].values())
        assert rp["threshold"][1] * 1.05 < best < rp["threshold"][2] * 0.95 and a["status"] == FAILED and b["status"] == EXCLUDED
    elif law == "tie_high":  # columns 5 and 6 are one observation twice
        T = right[row]["candidates"]
        assert ob[row, 5] == ob[row, 6] and T[5] == T[6] == min(T.values()) and (a["excluded"], b["excluded"]) == (5, 6)
        assert a["status"] == b["status"] == EXCLUDED
    # and the right law is not told from itself
    again = coarse_raim_ref.coarse_fix_raim(geo["ephs"], ob, prior, rp)
    assert not any(told_apart(x, y) for x, y in zip(right, again))


# ---- 4. the GPU batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.BATCHES)
def test_gpu_batches_meet_their_precondition(name):
    geo, ob, prior, rp = cases.batch(name)
    rows = cases.references(name)
    why = [(i, cases.precondition(r, rp)) for i, r in enumerate(rows) if cases.precondition(r, rp)]
    n_narrow = sum(cases.narrow(r) for r in rows)
    st = np.bincount([r["raim"]["status"] for r in rows], minlength=5)
    print("%s: %d rows x %d, NONE %d UNCHECKED %d PASS %d EXCLUDED %d FAILED %d, narrow %d" % ((name, len(rows), ob.shape[1]) + tuple(st) + (n_narrow,)))
    assert not why and 8 * n_narrow <= len(rows)


def test_gpu_batches_cover_the_issue():
    """what tests/test_gpu_coarse_raim.py is meant to meet is in the batches: every status, the reference column both ways, the last
    column, ref != 0, a narrow row, a weight-0 fault"""
    refs = {n: cases.references(n) for n in cases.BATCHES}
    seen = {r["raim"]["status"] for rows in refs.values() for r in rows}
    assert seen == {NONE, UNCHECKED, PASS, EXCLUDED, FAILED}
    assert {len(refs[n]) for n in ("one", "three", "sixtyseven", "mixed")} == {1, 3, 67, 130}
    assert {cases.batch(n)[1].shape[1] for n in cases.BATCHES} >= {12, 9, 8, 7, 6, 5, 4}
    south, mixed = refs["south"], refs["mixed"]
    assert south[0]["raim"]["excluded"] == 0 and not cases.narrow(south[0]) and south[6]["raim"]["excluded"] == 0  # 0.35 ms and 900 m on the reference
    assert mixed[64]["raim"]["excluded"] == 0 and mixed[65]["raim"]["excluded"] == 0 and mixed[129]["raim"]["excluded"] == 7
    assert cases.narrow(refs["narrow"][1]) and refs["narrow"][1]["raim"]["status"] == EXCLUDED
    assert all(r["raim"]["status"] == EXCLUDED for r in refs["all_faulted"]) and all(r["raim"]["status"] == PASS for r in refs["none_faulted"])
    own, table = refs["own_table"], refs["south"]
    assert [r["raim"]["status"] for r in own] == [r["raim"]["status"] for r in table] and own[0]["raim"]["threshold"] != table[0]["raim"]["threshold"]
