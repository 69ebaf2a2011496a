"""Fix integrity on the GPU (gpsacq_fix_raim_batch*) against tests/raim_ref.py, which tests/test_raim.py checks on its own, and
against the parent's own code (Engine.fix_atm on the row without the excluded observation).

Tolerances, derived and not measured.  Position 1e-4 m and receive time 1e-12 s: tests/test_gpu_atm.py's, by its derivation; DOP
1e-9 relative, likewise.  stat and stat_full: 1e-6 relative + 1e-9 absolute -- T is a sum of at most twelve squares of residuals
that both sides know to ~1e-8 m (the converged states differ by that much), over sigma^2 = 9 m^2: a residual of r metres moves
T by 2 r 1e-8 / 9, which is 2e-9 / r of T itself, and exact observations give T ~ 1e-16, hence the absolute term.  The integers
(status, dof, excluded, n_candidates, used_mask, n_used, n_masked) are equal.  `iterations` may differ by one per stage run, as
in tests/test_gpu_atm.py; FULL, the winning candidate and FINAL's rounds are stage runs.

Before any GPU result is looked at, every row's reference is asserted to stand clear of its decisions (raim_cases.precondition):
stat_full and the winning T_k 5 % from their thresholds, the runner-up 1.05 times the winner, 1 degree between every elevation
and the mask.  No row is left out of a comparison.  The batches are raim_cases.batch's; the satellites 9 and 10 of the twelve stand
below the horizon, so the 5-degree mask leaves ten and dof is 6.
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest

import nav_ref
import raim_cases
import raim_ref
from nav_helpers import to_records

pytestmark = pytest.mark.gpu

POS_TOL, TIME_TOL, DOP_RTOL = 1e-4, 1e-12, 1e-9
STAT_RTOL, STAT_ATOL = 1e-6, 1e-9
DOPS = ("gdop", "pdop", "hdop", "vdop", "tdop")


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as e:
        yield e


def gpu_atm(p):
    import gpsacq
    out = np.zeros(1, gpsacq.ATM_PARAMS_DTYPE)
    out["alpha"][0], out["beta"][0], out["elev_mask"], out["flags"] = p["alpha"], p["beta"], p["elev_mask"], p["flags"]
    return out


def gpu_raim(rp):
    """the reference's own thresholds, so that the two sides compare with the same numbers (the library's table is pinned to
    them to 1e-12 in tests/test_raim.py)"""
    import gpsacq
    out = np.zeros(1, gpsacq.RAIM_PARAMS_DTYPE)
    out["sigma_m"], out["p_fa"], out["threshold"][0], out["exclude"] = rp["sigma_m"], 1e-3, rp["threshold"], rp["exclude"]
    return out


def _xyz(fix):
    return np.stack([fix["x"], fix["y"], fix["z"]], -1)


def _assert_preconditions(name):
    geo, ob, p, rp = raim_cases.batch(name)
    refs = raim_cases.references(name)
    for k, ref in enumerate(refs):
        why = raim_cases.precondition(ref, p, rp)
        assert why is None, (name, k, why)
    return geo, ob, p, rp, refs


def _compare_row(label, ref, fix, dop, raim):
    """one row of the GPU's three records against the reference; returns (position, time, DOP relative, stat excess over its
    tolerance as a ratio)"""
    r = ref["raim"]
    got = tuple(int(raim[n]) for n in ("status", "dof", "excluded", "n_candidates"))
    assert got == (r["status"], r["dof"], ref["excluded"], r["n_candidates"]), (label, got, r)
    assert (int(fix["status"]), int(fix["n_used"]), int(dop["used_mask"]), int(dop["n_masked"])) == \
        (ref["status"], ref["n_used"], ref["used_mask"], ref["n_masked"]), (label, fix, dop)
    assert abs(int(fix["iterations"]) - ref["iterations"]) <= max(len(ref["stages"]), 1), (label, fix["iterations"], ref["stages"])
    if ref["status"] != 0:
        for n in ("rx_frac", "x", "y", "z", "lat", "lon", "alt", "rms"):
            assert fix[n] == 0.0, (label, n)
        assert fix["rx_ms"] == 0 and not any(dop[n] for n in DOPS)
        assert raim["stat"] == 0 and raim["stat_full"] == 0 and raim["threshold"] == 0
        return 0.0, 0.0, 0.0, 0.0
    dpos = float(np.abs(_xyz(fix) - ref["xyz"]).max())
    dt = abs(float(nav_ref.fold_ms(int(fix["rx_ms"]) - ref["rx_ms"])) * 1e-3 + (float(fix["rx_frac"]) - ref["rx_frac"]))
    ddop = float(np.abs(np.array([dop[n] for n in DOPS]) / np.array(ref["dop"]) - 1).max())
    dstat = max(abs(float(raim[n]) - r[n]) / (STAT_RTOL * abs(r[n]) + STAT_ATOL) for n in ("stat", "stat_full"))
    assert raim["threshold"] == r["threshold"], (label, raim["threshold"], r["threshold"])
    assert abs(float(fix["rms"]) - ref["rms"]) <= POS_TOL, (label, fix["rms"], ref["rms"])
    for n in ("lat", "lon"):
        assert abs(float(fix[n]) - ref["lla"][("lat", "lon").index(n)]) <= 1e-9
    assert abs(float(fix["alt"]) - ref["lla"][2]) <= 2 * POS_TOL
    return dpos, dt, ddop, dstat


def _compare(name, refs, fix, dop, raim):
    worst = np.zeros(4)
    for k, ref in enumerate(refs):
        worst = np.maximum(worst, _compare_row((name, k), ref, fix[k], dop[k], raim[k]))
    counts = {s: int((raim["status"] == s).sum()) for s in range(5) if (raim["status"] == s).any()}
    print("%s (%d rows, statuses %s): position %.3g m, receive time %.3g s, DOP %.3g relative, statistic %.3g of its tolerance" %
          ((name, len(refs), counts) + tuple(worst)))
    assert worst[0] <= POS_TOL and worst[1] <= TIME_TOL and worst[2] <= DOP_RTOL and worst[3] <= 1.0
    for rec in (fix, dop, raim):
        for n in rec.dtype.names:
            assert np.isfinite(rec[n].astype(np.float64)).all(), n


# ---- 1. parity with the reference, every shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", raim_cases.BATCHES)
def test_against_reference(eng, name):
    import gpsacq
    geo, ob, p, rp, refs = _assert_preconditions(name)
    fix, dop, raim = eng.fix_raim(to_records(geo["ephs"]), ob, gpu_atm(p), gpu_raim(rp))
    _compare(name, refs, fix, dop, raim)
    st = raim["status"]
    if name == "sixtyseven":
        assert len(ob) % 4 and len(ob) % 64 and {0, 2, 3} <= set(st)
        assert st[9] == gpsacq.RAIM_PASS and raim["dof"][9] == 5 and dop["used_mask"][9] >> 3 & 1  # weight 0: used, not counted
        assert st[13] == gpsacq.RAIM_NONE and st[14] == gpsacq.RAIM_NONE and fix["status"][13] == gpsacq.FIX_TOO_FEW
        assert (raim["excluded"][64], raim["excluded"][66], raim["excluded"][5]) == (0, 11, 2)
    elif name == "mixed":
        flips = int((np.diff((st == gpsacq.RAIM_EXCLUDED).astype(int)) != 0).sum())
        assert flips > 40 and (st == gpsacq.RAIM_PASS).sum() > 40 and (st == gpsacq.RAIM_EXCLUDED).sum() > 40
    elif name in ("plain", "plain_masked"):
        assert (dop["n_masked"] == (0 if name == "plain" else 2)).all() and (st == gpsacq.RAIM_EXCLUDED).any()
        # FINAL without rounds where nothing was masked: FULL's one stage run and the candidate's, nothing else
        runs = {len(r["stages"]) for r in refs if r["raim"]["status"] == raim_ref.EXCLUDED}
        assert runs == ({2} if name == "plain" else {4 + 1 + 3})
    elif name == "five":
        assert list(st) == [2, 4, 4, 2, 4, 2] and (raim["dof"] == 1).all() and (raim["n_candidates"] == 0).all()
    elif name == "four":
        assert (st == gpsacq.RAIM_UNCHECKED).all() and (raim["dof"] == 0).all() and (raim["threshold"] == 0).all()
    elif name == "six":
        assert (raim["dof"][st == gpsacq.RAIM_EXCLUDED] == 1).all() and (st == gpsacq.RAIM_EXCLUDED).any()
    elif name == "all_faulted":
        assert (st == gpsacq.RAIM_EXCLUDED).all() and (raim["n_candidates"] == 10).all()
    elif name == "none_faulted":
        assert (st == gpsacq.RAIM_PASS).all() and (raim["stat"] == raim["stat_full"]).all()
    elif name == "no_exclusion":
        assert list(st) == [2, 4, 4] and (raim["n_candidates"] == 0).all() and (raim["excluded"] == -1).all()
    elif name == "three":
        assert list(st) == [2, 3, 3] and list(raim["excluded"]) == [-1, 0, 11]


# ---- 2. against the parent's own code -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sixtyseven", "mixed", "plain", "weights", "six", "five", "four"])
def test_against_fix_atm(eng, name):
    import gpsacq
    geo, ob, p, rp, refs = _assert_preconditions(name)
    rec, ap = to_records(geo["ephs"]), gpu_atm(p)
    fix, dop, raim = eng.fix_raim(rec, ob, ap, gpu_raim(rp))
    st = raim["status"]
    without = ob.copy()
    ex = np.flatnonzero(st == gpsacq.RAIM_EXCLUDED)
    without["valid"][ex, raim["excluded"][ex]] = 0
    afix, adop = eng.fix_atm(rec, without, ap)
    ok = afix["status"] == 0
    assert (fix["status"] == afix["status"]).all() and (fix["n_used"] == afix["n_used"]).all()
    assert (dop["used_mask"] == adop["used_mask"]).all() and (dop["n_masked"] == adop["n_masked"]).all()
    dpos = np.abs(_xyz(fix) - _xyz(afix))[ok].max() if ok.any() else 0.0
    dt = np.abs(nav_ref.fold_ms(fix["rx_ms"].astype(np.int64) - afix["rx_ms"]) * 1e-3 + (fix["rx_frac"] - afix["rx_frac"]))[ok].max() if ok.any() else 0.0
    ddop = max(np.abs(dop[n][ok] / adop[n][ok] - 1).max() for n in DOPS) if ok.any() else 0.0
    print("%s: %d excluded rows of %d; %.3g m, %.3g s, DOP %.3g relative from Engine.fix_atm" % (name, len(ex), len(ob), dpos, dt, ddop))
    assert dpos <= POS_TOL and dt <= TIME_TOL and ddop <= DOP_RTOL
    same = np.flatnonzero(st != gpsacq.RAIM_EXCLUDED)  # nothing excluded: the same four stage runs at most
    assert (np.abs(fix["iterations"][same] - afix["iterations"][same]) <= 4).all()


# ---- 3. the library's own table -----------------------------------------------------------------------------------------------
def test_default_params_give_the_same_decisions(eng):
    import gpsacq
    geo, ob, p, rp, refs = _assert_preconditions("sixtyseven")
    rec = to_records(geo["ephs"])
    a = eng.fix_raim(rec, ob, gpu_atm(p), gpu_raim(rp))
    b = eng.fix_raim(rec, ob, gpu_atm(p), gpsacq.raim_params(raim_cases.SIGMA_M))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for n in ("status", "dof", "excluded", "n_candidates", "stat", "stat_full"):
        assert (a[2][n] == b[2][n]).all(), n
    assert np.abs(a[2]["threshold"] - b[2]["threshold"]).max() <= 1e-11
    # thresholds of the caller's own: with huge ones everything passes, with tiny ones nothing does and nothing can be mended
    big, small = gpu_raim(rp), gpu_raim(rp)
    big["threshold"][0], small["threshold"][0] = 1e9, 1e-9
    okrows = a[0]["status"] == 0
    assert (eng.fix_raim(rec, ob, gpu_atm(p), big)[2]["status"][okrows] == gpsacq.RAIM_PASS).all()
    f, d, r = eng.fix_raim(rec, ob, gpu_atm(p), small)
    assert (r["status"][okrows] == gpsacq.RAIM_FAILED).all() and (r["excluded"] == -1).all() and (r["n_candidates"][okrows] >= 9).all()
    plain_f, plain_d = eng.fix_atm(rec, ob, gpu_atm(p))
    assert np.abs(_xyz(f) - _xyz(plain_f)).max() <= POS_TOL and (d["used_mask"] == plain_d["used_mask"]).all()


# ---- 4. device form ---------------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form(eng):
    import gpsacq
    import torch
    geo, ob, p, rp, refs = _assert_preconditions("mixed")
    rec, ap, gp = to_records(geo["ephs"]), gpu_atm(p), gpu_raim(rp)
    n = len(ob)
    fix, dop, raim = eng.fix_raim(rec, ob, ap, gp)
    buf = lambda m: torch.full((m,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_obs = torch.from_numpy(ob.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_fix, d_dop, d_raim = buf(n * 80), buf(n * 48), buf(n * 40)
    torch.cuda.synchronize()
    eng.fix_raim_device(rec, d_obs.data_ptr(), n, 12, ap, gp, d_fix.data_ptr(), d_dop.data_ptr(), d_raim.data_ptr(), sync=True)
    t = eng.fix_raim_last_ms()
    print("n_fix %d: sat_state %.4f ms, detect %.4f ms, exclude %.4f ms" % ((n,) + t))
    assert len(t) == 3 and all(math.isfinite(x) for x in t) and t[0] >= 0 and t[1] > 0 and t[2] > 0  # the exclude kernel always runs
    assert d_fix.cpu().numpy().tobytes() == fix.tobytes() and d_dop.cpu().numpy().tobytes() == dop.tobytes()
    assert d_raim.cpu().numpy().tobytes() == raim.tobytes()
    # NULL dop in the device form
    d_fix2, d_raim2 = buf(n * 80), buf(n * 40)
    torch.cuda.synchronize()
    eng.fix_raim_device(rec, d_obs.data_ptr(), n, 12, ap, gp, d_fix2.data_ptr(), None, d_raim2.data_ptr(), sync=True)
    assert d_fix2.cpu().numpy().tobytes() == fix.tobytes() and d_raim2.cpu().numpy().tobytes() == raim.tobytes()
    # the device form cannot read the weights: a NaN or negative weight is an observation skipped, in a passing and an excluding row
    st = raim["status"]
    rows = [int(np.flatnonzero(st == gpsacq.RAIM_PASS)[0]), int(np.flatnonzero(st == gpsacq.RAIM_EXCLUDED)[0])]
    ob2 = ob.copy()
    for r, w in zip(rows, (float("nan"), -1.0)):
        col = 0 if raim["excluded"][r] != 0 else 1
        ob2["weight"][r, col] = w
    d_obs2 = torch.from_numpy(ob2.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.fix_raim_device(rec, d_obs2.data_ptr(), n, 12, ap, gp, d_fix2.data_ptr(), d_dop.data_ptr(), d_raim2.data_ptr(), sync=True)
    f2 = d_fix2.cpu().numpy().view(gpsacq.FIX_DTYPE)
    p2 = d_dop.cpu().numpy().view(gpsacq.FIX_DOP_DTYPE)
    r2 = d_raim2.cpu().numpy().view(gpsacq.FIX_RAIM_DTYPE)
    for r in rows:
        ref = raim_cases.reference(geo, ob2[r], p, rp)
        assert raim_cases.precondition(ref, p, rp) is None and ref["full"]["n_used"] == 9
        _compare_row(("skipped weight", r), ref, f2[r], p2[r], r2[r])
    others = [k for k in range(n) if k not in rows]
    assert f2[others].tobytes() == fix[others].tobytes() and r2[others].tobytes() == raim[others].tobytes()


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    import gpsacq
    import torch
    geo, ob, p, rp = raim_cases.batch("three")
    rec, ap, gp = to_records(geo["ephs"]), gpu_atm(p), gpu_raim(rp)
    ob = ob.copy()
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)
    poisoned = lambda dt: np.frombuffer(bytes([0xA5]) * (3 * dt.itemsize), dt).copy()
    fix, dop, raim = poisoned(gpsacq.FIX_DTYPE), poisoned(gpsacq.FIX_DOP_DTYPE), poisoned(gpsacq.FIX_RAIM_DTYPE)
    before = fix.tobytes() + dop.tobytes() + raim.tobytes()
    d_obs = torch.from_numpy(ob.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_out = [torch.full((3 * m,), 0xA5, dtype=torch.uint8, device="cuda:0") for m in (80, 48, 40)]
    torch.cuda.synchronize()

    def host(e=h, eph=rec, n_eph=12, o=ob, n=3, sats=12, a=ap, r=gp, f=fix, d=dop, m=raim):
        q = lambda x: None if x is None else ptr(x)
        return lib.gpsacq_fix_raim_batch(e, q(eph), n_eph, q(o), n, sats, q(a), q(r), q(f), q(d), q(m))

    def device(e=h, eph=rec, n_eph=12, o=d_obs.data_ptr(), n=3, sats=12, a=ap, r=gp, f=d_out[0].data_ptr(), d=d_out[1].data_ptr(), m=d_out[2].data_ptr()):
        q = lambda x: None if x is None else ptr(x)
        return lib.gpsacq_fix_raim_batch_device(e, q(eph), n_eph, o, n, sats, q(a), q(r), f, d, m, 1)

    for call in (host, device):
        assert call(a=None) == 1 and b"params" in lib.gpsacq_last_error()
        assert call(r=None) == 1 and b"params" in lib.gpsacq_last_error()
        assert call(e=None) == 1 and call(eph=None) == 1 and call(o=None) == 1 and call(f=None) == 1 and call(m=None) == 1
        assert call(n=0) == 1 and call(n_eph=0) == 1
        for sats in (0, 13, -1):
            assert call(sats=sats) == 1 and b"sats_per_fix" in lib.gpsacq_last_error()
        for name, value in (("sigma_m", 0.0), ("sigma_m", -3.0), ("sigma_m", float("nan")), ("sigma_m", float("inf")), ("exclude", 2),
                            ("exclude", -1)):
            bad = gp.copy()
            bad[name] = value
            assert call(r=bad) == 1, (name, value)
        for j in range(8):
            for value in (0.0, -1.0, float("nan"), float("inf")):
                bad = gp.copy()
                bad["threshold"][0, j] = value
                assert call(r=bad) == 1 and b"threshold" in lib.gpsacq_last_error(), (j, value)
        bad = ap.copy()
        bad["flags"] = 4
        assert call(a=bad) == 1
        bad = ap.copy()
        bad["elev_mask"] = math.pi / 2
        assert call(a=bad) == 1
    for bad_w in (float("nan"), -1.0, float("inf")):  # a bad weight in the host form
        b = ob.copy()
        b["weight"][1, 5] = bad_w
        assert host(o=b) == 1 and b"weight" in lib.gpsacq_last_error()
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.fix_raim(rec, b, ap, gp)
        assert ei.value.code == 1 and "weight" in str(ei.value)
    with pytest.raises(gpsacq.GpsAcqError):
        eng.fix_raim(rec, ob, ap, None)
    with pytest.raises(gpsacq.GpsAcqError):
        eng.fix_raim(rec, ob, None, gp)
    # nothing was launched, nothing written
    torch.cuda.synchronize()
    assert fix.tobytes() + dop.tobytes() + raim.tobytes() == before
    for t in d_out:
        assert (t.cpu().numpy() == 0xA5).all()
    assert host(d=None) == 0 and raim["status"].tolist() == [2, 3, 3]  # dop may be NULL; and the good call does write
    fresh = gpsacq.Engine(4.092e6, 5.456e6, 5000.0)
    try:
        with pytest.raises(gpsacq.GpsAcqError):
            fresh.fix_raim_last_ms()  # no call made on this engine
    finally:
        fresh.close()


# ---- 6. rank-deficient rows beside regular ones: lanes part ways at the Cholesky pivot ------------------------------------------------
N_DEFICIENT = 2 * 64 + 1  # two whole blocks of k_raim_detect and a row


def _pivot_ratios(A):
    """Cholesky's pivots over their diagonal entries, up to and with the first that is not positive"""
    n, L, out = len(A), np.zeros(A.shape), []
    for j in range(n):
        pv = A[j, j] - (L[j, :j] ** 2).sum()
        out.append(pv / A[j, j])
        if not pv > 0:
            break
        L[j, j] = math.sqrt(pv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return out


def _normal(xyz, t, w, pos, t_rx):
    import atm_ref
    d = pos - atm_ref.turned(xyz, t, t_rx)
    H = np.concatenate([d / np.sqrt((d * d).sum(1))[:, None], np.ones((len(d), 1))], 1)
    return H.T @ (w[:, None] * H)


def _regular(A):
    r = _pivot_ratios(A)
    return len(r) == 4 and min(r) > 1e-11


def _deficient(A):
    r = _pivot_ratios(A)
    return r[-1] < 1e-15 and all(x > 1e-11 for x in r[:-1])


@pytest.fixture(scope="module")
def deficient():
    """The first 129 rows of "mixed".  Every third row holds its first three observations four times over: three directions, FULL's
    matrix is singular at the first pass ("whole").  Every sixth row, from row 4, holds A B C D and then A B four times over, the first
    copy of A pulled by 150 m: FULL is regular and fails the test, the candidates without C and without D are left with three
    directions and are singular, the others are regular ("subset").  The rest are the rows of "mixed" with their shared references.
    A failing pivot is below 1e-15 of its diagonal entry and every passing one above 1e-11 in the reference's own matrices, a hundred
    either side of the 1e-13 of the rule: asserted here, before any GPU result."""
    geo, ob0, p, rp = raim_cases.batch("mixed")
    shared = raim_cases.references("mixed")
    ob = ob0[:N_DEFICIENT].copy()
    kind, refs = [], []
    for r in range(N_DEFICIENT):
        if r % 3 == 0:
            ob[r, 3:] = np.tile(ob[r, :3], 3)
            kind.append("whole")
        elif r % 6 == 4:  # of the other strides each has one row (73, 113, 128) whose failing pivot is 1.1e-15 of its entry
            ob[r, 4:] = np.tile(ob[r, :2], 4)
            ob[r, 4:5] = raim_cases.shift(ob[r, 4:5].copy(), raim_cases.FAULT_M)
            kind.append("subset")
        else:
            kind.append("regular")
    for r in range(N_DEFICIENT):
        ref = shared[r] if kind[r] == "regular" else raim_cases.reference(geo, ob[r], p, rp)
        refs.append(ref)
        row = ob[r]
        xyz, t, ms0, t0 = raim_ref._row(geo["ephs"], row["eph"], row["tx_ms"], row["tx_frac"])
        w = row["weight"].astype(np.float64)
        first = _normal(xyz, t, w, np.zeros(3), t0)  # the first pass: from the origin, every observation
        if kind[r] == "whole":
            assert _deficient(first), (r, _pivot_ratios(first))
            continue
        assert raim_cases.precondition(ref, p, rp) is None, (r, raim_cases.precondition(ref, p, rp))
        full = ref["full"]
        S = np.array(full["kept"], bool)
        assert _regular(first) and _regular(_normal(xyz[S], t[S], w[S], full["xyz"], full["t_rx"])), r
        if kind[r] == "subset":
            assert ref["raim"]["status"] == raim_ref.EXCLUDED and ref["excluded"] == 4 and sorted(ref["candidates"]) == [0, 1] + list(range(4, 12))
            for k in range(12):
                sub = S.copy()
                sub[k] = False
                A = _normal(xyz[sub], t[sub], w[sub], full["xyz"], full["t_rx"])
                assert _regular(A) if k in ref["candidates"] else _deficient(A), (r, k, _pivot_ratios(A))
    ob.setflags(write=False)
    return geo, ob, p, rp, refs, kind


def test_rank_deficient_rows_in_a_batch_of_regular_ones(eng, deficient):
    """The singular return of newton() in k_raim_detect (a whole row) and in k_raim_exclude (a candidate's subset), in lanes whose
    neighbours go on.  A regular or "subset" row is held to the reference in full.  So is a "whole" row where the reference's own
    solve gives up at the first pass (numpy's LU meets an exact zero: 17 of the 43); in the others it has no pivot rule and takes
    steps through the singular matrix, so every "whole" row is also held to what the rule says: no pass, nothing masked, zeros."""
    import gpsacq
    geo, ob, p, rp, refs, kind = deficient
    assert len(ob) == N_DEFICIENT and kind.count("whole") == 43 and kind.count("subset") == 21
    fix, dop, raim = eng.fix_raim(to_records(geo["ephs"]), ob, gpu_atm(p), gpu_raim(rp))
    worst, held = np.zeros(4), 0
    for k, ref in enumerate(refs):
        if kind[k] != "whole":
            worst = np.maximum(worst, _compare_row((kind[k], k), ref, fix[k], dop[k], raim[k]))
            continue
        if ref["status"] == gpsacq.FIX_NO_CONVERGE and ref["stages"] == [0]:
            _compare_row((kind[k], k), ref, fix[k], dop[k], raim[k])
            held += 1
        assert fix["status"][k] == gpsacq.FIX_NO_CONVERGE and fix["iterations"][k] == 0 and fix["n_used"][k] == 12, k
        assert fix[k].tobytes()[16:] == bytes(64) and fix["rx_ms"][k] == 0, k
        assert dop["used_mask"][k] == 0xFFF and dop[k].tobytes()[4:] == bytes(44), k
        assert raim["status"][k] == gpsacq.RAIM_NONE and raim["excluded"][k] == -1 and raim[k].tobytes()[4:8] == bytes(4) and raim[k].tobytes()[12:] == bytes(28), k
    assert held == 17
    print("deficient batch: position %.3g m, receive time %.3g s, DOP %.3g relative, statistic %.3g of its tolerance" % tuple(worst))
    assert worst[0] <= POS_TOL and worst[1] <= TIME_TOL and worst[2] <= DOP_RTOL and worst[3] <= 1.0
    sub = [k for k in range(N_DEFICIENT) if kind[k] == "subset"]
    assert (raim["n_candidates"][sub] == 10).all() and (raim["excluded"][sub] == 4).all() and (raim["status"][sub] == gpsacq.RAIM_EXCLUDED).all()
    # the regular rows are what they are without the deficient neighbours, bit for bit
    reg = [k for k in range(N_DEFICIENT) if kind[k] == "regular"]
    alone = eng.fix_raim(to_records(geo["ephs"]), ob[reg], gpu_atm(p), gpu_raim(rp))
    assert alone[0].tobytes() == fix[reg].tobytes() and alone[1].tobytes() == dop[reg].tobytes() and alone[2].tobytes() == raim[reg].tobytes()
