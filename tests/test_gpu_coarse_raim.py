"""Coarse-time fix integrity on the GPU (gpsacq_coarse_raim_batch*) against tests/coarse_raim_ref.py, the numpy restatement of
"Coarse-time fix integrity: residual test and one-satellite exclusion" of include/gpsacq.h, and against the library itself:
gpsacq_coarse_fix_batch on the same rows, and on the rows with the excluded column's `valid` cleared, byte for byte.

Every batch is compared only after its precondition (tests/coarse_raim_cases.py) has been asserted on the reference alone.
Tolerances of the output solution are tests/test_gpu_coarse.py's (its compare() is used as it is: POS_TOL, TIME_TOL, S_TOL, rms
within POS_TOL + 1e-9 rms where the two made as many steps).  T = rms^2 W / sigma^2, so an rms within e of the reference's puts T
within 2 e rms W / sigma^2 (e^2 is nothing), and that is what T is held to -- where the solve it comes from made as many steps
as the reference's.  Status, dof, excluded, n_candidates and ref must be equal; a NARROW row (coarse_raim_cases) is compared on
status, excluded and the output solution only.  `iterations` of an excluded row is FULL's and the winner's: the winner's part is
what is left after gpsacq_coarse_fix_batch's count for the whole row, and each part is held to the reference's within one step,
as compare() holds a single solve.
Each test prints its measured maxima before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_raim_cases as cases
import coarse_raim_ref
import coarse_ref
import nav_ref
from coarse_helpers import block_times, phases, priors, synth_sats
from coarse_raim_ref import EXCLUDED, FAILED, NONE, PASS, UNCHECKED
from nav_helpers import geometry, to_records
from test_coarse import POS_TOL
from test_gpu_coarse import FC, FS, compare
from test_gpu_raim import gpu_raim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


def cleared(ob, raim):
    """ob with `valid` of every excluded row's excluded column cleared"""
    cut = ob.copy()
    ex = np.nonzero(raim["status"] == EXCLUDED)[0]
    cut["valid"][ex, raim["excluded"][ex]] = 0
    return cut


def against_the_library(eng, rec, ob, prior, got, label):
    """rows not excluded: gpsacq_coarse_fix_batch's bytes; excluded rows: its bytes for the row without the column, `iterations`
    the sum.  Returns the plain fixes' iterations (FULL's)."""
    fix, info, oo, raim = got
    plain = eng.coarse_fix(rec, ob, prior)
    cut = eng.coarse_fix(rec, cleared(ob, raim), prior)
    ex = raim["status"] == EXCLUDED
    want = [a.copy() for a in plain]
    for w, c in zip(want, cut):
        w[ex] = c[ex]
    want[0]["iterations"][ex] += plain[0]["iterations"][ex]
    moved = [name for g, w in zip((fix, info, oo), want) for name in g.dtype.names if g[name].tobytes() != w[name].tobytes()]
    print("%s: %d rows as gpsacq_coarse_fix_batch gives them, %d as it gives them without the excluded column; fields that moved: %s" %
          (label, int((~ex).sum()), int(ex.sum()), moved or "none"))
    assert fix.tobytes() == want[0].tobytes() and info.tobytes() == want[1].tobytes() and oo.tobytes() == want[2].tobytes(), (label, moved)
    assert (oo[ex, raim["excluded"][ex]].view(np.uint8) == 0).all()
    return plain[0]["iterations"]


def against_the_reference(got, full_steps, rows, ob, rp, label):
    fix, info, oo, raim = got
    n = len(rows)
    nar = np.array([cases.narrow(r) for r in rows])
    want = lambda key: [r["raim"][key] for r in rows]
    assert raim["status"].tolist() == want("status") and raim["excluded"].tolist() == want("excluded"), (label, raim["status"], want("status"))
    ex = raim["status"] == EXCLUDED
    assert (raim["dof"][~nar] == np.array(want("dof"))[~nar]).all() and (raim["n_candidates"][~nar] == np.array(want("n_candidates"))[~nar]).all(), label
    assert (raim["threshold"] == want("threshold")).all(), label
    # the output solution, by test_gpu_coarse's compare(): of an excluded row the winner's own steps
    steps = fix.copy()
    steps["iterations"][ex] -= full_steps[ex]
    sol = [dict(r["out"], iterations=r["out"]["iterations"] - r["full"]["iterations"]) if r["raim"]["status"] == EXCLUDED else r["out"] for r in rows]
    compare(steps, info, oo, sol, ob, label)
    assert all(abs(int(full_steps[i]) - rows[i]["full"]["iterations"]) <= 1 for i in range(n) if not nar[i]), label
    # the statistics
    sigma2, worst = float(rp["sigma_m"]) ** 2, 0.0
    for i, r in enumerate(rows):
        ra = r["raim"]
        if ra["status"] == NONE:
            assert raim[i].tobytes() == np.array([(0, 0, -1, 0, 0.0, 0.0, 0.0)], raim.dtype).tobytes(), (label, i)
            continue
        if ra["status"] != EXCLUDED:
            assert raim["stat"][i] == raim["stat_full"][i], (label, i)
        checks = []
        if not nar[i] and full_steps[i] == r["full"]["iterations"]:
            checks.append(("stat_full", r["full"]["rms"], r["W"]))
        if ra["status"] == EXCLUDED and steps["iterations"][i] == sol[i]["iterations"]:
            checks.append(("stat", r["out"]["rms"], r["W"] - float(ob["weight"][i, ra["excluded"]])))
        for key, rms, W in checks:
            tol = 2 * (POS_TOL + 1e-9 * rms) * rms * W / sigma2
            diff = abs(float(raim[key][i]) - ra[key])
            worst = max(worst, diff / tol) if tol > 0 else worst
            assert diff <= tol, (label, i, key, raim[key][i], ra[key], tol)
    print("%s: statistics within %.3g of their tolerance; NONE %d UNCHECKED %d PASS %d EXCLUDED %d FAILED %d" %
          ((label, worst) + tuple(np.bincount(raim["status"], minlength=5))))


# ---- 1. the batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.BATCHES)
def test_batches(eng, name):
    geo, ob, prior, rp = cases.batch(name)
    rows = cases.references(name)
    assert not [cases.precondition(r, rp) for r in rows if cases.precondition(r, rp)] and 8 * sum(cases.narrow(r) for r in rows) <= len(rows)
    rec = to_records(geo["ephs"])
    got = eng.coarse_fix_raim(rec, ob, prior, gpu_raim(rp))
    full_steps = against_the_library(eng, rec, ob, prior, got, name)
    against_the_reference(got, full_steps, rows, ob, rp, name)
    fix_ms, exclude_ms = eng.coarse_raim_last_ms()
    assert fix_ms > 0 and exclude_ms > 0


def test_default_params_are_the_table(eng):
    """gpsacq_raim_default_params' table in place of the reference's, and coarse params of the caller's"""
    import gpsacq
    geo, ob, prior, rp = cases.batch("three")
    rec = to_records(geo["ephs"])
    a = eng.coarse_fix_raim(rec, ob, prior, gpu_raim(rp))
    b = eng.coarse_fix_raim(rec, ob, prior, gpsacq.raim_params(cases.SIGMA_M))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = eng.coarse_fix_raim(rec, ob, prior, gpu_raim(rp), params=gpsacq.coarse_params(rms_max_m=5.0))  # rms_max_m only sets the flag
    assert (a[1]["flags"] == 0).all() and (c[1]["flags"] == np.where(a[0]["rms"] > 5.0, gpsacq.COARSE_INCONSISTENT, 0)).all() and c[1]["flags"].any()
    assert c[0].tobytes() == a[0].tobytes() and c[3].tobytes() == a[3].tobytes()


# ---- 2. the device form ----------------------------------------------------------------------------------------------------------
def test_device_form_sentinels_and_nan_priors(eng):
    import gpsacq
    import torch
    geo, ob, prior, rp = cases.batch("sixtyseven")
    rec, gp = to_records(geo["ephs"]), gpu_raim(rp)
    n, m = ob.shape
    host = eng.coarse_fix_raim(rec, ob, prior, gp)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    tail = 64
    fill = lambda nbytes: torch.full((nbytes + tail,), 0xA5, dtype=torch.uint8, device="cuda:0")
    sizes = (n * 80, n * 40, n * m * 32, n * 40)
    d_obs, d_prior = dev(ob), dev(prior)

    def run(d_prior_, with_obs_out, sync):
        bufs = [fill(s) for s in sizes]
        torch.cuda.synchronize()
        eng.coarse_fix_raim_device(rec, d_obs.data_ptr(), d_prior_.data_ptr(), n, m, gp, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[3].data_ptr(),
                                   d_obs_out_ptr=bufs[2].data_ptr() if with_obs_out else None, sync=sync)
        torch.cuda.synchronize()
        out = [b.cpu().numpy() for b in bufs]
        assert all((o[s:] == 0xA5).all() for o, s in zip(out, sizes))  # nothing behind any output
        return [o[:s] for o, s in zip(out, sizes)]

    full = run(d_prior, True, False)
    assert all(d.tobytes() == h.tobytes() for d, h in zip(full, host))  # the host form byte for byte
    none = run(d_prior, False, True)
    assert none[0].tobytes() == host[0].tobytes() and none[1].tobytes() == host[1].tobytes() and none[3].tobytes() == host[3].tobytes()
    assert (none[2] == 0xA5).all()  # d_obs_out NULL: the same records, and nothing written there
    assert min(eng.coarse_raim_last_ms()) > 0
    # priors the device form cannot refuse: a row whose prior names no place or no instant has nothing usable
    bad = prior.copy()
    bad["x"][3], bad["rx_ms"][30], bad["z"][64] = np.nan, nav_ref.WEEK_MS, np.inf
    got = run(dev(bad), True, True)
    got = (got[0].view(gpsacq.FIX_DTYPE), got[1].view(gpsacq.COARSE_INFO_DTYPE), got[2].view(gpsacq.OBS_DTYPE).reshape(n, m), got[3].view(gpsacq.FIX_RAIM_DTYPE))
    rows = coarse_raim_ref.coarse_fix_raim(geo["ephs"], ob, bad, rp)
    assert [rows[i]["raim"]["status"] for i in (3, 30, 64)] == [NONE] * 3 and not [cases.precondition(r, rp) for r in rows if cases.precondition(r, rp)]
    assert got[0]["status"][[3, 30, 64]].tolist() == [gpsacq.FIX_TOO_FEW] * 3 and got[0]["n_used"][[3, 30, 64]].tolist() == [0, 0, 0]
    keep = np.ones(n, bool)
    keep[[3, 30, 64]] = False
    assert all(g[keep].tobytes() == h[keep].tobytes() for g, h in zip(got, host))
    full_steps = np.where(keep, eng.coarse_fix(rec, ob, prior)[0]["iterations"], 0)
    against_the_reference(got, full_steps, rows, ob, rp, "NaN priors")


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(eng):
    import gpsacq
    geo, ob, prior, rp = cases.batch("three")
    rec, gp = to_records(geo["ephs"]), gpu_raim(rp)
    n, m = ob.shape
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    ob = np.ascontiguousarray(ob)
    poison = lambda dt, shape: np.frombuffer(bytes([0xA5]) * (np.dtype(dt).itemsize * int(np.prod(shape))), dt).reshape(shape).copy()
    out = [poison(gpsacq.FIX_DTYPE, n), poison(gpsacq.COARSE_INFO_DTYPE, n), poison(gpsacq.OBS_DTYPE, (n, m)), poison(gpsacq.FIX_RAIM_DTYPE, n)]

    def call(rec_=rec, n_eph=12, ob_=ob, prior_=prior, n_=n, m_=m, cp=None, rp_=gp, fix=out[0], info=out[1], oo=out[2], raim=out[3]):
        q = lambda a: None if a is None else p(a)
        return lib.gpsacq_coarse_raim_batch(h, q(rec_), n_eph, q(ob_), q(prior_), n_, m_, q(cp), q(rp_), q(fix), q(info), q(oo), q(raim))

    def raim_with(**kw):
        r = gp.copy()
        for k, v in kw.items():
            if k == "threshold":
                r["threshold"][0][v[0]] = v[1]
            else:
                r[k] = v
        return r

    late, heavy = prior.copy(), ob.copy()
    late["rx_ms"][1] = nav_ref.WEEK_MS
    heavy["weight"][0, 3] = -1.0
    bad = [dict(rec_=None), dict(n_eph=0), dict(ob_=None), dict(prior_=None), dict(n_=0), dict(m_=0), dict(m_=13), dict(fix=None), dict(info=None),
           dict(raim=None), dict(oo=ob), dict(rp_=None), dict(cp=gpsacq.coarse_params(rms_max_m=0.0)), dict(prior_=late), dict(ob_=heavy),
           dict(rp_=raim_with(sigma_m=0.0)), dict(rp_=raim_with(sigma_m=np.nan)), dict(rp_=raim_with(exclude=2)), dict(rp_=raim_with(exclude=-1)),
           dict(rp_=raim_with(threshold=(7, 0.0))), dict(rp_=raim_with(threshold=(0, np.inf))), dict(rp_=raim_with(threshold=(3, -1.0)))]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert lib.gpsacq_last_error()
    assert all((a.view(np.uint8) == 0xA5).all() for a in out)
    # the device form refuses the same (what it can read), and the Python layer raises
    assert lib.gpsacq_coarse_raim_batch_device(h, p(rec), 12, p(ob), p(prior), n, m, None, None, p(out[0]), p(out[1]), None, p(out[3]), 1) == 1
    assert lib.gpsacq_coarse_raim_batch_device(h, p(rec), 12, p(ob), p(prior), n, m, None, p(gp), p(out[0]), p(out[1]), None, None, 1) == 1
    assert lib.gpsacq_coarse_raim_batch_device(h, p(rec), 12, p(ob), p(prior), n, m, None, p(gp), p(out[0]), p(out[1]), p(ob), p(out[3]), 1) == 1
    assert all((a.view(np.uint8) == 0xA5).all() for a in out)
    with pytest.raises(Exception):
        eng.coarse_fix_raim(rec, ob, prior, None)
    # obs_out NULL is no error, and a good call after the bad ones is the good call
    assert call(oo=None) == 0 and call() == 0
    want = eng.coarse_fix_raim(rec, ob, prior, gp)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, want))


# ---- 4. end to end: generated blocks, search, one false peak ---------------------------------------------------------------------
def test_end_to_end_a_false_search_peak_is_excluded(eng):
    """tests/test_gpu_coarse.py's scene and bound.  sigma_m is the README's measured whole-sample code-phase rms of this scene"""
    import gpsacq
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, spb = 4, gpsacq.BLOCK_BYTES * 8
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3
    sats, dops = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.2)
    bits = eng.generate(n_blocks * gpsacq.BLOCK_BYTES, sats, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = [(b, s[0] - 1) for b in range(n_blocks) for s in sats]
    _, peaks = eng.search(bits, tasks=tasks, want_cells=False)
    peaks = peaks.reshape(n_blocks, len(sel)).copy()
    blk_ms, blk_frac = block_times(ref_ms, ref_frac, n_blocks, spb, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    rec, rp = to_records(ephs), gpsacq.raim_params(19.93)
    clean = eng.coarse_fix_raim(rec, eng.coarse_obs(peaks), prior, rp)
    row, col = 1, 3
    peaks["ca_shift"][row, col] = (peaks["ca_shift"][row, col] + 1000) % 5456  # 183 us: 55 km
    fix, info, oo, raim = eng.coarse_fix_raim(rec, eng.coarse_obs(peaks), prior, rp)
    unchecked = eng.coarse_fix(rec, eng.coarse_obs(peaks), prior)[0]
    exact, _ = phases(geo, sel, blk_ms, blk_frac)
    H = coarse_ref.coarse_fix(geo["ephs"], exact, prior)[0]["H"]
    bound = np.linalg.norm(np.linalg.solve(H.T @ H, H.T)[:3], 2) * np.sqrt(8.0) * nav_ref.C / FS
    err = lambda f: np.linalg.norm(np.stack([f["x"], f["y"], f["z"]], 1) - geo["rx"], axis=1)
    print("clean: status %s T %s; faulted: status %s excluded %s T_full %s T %s; error %s m (unchecked %s m, bound %.0f m)" %
          (clean[3]["status"], np.round(clean[3]["stat"], 2), raim["status"], raim["excluded"], np.round(raim["stat_full"], 1), np.round(raim["stat"], 2),
           np.round(err(fix), 1), np.round(err(unchecked), 1), bound))
    assert raim["status"][row] == EXCLUDED and raim["excluded"][row] == col and fix["status"][row] == 0 and fix["n_used"][row] == 7
    assert err(fix)[row] <= bound < err(unchecked)[row]
    others = [b for b in range(n_blocks) if b != row]
    assert all(x[others].tobytes() == y[others].tobytes() for x, y in zip((fix, info, oo, raim), clean))  # the other blocks do not know
